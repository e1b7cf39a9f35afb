"""Hard swish (code 7) and hard sigmoid (code 8) on the device, every element against float64 of

    hswish(x) = x min(max(x + 3, 0), 6) / 6            hsigmoid(x) = min(max(x / 6 + 1/2, 0), 1)

(tests/test_hardswish.py: hswish64, hsigmoid64, forward64h).  The inequalities are those of tests/test_layer_gemm_gpu.py and
tests/test_resact_gpu.py with their tau (imported), and the two things the new functions force:

* the slope through the activation: max |hswish'| = 1.5 (hswish' = (2x + 3) / 6 on [-3, 3]) where those files carry 1.2 for GELU and
  swish; 1/6 for hsigmoid;
* eps_act, the activation's own roundings.  Both kernels' forms (kernels.hpp bh_act<ACT_HSWISH>, bh_hswish_slow) are g = fma(s, c,
  1/2) with c = float32(1/6), the clamp of g to [0, 1] (exact), and s g -- three f32 roundings.  Inside (-3, 3) the fma's rounding
  is half an ulp of a g below 1, 2^-25, and c is off by 5.0e-9 = 2^-27.6, at most 2^-26 in g at |s| <= 3: together under
  1.25 2^-24 |s| on the product s g; the last multiply adds 2^-24 |s g| <= 2^-24 |s|.  2.25 2^-24 |s| in all:
  eps_act(s) = 3 2^-23 |s| leaves x2.6.  Outside [-3, 3] the clamp is exact and only the multiply by 1 (or 0) remains.  hsigmoid is
  the fma alone, under 2^-24 while unsaturated:  eps_act = 2^-22.

before the add:   |got - (act(pre) + R)|  <=  tau (1.5 bound + |R|) + eps_act(pre),     bound = |A| |W| + |b|
after the add:    |got - act(pre + R)|    <=  1.5 tau (bound + |R|) + eps_act(pre + R)
hsigmoid:         the same with 1/6 for 1.5

Shapes: tests/test_resact_gpu.py's catalogues, one per dispatch branch -- 7, 48, 105, 3000 and 6151 rows (the skinny kernel, the
streaming one, pw_gemm16s at 2 / 4 / 8 column tiles a workgroup), the 5x7 and 9x11 convolutions at 3x3 stride 1 / 2 and 1x1 stride 2
-- with biases of +-7.5 in two columns, so that values lie in both saturated ranges and across +-3.  The head kernel at both
pixel-tile heights and both column-tile counts.  The gate through bh_debug_se_gate in its three forms with ReLU inside and the hard
sigmoid at its end, and a NaN channel sum that must come out as NaN gates.  Whole MobileNetV3-style models on the `.onnx` route in
every spelling and precision.  Every buffer the entry points allocate sits in NaN guard bands and every output starts as the payload
0x7fc0beef (api_debug.hip DebugLaunch).

The fused block kernel's hard-swish family (indices 3 n_base ...): every live row, forced, on every case of
tests/test_mbconv_block.py's catalogue through bh_debug_mbconv_block, pass A included, against a three-stage float64 block written
here from O.gemm64's / O.depthwise64's arithmetic (O.mbconv64 takes the activation by the oracle's code, which has no 7) with
tests/test_mbconv_block_gpu.py's stage-by-stage propagation, 1.5 for its 1.2 and this file's eps_act; the one-segment and
narrow-tile twins give their block's bits; the names that ran are the names shipped.  In the whole models every hard-swish block
runs fused on a family-3 entry.

Wall time on an MI355X: the module's 161 cases in 11.4 s; the slowest case 0.42 s (a slice of eight family-3 rows on all their
cases; the slices take 0.1-0.4 s), mobilenetv3_audio in four precisions 0.3 s, the big pointwise shapes 0.1-0.2 s each (their
float64 references are computed once per weight kind and shared)."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O
import test_gate_layers as CAT
from test_hardswish import HSIGMOID, HSWISH, act64h, family3_cases, family3_rows, forward64h, hard_swish_blocks, hsigmoid64, hswish64, names_ex
from test_layer_gemm_gpu import HEAD, _tau
from test_random_plans_gpu import F16_LOGIT_RTOL, LOGIT_RTOL
from test_resact_gpu import CONV_CASES, PW_BIG, _conv_reference, _f16_valued, _pw_reference

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
BH_ERR_NONFINITE = -8
SLOPE = {HSWISH: 1.5, HSIGMOID: 1.0 / 6.0}
REACHED = set()
WORST = {}


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _eps_act(s, act):
    return 3.0 * 2.0 ** -23 * np.abs(s) if act == HSWISH else np.full_like(s, 2.0 ** -22)


def _run(entry, *args):
    lib = _lib.load()
    name = C.create_string_buffer(160)
    rc = getattr(lib, entry)(0, *args, name, 160)
    assert rc == 0, (entry, rc, lib.bh_last_error())
    REACHED.add(name.value.decode())
    return name.value.decode()


def _conv(X, W, b, R, shape, act, terms, after):
    n = X.shape[0]
    out = np.empty((n * shape[2] * shape[3], shape[5]), np.float32)
    k = _run("bh_debug_conv_gemm_after" if after else "bh_debug_conv_gemm", _p(X), _p(W), _p(b), _p(R), _p(out), n, _p(np.asarray(shape, np.int32)), act, terms)
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"
    return out, k


def _layer(A, W, b, R, act, terms, after, pool_rows=0):
    M, K = A.shape
    N = W.shape[1]
    out = np.empty((M // pool_rows if pool_rows else M, N), np.float32)
    k = _run("bh_debug_layer_gemm_after" if after else "bh_debug_layer_gemm", _p(A), _p(W), _p(b), _p(R), _p(out), M, K, N, pool_rows, act, terms)
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"
    return out, k


def _check(got, name, pre, bound, R, act, terms, k_eff, after, what):
    r = R.astype(np.float64)
    slope = SLOPE[act]
    if after:
        s = pre + r
        ref, scale = act64h(s, act), slope * (bound + np.abs(r))
    else:
        s = pre
        ref, scale = act64h(s, act) + r, slope * bound + np.abs(r)
    assert np.isfinite(got).all(), (what, name, "non-finite output")
    err = np.abs(got.astype(np.float64) - ref)
    eps = _eps_act(s, act)
    tol = _tau(terms, k_eff) * scale + eps
    key = (name.split("<")[0], terms, act)
    WORST[key] = max(WORST.get(key, 0.0), float(np.max(err / tol)))
    print(f"{what} {name} {'after' if after else 'before'}: worst err / tol {float(np.max(err / tol)):.3f}")
    bad = err > tol
    if bad.any():
        i = np.unravel_index(np.argmax(err / tol), err.shape)
        pytest.fail(f"{what} {name} act {act}: {int(bad.sum())} of {bad.size} elements off, worst at {i}: got {got[i]!r} want {ref[i]!r} "
                    f"(argument {s[i]!r}), err {err[i]:.3e} > tol {tol[i]:.3e}")


def _both_ranges(s):
    assert (s < -3).any() and (s > 3).any() and ((s > -3) & (s < 0)).any() and ((s > 0) & (s < 3)).any(), "the arguments should lie in both saturated ranges and across +-3"


# ---- a. layer GEMMs and convolutions ----------------------------------------------------------------------------------------------
PW_SHAPES = [(7, 96, 136), (32, 32, 20), (48, 96, 136), (105, 96, 136), (297, 32, 72)] + PW_BIG
CONV_SHAPES = ["5x7_3x3s2_4to20", "5x7_1x1s2_36to72", "9x11_3x3s1_36to136", "9x11_3x3s2_36to72"]


def _pw_family(M, terms):
    return "pw_gemm_kernel" if terms == 0 else "pw_gemm16_skinny_kernel" if M <= 32 else "pw_gemm16_kernel" if M < 64 else "pw_gemm16s_kernel"


@pytest.mark.parametrize("after", [False, True], ids=["before", "after"])
@pytest.mark.parametrize("terms", [0, 1, 3, 2])
@pytest.mark.parametrize("mkn", PW_SHAPES, ids=lambda s: "M%d_K%d_N%d" % s)
def test_pointwise_hard_swish_matches_float64(mkn, terms, after):
    M, K, N = mkn
    A, W, b, R, pre, bound = _pw_reference(mkn, terms == 2)
    _both_ranges(pre + R if after else pre)
    got, k = _layer(A, W, b, R, HSWISH, terms, after)
    assert k.split("<")[0] == _pw_family(M, terms), k
    if terms:
        assert f"<{terms},HSWISH{',AFTER' if after else ''}" in k and (",AFTER" in k) == after, k
    if mkn in PW_BIG and terms:
        assert k.endswith("NTB=4>" if M == 3000 else "NTB=8>"), k
    _check(got, k, pre, bound, R, HSWISH, terms, K, after, "pw")


@pytest.mark.parametrize("after", [False, True], ids=["before", "after"])
@pytest.mark.parametrize("terms", [0, 1, 2, 3])
@pytest.mark.parametrize("name", CONV_SHAPES)
def test_convolution_hard_swish_matches_float64(name, terms, after):
    shape = CONV_CASES[name]
    X, W, b, R, pre, bound = _conv_reference(name, terms == 2)
    _both_ranges(pre + R if after else pre)
    got, k = _conv(X, W, b, R, shape, HSWISH, terms, after)
    assert (k == f"conv_gemm16_kernel<{terms},HSWISH{',AFTER' if after else ''}>") if terms else k.startswith("conv_gemm_kernel<BM="), k
    _check(got, k, pre, bound, R, HSWISH, terms, shape[6] * shape[7] * shape[4], after, name)


@pytest.mark.parametrize("after", [False, True], ids=["before", "after"])
def test_hard_sigmoid_on_the_f32_layer_kernels(after):
    """code 8 is never templated: terms 0 only -- the split-f16 entries refuse it -- on the pointwise and the convolution kernel"""
    lib = _lib.load()
    for mkn in ((7, 96, 136), (105, 96, 136)):
        A, W, b, R, pre, bound = _pw_reference(mkn, False)
        got, k = _layer(A, W, b, R, HSIGMOID, 0, after)
        assert k.startswith("pw_gemm_kernel<"), k
        _check(got, k, pre, bound, R, HSIGMOID, 0, mkn[1], after, "pw hsigmoid")
        out = np.empty((mkn[0], mkn[2]), np.float32)
        for terms in (1, 3):
            entry = lib.bh_debug_layer_gemm_after if after else lib.bh_debug_layer_gemm
            assert entry(0, _p(A), _p(W), _p(b), _p(R), _p(out), mkn[0], mkn[1], mkn[2], 0, HSIGMOID, terms, None, 0) != 0
    name = "9x11_3x3s1_36to136"
    X, W, b, R, pre, bound = _conv_reference(name, False)
    got, k = _conv(X, W, b, R, CONV_CASES[name], HSIGMOID, 0, after)
    assert k.startswith("conv_gemm_kernel<"), k
    _check(got, k, pre, bound, R, HSIGMOID, 0, 9 * 36, after, "conv hsigmoid")


@pytest.mark.parametrize("act", [HSWISH, HSIGMOID])
def test_grouped_convolution_takes_both_codes(act):
    from test_gconv_gpu import _reference
    shape, X, W, b, pre, bound, k_eff = _reference("24x3g", "3x3s1", (9, 11))
    b = b.copy()
    b[:2] = (7.5, -7.5)
    pre = pre + (b.astype(np.float64) - _reference("24x3g", "3x3s1", (9, 11))[3].astype(np.float64))
    bound = bound + np.abs(b.astype(np.float64)) - np.abs(_reference("24x3g", "3x3s1", (9, 11))[3].astype(np.float64))
    for terms in (0, 3, 1):          # (the grouped kernels take the activation at run time in every precision)
        out = np.empty((3 * shape[2] * shape[3], shape[5]), np.float32)
        k = _run("bh_debug_gconv", _p(X), _p(W), _p(b), _p(out), 3, _p(np.asarray(shape, np.int32)), act, terms)
        assert not (out.view(np.uint32) == UNWRITTEN).any()
        assert k == {0: "gconv_kernel", 3: "gconv16_kernel<3>", 1: "gconv16_kernel<1>"}[terms], k
        _check(out, k, pre, bound, np.zeros_like(out), act, terms, k_eff, False, "gconv")


def _head_check(case, terms):
    P, n_seg, K, N = case
    rng = np.random.default_rng(P * 7 + n_seg * 131 + K + N)
    A = (rng.standard_normal((n_seg * P, K)) * rng.uniform(0.2, 3.0, K)).astype(np.float32)
    W = (rng.standard_normal((K, N)) * math.sqrt(2.0 / K)).astype(np.float32)
    if terms == 2:
        W = _f16_valued(W)
    b = rng.standard_normal(N).astype(np.float32)
    b[:2] = (7.5, -7.5)
    got, k = _layer(A, W, b, None, HSWISH, terms, False, pool_rows=P)
    pre = O.gemm64(A, W, b)
    bound = np.abs(A.astype(np.float64)) @ np.abs(W.astype(np.float64)) + np.abs(b.astype(np.float64))
    v = hswish64(pre)
    # tests/test_layer_gemm_gpu.py _check_head: the mean of the per-element bounds plus the pool's own rounding
    pool_round = P * 2.0 ** -24 * O.head_pool64(np.abs(v), P)
    tol = _tau(terms, K) * 1.5 * O.head_pool64(bound, P) + O.head_pool64(_eps_act(pre, HSWISH), P) + pool_round
    err = np.abs(got.astype(np.float64) - O.head_pool64(v, P))
    print(f"head {case} {k}: worst err / tol {float(np.max(err / tol)):.3f}")
    assert np.isfinite(got).all() and (err <= tol).all(), (case, k, float(np.max(err / tol)))
    return k


@pytest.mark.parametrize("terms", [1, 2, 3])
@pytest.mark.parametrize("case", [(17, 9, 320, 128), (48, 33, 32, 1280), (49, 5, 32, 128), (80, 33, 320, 128)], ids=lambda c: "P%d_n%d_K%d_N%d" % c)
def test_head_convolution_and_pool_with_hard_swish(case, terms):
    assert {c[0] for c in HEAD} >= {17, 48, 49, 80}          # (the pixel counts are that catalogue's edges of the two tile heights)
    P, n_seg = case[:2]
    k = _head_check(case, terms)
    assert k == f"head_gap16_kernel<PT={3 if P <= 48 else 5},SW={2 if P <= 48 else 1},T={terms},HSWISH,CT={2 if n_seg <= 32 else 8}>", k


def test_every_hard_swish_instantiation_was_reached():
    """families x terms x position, built here; what the tests above did not launch (run alone, or under -k) is launched on zeros"""
    want = [f"{fam}<{t},HSWISH{a}>" for fam in ("conv_gemm16_kernel", "pw_gemm16_skinny_kernel", "pw_gemm16_kernel") for t in (1, 2, 3) for a in ("", ",AFTER")]
    want += [f"pw_gemm16s_kernel<{t},HSWISH{a},NTB={n}>" for t in (1, 2, 3) for a in ("", ",AFTER") for n in (2, 4, 8)]
    want += [f"head_gap16_kernel<PT={pt},SW={sw},T={t},HSWISH,CT={ct}>" for (pt, sw) in ((3, 2), (5, 1)) for t in (1, 2, 3) for ct in (2, 8)]
    assert len(want) == len(set(want)) == 18 + 18 + 12
    z = lambda *s: np.zeros(s, np.float32)
    for w in want:
        if w in REACHED:
            continue
        fam, args = w.split("<")[0], w.split("<")[1].rstrip(">").split(",")
        after = "AFTER" in args
        if fam == "head_gap16_kernel":
            P, n = (17 if "PT=3" in w else 49), (5 if "CT=2" in w else 33)
            _layer(z(n * P, 32), z(32, 128), z(128), None, HSWISH, int(args[2][2:]), False, pool_rows=P)
        elif fam == "conv_gemm16_kernel":
            shape = CONV_CASES["5x7_3x3s2_4to20"]
            _conv(z(3, shape[0], shape[1], 4), z(3, 3, 4, 20), z(20), z(105, 20), shape, HSWISH, int(args[0]), after)
        else:
            M, N = {"pw_gemm16_skinny_kernel": (7, 20), "pw_gemm16_kernel": (48, 20)}.get(fam) or {"NTB=2": (105, 20), "NTB=4": (3000, 1024), "NTB=8": (6151, 1024)}[args[-1]]
            _layer(z(M, 32), z(32, N), z(N), z(M, N), HSWISH, int(args[0]), after)
    assert not [w for w in want if w not in REACHED], sorted(REACHED)
    assert not [n for n in REACHED if "HSIGMOID" in n]                       # never templated
    for key, v in sorted(WORST.items()):
        print(f"  {key}: worst err / tol {v:.3f}")


# ---- b. the gate ---------------------------------------------------------------------------------------------------------------------
GATES = {"c72_cr24": (72, 24, 8), "c580_cr24": (580, 24, 4)}          # C, Cr, tiles; P = 7 tiles + 3 (tests/test_gate_layers.py)
FORMS = {0: "se_gate_kernel", 1: "se_hidden_kernel+se_gate16_kernel", 2: "se_pool_kernel+pw_gemm_kernel"}
_GATE_OPS = {}


def _gate_operands(name, n=3):
    if name not in _GATE_OPS:
        C_, Cr, tiles = GATES[name]
        P = 7 * tiles + 3
        rng = np.random.default_rng(C_ * 3 + Cr)
        ops = dict(W1=(rng.standard_normal((C_, Cr)) * math.sqrt(2.0 / C_)).astype(np.float32), b1=rng.standard_normal(Cr).astype(np.float32),
                   W2=(rng.standard_normal((Cr, C_)) * math.sqrt(2.0 / Cr) * 3.0).astype(np.float32), b2=(rng.standard_normal(C_) * 2.0).astype(np.float32))
        scale = rng.uniform(0.2, 3.0, C_) * (P / tiles)
        ops["part"] = np.ascontiguousarray(((rng.standard_normal((n, tiles, C_)) + 0.5) * scale).astype(np.float32))
        for a in ops.values():
            a.setflags(write=False)
        _GATE_OPS[name] = ops
    return _GATE_OPS[name]


def _run_gate(name, ops, act1, act2, form):
    C_, Cr, tiles = GATES[name]
    n = ops["part"].shape[0]
    gate = np.empty((n, C_), np.float32)
    k = _run("bh_debug_se_gate", _p(ops["part"]), n, tiles, 7 * tiles + 3, C_, Cr, _p(ops["W1"]), _p(ops["b1"]), act1, _p(ops["W2"]), _p(ops["b2"]), act2, form, _p(gate))
    assert not (gate.view(np.uint32) == UNWRITTEN).any()
    return gate, k


def _gate_forms(name):
    C_, Cr, _ = GATES[name]
    return [f for f, ok in ((0, CAT.se_gate_supports(C_, Cr)), (1, CAT.se_gate16_supports(C_, Cr)), (2, True)) if ok]


GATE_PARAMS = [(n, f) for n in GATES for f in _gate_forms(n)]          # every form that takes the widths


def test_the_two_widths_reach_all_three_forms():
    assert 0 in _gate_forms("c72_cr24") and {1, 2} <= set(_gate_forms("c580_cr24"))
    assert CAT.se_gate_form(580, 24) == 1 and CAT.se_gate_form(72, 24) == 0          # at C >= 577 the two-kernel form dispatches


@pytest.mark.parametrize("name,form", GATE_PARAMS)
def test_relu_hard_sigmoid_gate_against_float64(name, form):
    """pool -> 1x1 (ReLU) -> 1x1 (hard sigmoid): tests/test_gate_layers.py's propagation -- tau per stage on the stage's bound, the
    hidden error through |W2| -- with 1/6 for the sigmoid's 1/4 and eps_act = 2^-22 at the end"""
    C_, Cr, tiles = GATES[name]
    P = 7 * tiles + 3
    ops = _gate_operands(name)
    gate, k = _run_gate(name, ops, O.ACT_RELU, HSIGMOID, form)
    assert k == FORMS[form], k
    part, W1, b1, W2, b2 = (ops[q].astype(np.float64) for q in ("part", "W1", "b1", "W2", "b2"))
    _, pooled, preH, H, preG = O.se_gate64(part, P, W1, b1, O.ACT_RELU, W2, b2, O.ACT_NONE)
    aW1, aW2 = np.abs(W1), np.abs(W2)
    e_pool = _tau(0, tiles) * np.abs(part).sum(axis=1) / P
    e_H = 1.2 * (e_pool @ aW1 + _tau(0, C_) * (np.abs(pooled) @ aW1 + np.abs(b1)))          # (ReLU: no eps_act)
    tol = (1.0 / 6.0) * (e_H @ aW2 + _tau(0, Cr) * (np.abs(H) @ aW2 + np.abs(b2))) + 2.0 ** -22
    ref = hsigmoid64(preG)
    assert (ref == 0).any() and (ref == 1).any() and ((ref > 0) & (ref < 1)).any(), "the gates should saturate on both sides"
    err = np.abs(gate.astype(np.float64) - ref)
    print(f"gate {name} {k}: worst err / tol {float(np.max(err / tol)):.3f}")
    assert np.isfinite(gate).all() and (err <= tol).all(), (name, k, float(np.max(err / tol)))


@pytest.mark.parametrize("name,form", GATE_PARAMS)
def test_a_nan_channel_sum_comes_out_as_nan_gates(name, form):
    """One channel sum of segment 1 is NaN.  The hidden activation here is swish -- arithmetic on its argument all the way, so the NaN
    reaches every hidden unit of that segment and with it every one of the segment's gate sums (ReLU's fmaxf inside the gate would stop
    it in front of the activation under test).  The hard sigmoid must hand it on: all of segment 1's gates NaN, every other gate
    finite and bit for bit what it is without the NaN.  A clamp written with fminf / fmaxf / v_med3_f32 gives 0 or 1 for them and
    fails here (tests/test_hardswish.py evaluates both spellings in numpy)."""
    ops = dict(_gate_operands(name))
    clean, _ = _run_gate(name, ops, O.ACT_SWISH, HSIGMOID, form)
    part = ops["part"].copy()
    part[1, 0, 5] = np.nan
    ops["part"] = part
    gate, k = _run_gate(name, ops, O.ACT_SWISH, HSIGMOID, form)
    assert np.isnan(gate[1]).all(), (k, int(np.isnan(gate[1]).sum()), gate.shape[1])
    assert np.isfinite(gate[[0, 2]]).all() and (gate[[0, 2]].view(np.uint32) == clean[[0, 2]].view(np.uint32)).all(), k


# ---- c. the fused family -------------------------------------------------------------------------------------------------------------
from test_mbconv_block_gpu import _family as _mb_family, _hold as _mb_hold, operands as mb_operands, plane_excess          # noqa: E402
import test_mbconv_block as MBCAT                                                                                          # noqa: E402

MB_REACHED = set()
MB_SLICE = 8          # rows a pytest case: a few seconds each


def _mb_run(shape, n, ops, force, variant=0, ksplit=0, dnull=False):
    """tests/test_mbconv_block_gpu.py run_block, recording into this module's own set (that module's completeness test reads its)"""
    lib = _lib.load()
    Cexp, Cout, Ho, Wo, se = shape[3], shape[4], shape[5], shape[6], shape[14]
    rc0, rec0, _ = MBCAT.plan(shape, force, variant)
    assert rc0 == 0, (rc0, lib.bh_last_error(), shape)
    tiles = int(rec0[2] * rec0[3])
    Y = None if se else np.empty((n, Ho, Wo, Cout), np.float32)
    D = np.empty((n * Ho * Wo * Cexp,), np.float32) if (se and not dnull) else None
    PP = np.empty((n, tiles, Cexp), np.float32) if se else None
    rec = np.zeros(24, np.int32)
    name = C.create_string_buffer(160)
    rc = lib.bh_debug_mbconv_block(0, _p(np.asarray(shape, np.int32)), n, _p(ops["X"]), _p(ops["We"]), _p(ops["be"]), _p(ops["Wd"]), _p(ops["bd"]),
                                   _p(ops["Wp"]), _p(ops["bp"]), _p(ops["R"]), _p(ops["gate"]), force, variant, ksplit, _p(Y), _p(D), _p(PP), _p(rec), name, 160)
    assert rc == 0, (rc, lib.bh_last_error(), shape)
    nm = name.value.decode()
    MB_REACHED.add(nm)
    for what, a in (("Y", Y), ("D", D), ("pool_part", PP)):
        if a is not None:
            assert not (a.view(np.uint32) == UNWRITTEN).any(), (nm, what, "elements never written", shape)
    if D is not None:
        if shape[15]:
            D = D.reshape(n * Ho * Wo // 16, Cexp // 16, 16, 16).transpose(0, 2, 1, 3)
        D = np.ascontiguousarray(D).reshape(n, Ho, Wo, Cexp)
    return dict(Y=Y, D=D, PP=PP), rec, nm


def _mb_reference(shape, ops):
    """O.mbconv64's three stages with the float64 hard swish, and tests/test_mbconv_block_gpu.py reference()'s bounds e_E, e_D, e_Y
    with the slope 1.5 and this file's eps_act"""
    H, W, Cin, Cexp, Cout, Ho, Wo, pad_t, pad_l, KS, ST, act, prec, noexp = shape[:14]
    stem_c, stem_h, stem_w, stem_k, stem_s, stem_pt, stem_pl = shape[16:23]
    f = np.float64
    A = O.stem_rows64(ops["X"], stem_k, stem_s, stem_pt, stem_pl, H, W) if stem_c else np.asarray(ops["X"], f)
    if noexp:
        preE = E = A
    else:
        preE = A @ np.asarray(ops["We"], f) + np.asarray(ops["be"], f)
        E = hswish64(preE)
    preD = O.depthwise64(E, ops["Wd"], KS, ST, pad_t, pad_l, Ho, Wo) + np.asarray(ops["bd"], f)
    D = hswish64(preD)
    Dg = D if ops["gate"] is None else D * np.asarray(ops["gate"], f)[:, None, None, :]
    Y = Dg @ np.asarray(ops["Wp"], f) + np.asarray(ops["bp"], f)
    if ops["R"] is not None:
        Y = Y + np.asarray(ops["R"], f)
    aWd, aWp = np.abs(ops["Wd"].astype(f)), np.abs(ops["Wp"].astype(f))
    if noexp:
        e_E = np.zeros_like(E)
    else:
        aA, aWe = np.abs(A), np.abs(ops["We"].astype(f))
        e_E = _tau(prec, Cin) * 1.5 * (aA @ aWe + np.abs(ops["be"].astype(f))) + _eps_act(preE, HSWISH)
        dWe = plane_excess(ops["We"], prec, clamp21=False)
        if dWe is not None and dWe.any():
            e_E = e_E + 1.5 * (aA @ dWe)
    dw = lambda t: O.depthwise64(t, aWd, KS, ST, pad_t, pad_l, Ho, Wo)
    e_D = 1.5 * (dw(e_E) + _tau(prec, KS * KS) * (dw(np.abs(E)) + np.abs(ops["bd"].astype(f)))) + _eps_act(preD, HSWISH)
    e_Dg = e_D if ops["gate"] is None else e_D * np.abs(ops["gate"].astype(f))[:, None, None, :]
    aR = 0.0 if ops["R"] is None else np.abs(ops["R"].astype(f))
    e_Y = e_Dg @ aWp + _tau(prec, Cexp) * (np.abs(Dg) @ aWp + np.abs(ops["bp"].astype(f)) + aR)
    dWp = plane_excess(ops["Wp"], prec, clamp21=False)
    if dWp is not None and dWp.any():
        e_Y = e_Y + np.abs(Dg) @ dWp
    return dict(Y=Y, D=D, Dsum=D.sum(axis=(1, 2)), e_D=e_D, e_Y=e_Y)


def _mb_case(r, c, seed):
    shape, n = c["shape"], c["n"]
    ops = mb_operands(shape, n, c["residual"], c["gate"], seed)
    what = "family 3 entry %d %s %s n %d" % (r["base"], "+".join(sorted(c["tags"])), list(shape), n)
    out, rec, name = _mb_run(shape, n, ops, r["base"], ksplit=c["ksplit"], dnull=c["dnull"])
    assert rec[0] == r["ci"] and name == "mbconv<%s,%d>" % (r["name"], c["se"]), (what, rec, name)
    ref = _mb_reference(shape, ops)
    key = (_mb_family(shape, shape[14]) + "_hswish", shape[12])
    if not shape[14]:
        _mb_hold(out["Y"], ref["Y"], ref["e_Y"], key, what + " Y")
    else:
        if out["D"] is not None:
            _mb_hold(out["D"], ref["D"], ref["e_D"], key, what + " D")
        _mb_hold(out["PP"].astype(np.float64).sum(axis=1), ref["Dsum"], ref["e_D"].sum(axis=(1, 2)), key, what + " pool sums")
    if c["ksplit"]:
        assert rec[12] >= 2, (what, rec)
        ops2 = {k: (v[:2] if k in ("X", "R", "gate") and v is not None else v) for k, v in ops.items()}
        out2, rec2, _ = _mb_run(shape, 2, ops2, r["base"], ksplit=1)
        assert rec2[12] == rec[12] and (out2["Y"] == out["Y"][:2]).all(), (what, "the channel split's bits depend on n")
    if c["oversub"]:
        n_big = MBCAT.oversub_segments(r, rec)
        reps = -(-n_big // n)
        big = {k: (np.concatenate([v] * reps)[:n_big] if k in ("X", "R", "gate") and v is not None else v) for k, v in ops.items()}
        outb, _, _ = _mb_run(shape, n_big, big, r["base"])
        for k in range(n):
            assert (outb["Y"][k::n] == out["Y"][k]).all(), (what, "segment %d of the large launch depends on its place" % k)


_MB_ROWS = family3_rows()


@pytest.mark.parametrize("k0", range(0, len(_MB_ROWS), MB_SLICE))
def test_family_3_rows_at_their_edges(k0):
    for r in _MB_ROWS[k0:k0 + MB_SLICE]:
        cs = family3_cases(r)
        assert cs, r["base"]
        for k, c in enumerate(cs):
            _mb_case(r, c, seed=1000 * r["base"] + 10 * k + HSWISH)


def test_family_3_twins_give_the_same_bits():
    """the first row of each class -- a block with a one-segment twin, one with a narrow-tile twin, a pass A whose twin's sums match
    (tests/test_mbconv_block_gpu.py test_twins_give_the_same_bits, three rows)"""
    seen = {}
    for r in _MB_ROWS:
        if len(seen) == 3:
            break
        for c in family3_cases(r):
            if not ({"natural", "se_nhwc", "colth_low", "k_relaxed"} & c["tags"]):
                continue
            rc, rec, _ = MBCAT.plan(c["shape"], r["base"])
            kinds = [k for k, ok in (("twin", rec[13] and not c["se"]), ("sums", rec[13] and c["se"] and rec[15]), ("narrow", rec[14] and not c["se"])) if ok and k not in seen]
            if not kinds:
                continue
            ops = mb_operands(c["shape"], 3, c["residual"], c["gate"], seed=77 + r["base"])
            base, _, _ = _mb_run(c["shape"], 3, ops, r["base"])
            for kind in kinds:
                tw, rect, nm = _mb_run(c["shape"], 3, ops, r["base"], variant=2 if kind == "narrow" else 1)
                assert rect[0] != rec[0] and 3 * r["nbase"] <= rect[0] < 4 * r["nbase"], (kind, rect[0])
                if kind == "sums":
                    assert (tw["PP"] == base["PP"]).all() and (tw["D"] == base["D"]).all(), (r["base"], nm)
                else:
                    assert (tw["Y"] == base["Y"]).all(), (r["base"], nm, kind)
                seen[kind] = r["base"]
    assert set(seen) == {"twin", "sums", "narrow"} and len(set(seen.values())) == 3, seen


def test_the_family_3_names_that_ran_are_the_names_shipped():
    """no exemption list; run alone (or under -k) it launches every row's first case itself"""
    shipped = set()
    for r in _MB_ROWS:
        shipped.add("mbconv<%s,0>" % r["name"])
        if r["has_se"]:
            shipped.add("mbconv<%s,1>" % r["name"])
    for r in _MB_ROWS:
        for se in ((0, 1) if r["has_se"] else (0,)):
            if "mbconv<%s,%d>" % (r["name"], se) not in MB_REACHED:
                c = next(c for c in family3_cases(r) if c["se"] == se and not c["oversub"])
                _mb_run(c["shape"], c["n"], mb_operands(c["shape"], c["n"], c["residual"], c["gate"], 5), r["base"], ksplit=c["ksplit"], dnull=c["dnull"])
    assert MB_REACHED == shipped, (sorted(shipped - MB_REACHED)[:10], sorted(MB_REACHED - shipped)[:10])
    assert all(nm.split(",")[17] == str(HSWISH) for nm in MB_REACHED)


# ---- d. whole models ------------------------------------------------------------------------------------------------------------------
PRECISIONS = (("f32", LOGIT_RTOL), ("f16x3", LOGIT_RTOL), ("auto", LOGIT_RTOL), ("f16", F16_LOGIT_RTOL))
MODEL_SPELLINGS = ("op", "hsigmoid", "decomposed")
_MODELS = {}


def _model(which):
    """(model, three segments, float64 logits): built and evaluated once, shared, never modified"""
    if which not in _MODELS:
        m = synth.build_model("mobilenetv3_audio", n_classes=40) if which == "large" else synth.build_model("mnv3_plan", plan=synth.random_mnv3_plan(which))
        segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=11 + (0 if which == "large" else which))
        segs[2] *= np.float32(0.01)
        ref = forward64h(m, segs)
        segs.setflags(write=False); ref.setflags(write=False)
        _MODELS[which] = (m, segs, ref)
    return _MODELS[which]


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


@pytest.mark.parametrize("spelling", MODEL_SPELLINGS)
@pytest.mark.parametrize("which", [0, 1, 3, "large"])
def test_mobilenetv3_models_on_the_onnx_route(which, spelling, tmp_path):
    from birda_amd.classifier import BirdClassifier
    m, segs, ref = _model(which)
    onnx = _write(str(tmp_path / "m.onnx"), convert.model_to_onnx(m, frontend_spelling="stft", spell_hswish=spelling))
    scale = max(1.0, float(np.abs(ref).max()))
    n_base = len(names_ex()) // 4
    # (the hard-swish GEMM layers OUTSIDE the blocks: the head convolution and the hidden dense layer)
    inside = {i for i in hard_swish_blocks(m) if m.layers[i].op == mf.OP_PWCONV}          # (a fused block's expand convolution)
    hs_gemm = [i for i, L in enumerate(m.layers) if L.act == HSWISH and L.op in (mf.OP_PWCONV, mf.OP_DENSE) and i not in inside]
    assert hs_gemm and ((which in (1, 3, "large")) == any(L.act == HSIGMOID for L in m.layers))
    for prec, tol in PRECISIONS:
        clf = BirdClassifier(onnx, None, precision=prec)
        ctx = clf.create_batch_context(3)
        got = clf.predict_logits(ctx, segs)
        err = float(np.abs(got - ref).max())
        print(f"mnv3 {which} {spelling} {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (tol * scale):.3f})")
        assert np.isfinite(got).all() and err <= tol * scale, (prec, err, scale)
        # every hard-swish block fused on a family-3 entry (the f32 MFMA leaves a block whose best entry pads past 2.5 x its own steps
        # to the layer kernels: kernels_mbconv.hip mb_plan); the ReLU blocks of mobilenetv3_audio layer by layer, as before
        fb = clf.fused_blocks()
        assert fb and all(3 * n_base <= c < 4 * n_base for c in fb), (prec, fb)
        assert all(f",{HSWISH}," in clf.fused_kernel_name(c) for c in fb), [clf.fused_kernel_name(c) for c in fb]
        if prec != "f32":
            assert len(fb) == len(hard_swish_blocks(m)), (prec, len(fb), len(hard_swish_blocks(m)))
        if prec != "f32":
            terms = 1 if prec == "f16" else 3
            ran = [k for k in (clf.layer_kernel(i) for i in hs_gemm if m.layers[i].cin % 32 == 0) if k]
            assert (ran or which != "large") and all(f"<{terms},HSWISH" in k or f"T={terms},HSWISH" in k for k in ran), (prec, ran)
        ctx.close()
        if spelling == "op" and prec in ("auto", "f32"):          # the same bits in a launch of 3 and of 67 segments
            ctx = clf.create_batch_context(67)
            ctx.set_sub_slices(1)
            big = clf.predict_logits(ctx, np.ascontiguousarray(segs[np.arange(67) % 3]))
            assert (big.view(np.uint32) == got.view(np.uint32)[np.arange(67) % 3]).all(), (which, prec)
            ctx.close()
        clf.close()


@pytest.mark.parametrize("which", [1, "large"])
def test_a_float16_file_takes_two_term_planes_on_its_hard_swish_layers(which, tmp_path):
    from birda_amd.classifier import BirdClassifier
    m, segs, _ = _model(which)
    g16 = convert.graph_to_float16(convert.graph_from_model(m, frontend_spelling="conv1d", spell_hswish="hsigmoid"))
    p16, bhm = _write(str(tmp_path / "m16.onnx"), ox.dump(g16)), str(tmp_path / "m16.bhm")
    L = _lib.load()
    assert L.bh_onnx_to_bhm(p16.encode(), bhm.encode()) == 0, L.bh_last_error()
    conv = mf.read_model(bhm)
    assert [(a.op, a.act) for a in conv.layers] == [(a.op, a.act) for a in m.layers]
    ref = forward64h(conv, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    clf = BirdClassifier(p16, None, precision="auto")
    ws = clf.weight_summary()
    assert ws["float16_file"] == 1 and ws["two_term_layers"] > 0, ws
    ctx = clf.create_batch_context(3)
    got = clf.predict_logits(ctx, segs)
    err = float(np.abs(got - ref).max())
    print(f"mnv3 {which} float16 file auto: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    ran = [k for k in (clf.layer_kernel(i) for i, a in enumerate(conv.layers) if a.act == HSWISH and a.op in (mf.OP_PWCONV, mf.OP_DENSE) and a.cin % 32 == 0) if k]
    assert (ran or which != "large") and all("<2,HSWISH" in k or "T=2,HSWISH" in k for k in ran), ran
    ctx.close(); clf.close()


def test_f16_overflow_in_front_of_a_hard_swish_layer_is_not_laundered(tmp_path):
    """tests/test_resact_gpu.py overflow_model's recipe with hard swish on the flagged layer: the linear convolution times 2^20 (its
    output leaves the f16 range), the next one divided by 2^20 -- the same function in f32.  f16x3 ends in BH_ERR_NONFINITE; auto
    re-runs the rows on the f32 kernels and gives the float64 logits."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    from test_resact_gpu import overflow_model
    m0 = overflow_model()
    m0.layers[2].act = HSWISH
    m = copy.deepcopy(m0)
    blob = m.blob.copy()
    Lin, Fl = m.layers[1], m.layers[2]
    s = np.float32(2.0 ** 20)
    blob[Lin.w_off:Lin.w_off + Lin.kh * Lin.kw * Lin.cin * Lin.cout] *= s
    blob[Lin.b_off:Lin.b_off + Lin.cout] *= s
    blob[Fl.w_off:Fl.w_off + Fl.kh * Fl.kw * Fl.cin * Fl.cout] /= s
    m.blob = blob
    path = str(tmp_path / "overflow.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(4, m.sample_count, m.sample_rate, start=8)
    ref = forward64h(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    assert np.abs(ref - forward64h(m0, segs)).max() <= 1e-9 * scale
    clf = BirdClassifier(path, None, precision="f16x3")
    ctx = clf.create_batch_context(4)
    with pytest.raises(BirdaHipError) as e:
        clf.predict_batch_with_context(ctx, list(segs))
    assert e.value.code == BH_ERR_NONFINITE
    assert clf.layer_kernel(2) == "conv_gemm16_kernel<3,HSWISH,AFTER>", clf.layer_kernel(2)
    ctx.close(); clf.close()
    out = {}
    for prec in ("auto", "f32"):
        clf = BirdClassifier(path, None, precision=prec)
        ctx = clf.create_batch_context(4)
        out[prec] = clf.predict_logits(ctx, segs)
        if prec == "auto":
            assert clf.fallback_segments() > 0
        ctx.close(); clf.close()
    err = float(np.abs(out["auto"] - ref).max())
    print(f"overflow in front of a hard-swish layer, auto: max|dlogit| = {err:.3e} of {scale:.2f}")
    assert np.isfinite(out["auto"]).all() and err <= LOGIT_RTOL * scale
    assert (out["auto"].view(np.uint32) == out["f32"].view(np.uint32)).all()
