"""The activation AFTER the residual add, act(conv + b + R) -- the end of a ResNet block -- on the device.

Kernels alone, through bh_debug_conv_gemm_after / bh_debug_layer_gemm_after (include/birda_hip_resact_debug.h): every output
element of conv_gemm_kernel, conv_gemm16_kernel, pw_gemm_kernel, pw_gemm16_kernel, pw_gemm16_skinny_kernel and pw_gemm16s_kernel
in that form is held to

    |got - ref| <= 1.2 tau (bound + |R|) + eps_act(s),   s = A W + b + R in float64,  ref = act64(s),  bound = |A| |W| + |b|

with tau and eps_act exactly those of tests/test_layer_gemm_gpu.py (tau = 4e-7 max(1, sqrt(K / 1024)) for f32 and split f16, 1.5e-3
for plain f16; eps_act = 5e-7 max(|s|, 1) for GELU, 1e-6 max(|s|, 1) for swish / sigmoid / tanh-GELU, nothing for ReLU and ReLU6):
that file's inequality with the residual moved inside an activation whose slope is at most 1.2.  Shapes: the smallest that cross
each tile edge (105 and 297 rows in three segments; 20, 72 and 136 columns; 4 and 36 input channels; 3x3 stride 1 / 2 and 1x1
stride 2; K 32 and 96; 7 and 32 rows for the skinny kernel, 48 for the streaming one, and the grids that reach pw_gemm16s at 2, 4
and 8 column tiles a workgroup).  NaN, +inf and -inf in R come out where they went in; launches of 3 / 80 / 300 segments give the
same bits; every AFTER instantiation behind the launchers is reached, by a name of its own.

The product path, on synth.random_resnet_plan models written as `.onnx`: logits against the float64 forward of
tests/test_resact.py, the same bits at 3 / 80 / 300 segments, where each flagged layer ran, no flagged layer inside a fused block,
the MBConv block behind one still fused, each flagged layer's own output against the float64 layer of the device's own input and
residual; the same plans as float16 files (two-term products); an f16 overflow in front of a flagged ReLU layer ends in
BH_ERR_NONFINITE (f16x3) and in the float64 logits (auto); synth's resnet18_audio runs and matches.

Worst measured shares of the tolerance (MI355X; printed by test_every_after_instantiation_was_reached): see DESIGN.md section 3.
"""
import copy
import ctypes as C
import math
import re

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, synth
from oracle import oracle as O
from test_resact import AFTER, flagged, forward64, layer64

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
BH_ERR_NONFINITE = -8
LOGIT_RTOL = 2e-5          # max |dlogit| <= 2e-5 max(1, max |logit|) in the f32-grade modes
F16_LOGIT_RTOL = 3e-3      # plain f16 operands (tests/test_pool_gpu.py, tests/test_full_conv_gpu.py)
PRECISIONS = (("f32", LOGIT_RTOL), ("f16x3", LOGIT_RTOL), ("auto", LOGIT_RTOL), ("f16", F16_LOGIT_RTOL))
ACTS16 = [O.ACT_RELU, O.ACT_RELU6, O.ACT_SWISH, O.ACT_GELU_ERF]            # the AFTER instantiations of the split-f16 epilogues
ACTS32 = ACTS16 + [O.ACT_GELU_TANH, O.ACT_SIGMOID]                         # the f32 kernels' run-time switch: every code but none
AN = {O.ACT_RELU: "RELU", O.ACT_RELU6: "RELU6", O.ACT_SWISH: "SWISH", O.ACT_GELU_ERF: "GELU"}
REACHED = set()
WORST = {}                 # (family, terms) -> worst (err - eps_act) / (1.2 (bound + |R|))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _family(name):
    return name.split("<")[0]


def _conv_after(X, W, b, R, shape, act, terms):
    """shape = (in_h, in_w, out_h, out_w, cin, cout, kh, kw, sh, sw, pad_t, pad_l) -> (C [n out_h out_w][cout], kernel name)"""
    lib = _lib.load()
    n = X.shape[0]
    out = np.empty((n * shape[2] * shape[3], shape[5]), np.float32)
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_conv_gemm_after(0, _p(X), _p(W), _p(b), _p(R), _p(out), n, _p(np.asarray(shape, np.int32)), act, terms, name, 128)
    assert rc == 0, (rc, lib.bh_last_error())
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"
    REACHED.add(name.value.decode())
    return out, name.value.decode()


def _layer_after(A, W, b, R, act, terms):
    lib = _lib.load()
    M, K = A.shape
    N = W.shape[1]
    out = np.empty((M, N), np.float32)
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_layer_gemm_after(0, _p(A), _p(W), _p(b), _p(R), _p(out), M, K, N, 0, act, terms, name, 128)
    assert rc == 0, (rc, lib.bh_last_error())
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"
    REACHED.add(name.value.decode())
    return out, name.value.decode()


def _tau(terms, k_eff):
    return 1.5e-3 if terms == 1 else 4e-7 * max(1.0, math.sqrt(k_eff / 1024.0))


def _eps_act(s, act):
    if act == O.ACT_GELU_ERF:
        return 5e-7 * np.maximum(np.abs(s), 1.0)
    if act in (O.ACT_SWISH, O.ACT_SIGMOID, O.ACT_GELU_TANH):
        return 1e-6 * np.maximum(np.abs(s), 1.0)
    return np.zeros_like(s)


def _act64(s, act):
    """oracle.act64; the erf of a large array through torch's float64 erf (the oracle's goes through math.erf element by element)"""
    if act == O.ACT_GELU_ERF and s.size > (1 << 18):
        import torch
        return 0.5 * s * (1.0 + torch.erf(torch.from_numpy(s / math.sqrt(2.0))).numpy())
    return O.act64(s, act)


def _check(got, name, pre, bound, R, act, terms, k_eff, what):
    """Element by element: |got - act64(pre + R)| <= 1.2 tau (bound + |R|) + eps_act(pre + R)."""
    r = R.astype(np.float64)
    s = pre + r
    ref = _act64(s, act)
    assert np.isfinite(got).all(), (what, name, "non-finite output")
    scale = 1.2 * (bound + np.abs(r))
    err = np.abs(got.astype(np.float64) - ref)
    eps = _eps_act(s, act)
    tol = _tau(terms, k_eff) * scale + eps
    share = float(np.max(np.maximum(err - eps, 0.0) / np.maximum(scale, 1e-300)))
    key = (_family(name), terms)
    WORST[key] = max(WORST.get(key, 0.0), share)
    bad = err > tol
    if bad.any():
        i = np.unravel_index(np.argmax(err / tol), err.shape)
        pytest.fail(f"{what} {name} act {O.ACT_NAMES[act]}: {int(bad.sum())} of {bad.size} elements off, worst at {i}: got "
                    f"{got[i]!r} want {ref[i]!r} (sum {s[i]!r}), err {err[i]:.3e} > tol {tol[i]:.3e}")


def _f16_valued(W):
    return W.astype(np.float16).astype(np.float32)


def _operands(rng, a_shape, k_rows, N, M):
    """Channels of different scale (0.2-3x), He-scaled W (and its f16-valued twin, for two-term products), a bias of order 1 with
    two columns that sit above 6 / below 0, a residual of order 1."""
    A = (rng.standard_normal(a_shape) * rng.uniform(0.2, 3.0, a_shape[-1])).astype(np.float32)
    W = (rng.standard_normal((k_rows, N)) * math.sqrt(2.0 / k_rows)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    b[:2] = (7.5, -7.5)
    R = rng.standard_normal((M, N)).astype(np.float32)
    return A, W, b, R


# ---------------------------------------------------------------------------------------------------------------------------
# full convolutions
# ---------------------------------------------------------------------------------------------------------------------------
def _same(n_out, k, s):
    """an input size whose SAME_UPPER output is n_out, and the top / left pad"""
    n_in = n_out * s - (s - 1)          # odd at stride 2: 9 -> 5, 13 -> 7, 17 -> 9, 21 -> 11
    return n_in, max((n_out - 1) * s + k - n_in, 0) // 2


GEOMS = {"3x3s1": (3, 1), "3x3s2": (3, 2), "1x1s2": (1, 2)}
CONV_CASES = {}
for (oh, ow) in ((5, 7), (9, 11)):                  # 3 segments: 105 and 297 rows, neither a multiple of 16 or 128
    for gname, (k, s) in GEOMS.items():
        for cin in (4, 36):                         # a partial 32-deep step; one step + 4
            for cout in (20, 72, 136):              # a partial 16-column tile, a partial 8-tile block, past the 128-column block
                (ih, pt), (iw, pl) = _same(oh, k, s), _same(ow, k, s)
                CONV_CASES[f"{oh}x{ow}_{gname}_{cin}to{cout}"] = (ih, iw, oh, ow, cin, cout, k, k, s, s, pt, pl)
_CONV_REF = {}


def _conv_reference(name, f16w):
    """computed once per shape and weight kind, shared, never modified"""
    key = (name, f16w)
    if key not in _CONV_REF:
        ih, iw, oh, ow, cin, cout, kh, kw, sh, sw, pt, pl = CONV_CASES[name]
        rng = np.random.default_rng(sum(CONV_CASES[name]) * 11 + len(name))
        X, W, b, R = _operands(rng, (3, ih, iw, cin), kh * kw * cin, cout, 3 * oh * ow)
        if f16w:
            W = _f16_valued(W)
        W = W.reshape(kh, kw, cin, cout)
        pre, A = O.conv_nhwc64(X, W.astype(np.float64), b, sh, sw, pt, pl, oh, ow)
        bound = np.abs(A) @ np.abs(W.reshape(-1, cout).astype(np.float64)) + np.abs(b.astype(np.float64))
        for a in (X, W, b, R, pre, bound):
            a.setflags(write=False)
        _CONV_REF[key] = (X, W, b, R, pre, bound)
    return _CONV_REF[key]


def _conv_params():
    out = []
    for i, name in enumerate(sorted(CONV_CASES)):
        for terms in (0, 1, 2, 3):
            acts = ACTS32 if terms == 0 else ACTS16
            act = acts[(i + terms) % len(acts)]
            out.append(pytest.param(name, terms, act, id=f"{name}-t{terms}-{O.ACT_NAMES[act]}"))
    every = "9x11_3x3s1_36to136"                    # ... and every activation of every terms on one shape
    for terms in (0, 1, 2, 3):
        for act in (ACTS32 if terms == 0 else ACTS16):
            out.append(pytest.param(every, terms, act, id=f"every-{every}-t{terms}-{O.ACT_NAMES[act]}"))
    return out


@pytest.mark.parametrize("name,terms,act", _conv_params())
def test_conv_after_matches_float64(name, terms, act):
    shape = CONV_CASES[name]
    X, W, b, R, pre, bound = _conv_reference(name, terms == 2)
    got, kname = _conv_after(X, W, b, R, shape, act, terms)
    want = f"conv_gemm16_kernel<{terms},{AN[act]},AFTER>" if terms else None
    assert (kname == want) if terms else kname.startswith("conv_gemm_kernel<BM="), kname
    s = pre + R
    assert (s < 0).any() and (s > 6).any(), "the sums should make ReLU and ReLU6 clamp on both sides"
    _check(got, kname, pre, bound, R, act, terms, shape[6] * shape[7] * shape[4], name)


# ---------------------------------------------------------------------------------------------------------------------------
# pointwise / dense GEMMs
# ---------------------------------------------------------------------------------------------------------------------------
# (M, K, N): 7 and 32 rows: the skinny kernel (one and two row tiles); 48: the streaming kernel; 105 and 297: pw_gemm16s at two
# column tiles a workgroup; 3000 x 1024 and 6151 x 1024: the grids that take it to four and eight
PW_SMALL = [(M, K, N) for M in (7, 32, 48, 105, 297) for K in (32, 96) for N in (20, 72, 136)]
PW_BIG = [(3000, 32, 1024), (6151, 32, 1024)]
_PW_REF = {}


def _pw_reference(mkn, f16w):
    key = (mkn, f16w)
    if key not in _PW_REF:
        M, K, N = mkn
        rng = np.random.default_rng(M * 7 + K * 131 + N)
        A, W, b, R = _operands(rng, (M, K), K, N, M)
        if f16w:
            W = _f16_valued(W)
        pre = O.gemm64(A, W, b)
        bound = np.abs(A.astype(np.float64)) @ np.abs(W.astype(np.float64)) + np.abs(b.astype(np.float64))
        for a in (A, W, b, R, pre, bound):
            a.setflags(write=False)
        if M > 1000:
            _PW_REF.clear()          # (the big references are 50 MB each: one at a time)
        _PW_REF[key] = (A, W, b, R, pre, bound)
    return _PW_REF[key]


def _pw_family(M, terms):
    return "pw_gemm_kernel" if terms == 0 else "pw_gemm16_skinny_kernel" if M <= 32 else "pw_gemm16_kernel" if M < 64 else "pw_gemm16s_kernel"


def _pw_params():
    out = []
    for i, mkn in enumerate(PW_SMALL):
        for terms in (0, 1, 2, 3):
            acts = ACTS32 if terms == 0 else ACTS16
            act = acts[(i // 3 + i + terms) % len(acts)]
            out.append(pytest.param(mkn, terms, act, id="M%d_K%d_N%d" % mkn + f"-t{terms}-{O.ACT_NAMES[act]}"))
    # every activation of every terms in every split-f16 kernel family (K 96, 136 columns), and in the two big grids
    for mkn in [(7, 96, 136), (48, 96, 136), (105, 96, 136)] + PW_BIG:
        for f16w in (False, True):          # (ordered so that a big shape's reference is computed once per weight kind)
            for terms in ((2,) if f16w else (1, 3)):
                for act in ACTS16:
                    out.append(pytest.param(mkn, terms, act, id="every-M%d_K%d_N%d" % mkn + f"-t{terms}-{O.ACT_NAMES[act]}"))
    for act in ACTS32:
        out.append(pytest.param((105, 96, 136), 0, act, id=f"every-M105_K96_N136-t0-{O.ACT_NAMES[act]}"))
    return out


@pytest.mark.parametrize("mkn,terms,act", _pw_params())
def test_layer_gemm_after_matches_float64(mkn, terms, act):
    M, K, N = mkn
    A, W, b, R, pre, bound = _pw_reference(mkn, terms == 2)
    got, kname = _layer_after(A, W, b, R, act, terms)
    assert _family(kname) == _pw_family(M, terms), kname
    if terms:
        assert f"<{terms},{AN[act]},AFTER" in kname, kname
    if mkn in PW_BIG:
        assert kname.endswith("NTB=4>" if M == 3000 else "NTB=8>"), kname
    _check(got, kname, pre, bound, R, act, terms, K, "pw")


# ---------------------------------------------------------------------------------------------------------------------------
# non-finite sums come out where they went in
# ---------------------------------------------------------------------------------------------------------------------------
def _nonfinite_cases():
    out = []
    for fam in ("conv", "pw7", "pw48", "pw105"):
        for terms in (0, 1, 2, 3):
            for act in (ACTS32 if terms == 0 else ACTS16):
                out.append(pytest.param(fam, terms, act, id=f"{fam}-t{terms}-{O.ACT_NAMES[act]}"))
    return out


@pytest.mark.parametrize("fam,terms,act", _nonfinite_cases())
def test_nan_and_inf_in_the_residual_survive_the_epilogue(fam, terms, act):
    """NaN, +inf and -inf at chosen elements of R (first and last row, a partial tile's last column, the middle): the output is NaN
    exactly at the NaN elements, for every activation and every terms; +inf gives +inf and -inf gives 0 under ReLU (v_med3_f32 and
    fmaxf would have answered 0 for the NaN: BH_FLAG_AUTO and BH_ERR_NONFINITE rely on it reaching the logits)."""
    if fam == "conv":
        name = "5x7_3x3s2_36to136"
        X, W, b, R0, pre, bound = _conv_reference(name, terms == 2)
    else:
        mkn = (int(fam[2:]), 96, 136)
        X, W, b, R0, pre, bound = _pw_reference(mkn, terms == 2)
    R = R0.copy()
    M, N = R.shape
    nan_at = [(0, 0), (M - 1, N - 1), (M // 2, 17), (M - 1, 0), (3, 128)]
    pinf_at = [(0, 1), (M - 1, N - 2), (M // 2, 16), (2, 129)]
    ninf_at = [(0, 2), (M - 1, N - 3), (M // 2, 18), (1, 130)]
    for (i, j) in nan_at:
        R[i, j] = np.nan
    for (i, j) in pinf_at:
        R[i, j] = np.inf
    for (i, j) in ninf_at:
        R[i, j] = -np.inf
    got, kname = (_conv_after(X, W, b, R, CONV_CASES[name], act, terms) if fam == "conv" else _layer_after(X, W, b, R, act, terms))
    want_nan = np.zeros(R.shape, bool)
    want_nan[tuple(zip(*nan_at))] = True
    assert (np.isnan(got) == want_nan).all(), (kname, O.ACT_NAMES[act], np.argwhere(np.isnan(got) != want_nan)[:6].tolist())
    if act == O.ACT_RELU:
        assert all(got[i, j] == np.inf for (i, j) in pinf_at) and all(got[i, j] == 0.0 for (i, j) in ninf_at), kname
    # ... and every other element is what it is without them
    clean, _ = (_conv_after(X, W, b, R0, CONV_CASES[name], act, terms) if fam == "conv" else _layer_after(X, W, b, R0, act, terms))
    finite = np.isfinite(R)
    assert (got[finite].view(np.uint32) == clean[finite].view(np.uint32)).all(), kname


# ---------------------------------------------------------------------------------------------------------------------------
# launch invariance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", (0, 1, 2, 3))
def test_conv_after_bits_do_not_depend_on_the_launch(terms):
    """the same three segments repeated to 80 and to 300 (the f32 kernel's 128-row tile at 300): the same bits per segment"""
    name = "9x11_3x3s1_36to136"
    shape = CONV_CASES[name]
    X, W, b, R, pre, bound = _conv_reference(name, terms == 2)
    rows = shape[2] * shape[3]
    act = O.ACT_RELU if terms in (0, 3) else O.ACT_GELU_ERF
    small, ks = _conv_after(X, W, b, R, shape, act, terms)
    _check(small, ks, pre, bound, R, act, terms, 9 * 36, "launch")
    names = {ks}
    for n in (80, 300):
        idx = np.arange(n) % 3
        big, kb = _conv_after(np.ascontiguousarray(X[idx]), W, b, np.ascontiguousarray(R.reshape(3, rows, -1)[idx].reshape(n * rows, -1)), shape, act, terms)
        names.add(kb)
        assert (big.reshape(n, rows, -1).view(np.uint32) == small.reshape(3, rows, -1).view(np.uint32)[idx]).all(), (terms, n, kb)
    if terms == 0:
        assert any(k.startswith("conv_gemm_kernel<BM=128") for k in names) and any(k.startswith("conv_gemm_kernel<BM=64") for k in names), names


@pytest.mark.parametrize("terms", (0, 1, 2, 3))
def test_layer_gemm_after_bits_do_not_depend_on_the_launch(terms):
    """three segments of 35 rows (105) repeated to 80 (2 800 rows) and 300 (10 500): the same bits per segment"""
    mkn = (105, 96, 136)
    A, W, b, R, pre, bound = _pw_reference(mkn, terms == 2)
    act = O.ACT_RELU if terms in (0, 3) else O.ACT_SWISH
    small, ks = _layer_after(A, W, b, R, act, terms)
    for n in (80, 300):
        idx = np.arange(n) % 3
        tile = lambda a: np.ascontiguousarray(a.reshape(3, 35, -1)[idx].reshape(n * 35, -1))
        big, kb = _layer_after(tile(A), W, b, tile(R), act, terms)
        assert (big.reshape(n, 35, -1).view(np.uint32) == small.reshape(3, 35, -1).view(np.uint32)[idx]).all(), (terms, n, kb)


def test_pw32_after_at_the_128_row_tile():
    """pw_gemm_kernel<BM=128> (a grid of >= 512 blocks of 128 rows) takes the run-time position too: the first 256 rows against a
    launch of 256 (BM = 64), which is held to float64"""
    rng = np.random.default_rng(10)
    M, K, N = 8200, 32, 1024
    A, W, b, R = _operands(rng, (M, K), K, N, M)
    big, kb = _layer_after(A, W, b, R, O.ACT_RELU, 0)
    small, ks = _layer_after(A[:256].copy(), W, b, R[:256].copy(), O.ACT_RELU, 0)
    assert kb.startswith("pw_gemm_kernel<BM=128") and ks.startswith("pw_gemm_kernel<BM=64"), (kb, ks)
    assert np.array_equal(big[:256], small)
    pre = O.gemm64(A[:256], W, b)
    bound = np.abs(A[:256].astype(np.float64)) @ np.abs(W.astype(np.float64)) + np.abs(b.astype(np.float64))
    _check(small, ks, pre, bound, R[:256], O.ACT_RELU, 0, K, "pw32 bm64 / bm128")
    assert (big[256:] >= 0).all() and np.isfinite(big).all()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals of the debug entries
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_after_entries_refuse_what_has_no_instantiation():
    lib = _lib.load()
    z = np.zeros(1 << 16, np.float32)
    out = np.empty(1 << 16, np.float32)
    ok = np.asarray((6, 6, 6, 6, 8, 8, 3, 3, 1, 1, 1, 1), np.int32)
    conv = lambda act, terms, R=z: lib.bh_debug_conv_gemm_after(0, _p(z), _p(z), _p(z), _p(R), _p(out), 1, _p(ok), act, terms, None, 0)
    layer = lambda act, terms, R=z, P=0: lib.bh_debug_layer_gemm_after(0, _p(z), _p(z), _p(z), _p(R), _p(out), 16, 32, 8, P, act, terms, None, 0)
    for f in (conv, layer):
        assert f(O.ACT_RELU, 3) == 0 and f(O.ACT_RELU, 0) == 0 and f(O.ACT_SIGMOID, 0) == 0
        assert f(O.ACT_RELU, 3, None) != 0 and f(O.ACT_RELU, 0, None) != 0          # R is required
        for terms in (0, 1, 2, 3):
            assert f(O.ACT_NONE, terms) != 0                                         # ACT_NONE never takes the form
        for terms in (1, 2, 3):
            assert f(O.ACT_GELU_TANH, terms) != 0 and f(O.ACT_SIGMOID, terms) != 0
    assert layer(O.ACT_RELU, 3, z, 16) != 0                                          # no head pool


# ---------------------------------------------------------------------------------------------------------------------------
# the product path
# ---------------------------------------------------------------------------------------------------------------------------
def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def _check_layer_kernels(clf, m, prec, what, two_terms=False):
    """a flagged layer above 64 output channels ran an AFTER split-f16 instantiation in the f16 modes; at 64 or below, and in f32,
    the f32 kernel (layer_kernel names split-f16 launches only).  A 1x1 layer takes the split-f16 GEMMs at K % 32 == 0 only
    (pw_gemm16_after_supports: the rule of every pointwise layer; a ResNet-D shortcut from a 24- or 40-channel tensor stays f32)."""
    ran = set()
    for i in flagged(m):
        L, k = m.layers[i], clf.layer_kernel(i)
        if prec == "f32" or L.cout <= 64 or (L.op != mf.OP_CONV and L.cin % 32):
            assert k == "", (what, prec, i, k)
            continue
        fam = "conv_gemm16_kernel" if L.op == mf.OP_CONV else "pw_gemm16"
        terms = 1 if prec == "f16" else 2 if two_terms else 3
        assert k.startswith(fam) and f"<{terms},{AN[L.act]},AFTER" in k, (what, prec, i, k)
        ran.add(fam)
    return ran


@pytest.mark.parametrize("seed", range(6))
def test_random_resnet_plans_on_the_onnx_route(seed, tmp_path, monkeypatch):
    from birda_amd.classifier import BirdClassifier
    from test_arena_plan_gpu import PATH_FUSED, PATH_INNER, arena_plan
    plan = synth.random_resnet_plan(seed)
    m = synth.build_model("resnet_plan", plan=plan)
    onnx = _write(str(tmp_path / "r.onnx"), convert.model_to_onnx(m, frontend_spelling="stft"))
    fl = flagged(m)
    assert any(m.layers[i].cout <= 64 for i in fl) and any(m.layers[i].cout > 64 for i in fl)
    dws = [i for i, L in enumerate(m.layers) if L.op == mf.OP_DWCONV]
    assert len(dws) == 1 and m.layers[dws[0] - 1].in_tensor - 1 in fl          # the MBConv block reads a flagged layer's output
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=5 + seed)
    segs[2] *= np.float32(0.01)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    for prec, tol in PRECISIONS:
        clf = BirdClassifier(onnx, None, precision=prec)
        first = None
        for n in (3, 80, 300):
            ctx = clf.create_batch_context(n)
            ctx.set_sub_slices(1)
            got = clf.predict_logits(ctx, np.ascontiguousarray(segs[np.arange(n) % 3]))
            if first is None:
                first = got
                err = float(np.abs(got - ref).max())
                print(f"resnet plan {seed} {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (tol * scale):.3f})  {plan['stem']} {plan['items']}")
                assert np.isfinite(got).all() and err <= tol * scale, (prec, err, scale)
                ran = _check_layer_kernels(clf, m, prec, seed)
                # every plan holds a flagged 3x3 or 1x1 stride-2 convolution AND a flagged 1x1 layer (K = 32) above 64 channels
                assert ran == (set() if prec == "f32" else {"conv_gemm16_kernel", "pw_gemm16"}), (prec, ran)
                tags = arena_plan(clf, ctx, 0)[2]
                assert all(tags[i] not in (PATH_FUSED, PATH_INNER) for i in fl), (prec, tags, fl)      # no flagged layer inside a block
                if prec != "f32":      # (the f32 tile entries do not cover every block shape: tests/test_full_conv_gpu.py)
                    assert all(tags[d] in (PATH_FUSED, PATH_INNER) for d in dws), (prec, tags, dws)    # the MBConv block behind one is fused
            else:
                assert (got.view(np.uint32) == first.view(np.uint32)[np.arange(n) % 3]).all(), (prec, n)
            ctx.close()
        clf.close()
    # each flagged layer's own output against the float64 layer of the device's own input and residual, layer by layer in f32
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    clf = BirdClassifier(onnx, None, precision="f32")
    ctx = clf.create_batch_context(3)
    clf.predict_logits(ctx, segs)
    for i in fl:
        L = m.layers[i]
        X, R, Y = clf.read_tensor(ctx, L.in_tensor, 3), clf.read_tensor(ctx, L.res_tensor, 3), clf.read_tensor(ctx, i + 1, 3)
        assert np.isfinite(X).all() and np.isfinite(R).all()
        Wm = np.asarray(m.blob[L.w_off:L.w_off + L.kh * L.kw * L.cin * L.cout], np.float64)
        bias = np.asarray(m.blob[L.b_off:L.b_off + L.cout], np.float64)
        if L.op == mf.OP_CONV:
            pre, A = O.conv_nhwc64(X.reshape(3, L.in_h, L.in_w, L.cin), Wm.reshape(L.kh, L.kw, L.cin, L.cout), bias, L.sh, L.sw, L.pad_t, L.pad_l, L.out_h, L.out_w)
        else:
            A = X.reshape(-1, L.cin).astype(np.float64)
            pre = O.gemm64(A, Wm.reshape(L.cin, L.cout), bias)
        bound = np.abs(A) @ np.abs(Wm.reshape(-1, L.cout)) + np.abs(bias)
        Rr = R.reshape(-1, L.cout)
        _check(Y.reshape(-1, L.cout), "layer" + ("_conv" if L.op == mf.OP_CONV else "_pw") + "<f32,in a model>", pre, bound, Rr, L.act, 0, L.kh * L.kw * L.cin, (seed, i))
        ref_layer = layer64(m, L, X.astype(np.float64), R.astype(np.float64)).reshape(-1, L.cout)
        assert np.abs(ref_layer - O.act64(pre + Rr, L.act)).max() <= 1e-12 * max(1.0, np.abs(ref_layer).max())
    ctx.close(); clf.close()


@pytest.mark.parametrize("seed", range(6))
def test_random_resnet_plan_as_a_float16_file(seed, tmp_path):
    """graph_to_float16 of the same graph: the logits stay at LOGIT_RTOL of the float64 forward of the container the library's own
    reader makes of it (its weights are the file's float16 values), and the flagged layers run two-term products"""
    from birda_amd import onnx_io as ox
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("resnet_plan", plan=synth.random_resnet_plan(seed))
    g16 = convert.graph_to_float16(convert.graph_from_model(m, frontend_spelling="conv1d"))
    p16, bhm = _write(str(tmp_path / "r16.onnx"), ox.dump(g16)), str(tmp_path / "r16.bhm")
    L = _lib.load()
    assert L.bh_onnx_to_bhm(p16.encode(), bhm.encode()) == 0, L.bh_last_error()
    conv = mf.read_model(bhm)
    assert flagged(conv) == flagged(m) and [(a.op, a.act) for a in conv.layers] == [(a.op, a.act) for a in m.layers]
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=31)
    ref = forward64(conv, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    for prec, tol in PRECISIONS:
        clf = BirdClassifier(p16, None, precision=prec)
        assert clf.weight_summary()["float16_file"] == 1
        ctx = clf.create_batch_context(3)
        got = clf.predict_logits(ctx, segs)
        err = float(np.abs(got - ref).max())
        print(f"resnet plan {seed} float16 file {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (tol * scale):.3f})")
        assert np.isfinite(got).all() and err <= tol * scale, (prec, err, scale)
        ran = _check_layer_kernels(clf, conv, prec, ("f16 file", seed), two_terms=True)
        assert ran == (set() if prec == "f32" else {"conv_gemm16_kernel", "pw_gemm16"}), (prec, ran)
        ctx.close(); clf.close()


def overflow_model():
    """The mini front-end, a 3x3 stride-2 stem to 72 channels (t1), a LINEAR 3x3 convolution 72 -> 72 (t2), a flagged ReLU 3x3
    convolution 72 -> 72 with t1 as its residual -- relu(conv(t2) + t1) --, a 1x1 head, the global pool and a dense layer"""
    b = synth._Builder(np.random.default_rng(13))
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    t1, h, w = b.conv(0, br.n_mels, br.n_frames, 1, 72, 3, 2, mf.ACT_GELU_ERF, in_layout=1)
    t2, h, w = b.conv(t1, h, w, 72, 72, 3, 1, mf.ACT_NONE)
    t3, h, w = b.conv(t2, h, w, 72, 72, 3, 1, mf.ACT_RELU, res=t1, gain=0.5)
    b.layers[-1].reserved = AFTER
    t = b.pwconv(t3, h, w, 72, 64, mf.ACT_GELU_ERF)
    t = emb = b.gap(t, h, w, 64)
    b.dense(t, 64, 30, gain=1.5)
    return mf.Model(0, sr, n, n / sr, 30, 64, mf.OUT_SIGMOID, emb, br.n_mels, br.n_frames, 1e-6, [br], b.layers, np.concatenate(b.chunks))


def test_f16_overflow_in_front_of_a_flagged_relu_is_not_laundered(tmp_path):
    """The linear convolution's weights and bias times 2^20 (its output, ~1e6, is past 65 504) and the flagged convolution's weights
    divided by 2^20: the same function in f32 arithmetic.  The split-f16 kernel cannot represent its operand; the NaN / inf it
    computes must pass relu(. + R) -- f16x3 ends in BH_ERR_NONFINITE --, and auto re-runs the rows on the f32 kernels."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    m0 = overflow_model()
    m = copy.deepcopy(m0)
    blob = m.blob.copy()
    Lin, Fl = m.layers[1], m.layers[2]
    assert Lin.act == mf.ACT_NONE and flagged(m) == [2] and Fl.cout > 64 and Fl.act == mf.ACT_RELU
    s = np.float32(2.0 ** 20)
    blob[Lin.w_off:Lin.w_off + Lin.kh * Lin.kw * Lin.cin * Lin.cout] *= s
    blob[Lin.b_off:Lin.b_off + Lin.cout] *= s
    blob[Fl.w_off:Fl.w_off + Fl.kh * Fl.kw * Fl.cin * Fl.cout] /= s
    m.blob = blob
    path = str(tmp_path / "overflow.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(4, m.sample_count, m.sample_rate, start=8)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    assert np.abs(ref - forward64(m0, segs)).max() <= 1e-9 * scale
    clf = BirdClassifier(path, None, precision="f16x3")
    ctx = clf.create_batch_context(4)
    with pytest.raises(BirdaHipError) as e:
        clf.predict_batch_with_context(ctx, list(segs))
    assert e.value.code == BH_ERR_NONFINITE
    assert clf.layer_kernel(2) == "conv_gemm16_kernel<3,RELU,AFTER>", clf.layer_kernel(2)
    ctx.close(); clf.close()
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(4)
    got = clf.predict_logits(ctx, segs)
    assert clf.fallback_segments() > 0
    err = float(np.abs(got - ref).max())
    print(f"overflow in front of a flagged ReLU layer, auto: max|dlogit| = {err:.3e} of {scale:.2f}, {clf.fallback_segments()} segments re-run")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    ctx.close(); clf.close()


def test_resnet18_audio_runs_and_matches_float64(tmp_path):
    """synth's timing model, two segments in auto: finite logits at LOGIT_RTOL of the float64 forward (the numpy reference is this
    test's time; the device part is milliseconds), and the same bits at 2 and at 64 segments"""
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("resnet18_audio", n_classes=40)
    fl = flagged(m)
    assert len(fl) == 8 and [m.layers[i].cout for i in fl] == [64, 64, 128, 128, 256, 256, 512, 512]
    assert sum(m.layers[i].kh == 1 and m.layers[i].sh == 2 for i in fl) == 3          # the three projection shortcuts
    path = str(tmp_path / "resnet18.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=2)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(2)
    got = clf.predict_logits(ctx, segs)
    ctx.close()
    err = float(np.abs(got - ref).max())
    print(f"resnet18_audio auto: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    _check_layer_kernels(clf, m, "auto", "resnet18_audio")
    ctx = clf.create_batch_context(64)
    ctx.set_sub_slices(1)
    big = clf.predict_logits(ctx, np.ascontiguousarray(segs[np.arange(64) % 2]))
    ctx.close(); clf.close()
    assert (big.view(np.uint32) == got.view(np.uint32)[np.arange(64) % 2]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# every AFTER instantiation behind the launchers was reached (keep last: it reads what the tests above ran)
# ---------------------------------------------------------------------------------------------------------------------------
def _reach(name):
    """one launch of the shape that dispatches to `name`, on zero operands (zeros are f16 values: two terms take them)"""
    fam, args = name.split("<")[0], name.split("<")[1].rstrip(">").split(",")
    terms = int(args[0]) if args[0].isdigit() else 0
    act = {v: k for k, v in AN.items()}.get(args[1], O.ACT_RELU)
    if fam.startswith("conv"):
        n = 300 if "BM=128" in name else 3
        shape = CONV_CASES["9x11_3x3s1_36to136"]
        _conv_after(np.zeros((n, shape[0], shape[1], 36), np.float32), np.zeros((3, 3, 36, 136), np.float32), np.zeros(136, np.float32),
                    np.zeros((n * 99, 136), np.float32), shape, act, terms)
        return
    M, N = {"pw_gemm16_skinny_kernel": (7, 20), "pw_gemm16_kernel": (48, 20)}.get(fam, (None, None))
    if fam == "pw_gemm16s_kernel":
        M, N = {"NTB=2>": (105, 20), "NTB=4>": (3000, 1024), "NTB=8>": (6151, 1024)}[name[-6:]]
    if fam == "pw_gemm_kernel":
        M, N = (8200, 1024) if "BM=128" in name else (105, 20)
    _layer_after(np.zeros((M, 32), np.float32), np.zeros((32, N), np.float32), np.zeros(N, np.float32), np.zeros((M, N), np.float32), act, terms)


def test_every_after_instantiation_was_reached():
    """Run with the module, it reads what the tests above launched (and prints their worst shares); alone, under -k or on a
    distributing runner it launches what is missing itself, so the dispatch is held either way."""
    want = [f"conv_gemm16_kernel<{t},{a},AFTER>" for t in (1, 2, 3) for a in AN.values()]
    want += [f"pw_gemm16_skinny_kernel<{t},{a},AFTER>" for t in (1, 2, 3) for a in AN.values()]
    want += [f"pw_gemm16_kernel<{t},{a},AFTER>" for t in (1, 2, 3) for a in AN.values()]
    want += [f"pw_gemm16s_kernel<{t},{a},AFTER,NTB={b}>" for t in (1, 2, 3) for a in AN.values() for b in (2, 4, 8)]
    assert len(want) == len(set(want)) == 72
    for w in want:
        if w not in REACHED:
            _reach(w)
    missing = [w for w in want if w not in REACHED]
    assert not missing, (missing, sorted(REACHED))
    # the f32 kernels take the position at run time: no instantiation of their own, both row tiles reached
    for fam in ("conv_gemm_kernel", "pw_gemm_kernel"):
        for bm in ("<BM=64", "<BM=128"):
            if not any(n.startswith(fam + bm) for n in REACHED):
                _reach(fam + bm + ",NT=0>")
            assert any(n.startswith(fam + bm) for n in REACHED), (fam, bm, sorted(REACHED))
    # every new name is distinct from the names the launchers had: those end in an activation, or in NTB=, without ",AFTER"
    old = re.compile(r"(conv_gemm16_kernel|pw_gemm16_skinny_kernel|pw_gemm16_kernel)<[123],(NONE|GELU|SWISH|RELU6)>|pw_gemm16s_kernel<[123],(NONE|GELU|SWISH|RELU6),NTB=\d+>")
    assert not [w for w in want if old.fullmatch(w)]
    assert all(",AFTER" in n for n in REACHED if "16" in _family(n)), sorted(REACHED)
    print("\nworst (err - eps_act) / (1.2 (bound + |R|)) by kernel family and terms, and its share of tau:")
    for (fam, terms), v in sorted(WORST.items()):
        print(f"  {fam:28s} terms {terms}: {v:.3e}  ({v / (1.5e-3 if terms == 1 else 4e-7):.3f} of tau at K <= 1024)")
