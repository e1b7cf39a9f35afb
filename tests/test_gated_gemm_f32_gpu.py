"""The f32 gated project GEMM of the squeeze-excite blocks (kernels_conv.hip pw_gemm_kernel<BM, NT, GATE>: what SliceRun::fused_se
runs on a precision="f32" classifier, and what BH_FLAG_AUTO re-runs rows on when the f16 path gives up) alone through
bh_debug_gated_gemm_f32, every one of its sixteen instantiations by name, on the case table of tests/test_gated_gemm.py -- which
holds the reference, the expected names and the inputs on the CPU first (a float32 emulation of the kernel meets the inequality
below on every case; six mutants of its gate-row, K-tail and gate-column arithmetic each miss it).

Every element:   |got - ref| <= tau (1.2 bound + |R|) + eps_act,   bound = |A g| |W| + |b| in float64,
tau = 4e-7 max(1, sqrt(K / 1024)) + 2^-24 (tests/test_layer_gemm_gpu.py's figure for this kernel family and the one extra rounding
of a x g per product); no element keeps the payload 0x7fc0beef the output starts as.

Without a tolerance: the GATE instantiation gives the bits of its ungated twin (bh_debug_layer_gemm, terms 0) on float32(A x g) --
the product is rounded to f32 and stored to LDS before any sum; a gate of ones, the twin's bits on A; gates of 2^-s, the twin's bits
on A scaled row by row (a wrong gate row shows bit for bit); a gate of zeros, act(b) + R; a segment's bits do not depend on the
launch (BM = 128 against BM = 64)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gated_gemm as G  # noqa: E402
import test_layer_gemm_gpu as TL  # noqa: E402
from test_hardswish import HSIGMOID, HSWISH, act64h  # noqa: E402

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
BH_ERR_INVALID, BH_ERR_UNSUPPORTED = -1, -6
REACHED = set()
WORST = {}               # instantiation -> worst share of tau
RAN = set()              # the cases of G.CASES that ran


def _lib():
    from birda_amd import _lib
    return _lib.load()


_p = TL._p


def _gated(A, gate, W, b, R, P, act=O.ACT_NONE):
    lib = _lib()
    M, K = A.shape
    N = W.shape[1]
    out = np.empty((M, N), np.float32)
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_gated_gemm_f32(0, _p(A), _p(gate), _p(W), _p(b), _p(R), _p(out), M, K, N, P, act, name, 128)
    assert rc == 0, (rc, lib.bh_last_error())
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"
    REACHED.add(name.value.decode())
    return out, name.value.decode()


def _twin(A, W, b, R, act=O.ACT_NONE):
    """the ungated kernel on the same shape"""
    return TL._layer(np.ascontiguousarray(A, np.float32), W, b, R, act, 0)


def _same_bits(a, b, what):
    a, b = a.view(np.uint32), b.view(np.uint32)
    if not np.array_equal(a, b):
        i = np.unravel_index(np.argmax(a != b), a.shape)
        pytest.fail(f"{what}: {int((a != b).sum())} of {a.size} elements differ in their bits, first at {i}: "
                    f"{a[i]:#010x} != {b[i]:#010x}; rows {sorted(set(np.nonzero(a != b)[0].tolist()))[:12]}")


# ---------------------------------------------------------------------------------------------------------------------------
# every instantiation by name: float64 every element, and the ungated twin's bits
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_gated_f32_matches_float64_and_its_ungated_twin(case):
    n_seg, P, K, N, _ = case
    A, gate, W, b, R, pre, bound = G.reference(case)
    got, name = _gated(A, gate, W, b, R, P)
    assert name == G.kernel_name(n_seg * P, N), (name, G.kernel_name(n_seg * P, N))
    share = G.check(got, name, pre, bound, R, O.ACT_NONE, K, G.case_id(case))
    WORST[name] = max(WORST.get(name, 0.0), share)
    RAN.add(case)
    print(f"{G.case_id(case)} {name}: worst share of tau {share:.3f}")
    twin, tname = _twin(A * np.repeat(gate, P, axis=0), W, b, R)      # float32 x float32: rounded once, as on the way into LDS
    assert name == tname[:-1] + ",GATE>", (name, tname)
    _same_bits(got, twin, f"{name} against {tname} on float32(A g)")


IDENTITY = [c for c in G.SMALL if c[1] in (7, 50, 1000)] + [G.BIG[1], G.BIG[8]]       # tiles that straddle segments


@pytest.mark.parametrize("case", IDENTITY, ids=G.case_id)
def test_power_of_two_gates_give_the_bits_of_prescaled_rows(case):
    """gate[s][:] = 2^-(s mod 24): A x g is exact, so the result is the ungated kernel's on A scaled row by row -- a row that took
    a neighbouring segment's gate differs by a factor of two (or 2^23), in its bits."""
    n_seg, P, K, N, _ = case
    A, _, W, b, R, _, _ = G.reference(case)
    s = (2.0 ** -(np.arange(n_seg) % 24)).astype(np.float32)
    gate = np.repeat(s[:, None], K, axis=1)
    scaled = A * np.repeat(s, P)[:, None]
    assert np.array_equal(scaled.astype(np.float64), A.astype(np.float64) * np.repeat(s, P)[:, None].astype(np.float64))   # exact
    got, name = _gated(A, gate, W, b, R, P)
    twin, tname = _twin(scaled, W, b, R)
    assert name == tname[:-1] + ",GATE>"
    _same_bits(got, twin, f"{name}, gates of 2^-s")


@pytest.mark.parametrize("case", [G.SMALL[0], G.SMALL[2], G.SMALL[3], G.SMALL[11], G.SMALL[15], G.BIG[5]], ids=G.case_id)
def test_gates_of_ones_and_of_zeros(case):
    n_seg, P, K, N, _ = case
    A, gate, W, b, R, _, _ = G.reference(case)
    got, name = _gated(A, np.ones_like(gate), W, b, R, P)
    twin, tname = _twin(A, W, b, R)
    assert name == tname[:-1] + ",GATE>"
    _same_bits(got, twin, f"{name}, a gate of ones")
    got, name = _gated(A, np.zeros_like(gate), W, b, R, P)
    want = np.broadcast_to(b, got.shape) + (0 if R is None else R)      # float32: b, or the one rounding of b + R
    assert want.dtype == np.float32
    assert np.array_equal(got, want), (name, "a gate of zeros must leave act(b) + R")


@pytest.mark.parametrize("case,few", [(G.BIG[1], 20), (G.BIG[2], 10), (G.BIG[5], 33), (G.BIG[8], 3)], ids=lambda v: G.case_id(v) if isinstance(v, tuple) else str(v))
def test_a_segments_bits_do_not_depend_on_the_launch(case, few):
    """The first `few` segments of a BM = 128 launch as a launch of their own, on BM = 64: the k order of an element is not the
    tile's."""
    n_seg, P, K, N, _ = case
    A, gate, W, b, R, _, _ = G.reference(case)
    big, kb = _gated(A, gate, W, b, R, P)
    rows = few * P
    small, ks = _gated(A[:rows].copy(), gate[:few].copy(), W, b, None if R is None else R[:rows].copy(), P)
    assert "BM=128" in kb and ks == kb.replace("BM=128", "BM=64"), (kb, ks)
    _same_bits(big[:rows], small, f"{kb} against {ks}")


# ---------------------------------------------------------------------------------------------------------------------------
# the epilogue's run-time switch: every activation code, with R, so that act(. + b) + R is pinned
# ---------------------------------------------------------------------------------------------------------------------------
ACT_CASE = (5, 7, 36, 20, True)
ACT_NAMES = {**O.ACT_NAMES, HSWISH: "hswish", HSIGMOID: "hsigmoid"}


@pytest.mark.parametrize("act", sorted(ACT_NAMES), ids=lambda a: ACT_NAMES[a])
def test_every_activation_code(act):
    n_seg, P, K, N, _ = ACT_CASE
    A, gate, W, b, R = G.make_operands(77, *ACT_CASE)
    b[:2] = (7.5, -7.5)             # columns above 6 / below -3: ReLU6 and the hard functions saturate on both sides
    pre, bound = O.gated64(A, gate, W, b, None, P), O.gated_bound64(A, gate, W, b, P)
    assert (pre < -3).any() and (pre > 6).any() and (np.abs(pre) < 3).any()
    got, name = _gated(A, gate, W, b, R, P, act)
    assert name == G.kernel_name(n_seg * P, N)
    if act in (HSWISH, HSIGMOID):
        # tests/test_hardswish_gpu.py's inequality: the slope 1.5 (1 / 6) for 1.2, eps_act 3 2^-23 |s| (2^-22)
        slope, eps = (1.5, 3.0 * 2.0 ** -23 * np.abs(pre)) if act == HSWISH else (1.0 / 6.0, np.full_like(pre, 2.0 ** -22))
        r = R.astype(np.float64)
        err = np.abs(got.astype(np.float64) - (act64h(pre, act) + r))
        tol = G.tau(K) * (slope * bound + np.abs(r)) + eps
        assert np.isfinite(got).all() and (err <= tol).all(), (name, ACT_NAMES[act], float((err / tol).max()))
        print(f"{ACT_NAMES[act]} {name}: worst err / tol {float((err / tol).max()):.3f}")
    else:
        share = G.check(got, name, pre, bound, R, act, K, "act " + ACT_NAMES[act])
        print(f"{ACT_NAMES[act]} {name}: worst share of tau {share:.3f}")
    twin, _ = _twin(A * np.repeat(gate, P, axis=0), W, b, R, act)
    _same_bits(got, twin, f"{name} {ACT_NAMES[act]} against its ungated twin")


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: the code, and the output buffer left as it was
# ---------------------------------------------------------------------------------------------------------------------------
def test_refuses_what_the_kernel_does_not_take():
    lib = _lib()
    A, gate, W, b, R = G.make_operands(3, 4, 16, 24, 8, True)
    out = np.full((64, 8), 123.0, np.float32)

    def call(A=A, gate=gate, W=W, b=b, R=R, out=out, M=64, K=24, N=8, P=16, act=O.ACT_NONE):
        name = C.create_string_buffer(b"untouched", 128)
        rc = lib.bh_debug_gated_gemm_f32(0, _p(A), _p(gate), _p(W), _p(b), _p(R), _p(out), M, K, N, P, act, name, 128)
        assert (out == 123.0).all() and name.value == b"untouched", "a refused call wrote its outputs"
        return rc

    assert call(K=22) == BH_ERR_UNSUPPORTED and b"multiple of 4" in lib.bh_last_error()       # K % 4 != 0
    assert call(P=15) == BH_ERR_INVALID                                                         # M % rows_per_seg != 0
    assert call(P=0) == BH_ERR_INVALID and call(M=0) == BH_ERR_INVALID and call(N=0) == BH_ERR_INVALID and call(K=0) == BH_ERR_INVALID
    assert call(act=-1) == BH_ERR_INVALID and call(act=HSIGMOID + 1) == BH_ERR_INVALID
    for null in ("A", "gate", "W", "b"):
        assert call(**{null: None}) == BH_ERR_INVALID, null
    assert lib.bh_debug_gated_gemm_f32(0, _p(A), _p(gate), _p(W), _p(b), _p(R), None, 64, 24, 8, 16, 0, None, 0) == BH_ERR_INVALID
    got = np.empty((64, 8), np.float32)
    assert lib.bh_debug_gated_gemm_f32(0, _p(A), _p(gate), _p(W), _p(b), None, _p(got), 64, 24, 8, 16, 0, None, 0) == 0    # no R, no name: fine
    assert np.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the product path: SliceRun::fused_se's own call, on the device's own D and gate
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("which", ["mini_se", "fused_wide_se"])
def test_fused_se_blocks_on_the_devices_own_tensors(which, prec, tmp_path, monkeypatch):
    """A debug context that still runs the fused blocks keeps every tensor: for each fused squeeze-excite block that keeps D (one with
    an expand or stem convolution), the project output the forward wrote against gated64 of the D and the gate the forward itself
    produced (and its residual), every element, by the inequality above -- for f16x3 too: three products a MAC meet the f32 figure
    (tests/test_layer_gemm_gpu.py's tau is one for both), and D x gate is rounded to f32 there as well."""
    from birda_amd import modelfile as mf, synth
    from birda_amd.classifier import BirdClassifier
    import test_arena_plan_gpu as TA
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    monkeypatch.setenv("BIRDA_HIP_KEEP_FUSED", "1")
    m = synth.build_model("mini_se") if which == "mini_se" else synth.build_model("custom", plan=TA.FUSED_WIDE_SE_PLAN)
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    n = 3
    segs = synth.synth_segments(n, m.sample_count, m.sample_rate, start=5)
    clf = BirdClassifier(path, None, precision=prec)
    ctx = clf.create_batch_context(n)
    logits = clf.predict_logits(ctx, segs)
    assert np.isfinite(logits).all()
    _, _, tags = TA.arena_plan(clf, ctx, 0)
    blob = m.blob.astype(np.float32)
    held = 0
    for i, tag in enumerate(tags):
        if tag != TA.PATH_FUSED_SE:
            continue
        iD = i if m.layers[i].op == mf.OP_DWCONV else i + 1
        if iD == i:
            continue                # no expand convolution: D is computed twice and never kept
        iPw2, iP = iD + 3, iD + 5
        LD, LP = m.layers[iD], m.layers[iP]
        assert LD.op == mf.OP_DWCONV and LP.op == mf.OP_PWCONV and LP.in_tensor == iD + 5 and LP.act == mf.ACT_NONE
        P, K, N = LD.out_h * LD.out_w, LP.cin, LP.cout
        D = clf.read_tensor(ctx, iD + 1, n).reshape(n * P, K)
        if prec != "f32" and K % 16 == 0 and P % 16 == 0 and N % 4 == 0 and 6 <= -(-N // 16) <= 15:      # pw_gemm16_gated_wants_blocked
            D = np.ascontiguousarray(D.reshape(n * P // 16, K // 16, 16, 16).transpose(0, 2, 1, 3)).reshape(n * P, K)
        gate = clf.read_tensor(ctx, iPw2 + 1, n).reshape(n, K)
        R = None if LP.res_tensor == mf.NO_TENSOR else clf.read_tensor(ctx, LP.res_tensor, n).reshape(n * P, N)
        Y = clf.read_tensor(ctx, iP + 1, n).reshape(n * P, N)
        assert np.isfinite(D).all() and (gate >= 0).all() and (gate <= 1).all() and np.ptp(gate) > 0.01, (i, "not a gate")
        W, b = blob[LP.w_off:LP.w_off + K * N].reshape(K, N), blob[LP.b_off:LP.b_off + N]
        pre, bound = O.gated64(D, gate, W, b, None, P), O.gated_bound64(D, gate, W, b, P)
        share = G.check(Y, f"{which} {prec} block at layer {i}", pre, bound, R, O.ACT_NONE, K, "product path")
        print(f"{which} {prec} block at layer {i}: {n * P} x {K} -> {N}, residual {R is not None}: worst share of tau {share:.3f}")
        held += 1
    assert held >= 1, (which, prec, tags)
    ctx.close(); clf.close()


# ---------------------------------------------------------------------------------------------------------------------------
# every instantiation behind launch_pw_gemm_gated was reached (keep last: it reads what the tests above ran)
# ---------------------------------------------------------------------------------------------------------------------------
def test_every_gated_f32_kernel_was_reached():
    if RAN != set(G.CASES):
        pytest.skip("reads the kernels the module's other tests ran: run the module whole")
    assert set(WORST) == G.ALL_NAMES and G.ALL_NAMES <= REACHED, (sorted(G.ALL_NAMES - set(WORST)), sorted(REACHED))
    print("\nworst share of tau = 4e-7 max(1, sqrt(K / 1024)) + 2^-24 by instantiation:")
    for name, v in sorted(WORST.items()):
        print(f"  {name:36s} {v:.3f}")
    assert max(WORST.values()) <= 1.0
