"""The layer kernels outside the fused blocks on their own, element by element against float64 (oracle/oracle.py): the full
convolutions' implicit GEMMs (conv_gemm_kernel, f32 MFMA; conv_gemm16_kernel, split f16) through bh_debug_conv_gemm, and the
pointwise / dense GEMMs and the fused head convolution + pool through bh_debug_layer_gemm -- every kernel and epilogue
instantiation behind launch_conv_gemm, launch_conv_gemm16, launch_pw_gemm, launch_pw_gemm16 and launch_head_gap16, on shapes no
model of the suite has.  The logit-level tests average a wrong edge row or a wrong tile away; here every output element is held to

    |got - ref| <= tau (1.2 bound + |R|) + eps_act(pre),   bound = |A| |W| + |b| in float64 (A: the im2col rows for a convolution),

tau = 4e-7 max(1, sqrt(K / 1024)) for f32 and split f16 (three products a MAC), 1.5e-3 for plain f16; 1.2 bounds the slope of GELU
and swish; eps_act is the activation's own stated tolerance (GELU 5e-7 max(|v|, 1)).  Every device buffer
sits in NaN guard bands and C starts as a NaN payload of its own: an element never written, a read past an operand and a write
past C all fail.  Launches of different sizes must give the same bits where the sources say so."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
ACTS16 = [O.ACT_NONE, O.ACT_GELU_ERF, O.ACT_SWISH, O.ACT_RELU6]             # the split-f16 epilogues' instantiations
ACTS32 = ACTS16 + [O.ACT_RELU, O.ACT_GELU_TANH, O.ACT_SIGMOID]              # ... and the f32 kernels' run-time switch
REACHED = set()          # kernel instantiations the module ran
WORST = {}               # (family, terms) -> worst (err - eps_act) / (1.2 bound + |R|)


def _lib():
    from birda_amd import _lib
    return _lib.load()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _family(name):
    return name.split("<")[0]


def _record(name):
    REACHED.add(name)
    return name


def _conv(X, W, b, R, shape, act, terms):
    """shape = (in_h, in_w, out_h, out_w, cin, cout, kh, kw, sh, sw, pad_t, pad_l) -> (C [n * out_h * out_w][cout], kernel name)"""
    lib = _lib()
    n = X.shape[0]
    out = np.empty((n * shape[2] * shape[3], shape[5]), np.float32)
    sh = np.asarray(shape, np.int32)
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_conv_gemm(0, _p(X), _p(W), _p(b), _p(R), _p(out), n, _p(sh), act, terms, name, 128)
    assert rc == 0, (rc, lib.bh_last_error())
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"
    return out, _record(name.value.decode())


def _layer(A, W, b, R, act, terms, pool_rows=0):
    lib = _lib()
    M, K = A.shape
    N = W.shape[1]
    out = np.empty((M // pool_rows if pool_rows else M, N), np.float32)
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_layer_gemm(0, _p(A), _p(W), _p(b), _p(R), _p(out), M, K, N, pool_rows, act, terms, name, 128)
    assert rc == 0, (rc, lib.bh_last_error())
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"
    return out, _record(name.value.decode())


def _tau(terms, k_eff):
    return 1.5e-3 if terms == 1 else 4e-7 * max(1.0, math.sqrt(k_eff / 1024.0))


def _eps_act(pre, act):
    if act == O.ACT_GELU_ERF:
        return 5e-7 * np.maximum(np.abs(pre), 1.0)
    if act in (O.ACT_SWISH, O.ACT_SIGMOID, O.ACT_GELU_TANH):
        return 1e-6 * np.maximum(np.abs(pre), 1.0)
    return np.zeros_like(pre)


def _check(got, name, pre, bound, R, act, terms, k_eff, what, tau_extra=0.0):
    """Element by element against act(pre) (+ R); records the worst share of the GEMM part of the tolerance.  tau_extra: added to
    tau by a caller whose kernel rounds once more per product (tests/test_gated_gemm.py: the gate multiply, 2^-24)."""
    ref = O.act64(pre, act)
    r = np.zeros_like(ref) if R is None else R.astype(np.float64)
    ref = ref + r
    assert np.isfinite(got).all(), (what, name, "non-finite output")
    scale = 1.2 * bound + np.abs(r)
    err = np.abs(got.astype(np.float64) - ref)
    eps = _eps_act(pre, act)
    tol = (_tau(terms, k_eff) + tau_extra) * scale + eps
    bad = err > tol
    share = np.max(np.maximum(err - eps, 0.0) / np.maximum(scale, 1e-300))
    key = (_family(name), terms)
    WORST[key] = max(WORST.get(key, 0.0), float(share))
    if bad.any():
        i = np.unravel_index(np.argmax(err / tol), err.shape)
        pytest.fail(f"{what} {name} act {O.ACT_NAMES[act]}: {int(bad.sum())} of {bad.size} elements off, worst at {i}: got "
                    f"{got[i]!r} want {ref[i]!r} (pre {pre[i]!r}), err {err[i]:.3e} > tol {tol[i]:.3e}")


def _operands(rng, a_shape, k_rows, N, residual, M):
    """Channels of different scale (0.2-3x), He-scaled W, a bias of order 1, R on request."""
    k_in = a_shape[-1]
    A = (rng.standard_normal(a_shape) * rng.uniform(0.2, 3.0, k_in)).astype(np.float32)
    W = (rng.standard_normal((k_rows, N)) * math.sqrt(2.0 / k_rows)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    b[:2] = (7.5, -7.5)[:N]          # columns whose pre-activations mostly lie above 6 / below 0: ReLU6 clamps on both sides
    R = rng.standard_normal((M, N)).astype(np.float32) if residual else None
    return A, W, b, R


# ---------------------------------------------------------------------------------------------------------------------------
# full convolutions
# ---------------------------------------------------------------------------------------------------------------------------
def _same(n, k, s):
    out = -(-n // s)
    return out, max((out - 1) * s + k - n, 0) // 2


def _conv_case(name, n_seg, in_h, in_w, cin, cout, kh, kw, sh=1, sw=1, pad="same", out_hw=None, residual=False):
    if pad == "same":
        (oh, pt), (ow, pl) = _same(in_h, kh, sh), _same(in_w, kw, sw)
    elif pad == "valid":
        oh, ow, pt, pl = (in_h - kh) // sh + 1, (in_w - kw) // sw + 1, 0, 0
    else:
        pt, pl = pad
        oh, ow = out_hw
    return (name, n_seg, (in_h, in_w, oh, ow, cin, cout, kh, kw, sh, sw, pt, pl), residual)


CONV_CASES = [
    _conv_case("17x23_36to100", 3, 17, 23, 36, 100, 3, 3),                 # one 32-channel step + 4; 7 column tiles, the last partial
    _conv_case("v2l_32x125_64to256", 1, 32, 125, 64, 256, 3, 3, residual=True),
    _conv_case("v2l_32x125_64to256_s2", 1, 32, 125, 64, 256, 3, 3, 2, 2),   # SAME at stride 2: pad_t 0, pad_b 1
    _conv_case("5x5_valid_132to68", 3, 9, 9, 132, 68, 5, 5, pad="valid", residual=True),
    _conv_case("7x7_s2_12to384", 3, 7, 11, 12, 384, 7, 7, 2, 2),
    _conv_case("7x7_on_2x3", 5, 2, 3, 8, 132, 7, 7, residual=True),          # the kernel larger than the image
    _conv_case("1x7_s1x2_20to260", 2, 9, 20, 20, 260, 1, 7, 1, 2),
    _conv_case("7x1_s2x1_20to260", 2, 20, 9, 20, 260, 7, 1, 2, 1, residual=True),
    _conv_case("2x2_s2_valid_64to128", 3, 12, 15, 64, 128, 2, 2, 2, 2, pad="valid"),
    _conv_case("4x4_pad3_0_28to72", 2, 10, 10, 28, 72, 4, 4, pad=(3, 0), out_hw=(10, 7)),
    _conv_case("3x3_pad_t3_crop", 2, 8, 8, 16, 100, 3, 3, pad=(3, 1), out_hw=(8, 8), residual=True),   # a whole row of taps above
    _conv_case("1x1_s2_96to196", 3, 9, 13, 96, 196, 1, 1, 2, 2, pad="valid"),
    _conv_case("1px_wide_32to132", 4, 20, 1, 32, 132, 3, 3),
    _conv_case("37seg_17x23_36to100", 37, 17, 23, 36, 100, 3, 3, residual=True),   # row tiles straddle segments, M % 128 != 0
    _conv_case("1x1_image_64to136", 1, 1, 1, 64, 136, 3, 3),               # a single output row
    _conv_case("pad_b_past_kernel", 2, 5, 6, 24, 100, 3, 3, pad=(1, 1), out_hw=(9, 8)),   # bottom / right pad larger than kh, kw
    _conv_case("1x1_s1_4to20", 2, 6, 7, 4, 20, 1, 1, pad="valid"),
    _conv_case("3x3_s2_48to64_odd", 3, 13, 11, 48, 64, 3, 3, 2, 2, residual=True),
    _conv_case("5x3_s2x1_8to1000", 1, 6, 5, 8, 1000, 5, 3, 2, 1),          # eight column tiles of the f32 kernel, many of conv16
]
_REF_CACHE = {}


def _conv_reference(case):
    name, n_seg, shape, residual = case
    if name not in _REF_CACHE:
        in_h, in_w, oh, ow, cin, cout, kh, kw, sh, sw, pt, pl = shape
        rng = np.random.default_rng(sum(shape) * 7 + n_seg)
        M = n_seg * oh * ow
        X, W, b, R = _operands(rng, (n_seg, in_h, in_w, cin), kh * kw * cin, cout, residual, M)
        W = W.reshape(kh, kw, cin, cout)
        pre, A = O.conv_nhwc64(X, W.astype(np.float64), b, sh, sw, pt, pl, oh, ow)
        bound = np.abs(A) @ np.abs(W.reshape(-1, cout).astype(np.float64)) + np.abs(b.astype(np.float64))
        _REF_CACHE[name] = (X, W, b, R, pre, bound)
    return _REF_CACHE[name]


def _conv_params():
    out = []
    for i, case in enumerate(CONV_CASES):
        for terms in (0, 1, 3):
            acts = ACTS32 if terms == 0 else ACTS16
            out.append(pytest.param(case, terms, acts[(i + terms) % len(acts)], id=f"{case[0]}-t{terms}-{O.ACT_NAMES[acts[(i + terms) % len(acts)]]}"))
    res = _conv_case("res_96to96", 2, 10, 12, 96, 96, 3, 3, residual=True)
    for terms in (0, 1, 3):
        for act in (ACTS32 if terms == 0 else ACTS16):
            out.append(pytest.param(res, terms, act, id=f"res_96to96-t{terms}-{O.ACT_NAMES[act]}"))
    return out


@pytest.mark.parametrize("case,terms,act", _conv_params())
def test_conv_gemm_matches_float64(case, terms, act):
    name, n_seg, shape, residual = case
    X, W, b, R, pre, bound = _conv_reference(case)
    got, kname = _conv(X, W, b, R, shape, act, terms)
    assert _family(kname) == ("conv_gemm16_kernel" if terms else "conv_gemm_kernel"), kname
    if act == O.ACT_RELU6:
        assert (pre < 0).any() and (pre > 6).any(), "operands should make ReLU6 clamp on both sides"
    _check(got, kname, pre, bound, R, act, terms, shape[6] * shape[7] * shape[4], name)


def test_conv16_segment_bits_do_not_depend_on_the_launch():
    """Segment 0 alone against segment 0 of a 37-segment launch (more row tiles, tiles straddling segments)."""
    case = next(c for c in CONV_CASES if c[0] == "37seg_17x23_36to100")
    X, W, b, R, pre, bound = _conv_reference(case)
    shape = case[2]
    rows = shape[2] * shape[3]
    for terms in (1, 3):
        for act in (O.ACT_GELU_ERF, O.ACT_NONE):
            big, _ = _conv(X, W, b, R, shape, act, terms)
            one, _ = _conv(X[:1].copy(), W, b, R[:rows].copy(), shape, act, terms)
            assert np.array_equal(big[:rows], one), (terms, act)


def test_conv32_bits_do_not_depend_on_the_row_tile():
    """conv_gemm_kernel at BM 128 (a launch of >= 512 128-row blocks) against BM 64 (a few segments): the same bits."""
    rng = np.random.default_rng(5)
    shape = (17, 23, 17, 23, 36, 100, 3, 3, 1, 1, 1, 1)
    n_big, n_small = 170, 8
    X, W, b, R = _operands(rng, (n_big, 17, 23, 36), 9 * 36, 100, True, n_big * 17 * 23)
    W = W.reshape(3, 3, 36, 100)
    rows = n_small * 17 * 23
    for act in (O.ACT_SWISH, O.ACT_NONE):
        big, kb = _conv(X, W, b, R, shape, act, 0)
        small, ks = _conv(X[:n_small].copy(), W, b, R[:rows].copy(), shape, act, 0)
        assert kb.startswith("conv_gemm_kernel<BM=128") and ks.startswith("conv_gemm_kernel<BM=64"), (kb, ks)
        assert np.array_equal(big[:rows], small), act
    pre, A = O.conv_nhwc64(X[:n_small], W.astype(np.float64), b, 1, 1, 1, 1, 17, 23)
    bound = np.abs(A) @ np.abs(W.reshape(-1, 100).astype(np.float64)) + np.abs(b.astype(np.float64))
    _check(small, ks, pre, bound, R[:rows], O.ACT_NONE, 0, 9 * 36, "bm64_vs_128")


# ---------------------------------------------------------------------------------------------------------------------------
# pointwise / dense GEMMs
# ---------------------------------------------------------------------------------------------------------------------------
PW16 = [  # (M, K, N): skinny M <= 32, streaming 33 .. 63, staged from 64 (NTB 8 / 4 / 2 by grid size)
    (1, 32, 4), (7, 320, 1000), (16, 1024, 6522), (17, 320, 68), (32, 32, 132),
    (33, 320, 100), (48, 1024, 20), (63, 32, 1024),
    (64, 320, 4), (65, 1024, 132), (127, 32, 6522), (128, 320, 1000), (129, 320, 6522), (300, 32, 20),
    (3000, 320, 1024), (3000, 32, 1000), (3000, 32, 100),
    (6151, 32, 1024), (6151, 32, 1000),
]
PW32 = [  # (M, K, N): BM 64 below 512 blocks of 128 rows, BM 128 above
    (1, 4, 4), (7, 36, 20), (16, 1024, 100), (17, 100, 68), (33, 1028, 100), (64, 32, 132), (65, 320, 1000), (127, 1024, 1024),
    (129, 36, 6522), (300, 100, 4), (3000, 4, 1024), (6151, 36, 1024), (8200, 32, 1024), (1400, 36, 6522),
]


def _pw_params():
    out = []
    for i, (M, K, N) in enumerate(PW16):
        for terms in (1, 3):
            act = ACTS16[(i + terms) % 4]
            out.append(pytest.param((M, K, N), terms, act, id=f"M{M}_K{K}_N{N}-t{terms}-{O.ACT_NAMES[act]}"))
    for i, (M, K, N) in enumerate(PW32):
        act = ACTS32[i % 7]
        out.append(pytest.param((M, K, N), 0, act, id=f"M{M}_K{K}_N{N}-t0-{O.ACT_NAMES[act]}"))
    return out


@pytest.mark.parametrize("mkn,terms,act", _pw_params())
def test_layer_gemm_matches_float64(mkn, terms, act):
    M, K, N = mkn
    rng = np.random.default_rng(M * 7 + K * 131 + N)
    A, W, b, R = _operands(rng, (M, K), K, N, (M + N) % 2 == 0, M)
    got, kname = _layer(A, W, b, R, act, terms)
    pre = O.gemm64(A, W, b)
    bound = np.abs(A.astype(np.float64)) @ np.abs(W.astype(np.float64)) + np.abs(b.astype(np.float64))
    _check(got, kname, pre, bound, R, act, terms, K, "pw")


def test_pw16_row_bits_do_not_depend_on_the_kernel():
    """The first 16 rows, N = 1 024, K = 320, through the skinny, streaming and staged (NTB 2 / 4 / 8) kernels: the same bits."""
    rng = np.random.default_rng(9)
    M, K, N = 6151, 320, 1024
    A, W, b, R = _operands(rng, (M, K), K, N, True, M)
    for terms in (3, 1):
        outs = {}
        for m in (16, 48, 256, 3000, 6151):
            got, kname = _layer(A[:m].copy(), W, b, R[:m].copy(), O.ACT_GELU_ERF, terms)
            outs[kname] = got[:16]
        assert len(outs) == 5, sorted(outs)      # five different kernels
        first = next(iter(outs.values()))
        for kname, o in outs.items():
            assert np.array_equal(o, first), (terms, kname)
        pre = O.gemm64(A[:16], W, b)
        bound = np.abs(A[:16].astype(np.float64)) @ np.abs(W.astype(np.float64)) + np.abs(b.astype(np.float64))
        _check(first, kname, pre, bound, R[:16], O.ACT_GELU_ERF, terms, K, "pw16 bits")


def test_pw32_bits_do_not_depend_on_the_row_tile():
    rng = np.random.default_rng(10)
    M, K, N = 8200, 36, 1024
    A, W, b, R = _operands(rng, (M, K), K, N, False, M)
    big, kb = _layer(A, W, b, None, O.ACT_SIGMOID, 0)
    small, ks = _layer(A[:256].copy(), W, b, None, O.ACT_SIGMOID, 0)
    assert kb.startswith("pw_gemm_kernel<BM=128") and ks.startswith("pw_gemm_kernel<BM=64"), (kb, ks)
    assert np.array_equal(big[:256], small)


# ---------------------------------------------------------------------------------------------------------------------------
# the fused head convolution + pool
# ---------------------------------------------------------------------------------------------------------------------------
HEAD = [  # (P, n_seg, K, N): PT / SW 3 / 2 for P <= 48, 5 / 1 up to 80; CT 2 for launches of <= 32 segments, 8 above
    (1, 1, 32, 128), (15, 5, 320, 1280), (16, 8, 32, 1280), (17, 9, 320, 128), (33, 32, 32, 1280), (48, 33, 320, 1280),
    (16, 100, 320, 1280), (49, 100, 32, 128), (64, 1, 320, 1280), (80, 33, 320, 1280), (80, 32, 32, 128), (49, 5, 320, 128),
]
HEAD_ACTS = [O.ACT_GELU_ERF, O.ACT_SWISH, O.ACT_RELU6]


def _head_params():
    out = []
    for i, case in enumerate(HEAD):
        for terms in (1, 3):
            act = HEAD_ACTS[(i + terms) % 3]
            out.append(pytest.param(case, terms, act, id="P%d_n%d_K%d_N%d" % case + f"-t{terms}-{O.ACT_NAMES[act]}"))
    return out


def _check_head(got, kname, A, W, b, P, act, terms, what):
    pre = O.gemm64(A, W, b)
    bound = np.abs(A.astype(np.float64)) @ np.abs(W.astype(np.float64)) + np.abs(b.astype(np.float64))
    v = O.act64(pre, act)
    K = A.shape[1]
    # the mean of the per-element bounds, plus the pool's own rounding: P additions and the 1 / P multiply
    pool_round = P * 2.0 ** -24 * O.head_pool64(np.abs(v), P)
    eps = O.head_pool64(_eps_act(pre, act), P)
    ref = O.head_pool64(v, P)
    scale = 1.2 * O.head_pool64(bound, P)
    err = np.abs(got.astype(np.float64) - ref)
    tol = _tau(terms, K) * scale + eps + pool_round
    key = (_family(kname), terms)
    WORST[key] = max(WORST.get(key, 0.0), float(np.max(np.maximum(err - eps - pool_round, 0.0) / scale)))
    assert np.isfinite(got).all(), what
    if (err > tol).any():
        i = np.unravel_index(np.argmax(err / tol), err.shape)
        pytest.fail(f"{what} {kname}: {int((err > tol).sum())} of {err.size} off, worst at {i}: got {got[i]!r} want {ref[i]!r}, "
                    f"err {err[i]:.3e} > tol {tol[i]:.3e}")


@pytest.mark.parametrize("case,terms,act", _head_params())
def test_head_pool_matches_float64(case, terms, act):
    P, n_seg, K, N = case
    rng = np.random.default_rng(P * 1000 + n_seg * 10 + K + N)
    A, W, b, _ = _operands(rng, (n_seg * P, K), K, N, False, n_seg * P)
    got, kname = _layer(A, W, b, None, act, terms, pool_rows=P)
    assert _family(kname) == "head_gap16_kernel", kname
    _check_head(got, kname, A, W, b, P, act, terms, "head")


def test_head_pool_segment_bits_do_not_depend_on_the_launch():
    """The first 32 segments of a 32-segment launch (two column tiles a workgroup) against a 100-segment launch (eight)."""
    rng = np.random.default_rng(12)
    for P in (16, 49):
        A, W, b, _ = _operands(rng, (100 * P, 320), 320, 1280, False, 100 * P)
        for terms in (3, 1):
            big, kb = _layer(A, W, b, None, O.ACT_GELU_ERF, terms, pool_rows=P)
            few, kf = _layer(A[:32 * P].copy(), W, b, None, O.ACT_GELU_ERF, terms, pool_rows=P)
            assert kb.endswith("CT=8>") and kf.endswith("CT=2>"), (kb, kf)
            assert np.array_equal(big[:32], few), (P, terms)


# ---------------------------------------------------------------------------------------------------------------------------
# the activations across their range: A = 0, so pre = bias exactly in every kernel and mode
# ---------------------------------------------------------------------------------------------------------------------------
def _act_points(n):
    f = np.float32
    grid = np.linspace(-16.0, 16.0, 1 << 16, dtype=np.float64).astype(f)
    mags = np.logspace(-30, 30, 241).astype(f)
    sub = np.array([1.4e-45, 2.8e-45, 1e-42, 1e-40, 5.877472e-39, 1.1754942e-38, 1.1754944e-38], f)
    edges = np.array([0.0, -0.0, 6.0, np.nextafter(f(6), f(0)), np.nextafter(f(6), f(7)), np.nextafter(f(0), f(1)),
                      np.nextafter(f(0), f(-1))], f)
    pts = np.concatenate([grid, mags, -mags, sub, -sub, edges])
    fill = np.linspace(-7.0, 7.0, n - len(pts), dtype=np.float64).astype(f)   # more points where the activations bend
    return np.concatenate([pts, fill])


N_ACT = (1 << 16) + 1280       # a multiple of 128 (the head kernel's column block)


def _act_cases():
    out = []
    for act in ACTS32:
        out.append(pytest.param("pw", 0, act, id=f"pw-t0-{O.ACT_NAMES[act]}"))
        out.append(pytest.param("conv", 0, act, id=f"conv-t0-{O.ACT_NAMES[act]}"))
    for terms in (1, 3):
        for act in ACTS16:
            for fam in ("pw16_skinny", "pw16_stream", "pw16_staged", "conv16"):
                out.append(pytest.param(fam, terms, act, id=f"{fam}-t{terms}-{O.ACT_NAMES[act]}"))
            if act != O.ACT_NONE:
                for fam in ("head3", "head5"):
                    out.append(pytest.param(fam, terms, act, id=f"{fam}-t{terms}-{O.ACT_NAMES[act]}"))
    return out


@pytest.mark.parametrize("fam,terms,act", _act_cases())
def test_activation_across_its_range(fam, terms, act):
    b = _act_points(N_ACT)
    pre = b.astype(np.float64)
    rng = np.random.default_rng(1)
    if fam.startswith("conv"):
        K, rows = 4, 2
        W = rng.standard_normal((1, 1, K, N_ACT)).astype(np.float32)
        got, kname = _conv(np.zeros((1, 1, rows, K), np.float32), W, b, None, (1, rows, 1, rows, K, N_ACT, 1, 1, 1, 1, 0, 0), act, terms)
    elif fam.startswith("head"):
        P = 3 if fam == "head3" else 49
        K = 32
        W = rng.standard_normal((K, N_ACT)).astype(np.float32)
        got, kname = _layer(np.zeros((2 * P, K), np.float32), W, b, None, act, terms, pool_rows=P)
    else:
        rows = {"pw": 5, "pw16_skinny": 16, "pw16_stream": 40, "pw16_staged": 64}[fam]
        K = 32
        W = rng.standard_normal((K, N_ACT)).astype(np.float32)
        got, kname = _layer(np.zeros((rows, K), np.float32), W, b, None, act, terms)
    want = O.act64(pre, act)
    want_rows = want[None, :]
    tol = _eps_act(pre, act) + _tau(terms, K) * 1.2 * np.abs(pre)
    if fam.startswith("head"):
        tol += 49 * 2.0 ** -24 * np.abs(want)          # the pool's P additions and 1 / P multiply
    err = np.abs(got.astype(np.float64) - want_rows)
    assert np.isfinite(got).all(), kname
    if act in (O.ACT_NONE, O.ACT_RELU, O.ACT_RELU6) and not fam.startswith("head"):
        assert np.array_equal(got, np.broadcast_to(want_rows, got.shape).astype(np.float32)), (kname, "must match exactly")
    bad = err > tol[None, :]
    if bad.any():
        j = np.argmax((err / tol[None, :]).max(axis=0))
        pytest.fail(f"{kname} {O.ACT_NAMES[act]}: {int(bad.sum())} elements off, worst at v = {pre[j]!r}: got {got[:, j].tolist()} "
                    f"want {want[j]!r}, tol {tol[j]:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# quiet operands: A's lo halves are f16 subnormals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["pw16_skinny", "pw16_stream", "pw16_staged", "conv16"])
def test_quiet_operands_keep_the_subnormal_lo_halves(what):
    """A scaled by 2^-8: |a| < 2^-3, so the lo half a - f16(a) (<= 2^-15) is an f16 subnormal, resolution 2^-24.  If the conversion
    and the MFMA keep subnormals (the default mode), split f16 stays within tau bound + 2^-24 sum_k |W_kn|; flushed, the error is
    ~2^-11 |a| |w| a term."""
    rng = np.random.default_rng(21)
    if what == "conv16":
        case = next(c for c in CONV_CASES if c[0] == "17x23_36to100")
        shape = case[2]
        X, W, b, _ = _operands(rng, (3, 17, 23, 36), 9 * 36, 100, False, 3 * 17 * 23)
        X = (X * 2.0 ** -8).astype(np.float32)
        W = W.reshape(3, 3, 36, 100)
        got, kname = _conv(X, W, b, None, shape, O.ACT_NONE, 3)
        pre, A = O.conv_nhwc64(X, W.astype(np.float64), b, 1, 1, 1, 1, 17, 23)
        Wk = W.reshape(-1, 100).astype(np.float64)
    else:
        M = {"pw16_skinny": 16, "pw16_stream": 48, "pw16_staged": 1000}[what]
        A, Wk, b, _ = _operands(rng, (M, 320), 320, 1000, False, M)
        A = (A * 2.0 ** -8).astype(np.float32)
        got, kname = _layer(A, Wk, b, None, O.ACT_NONE, 3)
        pre = O.gemm64(A, Wk, b)
        Wk = Wk.astype(np.float64)
    assert (np.abs(A) < 2.0 ** -3).all() and (np.abs(A) > 2.0 ** -14).any()
    bound = np.abs(A.astype(np.float64)) @ np.abs(Wk) + np.abs(b.astype(np.float64))
    err = np.abs(got.astype(np.float64) - pre)
    tol = _tau(3, Wk.shape[0]) * bound + 2.0 ** -24 * np.abs(Wk).sum(axis=0)[None, :]
    assert (err <= tol).all(), (kname, float((err / tol).max()))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refuses_what_the_kernels_do_not_take():
    lib = _lib()
    z = np.zeros(1 << 16, np.float32)
    out = np.empty(1 << 16, np.float32)

    def conv(shape, act, terms):
        return lib.bh_debug_conv_gemm(0, _p(z), _p(z), _p(z), None, _p(out), 1, _p(np.asarray(shape, np.int32)), act, terms, None, 0)

    ok = (6, 6, 6, 6, 8, 8, 3, 3, 1, 1, 1, 1)
    assert conv(ok, O.ACT_NONE, 3) == 0 and conv(ok, O.ACT_GELU_TANH, 0) == 0
    for terms in (0, 1, 3):
        assert conv((6, 6, 6, 6, 6, 8, 3, 3, 1, 1, 1, 1), O.ACT_NONE, terms) != 0        # cin % 4 != 0
        assert conv((9, 9, 2, 2, 8, 8, 8, 8, 1, 1, 0, 0), O.ACT_NONE, terms) != 0        # kernel 8
        assert conv((9, 9, 3, 3, 8, 8, 3, 3, 3, 3, 0, 0), O.ACT_NONE, terms) != 0        # stride 3
        assert conv((6, 6, 0, 6, 8, 8, 3, 3, 1, 1, 1, 1), O.ACT_NONE, terms) != 0        # no output rows
    for terms in (1, 3):
        assert conv(ok, O.ACT_GELU_TANH, terms) != 0
        assert conv(ok, O.ACT_SIGMOID, terms) != 0

    def layer(M, K, N, P, act, terms, R=None):
        return lib.bh_debug_layer_gemm(0, _p(z), _p(z), _p(z), _p(R), _p(out), M, K, N, P, act, terms, None, 0)

    assert layer(16, 32, 8, 0, O.ACT_NONE, 3) == 0 and layer(16, 36, 8, 0, O.ACT_NONE, 0) == 0
    assert layer(16, 36, 8, 0, O.ACT_NONE, 3) != 0 and layer(16, 36, 8, 0, O.ACT_NONE, 1) != 0     # K % 32 != 0 on split f16
    assert layer(16, 34, 8, 0, O.ACT_NONE, 0) != 0                                                  # K % 4 != 0 on f32
    assert layer(16, 32, 8, 0, O.ACT_GELU_TANH, 3) != 0
    assert layer(2 * 80, 32, 128, 80, O.ACT_GELU_ERF, 3) == 0
    assert layer(81, 32, 128, 81, O.ACT_GELU_ERF, 3) != 0          # P = 81
    assert layer(16, 32, 136, 16, O.ACT_GELU_ERF, 3) != 0          # N % 128 != 0
    assert layer(16, 32, 128, 16, O.ACT_GELU_ERF, 0) != 0          # terms 0
    assert layer(16, 32, 128, 16, O.ACT_GELU_ERF, 3, R=z) != 0     # a residual with the pool
    assert layer(16, 32, 128, 16, O.ACT_NONE, 3) != 0              # no activation: the head kernel has none


# ---------------------------------------------------------------------------------------------------------------------------
# every kernel behind the dispatch was reached (keep last: it reads what the tests above ran)
# ---------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_was_reached():
    if not REACHED:
        pytest.skip("reads the kernels the module's other tests ran: run the module whole")
    acts = "(NONE|GELU|SWISH|RELU6)"
    want = [r"conv_gemm_kernel<BM=64,NT=\d>", r"conv_gemm_kernel<BM=128,NT=\d>", r"pw_gemm_kernel<BM=64,NT=\d>",
            r"pw_gemm_kernel<BM=128,NT=\d>"]
    want += [f"conv_gemm16_kernel<{t},{a}>" for t in (1, 3) for a in ("NONE", "GELU", "SWISH", "RELU6")]
    for t in (1, 3):
        want += [f"pw_gemm16_skinny_kernel<{t},{acts}>", f"pw_gemm16_kernel<{t},{acts}>"]
        want += [f"pw_gemm16s_kernel<{t},{acts},NTB={b}>" for b in (2, 4, 8)]
        want += [f"head_gap16_kernel<PT={pt},SW={sw},T={t},{acts},CT={ct}>" for pt, sw in ((3, 2), (5, 1)) for ct in (2, 8)]
    missing = [w for w in want if not any(re.fullmatch(w, n) for n in REACHED)]
    assert not missing, (missing, sorted(REACHED))
    nts = {re.fullmatch(r"conv_gemm_kernel<BM=\d+,NT=(\d)>", n).group(1) for n in REACHED if n.startswith("conv_gemm_kernel<")}
    assert len(nts) >= 5, sorted(nts)
    print("\nworst (err - eps_act) / (1.2 bound + |R|) by kernel family and terms:")
    for (fam, terms), v in sorted(WORST.items()):
        print(f"  {fam:28s} terms {terms}: {v:.3e}")
