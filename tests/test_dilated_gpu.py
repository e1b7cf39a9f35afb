"""Dilated layers on the device.  Through bh_debug_dilated_layer (include/birda_hip_dilated_debug.h) every output element of a dilated
full convolution (conv_gemm_kernel<BM,NT,DIL>, conv_gemm16_kernel<TERMS,ACT[,AFTER],DIL>) and of a dilated depthwise layer
(dwconv_kernel<KS,ST,DIL>) is held to
float64 (tests/test_dilated.py taps64: tap (dy, dx) reads pixel (oy sh - pad_t + dy dil_h, ox sw - pad_l + dx dil_w)):

    full convolution:  |got - ref| <= tau (1.2 bound + |R|) + eps_act,  bound = |A| |W| + |b|, A the dilated im2col rows,

tau = 4e-7 max(1, sqrt(K / 1024)) for f32 and split f16 (two or three products a MAC), 1.5e-3 for plain f16, eps_act the activation's
stated tolerance -- the rule and the constants of tests/test_layer_gemm_gpu.py: K and the arithmetic are those of the undilated
layer.  With the activation after the residual, ref = act(pre + R) and eps_act is taken at pre + R.

    depthwise:  |got - ref| <= tau(kh kw) 1.2 bound + eps_act,  bound = sum |tap| |w| + |b|  (tests/test_gate_layers_gpu.py's rule)

The shapes are the smallest at which the gather can go wrong: 3 segments of 4 x 5, 5 x 6 and 7 x 9 pixels (60, 90 and 189 rows: no
multiple of the 64- and 128-row tiles), extents larger than the image, per-axis dilation, stride 2 on odd images, 1 x 3 / 3 x 1 /
3 x 3 / 5 x 5 / 7 x 7 kernels, asymmetric pads and a cropped output, cin 4 / 36 / 64 (a partial step, a padded second step, two
whole steps per tap), cout 4 / 20 / 68 / 132.  Dilation 1 through the entry is bh_debug_conv_gemm bit for bit and name for name; one
NaN pixel makes exactly the outputs NaN that the reference says; 33 segments made of three repeated equal the three, bit for bit.

At model level synth's dilated_plan runs through the .onnx route and the .bhm route to the same bits, at 2e-5 of the logit scale of
tests/test_dilated.py's forward64 in f32, f16x3 and auto, with the same bits at 3, 80 and 300 segments and the kernels expected of
the dilated layers; an f16 overflow in front of a dilated layer ends in BH_ERR_NONFINITE (f16x3) and is re-run (auto);
dilated_resnet_audio at 40 classes is held to the same bound once."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, synth
from oracle import oracle as O
from test_dilated import conv64d, dilated, dw64d, forward64

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
BH_ERR_UNSUPPORTED, BH_ERR_NONFINITE = -6, -8
LOGIT_RTOL = 2e-5
OP_CONV, OP_DWCONV = 1, 2
AN = {O.ACT_NONE: "NONE", O.ACT_RELU: "RELU", O.ACT_RELU6: "RELU6", O.ACT_SWISH: "SWISH", O.ACT_GELU_ERF: "GELU"}


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _run(op, X, W, b, R, shape, act, terms, after, expect=0):
    """shape = (in_h, in_w, out_h, out_w, cin, cout, kh, kw, sh, sw, pad_t, pad_l, dil_h, dil_w) -> (C [n][out_h][out_w][cout], name)"""
    lib = _lib.load()
    n = X.shape[0]
    out = np.empty((n, shape[2], shape[3], shape[5]), np.float32)
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_dilated_layer(0, op, _p(X), _p(W), _p(b), _p(R), _p(out), n, _p(np.asarray(shape, np.int32)), act, terms, after, name, 128)
    if expect:
        assert rc == expect, (rc, lib.bh_last_error())
        return None, lib.bh_last_error().decode()
    assert rc == 0, (rc, lib.bh_last_error())
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"
    return out, name.value.decode()


def _tau(terms, k_eff):
    return 1.5e-3 if terms == 1 else 4e-7 * max(1.0, math.sqrt(k_eff / 1024.0))


def _eps_act(s, act):
    if act == O.ACT_GELU_ERF:
        return 5e-7 * np.maximum(np.abs(s), 1.0)
    if act in (O.ACT_SWISH, O.ACT_SIGMOID, O.ACT_GELU_TANH):
        return 1e-6 * np.maximum(np.abs(s), 1.0)
    return np.zeros_like(s)


def _hold(got, name, pre, bound, R, act, after, tau, what, ignore=None):
    """element by element; prints the worst share of the tolerance before it asserts.  ignore: a mask of elements held elsewhere"""
    r = np.zeros_like(pre) if R is None else R.astype(np.float64).reshape(pre.shape)
    s = pre + r if after else pre
    ref = O.act64(s, act) + (0.0 if after else r)
    tol = tau * (1.2 * bound + np.abs(r)) + _eps_act(s, act)
    err = np.abs(got.astype(np.float64).reshape(pre.shape) - ref)
    if ignore is not None:
        err, tol = np.where(ignore, 0.0, err), np.where(ignore, 1.0, tol)
    assert np.isfinite(err).all(), (what, name, "non-finite output")
    share = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{what} {name} act {O.ACT_NAMES[act]}{' after' if after else ''}: worst err / tol {share:.3f}")
    if share > 1.0:
        i = np.unravel_index(np.argmax(err / tol), err.shape)
        pytest.fail(f"{what} {name}: {int((err > tol).sum())} of {err.size} elements off, worst at {i}: got {got.reshape(pre.shape)[i]!r} want {ref[i]!r}, "
                    f"err {err[i]:.3e} > tol {tol[i]:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# full convolutions
# ---------------------------------------------------------------------------------------------------------------------------
def _same(n, k, s, d):
    out = -(-n // s)
    return out, max((out - 1) * s + (k - 1) * d + 1 - n, 0) // 2


def _case(name, in_h, in_w, cin, cout, kh, kw, dil, sh=1, sw=1, pad="same", out_hw=None):
    if pad == "same":
        (oh, pt), (ow, pl) = _same(in_h, kh, sh, dil[0]), _same(in_w, kw, sw, dil[1])
    else:
        (pt, pl), (oh, ow) = pad, out_hw
    return name, (in_h, in_w, oh, ow, cin, cout, kh, kw, sh, sw, pt, pl, dil[0], dil[1])


CASES = dict([
    _case("3x3_d3_on_4x5_4to4", 4, 5, 4, 4, 3, 3, (3, 3)),                      # extent 7 on 4 rows: only the middle tap row is ever inside
    _case("7x7_d2_on_5x6_36to20", 5, 6, 36, 20, 7, 7, (2, 2)),                 # extent 13
    _case("3x3_d1x2_7x9_64to68", 7, 9, 64, 68, 3, 3, (1, 2)),
    _case("3x3_d2x1_7x9_36to132", 7, 9, 36, 132, 3, 3, (2, 1)),
    _case("5x5_d2x3_7x9_4to68", 7, 9, 4, 68, 5, 5, (2, 3)),
    _case("3x3_s2_d2_7x9_36to132", 7, 9, 36, 132, 3, 3, (2, 2), 2, 2),         # stride 2 on an odd image: 4 x 5 out
    _case("3x3_s2x1_d2x3_5x6_64to20", 5, 6, 64, 20, 3, 3, (2, 3), 2, 1),
    _case("1x3_d1x2_4x5_64to20", 4, 5, 64, 20, 1, 3, (1, 2)),
    _case("3x1_d3x1_5x6_4to132", 5, 6, 4, 132, 3, 1, (3, 1)),
    _case("asym_pads_crop_d2_7x9_36to68", 7, 9, 36, 68, 3, 3, (2, 2), pad=(3, 1), out_hw=(5, 6)),    # a whole tap row above; rows and columns cropped
    _case("pad_b_past_extent_d2_4x5_4to20", 4, 5, 4, 20, 3, 3, (2, 2), pad=(0, 4), out_hw=(7, 9)),   # output rows whose every tap is outside
    _case("3x3_d16_7x9_36to4", 7, 9, 36, 4, 3, 3, (16, 16)),                   # the largest dilation: the centre tap alone
])
N_SEG = 3
_REF = {}


def _f16_valued(W):
    return W.astype(np.float16).astype(np.float32)


def _reference(name, f16w=False, n_seg=N_SEG):
    key = (name, f16w, n_seg)
    if key not in _REF:
        shape = CASES[name]
        in_h, in_w, oh, ow, cin, cout, kh, kw = shape[:8]
        rng = np.random.default_rng(sum(shape) * 11 + len(name))
        X = (rng.standard_normal((n_seg, in_h, in_w, cin)) * rng.uniform(0.2, 3.0, cin)).astype(np.float32)
        W = (rng.standard_normal((kh, kw, cin, cout)) * math.sqrt(2.0 / (kh * kw * cin))).astype(np.float32)
        if f16w:
            W = _f16_valued(W)
        b = rng.standard_normal(cout).astype(np.float32)
        b[:2] = (7.5, -7.5)
        R = rng.standard_normal((n_seg, oh, ow, cout)).astype(np.float32)
        pre, bound = conv64d(X, W, b, shape)
        _REF[key] = (X, W, b, R, pre.reshape(n_seg, oh, ow, cout), bound.reshape(n_seg, oh, ow, cout))
    return _REF[key]


BEFORE16 = [O.ACT_NONE, O.ACT_GELU_ERF, O.ACT_SWISH, O.ACT_RELU6]
AFTER16 = [O.ACT_RELU, O.ACT_RELU6, O.ACT_SWISH, O.ACT_GELU_ERF]


def _conv_params():
    """every case at terms 0, 1, 2 and 3; the residual's position (none / before / after) and the activation rotate, and one case runs
    every combination"""
    out = []
    for i, name in enumerate(CASES):
        for terms in (0, 1, 2, 3):
            pos = ("none", "before", "after")[(i + terms) % 3]
            act = (AFTER16 if pos == "after" else BEFORE16)[(i + terms) % 4]
            out.append(pytest.param(name, terms, pos, act, id=f"{name}-t{terms}-{pos}-{O.ACT_NAMES[act]}"))
    for terms in (0, 1, 2, 3):
        for pos in ("before", "after"):
            for act in (AFTER16 if pos == "after" else BEFORE16):
                out.append(pytest.param("3x3_d2x1_7x9_36to132", terms, pos, act, id=f"all-t{terms}-{pos}-{O.ACT_NAMES[act]}"))
    return out


@pytest.mark.parametrize("name,terms,pos,act", _conv_params())
def test_dilated_conv_matches_float64(name, terms, pos, act):
    shape = CASES[name]
    X, W, b, R, pre, bound = _reference(name, f16w=terms == 2)
    got, kname = _run(OP_CONV, X, W, b, None if pos == "none" else R, shape, act, terms, 1 if pos == "after" else 0)
    if terms == 0:
        assert kname.startswith("conv_gemm_kernel<BM=64,NT=") and kname.endswith(",DIL>"), kname
    else:
        assert kname == f"conv_gemm16_kernel<{terms},{AN[act]}{',AFTER' if pos == 'after' else ''},DIL>", kname
    if act == O.ACT_RELU6 and shape[5] >= 4:
        s = pre + R if pos == "after" else pre
        assert (s < 0).any() and (s > 6).any(), "operands should make ReLU6 clamp on both sides"
    _hold(got, kname, pre, bound, None if pos == "none" else R, act, pos == "after", _tau(terms, shape[6] * shape[7] * shape[4]), name)


def test_the_dilation_matters_in_every_case():
    """the float64 reference of each case differs from the undilated layer of the same record by far more than any tolerance here"""
    for name, shape in CASES.items():
        X, W, b, R, pre, bound = _reference(name)
        plain = conv64d(X, W, b, shape[:12] + (1, 1))[0].reshape(pre.shape)
        assert np.abs(plain - pre).max() > 1e-2 * np.abs(pre).max(), name


@pytest.mark.parametrize("terms", [0, 3])
def test_dilation_1_is_the_undilated_entry_bit_for_bit(terms):
    lib = _lib.load()
    name = "3x3_d2x1_7x9_36to132"
    X, W, b, R, _, _ = _reference(name)
    shape = CASES[name][:12] + (1, 1)
    for after, act in ((0, O.ACT_SWISH), (1, O.ACT_RELU6)):
        got, kname = _run(OP_CONV, X, W, b, R, shape, act, terms, after)
        want = np.empty_like(got)
        buf = C.create_string_buffer(128)
        fn = lib.bh_debug_conv_gemm_after if after else lib.bh_debug_conv_gemm
        rc = fn(0, _p(X), _p(W), _p(b), _p(R), _p(want), X.shape[0], _p(np.asarray(shape[:12], np.int32)), act, terms, buf, 128)
        assert rc == 0, lib.bh_last_error()
        assert kname == buf.value.decode() and "DIL" not in kname and (got.view(np.uint32) == want.view(np.uint32)).all(), (terms, after, kname)


@pytest.mark.parametrize("terms", [0, 3])
def test_one_nan_pixel_reaches_exactly_the_outputs_that_read_it(terms):
    for name in ("3x3_d2x1_7x9_36to132", "3x3_s2_d2_7x9_36to132", "5x5_d2x3_7x9_4to68"):
        shape = CASES[name]
        X, W, b, R, _, _ = _reference(name)
        X = X.copy()
        X[1, 2, 4, 2] = np.nan      # (an even row and column: the stride-2 dilation-2 case reads no odd one)
        pre, bound = conv64d(X, W, b, shape)
        pre, bound = pre.reshape(R.shape), bound.reshape(R.shape)
        want = np.isnan(pre)
        # whole output pixels of segment 1, not all of them, none of another segment
        assert want.any() and not want[0].any() and not want[2].any() and not want[1].all() and (want.all(axis=-1) == want.any(axis=-1)).all()
        got, kname = _run(OP_CONV, X, W, b, R, shape, O.ACT_NONE, terms, 0)
        assert (np.isnan(got) == want).all(), (name, terms, int(np.isnan(got).sum()), int(want.sum()))
        _hold(np.where(want, 0.0, got), kname, np.where(want, 0.0, pre), np.where(want, 1.0, bound), R, O.ACT_NONE, False,
              _tau(terms, shape[6] * shape[7] * shape[4]), name + " beside a NaN", ignore=want)


@pytest.mark.parametrize("terms", [0, 3])
def test_33_segments_of_three_repeated_equal_the_three(terms):
    for name in ("3x3_d1x2_7x9_64to68", "3x3_s2_d2_7x9_36to132"):
        shape = CASES[name]
        X, W, b, R, _, _ = _reference(name)
        idx = np.arange(33) % 3
        small, ks = _run(OP_CONV, X, W, b, R, shape, O.ACT_GELU_ERF, terms, 0)
        big, kb = _run(OP_CONV, np.ascontiguousarray(X[idx]), W, b, np.ascontiguousarray(R[idx]), shape, O.ACT_GELU_ERF, terms, 0)
        assert ks == kb and (big.view(np.uint32) == small.view(np.uint32)[idx]).all(), (name, terms)


def test_the_128_row_tile_of_the_dilated_f32_kernel_matches_float64():
    """conv_gemm_kernel<BM=128,NT,DIL>: a launch of 512 or more 128-row blocks (351 segments of 63 rows, three column blocks), made of
    the case's three segments repeated -- every element held to float64, and the bits those of the 64-row tile"""
    name = "3x3_d2x1_7x9_36to132"
    shape = CASES[name]
    X, W, b, R, pre, bound = _reference(name)
    idx = np.arange(351) % 3
    small, ks = _run(OP_CONV, X, W, b, R, shape, O.ACT_SWISH, 0, 0)
    big, kb = _run(OP_CONV, np.ascontiguousarray(X[idx]), W, b, np.ascontiguousarray(R[idx]), shape, O.ACT_SWISH, 0, 0)
    assert ks == "conv_gemm_kernel<BM=64,NT=3,DIL>" and kb == "conv_gemm_kernel<BM=128,NT=3,DIL>", (ks, kb)
    _hold(big, kb, pre[idx], bound[idx], R[idx], O.ACT_SWISH, False, _tau(0, shape[6] * shape[7] * shape[4]), name + " x 117")
    assert (big.view(np.uint32) == small.view(np.uint32)[idx]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# depthwise
# ---------------------------------------------------------------------------------------------------------------------------
def _dw_case(name, in_h, in_w, c, k, s, dil, act, pad="same", out_hw=None):
    if pad == "same":
        (oh, pt), (ow, pl) = _same(in_h, k, s, dil[0]), _same(in_w, k, s, dil[1])
    else:
        (pt, pl), (oh, ow) = pad, out_hw
    return name, ((in_h, in_w, oh, ow, c, c, k, k, s, s, pt, pl, dil[0], dil[1]), act)


DW_CASES = dict([
    _dw_case("dw3s1_d2_4x5_c4", 4, 5, 4, 3, 1, (2, 2), O.ACT_NONE),
    _dw_case("dw3s1_d3_4x5_c68", 4, 5, 68, 3, 1, (3, 3), O.ACT_RELU6),          # extent 7 on 4 rows
    _dw_case("dw3s2_d2x3_7x9_c12", 7, 9, 12, 3, 2, (2, 3), O.ACT_SWISH),
    _dw_case("dw5s1_d2x1_5x6_c68", 5, 6, 68, 5, 1, (2, 1), O.ACT_GELU_ERF),     # extent 9 on 5 rows
    _dw_case("dw5s2_d1x2_7x9_c4", 7, 9, 4, 5, 2, (1, 2), O.ACT_RELU),
    _dw_case("dw5s2_d2_7x9_c12_asym_crop", 7, 9, 12, 5, 2, (2, 2), O.ACT_SWISH, pad=(5, 1), out_hw=(3, 4)),
    _dw_case("dw3s2_d2_5x6_c12_pad_past", 5, 6, 12, 3, 2, (2, 2), O.ACT_NONE, pad=(0, 3), out_hw=(5, 6)),
])


def _dw_reference(name, n_seg=N_SEG):
    key = ("dw", name, n_seg)
    if key not in _REF:
        shape, act = DW_CASES[name]
        in_h, in_w, oh, ow, c, _, k = shape[:7]
        rng = np.random.default_rng(sum(shape) * 13 + len(name))
        X = (rng.standard_normal((n_seg, in_h, in_w, c)) * rng.uniform(0.2, 3.0, c)).astype(np.float32)
        W = (rng.standard_normal((k * k, c)) * math.sqrt(2.0 / (k * k))).astype(np.float32)
        b = rng.standard_normal(c).astype(np.float32)
        b[:2] = (7.5, -7.5)
        pre, bound = dw64d(X, W, b, shape)
        _REF[key] = (X, W, b, pre, bound)
    return _REF[key]


@pytest.mark.parametrize("name", sorted(DW_CASES))
def test_dilated_depthwise_matches_float64(name):
    shape, act = DW_CASES[name]
    X, W, b, pre, bound = _dw_reference(name)
    got, kname = _run(OP_DWCONV, X, W, b, None, shape, act, 0, 0)
    assert kname == f"dwconv_kernel<{shape[6]},{shape[8]},DIL>", kname
    plain = dw64d(X, W, b, shape[:12] + (1, 1))[0]
    assert np.abs(plain - pre).max() > 1e-2 * np.abs(pre).max()
    _hold(got, kname, pre, bound, None, act, False, _tau(0, shape[6] * shape[7]), name)


def test_depthwise_dilation_1_is_the_plain_layer_bit_for_bit():
    lib = _lib.load()
    shape, act = DW_CASES["dw3s2_d2x3_7x9_c12"]
    X, W, b, _, _ = _dw_reference("dw3s2_d2x3_7x9_c12")
    shape = shape[:12] + (1, 1)
    got, kname = _run(OP_DWCONV, X, W, b, None, shape, act, 0, 0)
    assert kname == "dwconv_kernel<3,2>", kname
    want = np.empty_like(got)
    buf = C.create_string_buffer(128)
    plain = np.asarray(shape[:4] + (shape[4],) + shape[6:12] + (shape[4],), np.int32)     # {in_h, in_w, out_h, out_w, c, kh, kw, sh, sw, pad_t, pad_l, .}
    rc = lib.bh_debug_plain_layer(0, OP_DWCONV, _p(X), _p(W), _p(b), None, _p(want), X.shape[0], _p(plain), act, buf, 128)
    assert rc == 0, lib.bh_last_error()
    assert buf.value.decode() == kname and (got.view(np.uint32) == want.view(np.uint32)).all()


def test_depthwise_nan_and_repeated_segments():
    name = "dw3s2_d2x3_7x9_c12"
    shape, _ = DW_CASES[name]
    X, W, b, _, _ = _dw_reference(name)
    Xn = X.copy()
    Xn[1, 2, 4, 5] = np.nan
    pre, bound = dw64d(Xn, W, b, shape)
    want = np.isnan(pre)
    assert want.any() and not want[0].any() and not want[2].any() and not want[..., :5].any() and not want[..., 6:].any() and not want[1, :, :, 5].all()
    got, kname = _run(OP_DWCONV, Xn, W, b, None, shape, O.ACT_NONE, 0, 0)
    assert (np.isnan(got) == want).all()
    _hold(np.where(want, 0.0, got), kname, np.where(want, 0.0, pre), np.where(want, 1.0, bound), None, O.ACT_NONE, False, _tau(0, 9), name + " beside a NaN", ignore=want)
    idx = np.arange(33) % 3
    small, _ = _run(OP_DWCONV, X, W, b, None, shape, O.ACT_SWISH, 0, 0)
    big, _ = _run(OP_DWCONV, np.ascontiguousarray(X[idx]), W, b, None, shape, O.ACT_SWISH, 0, 0)
    assert (big.view(np.uint32) == small.view(np.uint32)[idx]).all()


def test_the_entry_refuses_what_create_refuses():
    X, W, b, R, _, _ = _reference("3x3_d2x1_7x9_36to132")
    base = CASES["3x3_d2x1_7x9_36to132"]
    for dil in ((17, 1), (0, 1), (1, 40)):
        _, msg = _run(OP_CONV, X, W, b, None, base[:12] + dil, O.ACT_NONE, 0, 0, expect=BH_ERR_UNSUPPORTED)
        assert "dilation" in msg, msg
    one = CASES["1x3_d1x2_4x5_64to20"]
    X1, W1, b1, _, _, _ = _reference("1x3_d1x2_4x5_64to20")
    _, msg = _run(OP_CONV, X1, W1, b1, None, one[:12] + (2, 2), O.ACT_NONE, 0, 0, expect=BH_ERR_UNSUPPORTED)      # an axis with one tap
    assert "one tap" in msg, msg
    _, msg = _run(OP_CONV, X, W, b, None, base[:8] + (3, 1) + base[10:], O.ACT_NONE, 0, 0, expect=BH_ERR_UNSUPPORTED)   # stride 3
    _, msg = _run(OP_CONV, X, W, b, None, base, O.ACT_RELU, 3, 0, expect=BH_ERR_UNSUPPORTED)                    # ReLU before the add: not a split-f16 epilogue
    shape, act = DW_CASES["dw3s1_d2_4x5_c4"]
    Xd, Wd, bd, _, _ = _dw_reference("dw3s1_d2_4x5_c4")
    _, msg = _run(OP_DWCONV, Xd, Wd, bd, None, shape[:12] + (2, 17), act, 0, 0, expect=BH_ERR_UNSUPPORTED)
    assert "dilation" in msg, msg
    _, msg = _run(OP_DWCONV, Xd, Wd, bd, None, shape[:8] + (1, 2) + shape[10:], act, 0, 0, expect=BH_ERR_UNSUPPORTED)   # two strides
    assert "not built" in msg, msg


# ---------------------------------------------------------------------------------------------------------------------------
# the product path
# ---------------------------------------------------------------------------------------------------------------------------
def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def _expected_kernel(L, prec):
    """what bh_debug_layer_kernel names for a dilated layer: the dilated depthwise form in every mode; the split-f16 instantiation of a
    full convolution above 64 output channels whose activation that epilogue has, nothing ('') for one on the f32 kernel"""
    if L.op == mf.OP_DWCONV:
        return f"dwconv_kernel<{L.kh},{L.sh},DIL>"
    after = L.reserved == mf.RES_ACT_AFTER
    if prec == "f32" or L.cout <= 64 or L.act not in (AFTER16 if after else BEFORE16):
        return ""
    return f"conv_gemm16_kernel<3,{AN[L.act]}{',AFTER' if after else ''},DIL>"


def test_dilated_plan_on_both_routes(tmp_path):
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("dilated_plan")
    onnx = _write(str(tmp_path / "d.onnx"), convert.model_to_onnx(m, frontend_spelling="stft"))
    # the .bhm route: the container the library's reader writes of that file -- the same records (tests/test_dilated.py) and the same
    # front end, so the same bits.  synth's own container is held to the tolerance only: the mel matrix a reader recovers from the
    # STFT graph differs from synth's in its last bit (9e-9 of an entry; the front end is as it was), and so do the logits.
    bhm, own = str(tmp_path / "d.bhm"), str(tmp_path / "own.bhm")
    assert _lib.load().bh_onnx_to_bhm(onnx.encode(), bhm.encode()) == 0, _lib.load().bh_last_error()
    assert [(L.dil_h, L.dil_w) for L in mf.read_model(bhm).layers] == [(L.dil_h, L.dil_w) for L in m.layers]
    mf.write_model(own, m)
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=7)
    segs[2] *= np.float32(0.01)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    D = dilated(m)
    for prec in ("f32", "f16x3", "auto"):
        first = None
        for route, path in (("onnx", onnx), ("bhm", bhm), ("own", own)):
            clf = BirdClassifier(path, None, precision=prec)
            assert clf.fused_blocks() == []                       # the block with the dilated depthwise runs layer by layer
            for n in (3, 80, 300) if route == "onnx" else (3,):
                ctx = clf.create_batch_context(n)
                ctx.set_sub_slices(1)
                got = clf.predict_logits(ctx, np.ascontiguousarray(segs[np.arange(n) % 3]))
                ctx.close()
                if first is None:
                    first = got
                    err = float(np.abs(got - ref).max())
                    print(f"dilated_plan {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
                    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale, (prec, err, scale)
                elif route == "own":
                    err = float(np.abs(got - ref).max())
                    print(f"dilated_plan {prec}, synth's container: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
                    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale, (prec, err, scale)
                else:
                    assert (got.view(np.uint32) == first.view(np.uint32)[np.arange(n) % 3]).all(), (prec, route, n)
            names = {i: clf.layer_kernel(i) for i in D}
            assert names == {i: _expected_kernel(m.layers[i], prec) for i in D}, (prec, route, names)
            if prec != "f32":
                assert sum(k.startswith("conv_gemm16_kernel") for k in names.values()) >= 6 and any("AFTER" in k for k in names.values())
            clf.close()


def test_f16_overflow_in_front_of_a_dilated_layer_reaches_the_logits(tmp_path):
    """tests/test_resact_gpu.py's recipe on dilated layers: a LINEAR dilated convolution whose weights and bias carry 2^20 (its
    output is past 65 504) in front of a dilated convolution whose weights carry 2^-20 -- the same function in f32 arithmetic.  The
    split-f16 kernel cannot represent its operand: f16x3 ends in BH_ERR_NONFINITE, auto re-runs the rows on the f32 kernels."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    b = synth._Builder(np.random.default_rng(13))
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    t1, h, w = b.conv(0, br.n_mels, br.n_frames, 1, 72, 3, 2, mf.ACT_GELU_ERF, in_layout=1)
    t2, h, w = b.conv(t1, h, w, 72, 72, 3, 1, mf.ACT_NONE, dil=(2, 2))
    t3, h, w = b.conv(t2, h, w, 72, 72, 3, 1, mf.ACT_SWISH, res=t1, gain=0.5, dil=(2, 3))
    t = b.pwconv(t3, h, w, 72, 64, mf.ACT_GELU_ERF)
    t = emb = b.gap(t, h, w, 64)
    b.dense(t, 64, 30, gain=1.5)
    m0 = mf.Model(0, sr, n, n / sr, 30, 64, mf.OUT_SIGMOID, emb, br.n_mels, br.n_frames, 1e-6, [br], b.layers, np.concatenate(b.chunks))
    m = copy.deepcopy(m0)
    blob = m.blob.copy()
    Lin, Nx = m.layers[1], m.layers[2]
    s = np.float32(2.0 ** 20)
    blob[Lin.w_off:Lin.w_off + Lin.kh * Lin.kw * Lin.cin * Lin.cout] *= s
    blob[Lin.b_off:Lin.b_off + Lin.cout] *= s
    blob[Nx.w_off:Nx.w_off + Nx.kh * Nx.kw * Nx.cin * Nx.cout] /= s
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
    assert clf.layer_kernel(2) == "conv_gemm16_kernel<3,SWISH,DIL>", clf.layer_kernel(2)
    ctx.close(); clf.close()
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(4)
    got = clf.predict_logits(ctx, segs)
    assert clf.fallback_segments() > 0
    err = float(np.abs(got - ref).max())
    print(f"overflow in front of a dilated layer, auto: max|dlogit| = {err:.3e} of {scale:.2f}, {clf.fallback_segments()} segments re-run")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    ctx.close(); clf.close()


def test_dilated_resnet_audio_runs_and_matches_float64(tmp_path):
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("dilated_resnet_audio", n_classes=40)
    D = dilated(m)
    assert len(D) == 8 and [m.layers[i].dil_h for i in D] == [2, 2, 2, 2, 4, 4, 4, 4]
    path = str(tmp_path / "drn.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=2)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(2)
    got = clf.predict_logits(ctx, segs)
    ctx.close()
    err = float(np.abs(got - ref).max())
    print(f"dilated_resnet_audio auto: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    # ReLU before the add is no split-f16 epilogue (the first 3x3 of a block: f32 kernel); the flagged second one is, and so is the
    # linear one in front of a projection shortcut
    names = {i: clf.layer_kernel(i) for i in D}
    assert names == {i: _expected_kernel(m.layers[i], "auto") for i in D}, names
    assert sorted(set(names.values())) == ["", "conv_gemm16_kernel<3,NONE,DIL>", "conv_gemm16_kernel<3,RELU,AFTER,DIL>"], names
    clf.close()
