"""ConvNeXt layers on the device.

lnorm_kernel through bh_debug_lnorm (include/birda_hip_lnorm_debug.h), every output element against float64 (tests/test_convnext.py
lnorm64) under the first-order bound

    |got - ref| <= tau (|gamma| (2 |xhat| + (|x| + |mean|) / sigma) + |beta|),   tau = 4e-7 max(1, sqrt(C / 1024))

(the mean carries a few ulps of mean|x|, x - mean therefore u (|x| + |mean|), 1 / sigma a few ulps; tau and its width rule are those of
tests/test_layer_gemm_gpu.py) at C in {4, 36, 96, 100, 260, 768, 2048} x 1 and 105 pixels (3 segments of 5 x 7: no multiple of any
pixels-per-workgroup; 25 float4s are no power of two, 65 one past a wave, one leaves most of a group idle), on unit-scale data and on
the same data with a per-pixel offset of 100 -- where E[x^2] - mean^2 in float32 misses the bound by orders of magnitude
(tests/test_convnext.py shows that on the CPU).  Every element is written, the guard bands stay; 33 segments made of three repeated
equal the three bit for bit; a NaN and an inf make exactly their own pixels NaN; a constant pixel gives beta bit for bit; C = 6 and
C = 2052 are refused.

dwconv_kernel<7,1|2[,DIL]> through bh_debug_dilated_layer -- at dilation 1 the plain layer's launch, bits and name; bh_debug_plain_layer
keeps the 3x3 / 5x5 windows it always took, because tests/test_gate_layers_gpu.py holds it to refusing a 7x7 one -- under that file's
rule, tau(kh kw) 1.2 bound + eps_act with bound = sum |tap| |w| + |b|.

At model level synth's convnext_plan runs through the .onnx route -- PyTorch spellings, un-folded layer scale -- and the .bhm route
to the same bits, within 2e-5 of the logit scale of forward64 in f32, f16x3 and auto, the same bits at 3, 80 and 300 segments, with
lnorm_kernel and dwconv_kernel<7,1> where expected and no fused block; the embedding is the head LayerNorm's output; an f16 overflow
in front of a LayerNorm ends in BH_ERR_NONFINITE (f16x3) and is re-run (auto); convnext_audio at 40 classes is held to the bound once.

Measured on the MI355X, worst err / tolerance (every test prints its own): lnorm_kernel 0.20 on unit-scale data, 0.12 with the offset
(an all-float32 mean, emulated on these inputs, reaches 1.24 at C = 768: kernels_lnorm.hip accumulates the mean in float64);
dwconv_kernel<7,1> 0.41, <7,2> 0.44, the DIL forms 0.38; convnext_plan 0.04 of the logit bound in f32 and 0.03 in f16x3 / auto,
convnext_audio 0.03."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from birda_amd import _lib, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O
from test_convnext import forward64, lnorm64, lnorm_tol, torch_graph
from test_dilated import dw64d

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
BH_ERR_UNSUPPORTED, BH_ERR_NONFINITE = -6, -8
LOGIT_RTOL = 2e-5
OP_DWCONV = 2


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------
WIDTHS = (4, 36, 96, 100, 260, 768, 2048)
PIXELS = (1, 105)


def lnorm_form(C_):
    """kernels_lnorm.hip: (lanes a pixel, float4s a lane) -- the fewest idle float4 slots, the wider group on a tie"""
    c4n, best, form = C_ // 4, 1 << 30, None
    for g in (8, 16, 32, 64):
        nv = -(-c4n // g)
        if nv <= 8 and g * nv - c4n <= best:
            best, form = g * nv - c4n, (g, nv)
    return form


def run_lnorm(X, gamma, beta, eps, expect=0):
    lib = _lib.load()
    n, C_ = X.shape
    out = np.empty((n, C_), np.float32)
    name = C.create_string_buffer(b"untouched", 128)
    rc = lib.bh_debug_lnorm(0, _p(X), _p(gamma), _p(beta), C.c_float(eps), _p(out), n, C_, name, 128)
    if expect:
        assert rc == expect and name.value == b"untouched", (rc, lib.bh_last_error())
        return None, lib.bh_last_error().decode()
    assert rc == 0, (rc, lib.bh_last_error())
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"       # (the guards are checked by the entry itself)
    return out, name.value.decode()


def operands(C_, pixels, offset, seed=0):
    rng = np.random.default_rng(1000 * C_ + pixels + seed)
    X = rng.standard_normal((pixels, C_)).astype(np.float32)
    if offset:
        X = (X + (100.0 + rng.standard_normal((pixels, 1)))).astype(np.float32)           # a per-pixel offset of 100 at unit spread
    gamma = rng.standard_normal(C_).astype(np.float32)
    gamma[rng.integers(0, C_)] = 0.0
    gamma[rng.integers(0, C_)] = -abs(gamma[rng.integers(0, C_)]) - np.float32(0.5)
    beta = rng.standard_normal(C_).astype(np.float32)
    return X, gamma, beta, (1e-5, 1e-6)[(C_ // 4 + pixels) % 2]


@pytest.mark.parametrize("pixels", PIXELS)
@pytest.mark.parametrize("C_", WIDTHS)
def test_lnorm_against_float64(C_, pixels):
    tau = 4e-7 * max(1.0, math.sqrt(C_ / 1024.0))
    for offset in (False, True):
        X, gamma, beta, eps = operands(C_, pixels, offset)
        got, name = run_lnorm(X, gamma, beta, eps)
        assert name == "lnorm_kernel<%d,%d>" % lnorm_form(C_), name
        ref, tol = lnorm64(X, gamma, beta, eps), lnorm_tol(X, gamma, beta, eps, tau)
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - ref)
        share = float(np.max(err / np.maximum(tol, 1e-300)))
        print(f"lnorm C {C_} pixels {pixels} {'offset 100' if offset else 'unit scale'} eps {eps:g} {name}: worst err / tol {share:.3f}")
        if share > 1.0:
            i = np.unravel_index(np.argmax(err / np.maximum(tol, 1e-300)), err.shape)
            pytest.fail(f"C {C_} pixels {pixels} offset {offset}: {int((err > tol).sum())} of {err.size} elements off, worst at {i}: got {got[i]!r} "
                        f"want {ref[i]!r}, err {err[i]:.3e} > tol {tol[i]:.3e}")


@pytest.mark.parametrize("C_", WIDTHS)
def test_a_pixel_does_not_depend_on_its_launch(C_):
    """33 segments made of three repeated (1 155 pixels) against the three (105 pixels), bit for bit; and pixel by pixel alone"""
    X, gamma, beta, eps = operands(C_, 105, True)
    small, _ = run_lnorm(X, gamma, beta, eps)
    big, _ = run_lnorm(np.ascontiguousarray(np.tile(X.reshape(3, 35, C_), (11, 1, 1)).reshape(-1, C_)), gamma, beta, eps)
    assert (big.view(np.uint32).reshape(11, 105, C_) == small.view(np.uint32)).all()
    assert not np.array_equal(small[0], small[1])
    one, _ = run_lnorm(np.ascontiguousarray(X[17:18]), gamma, beta, eps)
    assert (one.view(np.uint32) == small.view(np.uint32)[17:18]).all()


@pytest.mark.parametrize("C_", WIDTHS)
def test_a_nan_and_an_inf_stay_in_their_pixels(C_):
    X, gamma, beta, eps = operands(C_, 105, False)
    clean, _ = run_lnorm(X, gamma, beta, eps)
    Xn = X.copy()
    Xn[10, C_ // 2] = np.nan
    Xn[50, C_ - 1] = np.inf
    Xn[77, 0] = -np.inf
    got, _ = run_lnorm(Xn, gamma, beta, eps)
    bad = np.zeros(105, bool)
    bad[[10, 50, 77]] = True
    assert np.isnan(got[bad]).all()                                  # every channel, gamma == 0 included
    assert (got.view(np.uint32)[~bad] == clean.view(np.uint32)[~bad]).all()


@pytest.mark.parametrize("C_", WIDTHS)
def test_a_constant_pixel_gives_beta(C_):
    _, gamma, beta, eps = operands(C_, 1, False)
    values = np.asarray([0.0, 0.1, -7.7, 100.3, 1e-3, 65504.0, 3.0e6, -1e-20, 1.0 / 3.0], np.float32)
    X = np.ascontiguousarray(np.broadcast_to(values[:, None], (values.size, C_)))
    got, _ = run_lnorm(X, gamma, beta, eps)
    assert (got.view(np.uint32) == np.broadcast_to(beta, got.shape).view(np.uint32)).all(), np.argwhere(got != beta)[:4]


def test_widths_the_kernel_does_not_take_are_refused():
    for C_ in (6, 2052):
        X = np.zeros((3, C_), np.float32)
        _, msg = run_lnorm(X, np.ones(C_, np.float32), np.zeros(C_, np.float32), 1e-5, expect=BH_ERR_UNSUPPORTED)
        assert "not built" in msg, msg
    _, msg = run_lnorm(np.zeros((3, 8), np.float32), np.ones(8, np.float32), np.zeros(8, np.float32), 0.0, expect=-1)       # BH_ERR_INVALID
    assert "eps" in msg


def test_create_refuses_a_width_the_kernel_does_not_take(tmp_path):
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    b = synth._Builder(np.random.default_rng(3))
    base = synth.build_model("mini")
    br = [copy.deepcopy(x) for x in base.branches]
    for x in br:
        x.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(x.n_mels, x.n_bins, base.sample_rate, x.fmin, x.fmax))
    t, h, w = b.conv(0, 32, 115, 2, 8, 4, 4, mf.ACT_NONE, in_layout=1)
    t = b.pwconv(t, h, w, 8, 2052, mf.ACT_NONE)
    t = b.lnorm(t, h, w, 2052)
    t = emb = b.gap(t, h, w, 2052)
    b.dense(t, 2052, 8)
    m = synth._finish(b, br, base.sample_rate, base.sample_count, 8, 2052, emb, mf.OUT_SIGMOID)
    path = str(tmp_path / "wide.bhm")
    mf.write_model(path, m)
    with pytest.raises(BirdaHipError) as e:
        BirdClassifier(path, None, precision="f32")
    assert e.value.code == BH_ERR_UNSUPPORTED and "layer norm" in str(e.value) and "not built" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------
# depthwise 7x7
# ---------------------------------------------------------------------------------------------------------------------------
def _tau(k_eff):
    return 4e-7 * max(1.0, math.sqrt(k_eff / 1024.0))


def _eps_act(s, act):
    return 5e-7 * np.maximum(np.abs(s), 1.0) if act == O.ACT_GELU_ERF else np.zeros_like(s)


def _same(n, k, s, d=1):
    out = -(-n // s)
    return out, max((out - 1) * s + (k - 1) * d + 1 - n, 0) // 2


def _dw(name, in_h, in_w, c, k, s, act, dil=(1, 1), pad="same", out_hw=None):
    if pad == "same":
        (oh, pt), (ow, pl) = _same(in_h, k, s, dil[0]), _same(in_w, k, s, dil[1])
    else:
        (pt, pl), (oh, ow) = pad, out_hw
    return name, ((in_h, in_w, oh, ow, c, c, k, k, s, s, pt, pl, dil[0], dil[1]), act)


DW_CASES = dict([
    _dw("dw7s1_4x5_c4", 4, 5, 4, 7, 1, O.ACT_NONE),                                        # the window is larger than the image
    _dw("dw7s1_4x5_c36_gelu", 4, 5, 36, 7, 1, O.ACT_GELU_ERF),
    _dw("dw7s1_7x9_c36", 7, 9, 36, 7, 1, O.ACT_NONE),
    _dw("dw7s1_7x9_c100_gelu", 7, 9, 100, 7, 1, O.ACT_GELU_ERF),
    _dw("dw7s2_7x9_c4_gelu", 7, 9, 4, 7, 2, O.ACT_GELU_ERF),                               # stride 2 on an odd image
    _dw("dw7s2_7x9_c100", 7, 9, 100, 7, 2, O.ACT_NONE),
    _dw("dw7s1_7x9_c36_asym_cropped", 7, 9, 36, 7, 1, O.ACT_NONE, pad=(2, 5), out_hw=(4, 8)),   # pads (2, 5) top / left, 7 + 2 + 3 - 7 + 1 = 6 rows cropped to 4
    _dw("dw7s2_7x9_c36_asym", 7, 9, 36, 7, 2, O.ACT_GELU_ERF, pad=(1, 4), out_hw=(3, 4)),
    _dw("dw7s1_d2x3_7x9_c36", 7, 9, 36, 7, 1, O.ACT_NONE, dil=(2, 3)),                      # extent 13 x 19
    _dw("dw7s2_d2x3_7x9_c4_gelu", 7, 9, 4, 7, 2, O.ACT_GELU_ERF, dil=(2, 3)),
])


def _dw_operands(name, n=3):
    shape, act = DW_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    X = rng.standard_normal((n, shape[0], shape[1], shape[4])).astype(np.float32)
    W = (rng.standard_normal((shape[6] * shape[7], shape[4])) / 7.0).astype(np.float32)
    b = (0.1 * rng.standard_normal(shape[4])).astype(np.float32)
    return X, W, b


def run_dw(name, X, W, b, act, entry="auto"):
    """a 7x7 window, dilated or not: bh_debug_dilated_layer; a 3x3 / 5x5 one at dilation 1: bh_debug_plain_layer (entry = "dilated" takes
    the other entry for it) -> (Y [n][oh][ow][c], the instantiation's name)"""
    lib = _lib.load()
    shape, _ = DW_CASES[name] if isinstance(name, str) else (name, None)
    n = X.shape[0]
    Y = np.empty((n, shape[2], shape[3], shape[4]), np.float32)
    buf = C.create_string_buffer(128)
    if (shape[12], shape[13]) == (1, 1) and shape[6] != 7 and entry != "dilated":
        plain = np.asarray(shape[:4] + (shape[4],) + shape[6:12] + (shape[4],), np.int32)     # {in_h, in_w, out_h, out_w, c, kh, kw, sh, sw, pad_t, pad_l, cin}
        rc = lib.bh_debug_plain_layer(0, OP_DWCONV, _p(X), _p(W), _p(b), None, _p(Y), n, _p(plain), act, buf, 128)
    else:
        rc = lib.bh_debug_dilated_layer(0, OP_DWCONV, _p(X), _p(W), _p(b), None, _p(Y), n, _p(np.asarray(shape, np.int32)), act, 0, 0, buf, 128)
    assert rc == 0, (rc, lib.bh_last_error())
    assert not (Y.view(np.uint32) == UNWRITTEN).any(), "elements never written"
    return Y, buf.value.decode()


def _hold_dw(got, name, pre, bound, act, what, ignore=None):
    ref = O.act64(pre, act)
    tol = _tau(49) * 1.2 * bound + _eps_act(pre, act)
    err = np.abs(got.astype(np.float64) - ref)
    if ignore is not None:
        err, tol = np.where(ignore, 0.0, err), np.where(ignore, 1.0, tol)
    assert np.isfinite(err).all(), (what, "non-finite output")
    share = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{what} {name} act {O.ACT_NAMES[act]}: worst err / tol {share:.3f}")
    if share > 1.0:
        i = np.unravel_index(np.argmax(err / tol), err.shape)
        pytest.fail(f"{what} {name}: {int((err > tol).sum())} of {err.size} elements off, worst at {i}: got {got[i]!r} want {ref[i]!r}, err {err[i]:.3e} > tol {tol[i]:.3e}")


@pytest.mark.parametrize("case", sorted(DW_CASES))
def test_depthwise_7x7_against_float64(case):
    shape, act = DW_CASES[case]
    X, W, b = _dw_operands(case)
    pre, bound = dw64d(X, W, b, shape)
    got, name = run_dw(case, X, W, b, act)
    assert name == "dwconv_kernel<7,%d%s>" % (shape[8], ",DIL" if (shape[12], shape[13]) != (1, 1) else ""), name
    _hold_dw(got, name, pre, bound, act, case)
    if case == "dw7s1_4x5_c4":
        assert shape[6] > shape[0] and shape[7] > shape[1]


def test_depthwise_7x7_nan_and_repeated_segments():
    case = "dw7s2_7x9_c100"
    shape, act = DW_CASES[case]
    X, W, b = _dw_operands(case)
    Xn = X.copy()
    Xn[1, 5, 8, 41] = np.nan
    pre, bound = dw64d(Xn, W, b, shape)
    want = np.isnan(pre)
    assert want.any() and not want[0].any() and not want[2].any() and not want[..., :41].any() and not want[..., 42:].any() and not want[1, :, :, 41].all()
    got, name = run_dw(case, Xn, W, b, act)
    assert (np.isnan(got) == want).all()                      # exactly the outputs whose taps read the pixel
    _hold_dw(np.where(want, 0.0, got), name, np.where(want, 0.0, pre), np.where(want, 1.0, bound), act, case + " beside a NaN", ignore=want)
    idx = np.arange(33) % 3
    small, _ = run_dw(case, X, W, b, O.ACT_GELU_ERF)
    big, _ = run_dw(case, np.ascontiguousarray(X[idx]), W, b, O.ACT_GELU_ERF)
    assert (big.view(np.uint32) == small.view(np.uint32)[idx]).all()


def test_the_3x3_and_5x5_instantiations_keep_their_names():
    rng = np.random.default_rng(5)
    for k, s in ((3, 1), (5, 2)):
        (oh, pt), (ow, pl) = _same(7, k, s), _same(9, k, s)
        shape = (7, 9, oh, ow, 12, 12, k, k, s, s, pt, pl, 1, 1)
        X = rng.standard_normal((2, 7, 9, 12)).astype(np.float32)
        W = (rng.standard_normal((k * k, 12)) / k).astype(np.float32)
        b = rng.standard_normal(12).astype(np.float32)
        got, name = run_dw(shape, X, W, b, O.ACT_NONE)
        assert name == f"dwconv_kernel<{k},{s}>", name
        pre, bound = dw64d(X, W, b, shape)
        assert (np.abs(got - pre) <= _tau(k * k) * 1.2 * bound).all()
        same, name2 = run_dw(shape, X, W, b, O.ACT_NONE, entry="dilated")       # the entry the 7x7 window takes: the same launch
        assert name2 == name and (same.view(np.uint32) == got.view(np.uint32)).all()


def test_the_plain_entry_keeps_refusing_a_7x7_window():
    """bh_debug_plain_layer is what it was (tests/test_gate_layers_gpu.py): 7x7 is refused there by name, and nothing is launched"""
    lib = _lib.load()
    shape, act = DW_CASES["dw7s1_7x9_c36"]
    X, W, b = _dw_operands("dw7s1_7x9_c36")
    Y = np.zeros((3, shape[2], shape[3], shape[4]), np.float32)
    buf = C.create_string_buffer(b"untouched", 128)
    plain = np.asarray(shape[:4] + (shape[4],) + shape[6:12] + (shape[4],), np.int32)
    rc = lib.bh_debug_plain_layer(0, OP_DWCONV, _p(X), _p(W), _p(b), None, _p(Y), 3, _p(plain), act, buf, 128)
    msg = lib.bh_last_error().decode()
    assert rc == BH_ERR_UNSUPPORTED and "depthwise 7x7" in msg and "bh_debug_dilated_layer" in msg, (rc, msg)
    assert not Y.any() and buf.value == b"untouched"


# ---------------------------------------------------------------------------------------------------------------------------
# the product path
# ---------------------------------------------------------------------------------------------------------------------------
def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def test_convnext_plan_on_both_routes(tmp_path):
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("convnext_plan", seed=1)
    # the .onnx route: the PyTorch spellings -- Transpose / LayerNormalization / MatMul + Add / Gelu / Mul by the un-folded layer scale
    onnx = _write(str(tmp_path / "c.onnx"), ox.dump(torch_graph(m, frontend="stft")))
    # the .bhm route: the container the library's reader writes of that file -- the same records (tests/test_convnext.py) and the
    # same front end, so the same bits; synth's own container is held to the tolerance only (its mel matrix differs in the last bit)
    bhm, own = str(tmp_path / "c.bhm"), str(tmp_path / "own.bhm")
    assert _lib.load().bh_onnx_to_bhm(onnx.encode(), bhm.encode()) == 0, _lib.load().bh_last_error()
    assert [L.op for L in mf.read_model(bhm).layers] == [L.op for L in m.layers]
    mf.write_model(own, m)
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=7)
    segs[2] *= np.float32(0.01)
    T = forward64(m, segs, tensors=True)
    ref = T[-1].reshape(3, -1)
    scale = max(1.0, float(np.abs(ref).max()))
    norms = [i for i, L in enumerate(m.layers) if L.op == mf.OP_LNORM]
    dws = [i for i, L in enumerate(m.layers) if L.op == mf.OP_DWCONV]
    head = m.layers[-1]
    Wd, bd = m.blob[head.w_off:head.w_off + head.cin * head.cout].reshape(head.cin, head.cout).astype(np.float64), m.blob[head.b_off:head.b_off + head.cout]
    for prec in ("f32", "f16x3", "auto"):
        first = None
        for route, path in (("onnx", onnx), ("bhm", bhm), ("own", own)):
            clf = BirdClassifier(path, None, precision=prec)
            assert clf.fused_blocks() == []                       # pw -> dw -> LayerNorm is no inverted-residual block
            for n in (3, 80, 300) if route == "onnx" else (3,):
                ctx = clf.create_batch_context(n)
                ctx.set_sub_slices(1)
                got, emb = clf.predict_logits(ctx, np.ascontiguousarray(segs[np.arange(n) % 3]), want_embeddings=True)
                ctx.close()
                if first is None:
                    first = got
                    err = float(np.abs(got - ref).max())
                    print(f"convnext_plan {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
                    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale, (prec, err, scale)
                    # the embedding is the head LayerNorm's output: what the dense head reads, not the pooled tensor in front of it
                    want_emb = np.asarray(T[m.embedding_tensor]).reshape(3, -1)
                    pooled = np.asarray(T[m.embedding_tensor - 1]).reshape(3, -1)
                    e_err = float(np.abs(emb - want_emb).max())
                    print(f"convnext_plan {prec}: max|dembedding| = {e_err:.3e} (the pooled tensor is {float(np.abs(pooled - want_emb).max()):.2f} away)")
                    assert emb.shape == (3, head.cin) and e_err <= 1e-3 and np.abs(pooled - want_emb).max() > 0.1
                    assert np.abs(emb.astype(np.float64) @ Wd + bd - got).max() <= LOGIT_RTOL * scale
                elif route == "own":
                    err = float(np.abs(got - ref).max())
                    print(f"convnext_plan {prec}, synth's container: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
                    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale, (prec, err, scale)
                else:
                    assert (got.view(np.uint32) == first.view(np.uint32)[np.arange(n) % 3]).all(), (prec, route, n)
            names = {i: clf.layer_kernel(i) for i in norms + dws}
            assert all(names[i] == "lnorm_kernel<%d,%d>" % lnorm_form(m.layers[i].cout) for i in norms), (prec, route, names)
            assert all(names[i] == "dwconv_kernel<7,1>" for i in dws), (prec, route, names)
            clf.close()


def test_every_norm_tensor_is_the_norm_of_its_input_in_a_model(tmp_path, monkeypatch):
    """BIRDA_HIP_KEEP_TENSORS, f32: every LayerNorm record's tensor, read back, is lnorm64 of its input tensor read back the same way,
    under the kernel's own bound; and the 7x7 depthwise outputs hold dw64d of theirs"""
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("convnext_plan", seed=1)
    path = str(tmp_path / "k.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=7)
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    clf = BirdClassifier(path, None, precision="f32")
    ctx = clf.create_batch_context(3)
    clf.predict_logits(ctx, segs)
    worst = 0.0
    for i, L in enumerate(m.layers):
        if L.op == mf.OP_LNORM:
            X = clf.read_tensor(ctx, L.in_tensor, 3).reshape(-1, L.cout)
            Y = clf.read_tensor(ctx, i + 1, 3).reshape(-1, L.cout)
            g, b, eps = m.blob[L.w_off:L.w_off + L.cout], m.blob[L.b_off:L.b_off + L.cout], mf.lnorm_eps(L.reserved)
            share = float(np.max(np.abs(Y - lnorm64(X, g, b, eps)) / lnorm_tol(X, g, b, eps, 4e-7)))
            worst = max(worst, share)
            assert share <= 1.0, (i, share)
        elif L.op == mf.OP_DWCONV:
            X = clf.read_tensor(ctx, L.in_tensor, 3).reshape(3, L.in_h, L.in_w, L.cout)
            Y = clf.read_tensor(ctx, i + 1, 3).reshape(3, L.out_h, L.out_w, L.cout)
            pre, bound = dw64d(X, m.blob[L.w_off:L.w_off + 49 * L.cout].reshape(49, L.cout), m.blob[L.b_off:L.b_off + L.cout],
                               (L.in_h, L.in_w, L.out_h, L.out_w, L.cout, L.cout, 7, 7, 1, 1, L.pad_t, L.pad_l, 1, 1))
            assert (np.abs(Y - pre) <= _tau(49) * 1.2 * bound).all(), i
    print(f"convnext_plan, kept tensors: worst LayerNorm err / tol {worst:.3f}")
    ctx.close(); clf.close()


def test_f16_overflow_in_front_of_a_layer_norm_reaches_the_logits(tmp_path):
    """tests/test_dilated_gpu.py's recipe with a LayerNorm behind it: a LINEAR convolution whose weights and bias carry 2^20 (its
    output is past 65 504) in front of a convolution whose weights carry 2^-20 -- the same function in f32 arithmetic.  The split-f16
    kernel cannot represent its operand, and the non-finite pixels it writes must pass THROUGH the LayerNorm (every channel of such a
    pixel NaN) to the logits: f16x3 ends in BH_ERR_NONFINITE, auto re-runs the rows on the f32 kernels."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    b = synth._Builder(np.random.default_rng(13))
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    t1, h, w = b.conv(0, br.n_mels, br.n_frames, 1, 72, 3, 2, mf.ACT_GELU_ERF, in_layout=1)
    t2, h, w = b.conv(t1, h, w, 72, 72, 3, 1, mf.ACT_NONE)
    t3, h, w = b.conv(t2, h, w, 72, 72, 3, 1, mf.ACT_NONE, gain=0.5)
    t = b.lnorm(t3, h, w, 72, 1e-6)
    t = b.pwconv(t, h, w, 72, 64, mf.ACT_GELU_ERF)
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
    assert clf.layer_kernel(2) == "conv_gemm16_kernel<3,NONE>", clf.layer_kernel(2)
    assert clf.layer_kernel(3) == "lnorm_kernel<%d,%d>" % lnorm_form(72)
    ctx.close(); clf.close()
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(4)
    got = clf.predict_logits(ctx, segs)
    assert clf.fallback_segments() > 0
    err = float(np.abs(got - ref).max())
    print(f"overflow in front of a LayerNorm, auto: max|dlogit| = {err:.3e} of {scale:.2f}, {clf.fallback_segments()} segments re-run")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    ctx.close(); clf.close()


def test_convnext_audio_runs_and_matches_float64(tmp_path):
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("convnext_audio", n_classes=40)
    path = str(tmp_path / "cnx.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=2)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    clf = BirdClassifier(path, None, precision="auto")
    assert clf.fused_blocks() == []
    ctx = clf.create_batch_context(2)
    got = clf.predict_logits(ctx, segs)
    ctx.close()
    err = float(np.abs(got - ref).max())
    print(f"convnext_audio auto: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    names = {clf.layer_kernel(i) for i, L in enumerate(m.layers) if L.op in (mf.OP_LNORM, mf.OP_DWCONV)}
    assert names == {"dwconv_kernel<7,1>"} | {"lnorm_kernel<%d,%d>" % lnorm_form(c) for c in (96, 192, 384, 768)}, names
    clf.close()
