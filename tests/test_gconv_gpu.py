"""Grouped convolutions (OP_GCONV) on the device: the three instantiations behind launch_gconv / launch_gconv16 -- gconv_kernel (f32
MFMA), gconv16_kernel<3> (split f16) and gconv16_kernel<1> (plain f16) -- alone through bh_debug_gconv, element by element against
float64, and inside models through bh_classifier_create.

Every output element is held to the inequality of tests/test_layer_gemm_gpu.py, with its tau, eps_act and operand recipe:

    |got - ref| <= tau 1.2 bound + eps_act(pre),   bound = |A| |W| + |b| in float64 over the GROUP'S OWN K (kh kw cin / G),

tau = 4e-7 max(1, sqrt(k_eff / 1024)) for terms 0 and 3, 1.5e-3 for terms 1, k_eff = kh kw cin / G.  The shapes are the smallest that
reach every path of the per-tile layout: a column tile inside one group (widths 16, 32), a tile of several groups (4, 8), a tile that
straddles two groups and a partial last tile (24 x 3 = 72 columns), unequal in / out widths; 5 x 7 and 9 x 11 images in three
segments (105 and 297 rows: partial row tiles, segment seams inside a tile).  Beyond the tolerance: the isolation test (a wrong span
or a misplaced weight block shows in the bits), the non-finite contract stated beside the kernels, launch independence, and the
product path on the .onnx route against the float64 forward of tests/test_gconv.py.
"""
import copy
import ctypes as C
import types

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O
from test_gconv import forward64, gconv_pre64
from test_layer_gemm_gpu import _eps_act, _operands, _tau
from test_resact_gpu import BH_ERR_NONFINITE, F16_LOGIT_RTOL, LOGIT_RTOL

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
KERNEL_OF = {0: "gconv_kernel", 3: "gconv16_kernel<3>", 1: "gconv16_kernel<1>"}
ACTS16 = [O.ACT_NONE, O.ACT_RELU, O.ACT_SWISH, O.ACT_GELU_ERF]
ACTS32 = ACTS16 + [O.ACT_RELU6, O.ACT_GELU_TANH, O.ACT_SIGMOID]            # every code of the f32 layer kernels' run-time switch
REACHED = set()
WORST = {}                 # (kernel, terms) -> worst (err - eps_act) / (1.2 bound)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _gconv(X, W, b, shape, act, terms, expect=0):
    """shape = (in_h, in_w, out_h, out_w, cin, cout, kh, kw, sh, sw, pad_t, pad_l, groups) -> (C [n out_h out_w][cout], kernel name)"""
    lib = _lib.load()
    n = X.shape[0]
    out = np.empty((n * shape[2] * shape[3], shape[5]), np.float32)
    sh = np.asarray(shape, np.int32)
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_gconv(0, _p(X), _p(W), _p(b), _p(out), n, _p(sh), act, terms, name, 128)
    if expect:
        assert rc == expect, (rc, lib.bh_last_error())
        return None, lib.bh_last_error().decode()
    assert rc == 0, (rc, lib.bh_last_error())
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"
    REACHED.add(name.value.decode())
    return out, name.value.decode()


def _rec(shape):
    """the shape as the record gconv_pre64 reads"""
    in_h, in_w, oh, ow, cin, cout, kh, kw, sh, sw, pt, pl, G = shape
    return types.SimpleNamespace(in_h=in_h, in_w=in_w, out_h=oh, out_w=ow, cin=cin, cout=cout, kh=kh, kw=kw, sh=sh, sw=sw, pad_t=pt, pad_l=pl, reserved=G)


def _check(got, name, pre, bound, act, terms, k_eff, what, where=None):
    """Element by element against act(pre) (where: a mask of the elements to hold); records the worst share of tau."""
    ref = O.act64(pre, act)
    where = np.ones(ref.shape, bool) if where is None else where
    assert np.isfinite(got[where]).all(), (what, name, "non-finite output")
    scale = 1.2 * bound
    err = np.where(where, np.abs(got.astype(np.float64) - ref), 0.0)
    eps = _eps_act(pre, act)
    tol = _tau(terms, k_eff) * scale + eps
    share = float(np.max(np.maximum(err - eps, 0.0) / np.maximum(scale, 1e-300)))
    WORST[(name, terms)] = max(WORST.get((name, terms), 0.0), share)
    bad = err > tol
    if bad.any():
        i = np.unravel_index(np.argmax(err / tol), err.shape)
        pytest.fail(f"{what} {name} act {O.ACT_NAMES[act]}: {int(bad.sum())} of {bad.size} elements off, worst at {i}: got "
                    f"{got[i]!r} want {ref[i]!r} (pre {pre[i]!r}), err {err[i]:.3e} > tol {tol[i]:.3e}")


# (in width, out width, groups): cin = G in, cout = G out
WIDTHS = {"4x8g": (4, 4, 8), "8x4g": (8, 8, 4), "16x3g": (16, 16, 3), "24x3g": (24, 24, 3), "32x2g": (32, 32, 2), "4to8x4g": (4, 8, 4), "8to4x6g": (8, 4, 6)}
IMAGES = ((5, 7), (9, 11))


def _geometry(geom, in_h, in_w):
    """-> (kh, kw, sh, sw, pad_t, pad_l, out_h, out_w)"""
    if geom == "3x3s1":
        return 3, 3, 1, 1, 1, 1, in_h, in_w
    if geom == "3x3s2":     # the output size of SAME at stride 2 with the whole padding at the bottom / right (pad_t = pad_l = 0: what SAME is on an even image)
        return 3, 3, 2, 2, 0, 0, -(-in_h // 2), -(-in_w // 2)
    if geom == "1x1":
        return 1, 1, 1, 1, 0, 0, in_h, in_w
    if geom == "5x5valid":
        return 5, 5, 1, 1, 0, 0, in_h - 4, in_w - 4
    if geom == "1x7asym":   # explicit pads (top, left, bottom, right) = (0, 2, 0, 4)
        return 1, 7, 1, 1, 0, 2, in_h, in_w
    raise ValueError(geom)


GEOMS = ("3x3s1", "3x3s2", "1x1", "5x5valid", "1x7asym")
_REF = {}


def _shape(width, geom, image):
    gi, go, G = WIDTHS[width]
    kh, kw, sh, sw, pt, pl, oh, ow = _geometry(geom, *image)
    return (image[0], image[1], oh, ow, G * gi, G * go, kh, kw, sh, sw, pt, pl, G)


def _reference(width, geom, image, n_seg=3):
    key = (width, geom, image, n_seg)
    if key not in _REF:
        shape = _shape(width, geom, image)
        gi = WIDTHS[width][0]
        rng = np.random.default_rng(sum(shape) * 7 + n_seg)
        k_rows = shape[6] * shape[7] * gi
        X, W, b, _ = _operands(rng, (n_seg, shape[0], shape[1], shape[4]), k_rows, shape[5], False, 0)
        W = np.ascontiguousarray(W.reshape(shape[6], shape[7], gi, shape[5]))
        pre, bound = gconv_pre64(X.astype(np.float64), W, b, _rec(shape))
        _REF[key] = (shape, X, W, b, pre, bound, k_rows)
    return _REF[key]


def _element_params():
    out, i = [], 0
    for width in WIDTHS:
        for geom in GEOMS:
            out.append(pytest.param(width, geom, i, id=f"{width}-{geom}"))
            i += 1
    return out


@pytest.mark.parametrize("width,geom,idx", _element_params())
def test_every_element_matches_float64(width, geom, idx):
    for j, image in enumerate(IMAGES):
        shape, X, W, b, pre, bound, k_eff = _reference(width, geom, image)
        for terms in (0, 3, 1):
            acts = ACTS32 if terms == 0 else ACTS16
            act = acts[(2 * idx + j) % len(acts)]
            got, name = _gconv(X, W, b, shape, act, terms)
            assert name == KERNEL_OF[terms], name
            if act == O.ACT_RELU6:
                assert (pre < 0).any() and (pre > 6).any(), "operands should make ReLU6 clamp on both sides"
            _check(got, name, pre, bound, act, terms, k_eff, (width, geom, image))


def test_every_activation_code_ran_on_terms_0():
    seen = set()
    for idx in range(len(WIDTHS) * len(GEOMS)):
        for j in range(len(IMAGES)):
            seen.add(ACTS32[(2 * idx + j) % len(ACTS32)])
    assert seen == set(ACTS32)
    for terms_acts in (ACTS16,):
        assert {terms_acts[(2 * idx + j) % 4] for idx in range(35) for j in range(2)} == set(ACTS16)


# ---- isolation: a wrong span or a misplaced weight block shows in the bits -------------------------------------------------------
@pytest.mark.parametrize("width", ["4x8g", "24x3g", "8to4x6g", "32x2g", "4to8x4g"])
def test_a_group_with_zero_weights_and_huge_inputs_touches_no_other_group(width):
    """Group g's weights zero and its input channels 1e30: 1e30 x 0 = 0 wherever the layout lets the two meet, so every other
    group's outputs are those of the run without the large values, bit for bit (terms 0: in f16 1e30 is inf)."""
    shape, X, W, b, _, _, _ = _reference(width, "3x3s1", (9, 11))
    gi, go, G = WIDTHS[width]
    for g in range(G):
        Wz = W.copy()
        Wz[..., g * go:(g + 1) * go] = 0.0
        base, name = _gconv(X, Wz, b, shape, O.ACT_NONE, 0)
        Xh = X.copy()
        Xh[..., g * gi:(g + 1) * gi] = np.float32(1e30)
        got, _ = _gconv(Xh, Wz, b, shape, O.ACT_NONE, 0)
        others = np.ones(shape[5], bool)
        others[g * go:(g + 1) * go] = False
        assert np.isfinite(got).all(), (width, g)
        assert (got.view(np.uint32)[:, others] == base.view(np.uint32)[:, others]).all(), (width, g)
        assert (got[:, ~others] == b[~others]).all(), (width, g)          # the zeroed group: its bias alone


# ---- the non-finite contract ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", (0, 3, 1))
@pytest.mark.parametrize("width,bad_channel", [("8x4g", 9), ("24x3g", 30), ("32x2g", 40)])
def test_a_non_finite_input_reaches_its_readers_and_no_other_pixel_or_tile(width, bad_channel, terms):
    """A NaN, a +inf and a -inf, each at one (pixel, channel) of a segment of its own: every output whose window and group read it
    is non-finite; every output at a pixel whose window misses it, and every output of a column tile that holds none of the group's
    output channels, is finite and within tolerance (the other channels of the readers' own column tiles may go either way)."""
    shape, X, W, b, pre, bound, k_eff = _reference(width, "3x3s1", (9, 11))
    gi, go, G = WIDTHS[width]
    in_h, in_w, oh, ow = shape[:4]
    cout = shape[5]
    Xb = X.copy()
    spots = [(0, 4, 5, np.float32(np.nan)), (1, 0, 0, np.float32(np.inf)), (2, 8, 10, np.float32(-np.inf))]
    for seg, y, x, v in spots:
        Xb[seg, y, x, bad_channel] = v
    got, name = _gconv(Xb, W, b, shape, O.ACT_NONE, terms)
    got = got.reshape(3, oh, ow, cout)
    g = bad_channel // gi
    readers = np.zeros(cout, bool)
    readers[g * go:(g + 1) * go] = True
    tiles = np.unique(np.nonzero(readers)[0] // 16)
    same_tile = np.isin(np.arange(cout) // 16, tiles)
    assert not same_tile.all(), "the case should leave a column tile that holds none of the group"
    hold = np.ones((3, oh, ow, cout), bool)
    for seg, y, x, v in spots:
        win = np.zeros((oh, ow), bool)
        win[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True          # 3x3, stride 1, pad 1: the outputs whose window holds (y, x)
        assert not np.isfinite(got[seg][win][:, readers]).any(), (name, seg, "a reader of the value is finite")
        hold[seg][win] &= ~same_tile          # the readers' own column tiles at those pixels: either way
    # (pre / bound are those of the finite X: the held elements read none of the three values)
    _check(got.reshape(-1, cout), name, pre, bound, O.ACT_NONE, terms, k_eff, (width, "non-finite"), where=hold.reshape(-1, cout))
    assert hold.reshape(-1, cout)[:, ~same_tile].all()                # every other column tile is held at every pixel


def test_relu_keeps_a_nan_and_plus_inf():
    """the activation does not launder what the sum holds: ReLU of NaN stays NaN, of +inf stays +inf (f32 kernel)"""
    shape, X, W, b, _, _, _ = _reference("8x4g", "1x1", (5, 7))
    Xb = X.copy()
    Xb[0, 0, 0, 0] = np.float32(np.nan)
    got, _ = _gconv(Xb, W, b, shape, O.ACT_RELU, 0)
    assert np.isnan(got[0, :8]).all() and np.isfinite(got[1:]).all()
    Xb[0, 0, 0, 0] = np.float32(np.inf)
    Wp = np.abs(W)
    got, _ = _gconv(Xb, Wp, b, shape, O.ACT_RELU, 0)
    assert np.isposinf(got[0, :8]).all()


# ---- launch independence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", (0, 3, 1))
def test_segment_bits_do_not_depend_on_the_launch(terms):
    """3 / 80 / 300 segments: the same bits per segment; 600 segments of the 72-column layer are 465 row blocks x 5 column tiles =
    2 325 workgroups, more than are resident at once (256 CUs x 8), held element by element"""
    shape, X, W, b, pre, bound, k_eff = _reference("24x3g", "3x3s1", (9, 11))
    first, name = _gconv(X, W, b, shape, O.ACT_SWISH, terms)
    rows = shape[2] * shape[3]
    for n in (80, 300, 600):
        pick = np.arange(n) % 3
        got, name_n = _gconv(np.ascontiguousarray(X[pick]), W, b, shape, O.ACT_SWISH, terms)
        assert name_n == name
        assert -(-n * rows // 128) * 5 > 2048 or n < 600
        want = first.reshape(3, rows, -1)[pick].reshape(n * rows, -1)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), (terms, n)
        if n == 600:
            _check(got, name, np.tile(pre.reshape(3, rows, -1), (200, 1, 1)).reshape(n * rows, -1),
                   np.tile(bound.reshape(3, rows, -1), (200, 1, 1)).reshape(n * rows, -1), O.ACT_SWISH, terms, k_eff, "600 segments")


def test_the_entry_refuses_what_has_no_kernel():
    shape, X, W, b, _, _, _ = _reference("8x4g", "3x3s1", (5, 7))
    UNSUPPORTED = -6          # BH_ERR_UNSUPPORTED
    _, msg = _gconv(X, W, b, shape, 0, 2, expect=UNSUPPORTED)        # no two-term form
    assert "terms 2" in msg, msg
    for change in ({12: 1}, {12: 5}, {12: 16}, {6: 8}, {8: 3}):     # one group; 32 % 5; width 2; kernel 8; stride 3
        bad = list(shape)
        for k, v in change.items():
            bad[k] = v
        _gconv(X, W, b, tuple(bad), 0, 0, expect=UNSUPPORTED)


# ---- the product path ---------------------------------------------------------------------------------------------------------------
def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def _grouped(m):
    return [i for i, L in enumerate(m.layers) if L.op == mf.OP_GCONV]


def _check_grouped_kernels(clf, m, prec, what):
    want = "gconv_kernel" if prec == "f32" else "gconv16_kernel<1>" if prec == "f16" else "gconv16_kernel<3>"
    for i in _grouped(m):
        assert clf.layer_kernel(i) == want, (what, prec, i, clf.layer_kernel(i))


@pytest.mark.parametrize("seed", range(6))
def test_random_resnext_plans_on_the_onnx_route(seed, tmp_path):
    from birda_amd.classifier import BirdClassifier
    plan = synth.random_resnext_plan(seed)
    m = synth.build_model("resnext_plan", plan=plan)
    assert len(_grouped(m)) == 4
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=5 + seed)
    segs[2] *= np.float32(0.01)
    precisions = [("f32", LOGIT_RTOL), ("f16x3", LOGIT_RTOL), ("auto", LOGIT_RTOL)] + ([("f16", F16_LOGIT_RTOL)] if seed in (1, 2) else [])
    # the float32 file, and its float16 rewrite: the reference of that one is the float64 forward of the container the library's
    # own reader makes of it (its weights are the file's float16 values)
    g32 = convert.graph_from_model(m, frontend_spelling="stft")
    files = [("float32", _write(str(tmp_path / "x.onnx"), ox.dump(g32)), m)]
    p16, bhm = _write(str(tmp_path / "x16.onnx"), ox.dump(convert.graph_to_float16(convert.graph_from_model(m, frontend_spelling="conv1d")))), str(tmp_path / "x16.bhm")
    L = _lib.load()
    assert L.bh_onnx_to_bhm(p16.encode(), bhm.encode()) == 0, L.bh_last_error()
    m16 = mf.read_model(bhm)
    assert [(a.op, a.act, a.reserved) for a in m16.layers] == [(a.op, a.act, a.reserved) for a in m.layers]
    files.append(("float16", p16, m16))
    for kind, path, model in files:
        ref = forward64(model, segs)
        scale = max(1.0, float(np.abs(ref).max()))
        for prec, tol in precisions:
            clf = BirdClassifier(path, None, precision=prec)
            assert clf.weight_summary()["float16_file"] == (kind == "float16")
            ctx = clf.create_batch_context(3)
            got = clf.predict_logits(ctx, segs)
            err = float(np.abs(got - ref).max())
            print(f"resnext plan {seed} {kind} file {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (tol * scale):.3f})  {plan['items']}")
            assert np.isfinite(got).all() and err <= tol * scale, (kind, prec, err, scale)
            _check_grouped_kernels(clf, model, prec, (seed, kind))      # a float16 file: three terms too (there is no two-term form)
            ctx.close()
            if kind == "float32" and prec == "auto":       # a segment's bits do not depend on its launch
                ctx = clf.create_batch_context(80)
                ctx.set_sub_slices(1)
                big = clf.predict_logits(ctx, np.ascontiguousarray(segs[np.arange(80) % 3]))
                assert (big.view(np.uint32) == got.view(np.uint32)[np.arange(80) % 3]).all()
                ctx.close()
            clf.close()


def test_grouped_layers_match_float64_layer_by_layer_in_a_model(tmp_path, monkeypatch):
    """BIRDA_HIP_KEEP_TENSORS: every grouped layer's own output against the float64 layer of the device's own input (f32 kernel)"""
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("resnext_plan", plan=synth.random_resnext_plan(3))
    path = str(tmp_path / "k.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=9)
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(3)
    clf.predict_logits(ctx, segs)
    for i in _grouped(m):
        Lr = m.layers[i]
        gi = Lr.cin // Lr.reserved
        X, Y = clf.read_tensor(ctx, Lr.in_tensor, 3), clf.read_tensor(ctx, i + 1, 3)
        W = np.asarray(m.blob[Lr.w_off:Lr.w_off + Lr.kh * Lr.kw * gi * Lr.cout], np.float64).reshape(Lr.kh, Lr.kw, gi, Lr.cout)
        pre, bound = gconv_pre64(X.reshape(3, Lr.in_h, Lr.in_w, Lr.cin).astype(np.float64), W, m.blob[Lr.b_off:Lr.b_off + Lr.cout], Lr)
        assert clf.layer_kernel(i) == "gconv_kernel"
        _check(Y.reshape(-1, Lr.cout), "gconv_kernel", pre, bound, Lr.act, 0, Lr.kh * Lr.kw * gi, ("in a model", i))
    ctx.close(); clf.close()


def overflow_model():
    """The mini front-end, a 3x3 stride-2 stem to 32 channels, a LINEAR 1x1 layer 32 -> 32, a grouped 3x3 ReLU layer 32 -> 32 in 4
    groups, a 1x1 head, the global pool and a dense layer"""
    b = synth._Builder(np.random.default_rng(13))
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    t, h, w = b.conv(0, br.n_mels, br.n_frames, 1, 32, 3, 2, mf.ACT_GELU_ERF, in_layout=1)
    t = b.pwconv(t, h, w, 32, 32, mf.ACT_NONE)
    t, h, w = b.gconv(t, h, w, 32, 32, 3, 1, 4, mf.ACT_RELU)
    t = b.pwconv(t, h, w, 32, 64, mf.ACT_GELU_ERF)
    t = emb = b.gap(t, h, w, 64)
    b.dense(t, 64, 30, gain=1.5)
    return mf.Model(0, sr, n, n / sr, 30, 64, mf.OUT_SIGMOID, emb, br.n_mels, br.n_frames, 1e-6, [br], b.layers, np.concatenate(b.chunks))


def test_f16_overflow_in_front_of_a_grouped_layer_is_not_laundered(tmp_path):
    """The linear layer's weights and bias times 2^20 (its output, ~1e6, is past 65 504) and the grouped layer's weights divided by
    2^20: the same function in f32 arithmetic.  The split-f16 kernel cannot represent its operand; the NaN / inf it computes must
    pass its ReLU -- f16x3 ends in BH_ERR_NONFINITE --, and auto re-runs the rows on the f32 kernels."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    m0 = overflow_model()
    m = copy.deepcopy(m0)
    blob = m.blob.copy()
    Lin, Gr = m.layers[1], m.layers[2]
    assert Lin.act == mf.ACT_NONE and Lin.op == mf.OP_PWCONV and Gr.op == mf.OP_GCONV and Gr.act == mf.ACT_RELU
    s = np.float32(2.0 ** 20)
    blob[Lin.w_off:Lin.w_off + Lin.cin * Lin.cout] *= s
    blob[Lin.b_off:Lin.b_off + Lin.cout] *= s
    blob[Gr.w_off:Gr.w_off + Gr.kh * Gr.kw * (Gr.cin // Gr.reserved) * Gr.cout] /= s
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
    assert clf.layer_kernel(2) == "gconv16_kernel<3>", clf.layer_kernel(2)
    ctx.close(); clf.close()
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(4)
    got = clf.predict_logits(ctx, segs)
    assert clf.fallback_segments() > 0
    err = float(np.abs(got - ref).max())
    print(f"overflow in front of a grouped layer, auto: max|dlogit| = {err:.3e} of {scale:.2f}, {clf.fallback_segments()} segments re-run")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    ctx.close(); clf.close()


def test_resnext_audio_runs_and_matches_float64(tmp_path):
    """synth's timing model, three segments in auto: finite logits at LOGIT_RTOL of the float64 forward (the numpy reference is this
    test's time; the device part is milliseconds), every grouped layer on gconv16_kernel<3>"""
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("resnext_audio", n_classes=40)
    assert len(_grouped(m)) == 8
    path = str(tmp_path / "resnext.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=2)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(3)
    got = clf.predict_logits(ctx, segs)
    ctx.close()
    err = float(np.abs(got - ref).max())
    print(f"resnext_audio auto: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    _check_grouped_kernels(clf, m, "auto", "resnext_audio")
    clf.close()


# ---- all three instantiations were reached (keep last: it reads what the tests above ran) --------------------------------------------
def test_all_three_instantiations_were_reached():
    """Run with the module, it reads what the tests above launched (and prints their worst shares); alone or under -k it launches
    what is missing itself."""
    shape, X, W, b, _, _, _ = _reference("8x4g", "1x1", (5, 7))
    for terms, name in KERNEL_OF.items():
        if name not in REACHED:
            _gconv(X, W, b, shape, 0, terms)
    assert REACHED == set(KERNEL_OF.values()), sorted(REACHED)
    print("\nworst (err - eps_act) / (1.2 bound) by kernel and terms, and its share of tau:")
    for (name, terms), v in sorted(WORST.items()):
        print(f"  {name:20s} terms {terms}: {v:.3e}  ({v / (1.5e-3 if terms == 1 else 4e-7):.3f} of tau at K <= 1024)")
