"""Dilated convolutions on the host side: the container's two dilation words, both ONNX readers, the writer, the validator and the
planner.

* the yardstick: taps64 gathers a layer's dilated taps in float64 (tap (dy, dx) of output pixel (oy, ox) is input pixel
  (oy sh - pad_t + dy dil_h, ox sw - pad_l + dx dil_w), zero outside the image); conv64d / dw64d and forward64 compose a model's
  logits from it -- the plain-C oracle and oracle/oracle.py do not know the words and are never fed a dilated model.  The forward of
  `dilated_plan` is held to a torch float64 composition with conv2d(dilation = ...) of the same weights;
* hand-written graphs -- explicit pads, SAME_UPPER, SAME_LOWER, VALID; dilation (2, 2), (1, 3), (2, 1); stride 2 with dilation 2; a
  dilated depthwise; a float16 file -- go through the library's reader and convert.py to the stated record (worked out by hand), the
  same layer table and the same blob, bit for bit;
* .bhm -> .onnx -> .bhm is record-exact through either reader; undilated layers and the existing synth models write a zero tail;
* validate_model refuses, with a reason of its own, a dilation word on a pool, grouped, pointwise, dense, concat or stem record, a
  value above 16 and a value on an axis with one tap; the readers refuse stem, grouped and pool dilation with "dilation" in the message;
* bh_plan_fused_blocks leaves the inverted-residual block with the dilated depthwise unfused, and fuses its undilated twin.
"""
import copy
import struct

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O
from test_gconv import gconv_graph, layer64g
from test_pool import RECORD, both_readers, pool_graph, same_tables_and_blob
from test_resact import N_W


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------
def taps64(X, shape):
    """X [n][in_h][in_w][c], shape = (in_h, in_w, out_h, out_w, ., ., kh, kw, sh, sw, pad_t, pad_l, dil_h, dil_w) ->
    A [n][out_h][out_w][kh * kw][c] in float64: the pixel each tap reads, zero where it lies outside the image (written, never
    multiplied: a NaN pixel reaches exactly the taps that read it)."""
    in_h, in_w, oh, ow, _, _, kh, kw, sh, sw, pt, pl, dh, dw = shape
    X = np.asarray(X, np.float64)
    n, c = X.shape[0], X.shape[3]
    A = np.zeros((n, oh, ow, kh * kw, c))
    for oy in range(oh):
        for dy in range(kh):
            iy = oy * sh - pt + dy * dh
            if not 0 <= iy < in_h:
                continue
            for dx in range(kw):
                ix = np.arange(ow) * sw - pl + dx * dw
                ok = (ix >= 0) & (ix < in_w)
                A[:, oy, ok, dy * kw + dx] = X[:, iy, ix[ok]]
    return A


def conv64d(X, W, bias, shape):
    """a dilated full convolution in float64: W [kh][kw][cin][cout] -> (pre [rows][cout], bound = |A| |W| + |b|)"""
    cout = W.shape[3]
    A = taps64(X, shape).reshape(-1, W.shape[0] * W.shape[1] * W.shape[2])
    W2, b = np.asarray(W, np.float64).reshape(-1, cout), np.asarray(bias, np.float64)
    return A @ W2 + b, np.abs(A) @ np.abs(W2) + np.abs(b)


def dw64d(X, W, bias, shape):
    """a dilated depthwise convolution in float64: W [kh * kw][c] -> (pre [n][oh][ow][c], bound = |taps| . |W| + |b|)"""
    A, W, b = taps64(X, shape), np.asarray(W, np.float64), np.asarray(bias, np.float64)
    return (A * W).sum(axis=3) + b, (np.abs(A) * np.abs(W)).sum(axis=3) + np.abs(b)


def shape_of(L):
    return (L.in_h, L.in_w, L.out_h, L.out_w, L.cin, L.cout, L.kh, L.kw, L.sh, L.sw, L.pad_t, L.pad_l, L.dil_h, L.dil_w)


def layer64d(m, L, X, R):
    """tests/test_gconv.py's layer64g, with the dilated OP_CONV (NHWC) and OP_DWCONV records computed here"""
    if (L.dil_h, L.dil_w) == (1, 1):
        return layer64g(m, L, X, R)
    n = X.shape[0]
    bias = m.blob[L.b_off:L.b_off + L.cout]
    if L.op == mf.OP_CONV:
        assert L.in_layout == 0
        W = m.blob[L.w_off:L.w_off + L.kh * L.kw * L.cin * L.cout].reshape(L.kh, L.kw, L.cin, L.cout)
        pre = conv64d(np.asarray(X).reshape(n, L.in_h, L.in_w, L.cin), W, bias, shape_of(L))[0].reshape(n, L.out_h, L.out_w, L.cout)
    else:
        assert L.op == mf.OP_DWCONV and R is None
        W = m.blob[L.w_off:L.w_off + L.kh * L.kw * L.cout].reshape(L.kh * L.kw, L.cout)
        pre = dw64d(np.asarray(X).reshape(n, L.in_h, L.in_w, L.cout), W, bias, shape_of(L))[0]
    if L.op == mf.OP_CONV and L.reserved == mf.RES_ACT_AFTER:
        return O.act64(pre + np.asarray(R, np.float64).reshape(pre.shape), L.act)
    Y = O.act64(pre, L.act)
    return Y if R is None else Y + np.asarray(R, np.float64).reshape(Y.shape)


def forward64(m, segs, tensors=False):
    """-> logits [n][n_classes] in float64 (tensors=True: every tensor, T[0] the spectrogram)"""
    spec, _ = O.frontend64(m, segs)
    T = [spec]
    for L in m.layers:
        T.append(layer64d(m, L, T[L.in_tensor], None if L.res_tensor == mf.NO_TENSOR else T[L.res_tensor]))
    return T if tensors else T[-1].reshape(segs.shape[0], -1)


def dilated(m):
    return [i for i, L in enumerate(m.layers) if (L.dil_h, L.dil_w) != (1, 1)]


@pytest.fixture(scope="module")
def plan():
    return synth.build_model("dilated_plan")


def test_dilated_plan_holds_what_it_promises(plan):
    m = plan
    D = [m.layers[i] for i in dilated(m)]
    assert {(L.dil_h, L.dil_w) for L in D if L.op == mf.OP_CONV} == {(2, 2), (4, 4), (1, 2), (2, 1)}
    assert any(L.sh == 2 and L.dil_h == 2 for L in D)                                    # one stride-2 dilated layer
    assert any(L.reserved == mf.RES_ACT_AFTER for L in D) and any(L.res_tensor != mf.NO_TENSOR and L.reserved == 0 for L in D)
    assert any(L.cout > 64 for L in D) and any(L.cout <= 64 for L in D)                   # both GEMM kernels in the f16 modes
    assert [L.op for L in D].count(mf.OP_DWCONV) == 1
    assert all(L.dil_h == 1 and L.dil_w == 1 for L in m.layers if L.op not in (mf.OP_CONV, mf.OP_DWCONV) or L.in_layout == 1)
    big = synth.build_model("dilated_resnet_audio", n_classes=40)
    assert sorted({L.dil_h for L in big.layers}) == [1, 2, 4] and all(L.dil_h == L.dil_w for L in big.layers)
    assert {(L.out_h, L.out_w) for L in big.layers if L.dil_h > 1} == {(12, 64)}           # output stride 8 of the 96 x 511 spectrogram


def test_forward64_is_the_torch_float64_composition(plan):
    """every layer of dilated_plan composed in torch float64 -- conv2d(dilation = ...) of the record's own weights, the activation
    before or after the residual as the record says -- against forward64, tensor by tensor"""
    import torch
    import torch.nn.functional as F
    m = plan
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=5)
    T = forward64(m, segs, tensors=True)
    act = {mf.ACT_NONE: lambda v: v, mf.ACT_RELU: F.relu, mf.ACT_RELU6: lambda v: torch.clamp(v, 0.0, 6.0), mf.ACT_SWISH: lambda v: v * torch.sigmoid(v)}
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    Y = [t64(T[0])]                                                                      # NCHW throughout
    for i, L in enumerate(m.layers):
        x, b = Y[L.in_tensor], t64(m.blob[L.b_off:L.b_off + L.cout])
        if L.op in (mf.OP_CONV, mf.OP_DWCONV, mf.OP_PWCONV):
            if L.op == mf.OP_CONV:
                w, groups = m.blob[L.w_off:L.w_off + L.kh * L.kw * L.cin * L.cout].reshape(L.kh, L.kw, L.cin, L.cout).transpose(3, 2, 0, 1), 1
            elif L.op == mf.OP_DWCONV:
                w, groups = m.blob[L.w_off:L.w_off + L.kh * L.kw * L.cout].reshape(L.kh, L.kw, L.cout).transpose(2, 0, 1)[:, None], L.cout
            else:
                w, groups = m.blob[L.w_off:L.w_off + L.cin * L.cout].reshape(L.cin, L.cout).T[:, :, None, None], 1
            pad_b = max((L.out_h - 1) * L.sh + (L.kh - 1) * L.dil_h + 1 - L.in_h - L.pad_t, 0)
            pad_r = max((L.out_w - 1) * L.sw + (L.kw - 1) * L.dil_w + 1 - L.in_w - L.pad_l, 0)
            y = F.conv2d(F.pad(x, (L.pad_l, pad_r, L.pad_t, pad_b)), t64(w), b, stride=(L.sh, L.sw), dilation=(L.dil_h, L.dil_w), groups=groups)
            assert tuple(y.shape[2:]) == (L.out_h, L.out_w), i
            if L.res_tensor != mf.NO_TENSOR and L.reserved == mf.RES_ACT_AFTER:
                y = act[L.act](y + Y[L.res_tensor])
            else:
                y = act[L.act](y)
                if L.res_tensor != mf.NO_TENSOR:
                    y = y + Y[L.res_tensor]
        elif L.op == mf.OP_GAP:
            y = x.mean(dim=(2, 3), keepdim=True)
        else:
            assert L.op == mf.OP_DENSE and L.act == mf.ACT_NONE
            y = (x.reshape(x.shape[0], -1) @ t64(m.blob[L.w_off:L.w_off + L.cin * L.cout].reshape(L.cin, L.cout)) + b)[:, :, None, None]
        Y.append(y)
        want = y.numpy().transpose(0, 2, 3, 1)
        got = np.asarray(T[i + 1]).reshape(want.shape)
        assert np.abs(got - want).max() <= 1e-11 * max(np.abs(want).max(), 1.0), (i, L.op)
    # ... and the words matter: the same records without them are another function
    twin = copy.deepcopy(m)
    for L in twin.layers:
        L.dil_h = L.dil_w = 1
    other = forward64(twin, segs)
    assert np.abs(other - T[-1].reshape(other.shape)).max() > 1e-3 * np.abs(other).max()


# ---- hand-written graphs through both readers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return synth.build_model("mini")


# case -> (graph arguments, the stated record (op, kh, kw, sh, sw, pad_t, pad_l, out_h, out_w, dil_h, dil_w)) on the 16 x 58 image
# behind the stem.  extent e = (k - 1) d + 1; explicit / VALID: out = floor((in + pads - e) / s) + 1; SAME: out = ceil(in / s),
# total = (out - 1) s + e - in, UPPER puts the odd row / column at the end, LOWER at the start.
CONV, DW = mf.OP_CONV, mf.OP_DWCONV
ACCEPTED = {
    # e = 5 x 5, pads 2: 16 x 58 stays
    "explicit_d2x2": (dict(group=1, attrs={"pads": [2, 2, 2, 2], "dilations": [2, 2]}), (CONV, 3, 3, 1, 1, 2, 2, 16, 58, 2, 2)),
    # e = 3 x 7: totals (2, 6) -> (1, 3)
    "same_upper_d1x3": (dict(group=1, attrs={"auto_pad": "SAME_UPPER", "dilations": [1, 3]}), (CONV, 3, 3, 1, 1, 1, 3, 16, 58, 1, 3)),
    # stride 2, e = 5 x 3: out 8 x 29, totals (7 * 2 + 5 - 16, 28 * 2 + 3 - 58) = (3, 1); LOWER: the larger half first -> (2, 1)
    "same_lower_s2_d2x1": (dict(group=1, attrs={"auto_pad": "SAME_LOWER", "strides": [2, 2], "dilations": [2, 1]}), (CONV, 3, 3, 2, 2, 2, 1, 8, 29, 2, 1)),
    # the same under UPPER: (1, 0)
    "same_upper_s2_d2x1": (dict(group=1, attrs={"auto_pad": "SAME_UPPER", "strides": [2, 2], "dilations": [2, 1]}), (CONV, 3, 3, 2, 2, 1, 0, 8, 29, 2, 1)),
    # e = 5 x 5, no pads: 12 x 54
    "valid_d2x2": (dict(group=1, attrs={"auto_pad": "VALID", "dilations": [2, 2]}), (CONV, 3, 3, 1, 1, 0, 0, 12, 54, 2, 2)),
    # stride 2 with dilation 2, pads 2: floor((16 + 4 - 5) / 2) + 1 = 8, floor((58 + 4 - 5) / 2) + 1 = 29
    "explicit_s2_d2x2": (dict(group=1, attrs={"pads": [2, 2, 2, 2], "strides": [2, 2], "dilations": [2, 2]}), (CONV, 3, 3, 2, 2, 2, 2, 8, 29, 2, 2)),
    # asymmetric pads (3, 0, 1, 2) with e = 5 x 5: 16 + 4 - 5 + 1 = 16, 58 + 2 - 5 + 1 = 56
    "asymmetric_pads_d2x2": (dict(group=1, attrs={"pads": [3, 0, 1, 2], "dilations": [2, 2]}), (CONV, 3, 3, 1, 1, 3, 0, 16, 56, 2, 2)),
    # 5 x 5 at dilation 3: e = 13, SAME total 12 -> 6
    "same_upper_5x5_d3": (dict(group=1, kernel=(5, 5), attrs={"auto_pad": "SAME_UPPER", "dilations": [3, 3]}), (CONV, 5, 5, 1, 1, 6, 6, 16, 58, 3, 3)),
    # an axis with one tap is dilation 1 whatever the file says: 1 x 3 at "(5, 2)" is (1, 2), e = 1 x 5
    "one_tap_axis_is_1": (dict(group=1, kernel=(1, 3), attrs={"pads": [0, 2, 0, 2], "dilations": [5, 2]}), (CONV, 1, 3, 1, 1, 0, 2, 16, 58, 1, 2)),
    # the largest: 16 on 3 taps, e = 33, SAME total 32 -> 16 a side
    "d16": (dict(group=1, attrs={"auto_pad": "SAME_UPPER", "dilations": [16, 16]}), (CONV, 3, 3, 1, 1, 16, 16, 16, 58, 16, 16)),
    "depthwise_d2x2": (dict(group=32, attrs={"pads": [2, 2, 2, 2], "dilations": [2, 2]}), (DW, 3, 3, 1, 1, 2, 2, 16, 58, 2, 2)),
    "depthwise_s2_d2x3_same": (dict(group=32, attrs={"auto_pad": "SAME_UPPER", "strides": [2, 2], "dilations": [2, 3]}), (DW, 3, 3, 2, 2, 1, 2, 8, 29, 2, 3)),
    "dilations_of_one": (dict(group=1, attrs={"pads": [1, 1, 1, 1], "dilations": [1, 1]}), (CONV, 3, 3, 1, 1, 1, 1, 16, 58, 1, 1)),
}
STATED = ("op", "kh", "kw", "sh", "sw", "pad_t", "pad_l", "out_h", "out_w", "dil_h", "dil_w")


def same_records(a, b):
    same_tables_and_blob(a, b)
    assert [(L.dil_h, L.dil_w) for L in a.layers] == [(L.dil_h, L.dil_w) for L in b.layers]


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_both_readers_give_the_stated_record(case, base, tmp_path):
    args, stated = ACCEPTED[case]
    want, got = both_readers(gconv_graph(**args), base, tmp_path)
    same_records(want, got)
    L = got.layers[1]
    assert tuple(getattr(L, f) for f in STATED) == stated
    assert (L.act, L.in_tensor, L.in_h, L.in_w, L.cin, L.cout) == (mf.ACT_RELU, 1, 16, 58, 32, 32)      # BatchNormalization folded, ReLU on it
    assert (got.layers[2].in_h, got.layers[2].in_w) == (L.out_h, L.out_w)
    # the words in the file: dilation - 1 at bytes 88 .. 95 of the record, zeros behind
    raw = open(str(tmp_path / "case.bhm"), "rb").read()
    off = mf.HEADER_SIZE + len(got.branches) * mf.BRANCH_SIZE + mf.LAYER_SIZE
    assert struct.unpack_from("<II", raw, off + 88) == (L.dil_h - 1, L.dil_w - 1) and raw[off + 96:off + 128] == bytes(32)


def test_both_readers_read_a_float16_file_alike(base, tmp_path):
    g16 = convert.graph_to_float16(gconv_graph(group=1, attrs={"auto_pad": "SAME_UPPER", "dilations": [2, 3]}))
    assert all(a.dtype == np.float16 for a in g16.initializers.values())
    want, got = both_readers(g16, base, tmp_path)
    same_records(want, got)
    L = got.layers[1]
    assert (L.op, L.dil_h, L.dil_w, L.pad_t, L.pad_l) == (mf.OP_CONV, 2, 3, 2, 3)


REFUSED = {
    "stem": (gconv_graph, dict(group=1, cin=2, cout=8, on_spectrogram=True, attrs={"pads": [2, 2, 2, 2], "dilations": [2, 2]}), "dilation"),
    "grouped": (gconv_graph, dict(group=8, attrs={"pads": [2, 2, 2, 2], "dilations": [2, 2]}), "dilation"),
    "above_16": (gconv_graph, dict(group=1, attrs={"auto_pad": "SAME_UPPER", "dilations": [17, 1]}), "dilation"),
    "zero": (gconv_graph, dict(group=1, attrs={"auto_pad": "SAME_UPPER", "dilations": [0, 1]}), "dilation"),
    "three_values": (gconv_graph, dict(group=1, attrs={"auto_pad": "SAME_UPPER", "dilations": [2, 2, 2]}), "dilations"),
    "extent_past_the_padded_input": (gconv_graph, dict(group=1, attrs={"dilations": [8, 1]}), "kernel larger than the padded input"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_both_readers_refuse_by_name(case, base, tmp_path):
    make, args, word = REFUSED[case]
    g = make(**args)
    with pytest.raises(convert.ConvertError, match=word):
        convert.model_from_graph(g, base)
    with pytest.raises(RuntimeError, match=word):
        both_readers_native(g, tmp_path)


def both_readers_native(g, tmp_path):
    onnx_path, out = str(tmp_path / "case.onnx"), str(tmp_path / "case.bhm")
    with open(onnx_path, "wb") as f:
        f.write(ox.dump(g))
    L = _lib.load()
    rc = L.bh_onnx_to_bhm(onnx_path.encode(), out.encode())
    if rc != 0:
        raise RuntimeError(f"rc {rc}: {L.bh_last_error().decode()}")
    return mf.read_model(out)


def native_from_model(m, tmp_path):
    """the library's reader on the model's .onnx spelling with its front end (an STFT graph: any spectrogram size is read off it)"""
    onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m_native.bhm")
    with open(onnx_path, "wb") as f:
        f.write(convert.model_to_onnx(m, frontend_spelling="stft"))
    L = _lib.load()
    assert L.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, L.bh_last_error()
    return mf.read_model(out)


def test_a_dilated_pool_stays_refused(base, tmp_path):
    g = pool_graph(base, "MaxPool", {"kernel_shape": [2, 2], "dilations": [2, 1]})
    with pytest.raises(convert.ConvertError, match="dilation"):
        convert.model_from_graph(g, base)
    with pytest.raises(RuntimeError, match="dilation"):
        both_readers_native(g, tmp_path)


# ---- the container -----------------------------------------------------------------------------------------------------------------
def _records(path):
    raw = open(path, "rb").read()
    n_b, n_l = struct.unpack_from("<II", raw, 32)
    off = mf.HEADER_SIZE + n_b * mf.BRANCH_SIZE
    return [raw[off + i * mf.LAYER_SIZE:off + (i + 1) * mf.LAYER_SIZE] for i in range(n_l)]


@pytest.mark.parametrize("kind", ["dilated_plan", "dilated_resnet_audio"])
def test_the_round_trip_is_record_exact(kind, tmp_path):
    m = synth.build_model(kind, n_classes=None if kind == "dilated_plan" else 24)
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    back = mf.read_model(path)
    assert back.layers == m.layers and np.array_equal(back.blob, m.blob)
    for L, rec in zip(m.layers, _records(path)):
        assert struct.unpack_from("<II", rec, 88) == (L.dil_h - 1, L.dil_w - 1) and rec[96:] == bytes(32)
    assert dilated(m)
    # .bhm -> .onnx -> .bhm: convert.py reads back the model that was written, layer table and blob, bit for bit ...
    g = convert.graph_from_model(m)
    assert [n.attrs["dilations"] for n in g.nodes if n.op_type == "Conv"] == [[L.dil_h, L.dil_w] for L in m.layers if L.op in (CONV, DW, mf.OP_PWCONV)]
    same_records(m, convert.model_from_graph(ox.load(ox.dump(g)), m))
    # ... and the library's reader, from the audio input (the front end read off the graph; its blob is laid out in its own order),
    # the same records and the same weights
    native = native_from_model(m, tmp_path)
    assert len(native.layers) == len(m.layers)
    for i, (x, y) in enumerate(zip(m.layers, native.layers)):
        for f in RECORD[:-2] + ("dil_h", "dil_w"):
            assert getattr(x, f) == getattr(y, f), (i, f, getattr(x, f), getattr(y, f))
        k = N_W.get(x.op, lambda a: 0)(x)
        assert m.blob[x.w_off:x.w_off + k].tobytes() == native.blob[y.w_off:y.w_off + k].tobytes(), i
        if x.op in N_W:
            assert m.blob[x.b_off:x.b_off + x.cout].tobytes() == native.blob[y.b_off:y.b_off + y.cout].tobytes(), i


def test_header_fields_are_where_the_records_are_read(tmp_path):
    """(the helper above reads n_branches, n_layers at bytes 32, 36 of the header)"""
    m = synth.build_model("dilated_plan")
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    assert len(_records(path)) == len(m.layers)


@pytest.mark.parametrize("kind", ["mini", "mini_se", "resnet_plan", "resnext_plan", "branchy_plan", "pool_plan", "mnv3_plan"])
def test_existing_models_write_a_zero_tail(kind, tmp_path):
    plans = {"resnet_plan": synth.random_resnet_plan, "resnext_plan": synth.random_resnext_plan, "branchy_plan": synth.random_branchy_plan,
             "pool_plan": synth.random_pool_plan, "mnv3_plan": synth.random_mnv3_plan}
    m = synth.build_model(kind, plan=plans[kind](1)) if kind in plans else synth.build_model(kind)
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    assert all(rec[88:] == bytes(40) for rec in _records(path))
    # ... and through the library's writer, from the .onnx spelling
    native = native_from_model(m, tmp_path)
    assert all(rec[88:] == bytes(40) for rec in _records(str(tmp_path / "m_native.bhm"))) and len(native.layers) == len(m.layers)


# ---- the validator -----------------------------------------------------------------------------------------------------------------
def _load(path):
    """bh_plan_fused_blocks walks a model file on the host: load_model + validate_model; >= 0 = loaded (the fused blocks' count)"""
    L = _lib.load()
    rc = L.bh_plan_fused_blocks(path.encode(), 0, None, None, 0)
    return rc, L.bh_last_error().decode()


def _first(m, op, **where):
    return next(i for i, L in enumerate(m.layers) if L.op == op and all(getattr(L, k) == v for k, v in where.items()))


# case -> (the model, which record, the change, the validator's reason)
BAD_RECORDS = {
    "pool": (lambda: synth.build_model("pool_plan", plan=synth.random_pool_plan(1)), lambda m: _first(m, mf.OP_POOL), dict(dil_h=2), "dilation on a pool layer"),
    "grouped": (lambda: synth.build_model("resnext_plan", plan=synth.random_resnext_plan(1)), lambda m: _first(m, mf.OP_GCONV), dict(dil_w=2), "dilation on a grouped convolution layer"),
    "concat": (lambda: synth.build_model("branchy_plan", plan=synth.random_branchy_plan(1)), lambda m: _first(m, mf.OP_CONCAT), dict(dil_h=2), "dilation on a concat layer"),
    "pointwise": (lambda: synth.build_model("dilated_plan"), lambda m: _first(m, mf.OP_PWCONV), dict(dil_h=2, dil_w=2), "dilation on a pointwise layer"),
    "dense": (lambda: synth.build_model("dilated_plan"), lambda m: _first(m, mf.OP_DENSE), dict(dil_w=3), "dilation on a dense layer"),
    "global_pool": (lambda: synth.build_model("dilated_plan"), lambda m: _first(m, mf.OP_GAP), dict(dil_w=3), "dilation on a global pool layer"),
    "stem": (lambda: synth.build_model("dilated_plan"), lambda m: 0, dict(dil_h=2), "dilation on a stem convolution layer"),
    "above_16": (lambda: synth.build_model("dilated_plan"), lambda m: dilated(m)[0], dict(dil_h=17), "dilation above 16"),
    "above_16_depthwise": (lambda: synth.build_model("dilated_plan"), lambda m: _first(m, mf.OP_DWCONV), dict(dil_w=18), "dilation above 16"),
    "one_tap_axis": (lambda: synth.build_model("dilated_plan"), lambda m: dilated(m)[0], dict(kh=1, pad_t=0), "axis with one tap"),
}


@pytest.mark.parametrize("case", sorted(BAD_RECORDS))
def test_the_validator_refuses_a_bad_dilation_word(case, tmp_path):
    build, which, change, reason = BAD_RECORDS[case]
    m = build()
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc >= 0, msg                                   # the model loads as it stands
    L = m.layers[which(m)]
    for k, v in change.items():
        setattr(L, k, v)
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and reason in msg, (rc, msg)


def test_sixteen_loads(tmp_path):
    m = synth.build_model("dilated_plan")
    L = m.layers[dilated(m)[0]]
    L.dil_h = L.dil_w = 16
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc >= 0, msg


# ---- the planner -------------------------------------------------------------------------------------------------------------------
def test_the_block_with_the_dilated_depthwise_runs_layer_by_layer(plan, tmp_path):
    L = _lib.load()
    path = str(tmp_path / "m.bhm")
    i = _first(plan, mf.OP_DWCONV)
    assert plan.layers[i - 1].op == mf.OP_PWCONV and plan.layers[i + 1].op == mf.OP_PWCONV and plan.layers[i].dil_h == 2
    twin = copy.deepcopy(plan)
    D = twin.layers[i]
    D.dil_h = D.dil_w = D.pad_t = D.pad_l = 1               # the undilated 3x3 SAME layer of the same image
    for flags in (0, 1, 2, 3):          # BH_FLAG_AUTO, _F16X3, _F16, _F32
        mf.write_model(path, plan)
        layers = np.zeros(64, np.int32)
        n = L.bh_plan_fused_blocks(path.encode(), flags, None, layers.ctypes.data, 64)
        assert n == 0, (flags, n, L.bh_last_error(), layers[:max(n, 0)])
        mf.write_model(path, twin)
        n = L.bh_plan_fused_blocks(path.encode(), flags, None, layers.ctypes.data, 64)
        assert n == 1 and int(layers[0]) == i - 1, (flags, n, layers[:max(n, 0)])
