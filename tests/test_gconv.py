"""Grouped convolutions on the host side: the container's OP_GCONV record, both ONNX readers, the writer and the validator.

* hand-written graphs -- grouped 3x3 + BatchNormalization + ReLU, a grouped 1x1, a float16 file, SAME_UPPER at stride 2 -- go through
  the library's reader (bh_onnx_to_bhm) and through convert.py to the stated record, the same layer table and the same blob, bit for
  bit;
* forward64 -- tests/test_resact.py's float64 forward with OP_GCONV (oracle.oracle's conv_nhwc64 on every group's own channels) and
  OP_SCALE added; the device tests (tests/test_gconv_gpu.py) are held to it -- against a torch float64 composition with
  conv2d(groups = G);
* convert.model_to_onnx -> either reader reproduces the records of the random ResNeXt plans;
* every refusal of the readers and of the validator (model.hpp validate_model, through the library's host-only loader) is checked by
  its message;
* the OP_CONV / OP_DWCONV records of a model without a grouped layer are what they always were.
"""
import copy

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O
from test_pool import RECORD, both_readers, same_tables_and_blob
from test_resact import layer64


# ---- the yardstick: the model's logits in float64 ----------------------------------------------------------------------------------
def gconv_pre64(X, W, bias, L):
    """conv + bias of a grouped layer in float64: X [n][in_h][in_w][cin], W compact [kh][kw][cin / G][cout]; every group is an
    ordinary convolution (oracle.oracle conv_nhwc64) of its own input channels -> (pre [rows][cout], bound = |A| |W| + |b| over the
    group's own K)"""
    G, gi, go = L.reserved, L.cin // L.reserved, L.cout // L.reserved
    pre, bound = [], []
    for g in range(G):
        Wg = np.asarray(W[:, :, :, g * go:(g + 1) * go], np.float64)
        bg = np.asarray(bias[g * go:(g + 1) * go], np.float64)
        p, A = O.conv_nhwc64(X[..., g * gi:(g + 1) * gi], Wg, bg, L.sh, L.sw, L.pad_t, L.pad_l, L.out_h, L.out_w)
        pre.append(p)
        bound.append(np.abs(A) @ np.abs(Wg.reshape(-1, go)) + np.abs(bg))
    return np.concatenate(pre, axis=1), np.concatenate(bound, axis=1)


def layer64g(m, L, X, R):
    n = X.shape[0]
    if L.op == mf.OP_GCONV:
        assert R is None
        gi = L.cin // L.reserved
        W = np.asarray(m.blob[L.w_off:L.w_off + L.kh * L.kw * gi * L.cout], np.float64).reshape(L.kh, L.kw, gi, L.cout)
        pre, _ = gconv_pre64(np.asarray(X, np.float64).reshape(n, L.in_h, L.in_w, L.cin), W, m.blob[L.b_off:L.b_off + L.cout], L)
        return O.act64(pre, L.act).reshape(n, L.out_h, L.out_w, L.cout)
    if L.op == mf.OP_SCALE:      # the feature map times its [n][C] gate
        return np.asarray(X, np.float64).reshape(n, L.out_h, L.out_w, L.cout) * np.asarray(R, np.float64).reshape(n, 1, 1, L.cout)
    return layer64(m, L, X, R)


def forward64(m, segs, tensors=False):
    """-> logits [n][n_classes] in float64 (tensors=True: every tensor, T[0] the spectrogram)"""
    spec, _ = O.frontend64(m, segs)
    T = [spec]
    for L in m.layers:
        T.append(layer64g(m, L, T[L.in_tensor], None if L.res_tensor == mf.NO_TENSOR else T[L.res_tensor]))
    return T if tensors else T[-1].reshape(segs.shape[0], -1)


# ---- hand-written graphs through both readers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return synth.build_model("mini")          # the two-branch 32 x 115 front-end: a graph that starts at the spectrogram


def gconv_graph(group=8, cin=32, cout=32, kernel=(3, 3), attrs=None, bn=True, act="Relu", on_spectrogram=False, residual=False, bias=True,
                stem_c=None):
    """spectrogram [N, 2, 32, 115] -> Conv 3x3 stride 2 SAME (a 16 x 58 image of `cin` channels) -> Relu -> the grouped Conv under
    test [-> BatchNormalization] [-> activation] [-> Add with the stem] -> Conv 1x1 -> GlobalAveragePool -> Flatten -> Gemm"""
    rng = np.random.default_rng(11)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    g = ox.Graph(name="gconv_case", producer="tests")
    g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", 2, 32, 115]))
    x, c = "spectrogram", 2
    if not on_spectrogram:
        c = stem_c or cin
        g.initializers["w0"], g.initializers["b0"] = f32(c, 2, 3, 3) * np.float32(0.3), f32(c) * np.float32(0.1)
        g.nodes.append(ox.Node("Conv", ["spectrogram", "w0", "b0"], ["c0"], {"kernel_shape": [3, 3], "strides": [2, 2], "auto_pad": "SAME_UPPER"}, name="stem"))
        g.nodes.append(ox.Node("Relu", ["c0"], ["r0"]))
        x = "r0"
    kh, kw = kernel
    g.initializers["wg"] = f32(cout, max(cin // group, 1), kh, kw) * np.float32(0.2)
    ins = [x, "wg"]
    if bias:
        g.initializers["bg"] = f32(cout) * np.float32(0.1)
        ins.append("bg")
    a = {"group": group, "kernel_shape": [kh, kw]}
    a.update(attrs if attrs is not None else {"pads": [kh // 2, kw // 2, kh // 2, kw // 2]})
    g.nodes.append(ox.Node("Conv", ins, ["cg"], a, name="the_gconv"))
    x = "cg"
    if bn:
        for k in ("g", "b", "m", "v"):
            g.initializers["bn_" + k] = np.abs(f32(cout)) + np.float32(0.5)
        g.nodes.append(ox.Node("BatchNormalization", [x, "bn_g", "bn_b", "bn_m", "bn_v"], ["bn"], {"epsilon": 1e-3}, name="bn"))
        x = "bn"
    if residual:
        g.nodes.append(ox.Node("Add", [x, "r0"], ["sum"]))
        x = "sum"
    if act == "Relu":
        g.nodes.append(ox.Node("Relu", [x], ["ag"]))
        x = "ag"
    elif act == "swish":
        g.nodes.append(ox.Node("Sigmoid", [x], ["sg"]))
        g.nodes.append(ox.Node("Mul", [x, "sg"], ["ag"]))
        x = "ag"
    g.initializers["w1"], g.initializers["b1"] = f32(16, cout, 1, 1) * np.float32(0.2), f32(16) * np.float32(0.1)
    g.nodes.append(ox.Node("Conv", [x, "w1", "b1"], ["c1"], {"kernel_shape": [1, 1]}, name="head"))
    g.nodes.append(ox.Node("GlobalAveragePool", ["c1"], ["gap"]))
    g.nodes.append(ox.Node("Flatten", ["gap"], ["flat"], {"axis": 1}))
    g.initializers["w2"], g.initializers["b2"] = f32(16, 10), f32(10)
    g.nodes.append(ox.Node("Gemm", ["flat", "w2", "b2"], ["logits"]))
    g.outputs.append(ox.ValueInfo("logits", ox.FLOAT, ["N", 10]))
    return g


# case -> (graph arguments, the stated record: (cin, cout, kh, kw, sh, sw, pad_t, pad_l, out_h, out_w, act, groups)); the image
# behind the stem is 16 x 58; SAME_UPPER at stride 2 with a 3x3 kernel: out 8 x 29, total pad (7 * 2 + 3 - 16, 28 * 2 + 3 - 58) =
# (1, 1), the odd row / column at the end -> pad_t = pad_l = 0
ACCEPTED = {
    "g8_3x3_bn_relu": (dict(group=8), (32, 32, 3, 3, 1, 1, 1, 1, 16, 58, mf.ACT_RELU, 8)),
    "g4_1x1_swish_unequal": (dict(group=4, cin=32, cout=64, kernel=(1, 1), bn=False, act="swish"), (32, 64, 1, 1, 1, 1, 0, 0, 16, 58, mf.ACT_SWISH, 4)),
    "g2_same_upper_s2": (dict(group=2, attrs={"strides": [2, 2], "auto_pad": "SAME_UPPER"}, act=None), (32, 32, 3, 3, 2, 2, 0, 0, 8, 29, mf.ACT_NONE, 2)),
    "g3_width24_no_bias": (dict(group=3, cin=72, cout=72, bias=False), (72, 72, 3, 3, 1, 1, 1, 1, 16, 58, mf.ACT_RELU, 3)),
    "cin_groups_of_4_to_8": (dict(group=8, cin=32, cout=64, kernel=(1, 7), attrs={"pads": [0, 2, 0, 4]}, bn=False),
                             (32, 64, 1, 7, 1, 1, 0, 2, 16, 58, mf.ACT_RELU, 8)),
}


def _stated(rec):
    cin, cout, kh, kw, sh, sw, pt, pl, oh, ow, act, G = rec
    return dict(op=mf.OP_GCONV, act=act, in_tensor=1, res_tensor=mf.NO_TENSOR, cin=cin, cout=cout, kh=kh, kw=kw, sh=sh, sw=sw, pad_t=pt,
                pad_l=pl, in_h=16, in_w=58, out_h=oh, out_w=ow, in_layout=0, reserved=G)


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_both_readers_give_the_stated_record(case, base, tmp_path):
    kw, rec = ACCEPTED[case]
    want, got = both_readers(gconv_graph(**kw), base, tmp_path)
    same_tables_and_blob(want, got)
    assert [L.op for L in got.layers] == [mf.OP_CONV, mf.OP_GCONV, mf.OP_PWCONV, mf.OP_GAP, mf.OP_DENSE]
    for k, v in _stated(rec).items():
        assert getattr(got.layers[1], k) == v, (k, getattr(got.layers[1], k), v)
    assert got.layers[0].act == mf.ACT_RELU and got.layers[2].in_tensor == 2


def test_both_readers_read_a_float16_file_alike(base, tmp_path):
    g16 = convert.graph_to_float16(gconv_graph(group=8))
    assert all(a.dtype == np.float16 for a in g16.initializers.values())
    want, got = both_readers(g16, base, tmp_path)
    same_tables_and_blob(want, got)
    L = got.layers[1]
    assert (L.op, L.reserved, L.act) == (mf.OP_GCONV, 8, mf.ACT_RELU)
    # the compact weights are the float16 values times the folded BatchNormalization scale
    w16 = g16.initializers["wg"].astype(np.float64)
    scale = g16.initializers["bn_g"].astype(np.float64) / np.sqrt(g16.initializers["bn_v"].astype(np.float64) + float(np.float32(1e-3)))
    W = got.blob[L.w_off:L.w_off + 3 * 3 * 4 * 32].reshape(3, 3, 4, 32)
    assert np.array_equal(W, (w16.transpose(2, 3, 1, 0).astype(np.float32) * scale.astype(np.float32)))


def test_the_record_is_the_torch_grouped_convolution(base):
    """relu(bn(conv2d(x, groups = 8))) and the other accepted graphs composed in torch float64 from the graph's own initializers,
    against forward64's tensor behind the grouped layer of the converted model"""
    import torch
    import torch.nn.functional as F
    segs = synth.synth_segments(2, base.sample_count, base.sample_rate, start=3)
    for case in sorted(ACCEPTED):
        kw, rec = ACCEPTED[case]
        g = gconv_graph(**kw)
        m = convert.model_from_graph(ox.load(ox.dump(g)), base)
        T = forward64(m, segs, tensors=True)
        P = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in g.initializers.items()}
        x = torch.from_numpy(np.ascontiguousarray(T[1].transpose(0, 3, 1, 2)))          # the stem's output, NCHW
        L = m.layers[1]
        pad_b = max((L.out_h - 1) * L.sh + L.kh - L.in_h - L.pad_t, 0)
        pad_r = max((L.out_w - 1) * L.sw + L.kw - L.in_w - L.pad_l, 0)
        y = F.conv2d(F.pad(x, (L.pad_l, pad_r, L.pad_t, pad_b)), P["wg"], P.get("bg"), stride=(L.sh, L.sw), groups=L.reserved)
        if kw.get("bn", True):
            y = F.batch_norm(y, P["bn_m"], P["bn_v"], P["bn_g"], P["bn_b"], False, 0.0, float(np.float32(1e-3)))
        act = kw.get("act", "Relu")
        y = F.relu(y) if act == "Relu" else y * torch.sigmoid(y) if act == "swish" else y
        want = y.numpy().transpose(0, 2, 3, 1)
        got = T[2]
        assert got.shape == want.shape
        # (the folded weights are float32 products: 2^-24 relative per weight, summed over the group's K)
        assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (case, np.abs(got - want).max())
        # ... and the groups matter: the same weights read as groups of other channels give another tensor
        twin = copy.deepcopy(m)
        twin.blob = twin.blob.copy()
        gi = L.cin // L.reserved
        Wc = twin.blob[L.w_off:L.w_off + L.kh * L.kw * gi * L.cout].reshape(L.kh, L.kw, gi, L.cout)
        Wc[:] = np.roll(Wc, L.cout // L.reserved, axis=3)
        other = forward64(twin, segs, tensors=True)[2]
        assert np.abs(other - want).max() > 1e-3 * np.abs(want).max()


# ---- the writer, and the random plans -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_model_to_onnx_round_trip_reproduces_the_records(seed, tmp_path):
    plan = synth.random_resnext_plan(seed)
    assert plan == synth.random_resnext_plan(seed)
    m = synth.build_model("resnext_plan", plan=plan)
    grouped = [L for L in m.layers if L.op == mf.OP_GCONV]
    assert len(grouped) == 4 and sum(L.kh == 1 for L in grouped) == 1
    assert any(L.cin != L.cout for L in grouped) and {L.sh for L in grouped} == {1, 2}
    assert all(L.res_tensor == mf.NO_TENSOR and L.reserved >= 2 for L in grouped)
    data = convert.model_to_onnx(m)
    g = ox.load(data)
    convs = [n for n in g.nodes if n.op_type == "Conv" and int(n.attrs.get("group", 1)) > 1]
    assert len(convs) == 4
    for n, L in zip(convs, grouped):
        assert int(n.attrs["group"]) == L.reserved and g.initializers[n.inputs[1]].shape == (L.cout, L.cin // L.reserved, L.kh, L.kw)
    back = convert.model_from_graph(g, m)
    same_tables_and_blob(m, back)
    # ... and through the library's reader, from the audio input (the front-end read off the graph): the same records and weights
    onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m.bhm")
    with open(onnx_path, "wb") as f:
        f.write(convert.model_to_onnx(m, frontend_spelling="stft"))
    L_ = _lib.load()
    assert L_.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, L_.bh_last_error()
    native = mf.read_model(out)
    assert len(native.layers) == len(m.layers)
    for i, (x, y) in enumerate(zip(m.layers, native.layers)):
        for f in RECORD[:-2]:
            assert getattr(x, f) == getattr(y, f), (i, f)
        nw = {mf.OP_CONV: x.kh * x.kw * x.cin * x.cout, mf.OP_PWCONV: x.cin * x.cout, mf.OP_DENSE: x.cin * x.cout,
              mf.OP_GCONV: x.kh * x.kw * (x.cin // max(x.reserved, 1)) * x.cout}.get(x.op, 0)
        assert m.blob[x.w_off:x.w_off + nw].tobytes() == native.blob[y.w_off:y.w_off + nw].tobytes(), i
    # the float16 rewrite keeps the grouped layers
    m16 = convert.model_from_graph(convert.graph_to_float16(convert.graph_from_model(m)), m, "spectrogram")
    assert [(L.op, L.reserved) for L in m16.layers] == [(L.op, L.reserved) for L in m.layers]


def test_random_resnext_plans_hold_what_they_promise():
    widths, shortcuts, acts, gated = set(), set(), set(), 0
    for seed in range(6):
        plan = synth.random_resnext_plan(seed)
        m = synth.build_model("resnext_plan", plan=plan)
        for L in m.layers:
            if L.op == mf.OP_GCONV:
                widths |= {L.cin // L.reserved, L.cout // L.reserved}
        shortcuts |= {it[1] for it in plan["items"] if it[0] == "block"}
        acts.add(plan["act"])
        gated += any(L.op == mf.OP_SCALE for L in m.layers)
        assert sum(L.reserved == mf.RES_ACT_AFTER and L.op != mf.OP_GCONV and L.op != mf.OP_POOL for L in m.layers) == 3
        assert mf.Model.macs_per_segment(m) > 0
    assert widths == {4, 8, 16, 24, 32}
    assert shortcuts >= {"identity"} and shortcuts & {"proj", "resnetd"}
    assert acts == {mf.ACT_RELU, mf.ACT_RELU6, mf.ACT_SWISH, mf.ACT_GELU_ERF}
    assert 1 <= gated < 6


def test_resnext_audio_is_a_32x4d_trunk():
    m = synth.build_model("resnext_audio", n_classes=50)
    grouped = [L for L in m.layers if L.op == mf.OP_GCONV]
    assert len(grouped) == 8 and all(L.reserved == 32 and L.kh == 3 for L in grouped)
    assert sorted({L.cin // 32 for L in grouped}) == [4, 8, 16, 32]


# ---- refusals of the readers --------------------------------------------------------------------------------------------------------
REFUSED = {
    "dilation": (dict(group=8, attrs={"pads": [2, 2, 2, 2], "dilations": [2, 2]}), "dilation"),
    "width_2": (dict(group=16, cin=32, cout=32), "not a multiple of 4"),
    "out_width_6": (dict(group=4, cin=32, cout=24), "not a multiple of 4"),
    "depthwise_multiplier": (dict(group=32, cin=32, cout=64), "not a multiple of 4"),
    "on_the_spectrogram": (dict(group=2, cin=2, cout=8, on_spectrogram=True), "spectrogram"),
    "group_does_not_divide": (dict(group=5, cin=32, cout=40), "does not divide"),
    "weights_of_another_width": (dict(group=4, cin=64, cout=32, stem_c=32), "does not divide"),
    "kernel_9": (dict(group=8, kernel=(9, 3)), "1 .. 7"),
    "stride_3": (dict(group=8, attrs={"strides": [3, 3], "pads": [1, 1, 1, 1]}), "1 .. 2"),
    "residual": (dict(group=8, bn=False, residual=True), "no convolution to fold the residual into"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_both_readers_refuse_by_name(case, base, tmp_path):
    kw, reason = REFUSED[case]
    data = ox.dump(gconv_graph(**kw))
    with pytest.raises(convert.ConvertError) as e:
        convert.model_from_graph(ox.load(data), base)
    assert reason in str(e.value), str(e.value)
    onnx_path = str(tmp_path / "refused.onnx")
    with open(onnx_path, "wb") as f:
        f.write(data)
    L = _lib.load()
    assert L.bh_onnx_to_bhm(onnx_path.encode(), str(tmp_path / "refused.bhm").encode()) != 0
    msg = L.bh_last_error().decode()
    assert reason in msg, msg
    if case != "residual":
        assert "the_gconv" in msg, msg


# ---- the validator, through the library's host-only loader -------------------------------------------------------------------------
def _load(path):
    """bh_plan_fused_blocks walks a model file on the host: load_model + validate_model; >= 0 = loaded"""
    L = _lib.load()
    rc = L.bh_plan_fused_blocks(path.encode(), 0, None, None, 0)
    return rc, L.bh_last_error().decode()


def _grouped_model():
    """stem -> grouped 3x3 stride 1 (32 -> 32 in 4 groups: a residual of the right size exists) -> head -> pool -> dense"""
    b = synth._Builder(np.random.default_rng(1))
    base = synth.build_model("mini")
    m = copy.deepcopy(base)
    b.chunks, b.off = [np.asarray(base.blob)], base.blob.size
    t, h, w = b.conv(0, 32, 115, 2, 32, 3, 2, mf.ACT_RELU, in_layout=1)
    t, h, w = b.gconv(t, h, w, 32, 32, 3, 1, 4, mf.ACT_RELU)
    t = b.pwconv(t, h, w, 32, 16, mf.ACT_RELU)
    t = emb = b.gap(t, h, w, 16)
    b.dense(t, 16, 10)
    m.layers, m.blob, m.n_classes, m.embedding_dim, m.embedding_tensor = b.layers, np.concatenate(b.chunks), 10, 16, emb
    return m


BAD_RECORDS = {
    "one_group": (dict(reserved=1), "fewer than two groups"),
    "no_groups": (dict(reserved=0), "fewer than two groups"),
    "group_does_not_divide": (dict(reserved=3), "does not divide"),
    "width_2": (dict(reserved=16), "multiple of 4"),
    "residual": (dict(res_tensor=1), "residual"),
    "planar_layout": (dict(in_layout=1), "spectrogram"),
    "kernel_8": (dict(kh=8, pad_t=3, out_h=15), "kernel"),
    "stride_3": (dict(sh=3, out_h=6), "stride"),
    "weights_past_the_blob": (dict(reserved=2), "outside blob"),     # twice the weights of the 4-group layer, at the blob's end
}


def test_a_valid_grouped_container_loads(tmp_path):
    path = str(tmp_path / "ok.bhm")
    m = _grouped_model()
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc >= 0, msg
    back = mf.read_model(path)
    assert back.layers[1].op == mf.OP_GCONV == 8 and back.layers[1].reserved == 4
    # every activation code of the f32 layer kernels' switch is a valid one
    for act in range(7):
        m.layers[1].act = act
        mf.write_model(path, m)
        assert _load(path)[0] >= 0
    # op 9 is unknown
    m.layers[1].op = 9
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and "unknown layer op" in msg, msg


@pytest.mark.parametrize("case", sorted(BAD_RECORDS))
def test_the_validator_refuses_a_bad_grouped_record(case, tmp_path):
    change, reason = BAD_RECORDS[case]
    m = _grouped_model()
    if case == "weights_past_the_blob":      # move the grouped layer's weights to the end of the blob: G = 4 fits, G = 2 does not
        L = m.layers[1]
        n = 3 * 3 * 8 * 32
        m.blob = np.concatenate([m.blob, m.blob[L.w_off:L.w_off + n]])
        L.w_off = m.blob.size - n
        path = str(tmp_path / "fits.bhm")
        mf.write_model(path, m)
        assert _load(path)[0] >= 0
    for k, v in change.items():
        setattr(m.layers[1], k, v)
    path = str(tmp_path / "bad.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and reason in msg, (rc, msg)
    if case != "weights_past_the_blob":
        assert "grouped convolution" in msg, msg


# ---- nothing changes for a model without a grouped layer ----------------------------------------------------------------------------
def test_conv_and_depthwise_records_are_what_they_were(tmp_path):
    """synth's "mini" through the writer and both readers: OP_CONV and OP_DWCONV records (group 1, group == channels) and their
    weights come back as they went in, and the two readers write the same container, byte for byte"""
    m = synth.build_model("mini")
    assert {mf.OP_CONV, mf.OP_DWCONV} <= {L.op for L in m.layers} and not any(L.op == mf.OP_GCONV for L in m.layers)
    data = ox.dump(convert.graph_from_model(m))
    want = convert.model_from_graph(ox.load(data), m)
    same_tables_and_blob(m, want)
    onnx_path, native, py = (str(tmp_path / n) for n in ("mini.onnx", "native.bhm", "py.bhm"))
    with open(onnx_path, "wb") as f:
        f.write(data)
    L = _lib.load()
    assert L.bh_onnx_to_bhm(onnx_path.encode(), native.encode()) == 0, L.bh_last_error()
    mf.write_model(py, want)
    tables = mf.HEADER_SIZE + len(want.branches) * mf.BRANCH_SIZE
    assert open(native, "rb").read()[tables:] == open(py, "rb").read()[tables:]
    assert all(L.reserved == 0 for L in want.layers if L.op in (mf.OP_DWCONV,))
