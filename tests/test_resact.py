"""The activation AFTER a residual add -- act(conv + b + R), the end of a ResNet block -- on the host side: the container's
position word (Layer.reserved = RES_ACT_AFTER on OP_CONV / OP_PWCONV / OP_DENSE), the validator, both ONNX readers, the writer and
the block planner; and the float64 forward the device tests (tests/test_resact_gpu.py) are held to.

* a flagged model round-trips through write_model / read_model and loads; the validator (model.hpp validate_model, through the
  library's host-only loader) refuses a position above 1, the position without a residual, without an activation and on the NCHW stem,
  each with a reason of its own;
* synth.random_resnet_plan, 6 seeds: convert.model_to_onnx -> the library's reader (bh_onnx_to_bhm) and convert.model_from_graph
  give the same container, bit for bit, which is the model that was written -- layers, flags, weights --, and the same through
  graph_to_float16;
* act2(act1(conv) + x), a sum with a second reader and a sum that is a graph output with an activation behind it are refused by
  both readers, each by name; Mul(Sigmoid), the erf-GELU pattern and Clip(0, 6) behind an Add are accepted;
* the planner never takes a flagged layer as a fused block's project convolution, plain or squeeze-excite;
* forward64 -- tests/test_pool_gpu.py's float64 forward restated with the flag -- against a torch float64 composition
  (F.conv2d, F.relu(y + x)) of a basic block and a bottleneck, to 1e-12 of the output scale.
"""
import copy

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O
from test_pool import RECORD, both_readers, same_tables_and_blob
from test_pool_gpu import pool64

AFTER = mf.RES_ACT_AFTER
GEMM_OPS = (mf.OP_CONV, mf.OP_PWCONV, mf.OP_DENSE)


def flagged(m):
    """indices of the layers whose activation follows the residual add"""
    return [i for i, L in enumerate(m.layers) if L.op in GEMM_OPS and L.reserved == AFTER]


# ---- the yardstick: the model's logits in float64 ----------------------------------------------------------------------------------
def layer64(m, L, X, R):
    """One layer in float64 on the input X [n][...] and the residual R (or None): oracle.oracle's helpers, pool64 for OP_POOL, and
    the activation where the record puts it -- act(conv + b) + R, or act(conv + b + R) for Layer.reserved = RES_ACT_AFTER."""
    n = X.shape[0]
    w = lambda k: np.asarray(m.blob[L.w_off:L.w_off + k], np.float64)
    bias = np.asarray(m.blob[L.b_off:L.b_off + L.cout], np.float64)
    after = L.op in GEMM_OPS and L.reserved == AFTER
    act = (lambda v: v) if after else (lambda v: O.act64(v, L.act))
    if L.op == mf.OP_CONV and L.in_layout == 1:
        assert L.kh == L.kw and L.sh == L.sw and not after
        rows = O.stem_rows64(X, L.kh, L.sh, L.pad_t, L.pad_l, L.out_h, L.out_w)
        Y = act(O.gemm64(rows.reshape(-1, rows.shape[-1]), w(L.kh * L.kw * L.cin * L.cout).reshape(-1, L.cout), bias))
    elif L.op == mf.OP_CONV:
        X = X.reshape(n, L.in_h, L.in_w, L.cin)
        Y = act(O.conv_nhwc64(X, w(L.kh * L.kw * L.cin * L.cout).reshape(L.kh, L.kw, L.cin, L.cout), bias, L.sh, L.sw, L.pad_t, L.pad_l, L.out_h, L.out_w)[0])
    elif L.op == mf.OP_DWCONV:
        assert L.kh == L.kw and L.sh == L.sw
        X = X.reshape(n, L.in_h, L.in_w, L.cout)
        Y = act(O.depthwise64(X, w(L.kh * L.kw * L.cout).reshape(L.kh * L.kw, L.cout), L.kh, L.sh, L.pad_t, L.pad_l, L.out_h, L.out_w) + bias)
    elif L.op in (mf.OP_PWCONV, mf.OP_DENSE):
        Y = act(O.gemm64(X.reshape(-1, L.cin), w(L.cin * L.cout).reshape(L.cin, L.cout), bias))
    elif L.op == mf.OP_GAP:
        Y = X.reshape(n, -1, L.cout).mean(axis=1)
    elif L.op == mf.OP_POOL:
        Y = pool64(X, (L.in_h, L.in_w, L.out_h, L.out_w, L.cout, L.kh, L.kw, L.sh, L.sw, L.pad_t, L.pad_l), L.reserved)["ref"]
    else:
        raise AssertionError(L.op)
    Y = Y.reshape(n, L.out_h, L.out_w, L.cout)
    if R is not None:
        Y = Y + np.asarray(R, np.float64).reshape(Y.shape)
    return O.act64(Y, L.act) if after else Y


def forward64(m, segs, tensors=False):
    """-> logits [n][n_classes] in float64 (tensors=True: every tensor, T[0] the spectrogram)"""
    spec, _ = O.frontend64(m, segs)
    T = [spec]
    for L in m.layers:
        assert L.op != mf.OP_SCALE
        T.append(layer64(m, L, T[L.in_tensor], None if L.res_tensor == mf.NO_TENSOR else T[L.res_tensor]))
    return T if tensors else T[-1].reshape(segs.shape[0], -1)


def _block_model(kind, shortcut, act, c=8, cout=8, mid=4):
    """the mini front-end of one branch, a 3x3 stem to c channels, ONE ResNet block, the global pool and a dense layer"""
    b = synth._Builder(np.random.default_rng(5))
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    t, h, w = b.conv(0, br.n_mels, br.n_frames, 1, c, 3, 2, act, in_layout=1)
    t, h, w = synth._res_block(b, t, h, w, c, kind, shortcut, cout, mid, act)
    t = emb = b.gap(t, h, w, cout)
    b.dense(t, cout, 12, gain=1.5)
    return mf.Model(0, sr, n, n / sr, 12, cout, mf.OUT_SIGMOID, emb, br.n_mels, br.n_frames, 1e-6, [br], b.layers, np.concatenate(b.chunks))


@pytest.mark.parametrize("kind", ["basic", "bottleneck"])
def test_forward64_is_the_torch_float64_composition(kind):
    """relu(conv(relu(conv(x))) + x) and relu(conv1x1(relu(conv3x3(relu(conv1x1(x))))) + x), composed in torch float64 from the
    block's own weights, against forward64's tensor behind the block"""
    import torch
    import torch.nn.functional as F
    m = _block_model(kind, "identity", mf.ACT_RELU)
    assert len(flagged(m)) == 1
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=3)
    T = forward64(m, segs, tensors=True)
    x = torch.from_numpy(np.ascontiguousarray(T[1].transpose(0, 3, 1, 2)))          # the stem's output, NCHW

    def conv(y, L):
        if L.op == mf.OP_CONV:
            w = m.blob[L.w_off:L.w_off + L.kh * L.kw * L.cin * L.cout].astype(np.float64).reshape(L.kh, L.kw, L.cin, L.cout).transpose(3, 2, 0, 1)
        else:
            w = m.blob[L.w_off:L.w_off + L.cin * L.cout].astype(np.float64).reshape(L.cin, L.cout).T[:, :, None, None]
        pad_b = max((L.out_h - 1) * L.sh + L.kh - L.in_h - L.pad_t, 0)
        pad_r = max((L.out_w - 1) * L.sw + L.kw - L.in_w - L.pad_l, 0)
        y = F.pad(y, (L.pad_l, pad_r, L.pad_t, pad_b))
        return F.conv2d(y, torch.from_numpy(np.ascontiguousarray(w)), torch.from_numpy(m.blob[L.b_off:L.b_off + L.cout].astype(np.float64)), stride=(L.sh, L.sw))

    block = m.layers[1:-2]
    y = x
    for L in block[:-1]:
        y = F.relu(conv(y, L))
    y = F.relu(conv(y, block[-1]) + x)
    want = y.numpy().transpose(0, 2, 3, 1)
    got = T[len(m.layers) - 2]
    assert got.shape == want.shape and (want > 0).any() and (want == 0).any()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # ... and the position matters: the unflagged twin computes relu(conv) + x, a different tensor
    twin = copy.deepcopy(m)
    twin.layers[flagged(m)[0]].reserved = 0
    other = forward64(twin, segs, tensors=True)[len(m.layers) - 2]
    assert np.abs(other - want).max() > 1e-3 * np.abs(want).max()


# ---- the container and the validator ---------------------------------------------------------------------------------------------
def _load(path):
    """bh_plan_fused_blocks walks a model file on the host: load_model + validate_model; >= 0 = loaded (the fused blocks' count)"""
    L = _lib.load()
    rc = L.bh_plan_fused_blocks(path.encode(), 0, None, None, 0)
    return rc, L.bh_last_error().decode()


def test_a_flagged_container_round_trips_and_loads(tmp_path):
    assert mf.RES_ACT_AFTER == 1
    for kind, shortcut in (("basic", "identity"), ("bottleneck", "identity"), ("basic", "proj"), ("bottleneck", "resnetd")):
        m = _block_model(kind, shortcut, mf.ACT_RELU, cout=8 if shortcut == "identity" else 16)
        (i,) = flagged(m)
        assert m.layers[i].res_tensor != mf.NO_TENSOR and m.layers[i].act == mf.ACT_RELU
        assert m.layers[i].op == (mf.OP_PWCONV if (kind, shortcut) == ("bottleneck", "identity") or shortcut == "resnetd" else mf.OP_CONV)
        path = str(tmp_path / "m.bhm")
        mf.write_model(path, m)
        back = mf.read_model(path)
        same_tables_and_blob(m, back)
        assert flagged(back) == [i]
        rc, msg = _load(path)
        assert rc >= 0, msg


def _dense_residual_model():
    """a dense layer with a residual (two dense layers of equal width): the position word on OP_DENSE"""
    m = _block_model("basic", "identity", mf.ACT_RELU)
    b = synth._Builder(np.random.default_rng(2))
    b.chunks, b.off, b.layers = [np.asarray(m.blob)], m.blob.size, list(m.layers[:-1])
    t = len(b.layers)
    t1 = b.dense(t, 8, 12, logits=False)
    b.dense(t1, 12, 12)
    b.layers[-1].res_tensor, b.layers[-1].act, b.layers[-1].reserved = t1, mf.ACT_RELU, AFTER
    m.layers, m.blob = b.layers, np.concatenate(b.chunks)
    return m


BAD_RECORDS = {   # (which layer, the change) -> a word of the validator's reason
    "position_2": ("flagged", dict(reserved=2), "unknown activation position"),
    "position_2_on_a_dense_layer": ("dense", dict(reserved=2), "unknown activation position"),
    "position_2_on_an_unflagged_1x1": ("pw", dict(reserved=2), "unknown activation position"),
    "without_a_residual": ("flagged", dict(res_tensor=mf.NO_TENSOR), "without a residual"),
    "without_an_activation": ("flagged", dict(act=mf.ACT_NONE), "without an activation"),
    "on_the_nchw_stem": ("stem", dict(reserved=1), "NCHW stem"),
}


@pytest.mark.parametrize("case", sorted(BAD_RECORDS))
def test_the_validator_refuses_a_bad_position(case, tmp_path):
    which, change, reason = BAD_RECORDS[case]
    m = _block_model("bottleneck", "identity", mf.ACT_RELU)
    i = {"flagged": flagged(m)[0], "dense": len(m.layers) - 1, "stem": 0, "pw": 1}[which]
    assert which != "pw" or (m.layers[1].op == mf.OP_PWCONV and m.layers[1].reserved == 0)
    for k, v in change.items():
        setattr(m.layers[i], k, v)
    path = str(tmp_path / "bad.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and reason in msg, (rc, msg)
    reasons = {r for _, _, r in BAD_RECORDS.values()}
    assert sum(r in msg for r in reasons) == 1, msg            # a reason of its own


def test_the_position_on_a_dense_layer_loads_and_other_ops_stay_unchecked(tmp_path):
    m = _dense_residual_model()
    path = str(tmp_path / "dense.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc >= 0, msg
    assert flagged(mf.read_model(path))[-1] == len(m.layers) - 1
    # the reserved word of a depthwise / global-pool record is as unchecked as it was
    m = synth.build_model("mini")
    for L in m.layers:
        if L.op in (mf.OP_DWCONV, mf.OP_GAP):
            L.reserved = 7
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc >= 0, msg


# ---- the readers and the writer ------------------------------------------------------------------------------------------------------
N_W = {mf.OP_CONV: lambda a: a.kh * a.kw * a.cin * a.cout, mf.OP_DWCONV: lambda a: a.kh * a.kw * a.cout,
       mf.OP_PWCONV: lambda a: a.cin * a.cout, mf.OP_DENSE: lambda a: a.cin * a.cout}


@pytest.mark.parametrize("seed", range(6))
def test_both_readers_reproduce_a_random_resnet_plan(seed, tmp_path):
    plan = synth.random_resnet_plan(seed)
    assert plan == synth.random_resnet_plan(seed)
    m = synth.build_model("resnet_plan", plan=plan)
    fl = flagged(m)
    assert len(fl) >= 3 and any(m.layers[i].cout <= 64 for i in fl) and any(m.layers[i].cout > 64 for i in fl)
    assert all(m.layers[i].res_tensor != mf.NO_TENSOR and m.layers[i].act == plan["act"] for i in fl)
    # a flagged 1x1 layer above 64 channels that the split-f16 pointwise GEMMs take (K % 32 == 0), and a flagged full convolution there
    assert any(m.layers[i].op == mf.OP_PWCONV and m.layers[i].cout > 64 and m.layers[i].cin % 32 == 0 for i in fl), plan["items"]
    assert any(m.layers[i].op == mf.OP_CONV and m.layers[i].cout > 64 for i in fl), plan["items"]
    assert plan["act"] == (mf.ACT_RELU if seed % 2 == 0 else plan["act"]) and plan["act"] in (mf.ACT_RELU, mf.ACT_RELU6, mf.ACT_SWISH, mf.ACT_GELU_ERF)
    # an MBConv block whose input is a flagged layer's output
    dws = [i for i, L in enumerate(m.layers) if L.op == mf.OP_DWCONV]
    assert len(dws) == 1 and m.layers[dws[0] - 1].op == mf.OP_PWCONV and m.layers[dws[0] - 1].in_tensor - 1 in fl
    # the writer: Conv -> Add -> activation for a flagged layer
    g = convert.graph_from_model(m, spell_gelu="erf")
    assert convert.model_to_onnx(m) == ox.dump(g)
    prod = {o: n for n in g.nodes for o in n.outputs}
    for i in fl:
        add = next(n for n in g.nodes if n.op_type == "Add" and f"l{i}_conv" in n.inputs)
        assert prod[f"l{i}_conv"].op_type == "Conv" and add.outputs == [f"l{i}_res"]
        readers = [n for n in g.nodes if f"l{i}_res" in n.inputs]
        assert readers and all(n.op_type in ("Relu", "Clip", "Sigmoid", "Mul", "Div") for n in readers), [n.op_type for n in readers]
    # convert.py reads back the model that was written: layer table and blob, bit for bit
    want = convert.model_from_graph(ox.load(ox.dump(g)), m)
    same_tables_and_blob(m, want)
    # ... and the library's reader, from the audio input (the front-end read off the graph: the one-branch spectrogram is in no
    # family table), gives the same records and the same weights, bit for bit
    onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m.bhm")
    with open(onnx_path, "wb") as f:
        f.write(convert.model_to_onnx(m, frontend_spelling="stft"))
    L = _lib.load()
    assert L.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, L.bh_last_error()
    audio = mf.read_model(out)
    assert len(audio.layers) == len(m.layers)
    for i, (x, y) in enumerate(zip(m.layers, audio.layers)):
        for f in RECORD[:-2]:
            assert getattr(x, f) == getattr(y, f), (i, f)
        k = N_W.get(x.op, lambda a: 0)(x)
        assert m.blob[x.w_off:x.w_off + k].tobytes() == audio.blob[y.w_off:y.w_off + k].tobytes(), i
        if x.op in N_W:
            assert m.blob[x.b_off:x.b_off + x.cout].tobytes() == audio.blob[y.b_off:y.b_off + y.cout].tobytes(), i
    assert flagged(audio) == fl
    # the float16 rewrite carries the structure unchanged; both readers give the same container of it, bit for bit, and its
    # weights are float32(float16(w)) of the model's
    g16 = convert.graph_to_float16(convert.graph_from_model(m, frontend_spelling="conv1d"))
    assert [n.op_type for n in g16.nodes if n.op_type != "Cast"] == [n.op_type for n in convert.graph_from_model(m, frontend_spelling="conv1d").nodes]
    p16, bhm16 = str(tmp_path / "m16.onnx"), str(tmp_path / "m16.bhm")
    with open(p16, "wb") as f:
        f.write(ox.dump(g16))
    assert L.bh_onnx_to_bhm(p16.encode(), bhm16.encode()) == 0, L.bh_last_error()
    nat16 = mf.read_model(bhm16)
    want16 = convert.model_from_graph(ox.load(ox.dump(g16)), None, sample_rate=m.sample_rate)
    key = lambda a: (a.op, a.act, a.reserved, a.in_tensor, a.res_tensor, a.cin, a.cout, a.kh, a.kw, a.sh, a.sw, a.pad_t, a.pad_l, a.out_h, a.out_w)
    assert [key(a) for a in want16.layers] == [key(a) for a in nat16.layers] == [key(a) for a in m.layers]
    for a, b, c in zip(want16.layers, nat16.layers, m.layers):
        if a.op in N_W:
            k = N_W[a.op](a)
            wa, wb, wc = want16.blob[a.w_off:a.w_off + k], nat16.blob[b.w_off:b.w_off + k], m.blob[c.w_off:c.w_off + k]
            assert (wa.view(np.uint32) == wb.view(np.uint32)).all() and (wa == wc.astype(np.float16).astype(np.float32)).all()
            assert (want16.blob[a.b_off:a.b_off + a.cout].view(np.uint32) == nat16.blob[b.b_off:b.b_off + b.cout].view(np.uint32)).all()


def test_an_unflagged_residual_is_written_as_before():
    """act(conv) + x stays Conv -> activation -> Add: the bytes of a model without the flag are what they were"""
    m = synth.build_model("mini")
    g = convert.graph_from_model(m)
    for i, L in enumerate(m.layers):
        if L.op == mf.OP_PWCONV and L.res_tensor != mf.NO_TENSOR:
            add = next(n for n in g.nodes if n.outputs == [f"l{i}_res"])
            assert add.op_type == "Add" and not any(f"l{i}_res" in n.inputs and n.op_type in ("Relu", "Clip", "Sigmoid") for n in g.nodes)
    assert not flagged(convert.model_from_graph(g, m))


def block_graph(act_after, act_before=None, second_reader=False, sum_is_output=False, res_act=None):
    """spectrogram [N, 2, 32, 115] -> Conv 3x3 stride 2 (8) -> Relu -> r0; Conv 3x3 (8) on r0 [-> act_before] -> Add(., r0) ->
    act_after -> y; [a second reader of the sum: Conv 1x1 on it, added to y's 1x1]; Conv 1x1 -> GlobalAveragePool -> Flatten -> Gemm"""
    rng = np.random.default_rng(4)
    f32 = lambda *s: (rng.standard_normal(s) * 0.3).astype(np.float32)
    g = ox.Graph(name="resact_case", producer="tests")
    g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", 2, 32, 115]))
    g.initializers.update(w0=f32(8, 2, 3, 3), b0=f32(8), w1=f32(8, 8, 3, 3), b1=f32(8), w2=f32(16, 8, 1, 1), b2=f32(16), w3=f32(16, 10), b3=f32(10))
    g.nodes.append(ox.Node("Conv", ["spectrogram", "w0", "b0"], ["c0"], {"kernel_shape": [3, 3], "strides": [2, 2], "auto_pad": "SAME_UPPER"}, name="stem"))
    g.nodes.append(ox.Node("Relu", ["c0"], ["r0"]))
    g.nodes.append(ox.Node("Conv", ["r0", "w1", "b1"], ["c1"], {"kernel_shape": [3, 3], "auto_pad": "SAME_UPPER"}, name="main"))

    def activation(x, kind, tag):
        if kind == "relu":
            g.nodes.append(ox.Node("Relu", [x], [tag]))
        elif kind == "clip":
            g.initializers[tag + "_lo"], g.initializers[tag + "_hi"] = np.float32(0.0), np.float32(6.0)
            g.nodes.append(ox.Node("Clip", [x, tag + "_lo", tag + "_hi"], [tag]))
        elif kind == "swish":
            g.nodes.append(ox.Node("Sigmoid", [x], [tag + "_s"]))
            g.nodes.append(ox.Node("Mul", [x, tag + "_s"], [tag]))
        elif kind == "gelu":
            g.initializers[tag + "_q"], g.initializers[tag + "_1"], g.initializers[tag + "_h"] = np.float32(np.sqrt(2.0)), np.float32(1.0), np.float32(0.5)
            g.nodes.append(ox.Node("Div", [x, tag + "_q"], [tag + "_d"]))
            g.nodes.append(ox.Node("Erf", [tag + "_d"], [tag + "_e"]))
            g.nodes.append(ox.Node("Add", [tag + "_e", tag + "_1"], [tag + "_a"]))
            g.nodes.append(ox.Node("Mul", [x, tag + "_a"], [tag + "_m"]))
            g.nodes.append(ox.Node("Mul", [tag + "_m", tag + "_h"], [tag]))
        else:
            raise ValueError(kind)
        return tag

    x = "c1"
    if act_before:
        x = activation(x, act_before, "before")
    g.nodes.append(ox.Node("Add", [x, "r0"], ["sum"], name="the_add"))
    y = activation("sum", act_after, "after") if act_after else "sum"
    g.nodes.append(ox.Node("Conv", [y, "w2", "b2"], ["c2"], {"kernel_shape": [1, 1]}, name="head"))
    last = "c2"
    if second_reader:
        g.initializers["w2b"], g.initializers["b2b"] = f32(16, 8, 1, 1), f32(16)
        g.nodes.append(ox.Node("Conv", ["sum", "w2b", "b2b"], ["c2b"], {"kernel_shape": [1, 1]}, name="second_reader"))
        g.nodes.append(ox.Node("Add", ["c2b", "c2"], ["c2s"]))
        last = "c2s"
    g.nodes.append(ox.Node("GlobalAveragePool", [last], ["gap"]))
    g.nodes.append(ox.Node("Flatten", ["gap"], ["flat"], {"axis": 1}))
    g.nodes.append(ox.Node("Gemm", ["flat", "w3", "b3"], ["logits"]))
    g.outputs.append(ox.ValueInfo("logits", ox.FLOAT, ["N", 10]))
    if sum_is_output:
        g.outputs.append(ox.ValueInfo("sum", ox.FLOAT, ["N", 8, 16, 58]))
    return g


@pytest.fixture(scope="module")
def base():
    return synth.build_model("mini")


SPELLINGS = {"relu": mf.ACT_RELU, "clip": mf.ACT_RELU6, "swish": mf.ACT_SWISH, "gelu": mf.ACT_GELU_ERF}


@pytest.mark.parametrize("spelling", sorted(SPELLINGS))
def test_every_spelling_behind_an_add_sets_the_flag(spelling, base, tmp_path):
    want, got = both_readers(block_graph(spelling), base, tmp_path)
    same_tables_and_blob(want, got)
    assert [L.op for L in got.layers] == [mf.OP_CONV, mf.OP_CONV, mf.OP_PWCONV, mf.OP_GAP, mf.OP_DENSE]
    B = got.layers[1]
    assert (B.act, B.reserved, B.res_tensor) == (SPELLINGS[spelling], AFTER, 1)
    assert got.layers[0].act == mf.ACT_RELU and got.layers[0].reserved == 0 and got.layers[2].in_tensor == 2 and got.layers[2].reserved == 0


def test_without_an_activation_behind_it_the_add_is_what_it_was(base, tmp_path):
    for before, act in ((None, mf.ACT_NONE), ("swish", mf.ACT_SWISH)):
        want, got = both_readers(block_graph(None, act_before=before), base, tmp_path)
        same_tables_and_blob(want, got)
        assert (got.layers[1].act, got.layers[1].reserved, got.layers[1].res_tensor) == (act, 0, 1)


REFUSED = {
    "an_activation_on_both_sides": (dict(act_after="relu", act_before="relu"), "both sides of a residual Add"),
    "both_sides_multi_node": (dict(act_after="swish", act_before="gelu"), "both sides of a residual Add"),
    "a_second_reader_of_the_sum": (dict(act_after="relu", second_reader=True), "another reader"),
    "a_second_reader_multi_node": (dict(act_after="gelu", second_reader=True), "another reader"),
    "the_sum_is_a_graph_output": (dict(act_after="clip", sum_is_output=True), "graph output"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_both_readers_refuse_by_name(case, base, tmp_path):
    kw, reason = REFUSED[case]
    data = ox.dump(block_graph(**kw))
    with pytest.raises(convert.ConvertError) as e:
        convert.model_from_graph(ox.load(data), base)
    assert reason in str(e.value) and "'sum'" in str(e.value), str(e.value)
    onnx_path = str(tmp_path / "refused.onnx")
    with open(onnx_path, "wb") as f:
        f.write(data)
    L = _lib.load()
    assert L.bh_onnx_to_bhm(onnx_path.encode(), str(tmp_path / "refused.bhm").encode()) != 0
    msg = L.bh_last_error().decode()
    assert reason in msg and "'sum'" in msg, msg


def test_what_was_refused_behind_an_add_stays_refused(base):
    """BatchNormalization behind the sum, and a second activation behind a flagged layer's"""
    g = block_graph("relu")
    i = next(k for k, n in enumerate(g.nodes) if n.name == "head")
    g.nodes.insert(i, ox.Node("Relu", ["after"], ["again"]))
    g.nodes[i + 1].inputs[0] = "again"
    with pytest.raises(convert.ConvertError, match="cannot be folded"):
        convert.model_from_graph(g, base)
    g = block_graph(None)
    for k in ("g", "b", "m", "v"):
        g.initializers["bn_" + k] = np.full(8, 0.7, np.float32)
    i = next(k for k, n in enumerate(g.nodes) if n.name == "head")
    g.nodes.insert(i, ox.Node("BatchNormalization", ["sum", "bn_g", "bn_b", "bn_m", "bn_v"], ["bn"], {"epsilon": 1e-3}))
    g.nodes[i + 1].inputs[0] = "bn"
    with pytest.raises(convert.ConvertError, match="BatchNormalization after a residual Add"):
        convert.model_from_graph(g, base)


# ---- the planner ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mini", "mini_se"])
def test_a_flagged_project_convolution_is_never_fused(kind, tmp_path):
    """every residual MBConv block of the toy stack with act(project + x) instead of project + x: those blocks run layer by layer
    (fewer fused blocks, none of them ending in a flagged layer), in every precision"""
    L = _lib.load()
    m = synth.build_model(kind)
    proj = [i for i, Lr in enumerate(m.layers) if Lr.op == mf.OP_PWCONV and Lr.res_tensor != mf.NO_TENSOR and i >= 2 and
            m.layers[i - 1].op in (mf.OP_DWCONV, mf.OP_SCALE)]
    assert proj
    path = str(tmp_path / "m.bhm")
    def project_of(first):
        return next(j for j in range(first + 1, len(m.layers)) if m.layers[j].op == mf.OP_PWCONV and m.layers[j - 1].op in (mf.OP_DWCONV, mf.OP_SCALE))

    for flags in (0, 1, 2, 3):          # BH_FLAG_AUTO, _F16X3, _F16, _F32
        mf.write_model(path, m)
        layers = np.zeros(64, np.int32)
        before = L.bh_plan_fused_blocks(path.encode(), flags, None, layers.ctypes.data, 64)
        assert before > 0, L.bh_last_error()
        fused_before = {project_of(int(f)) for f in layers[:before]}
        assert fused_before & set(proj), (flags, fused_before, proj)          # residual blocks run fused as the model stands
        m2 = copy.deepcopy(m)
        for i in proj:
            m2.layers[i].act, m2.layers[i].reserved = mf.ACT_RELU6, AFTER
        mf.write_model(path, m2)
        layers2 = np.zeros(64, np.int32)
        after = L.bh_plan_fused_blocks(path.encode(), flags, None, layers2.ctypes.data, 64)
        assert after >= 0, L.bh_last_error()
        fused_after = {project_of(int(f)) for f in layers2[:after]}
        assert not (fused_after & set(proj)) and fused_after == fused_before - set(proj), (flags, fused_before, fused_after, proj)
