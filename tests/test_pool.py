"""MaxPool / AveragePool on the host side: the container's OP_POOL record, both ONNX readers, the writer and the validator.

* every accepted spelling gives the stated record (mode included) through the library's reader (bh_onnx_to_bhm) and through
  convert.py, and the two give the same layer table and the same blob, bit for bit;
* convert.model_to_onnx -> either reader reproduces the records of the synth models that hold pools;
* every refused spelling is refused by both readers, the library's message naming the operator and the reason;
* the validator (model.hpp validate_model, through the library's host-only loader) refuses a pool record with an unknown mode, a
  channel change, an activation, a residual or a window in the padding alone;
* a graph without a pool converts to the bytes it always did, and a model without a pool is written with a zero reserved word.
"""
import copy
import ctypes as C
import struct

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth

RECORD = ("op", "act", "in_tensor", "res_tensor", "cin", "cout", "kh", "kw", "sh", "sw", "pad_t", "pad_l", "in_h", "in_w", "out_h",
          "out_w", "in_layout", "reserved", "w_off", "b_off")


@pytest.fixture(scope="module")
def base():
    return synth.build_model("mini")          # the two-branch 32 x 115 front-end: a graph that starts at the spectrogram


def pool_graph(base, op, attrs, image="7x9", after=None, indices=False, on_spectrogram=False):
    """spectrogram [N, 2, 32, 115] -> Conv (2x7 stride 5x13: a 7 x 9 image of 8 channels; or 3x3 SAME: 32 x 115) -> Relu -> the pool
    under test [-> `after`] -> Conv 1x1 -> GlobalAveragePool -> Flatten -> Gemm"""
    rng = np.random.default_rng(3)
    g = ox.Graph(name="pool_case", producer="tests")
    g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", 2, 32, 115]))
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    c = 2
    x = "spectrogram"
    if not on_spectrogram:
        c = 8
        if image == "7x9":
            g.initializers["w0"] = f32(8, 2, 2, 7)
            g.nodes.append(ox.Node("Conv", ["spectrogram", "w0", "b0"], ["c0"], {"kernel_shape": [2, 7], "strides": [5, 13]}, name="stem"))
        else:
            g.initializers["w0"] = f32(8, 2, 3, 3)
            g.nodes.append(ox.Node("Conv", ["spectrogram", "w0", "b0"], ["c0"], {"kernel_shape": [3, 3], "auto_pad": "SAME_UPPER"}, name="stem"))
        g.initializers["b0"] = f32(8)
        g.nodes.append(ox.Node("Relu", ["c0"], ["r0"]))
        x = "r0"
    g.nodes.append(ox.Node(op, [x], ["p"] + (["p_idx"] if indices else []), dict(attrs), name="the_pool"))
    x = "p"
    if after == "Relu":
        g.nodes.append(ox.Node("Relu", [x], ["pa"]))
        x = "pa"
    elif after == "BatchNormalization":
        for k in ("g", "b", "m", "v"):
            g.initializers["bn_" + k] = np.abs(f32(c)) + np.float32(0.5)
        g.nodes.append(ox.Node("BatchNormalization", [x, "bn_g", "bn_b", "bn_m", "bn_v"], ["pa"], {"epsilon": 1e-3}, name="bn"))
        x = "pa"
    g.initializers["w1"], g.initializers["b1"] = f32(16, c, 1, 1), f32(16)
    g.nodes.append(ox.Node("Conv", [x, "w1", "b1"], ["c1"], {"kernel_shape": [1, 1]}, name="head"))
    g.nodes.append(ox.Node("GlobalAveragePool", ["c1"], ["gap"]))
    g.nodes.append(ox.Node("Flatten", ["gap"], ["flat"], {"axis": 1}))
    g.initializers["w2"], g.initializers["b2"] = f32(16, 10), f32(10)
    g.nodes.append(ox.Node("Gemm", ["flat", "w2", "b2"], ["logits"]))
    g.outputs.append(ox.ValueInfo("logits", ox.FLOAT, ["N", 10]))
    return g


def both_readers(g, base, tmp_path):
    """-> (convert.py's model, the library's model) of graph g"""
    data = ox.dump(g)
    onnx_path, out = str(tmp_path / "case.onnx"), str(tmp_path / "case.bhm")
    with open(onnx_path, "wb") as f:
        f.write(data)
    want = convert.model_from_graph(ox.load(data), base)
    L = _lib.load()
    rc = L.bh_onnx_to_bhm(onnx_path.encode(), out.encode())
    if rc != 0:
        raise RuntimeError(f"rc {rc}: {L.bh_last_error().decode()}")
    return want, mf.read_model(out)


def same_tables_and_blob(a, b):
    assert len(a.layers) == len(b.layers)
    for i, (x, y) in enumerate(zip(a.layers, b.layers)):
        for f in RECORD:
            assert getattr(x, f) == getattr(y, f), (i, f, getattr(x, f), getattr(y, f))
    assert np.asarray(a.blob, "<f4").tobytes() == np.asarray(b.blob, "<f4").tobytes()


MAX, AVG, AVG_PAD = mf.POOL_MAX, mf.POOL_AVG, mf.POOL_AVG_PAD
# (operator, attributes) on the 7 x 9 x 8 image -> (kh, kw, sh, sw, pad_t, pad_l, out_h, out_w, mode), worked out by hand from the
# ONNX definition: out = floor((in + pad_begin + pad_end - k) / s) + 1; SAME: out = ceil(in / s), total = (out - 1) s + k - in,
# UPPER puts the odd row / column at the end, LOWER at the start
ACCEPTED = {
    "max_2x2_default_strides": ("MaxPool", {"kernel_shape": [2, 2]}, (2, 2, 1, 1, 0, 0, 6, 8, MAX)),
    "max_2x2_s2": ("MaxPool", {"kernel_shape": [2, 2], "strides": [2, 2]}, (2, 2, 2, 2, 0, 0, 3, 4, MAX)),
    "avg_3x3_s1_pads1": ("AveragePool", {"kernel_shape": [3, 3], "strides": [1, 1], "pads": [1, 1, 1, 1]}, (3, 3, 1, 1, 1, 1, 7, 9, AVG)),
    "max_5x3_s21_pads_asym": ("MaxPool", {"kernel_shape": [5, 3], "strides": [2, 1], "pads": [2, 0, 1, 0]}, (5, 3, 2, 1, 2, 0, 3, 7, MAX)),
    "avg_1x2_s3": ("AveragePool", {"kernel_shape": [1, 2], "strides": [3, 3]}, (1, 2, 3, 3, 0, 0, 3, 3, AVG)),
    "max_same_upper_even": ("MaxPool", {"kernel_shape": [2, 2], "strides": [2, 2], "auto_pad": "SAME_UPPER"}, (2, 2, 2, 2, 0, 0, 4, 5, MAX)),
    "max_same_lower_even": ("MaxPool", {"kernel_shape": [2, 2], "strides": [2, 2], "auto_pad": "SAME_LOWER"}, (2, 2, 2, 2, 1, 1, 4, 5, MAX)),
    "avg_same_upper_even": ("AveragePool", {"kernel_shape": [4, 2], "strides": [2, 2], "auto_pad": "SAME_UPPER"}, (4, 2, 2, 2, 1, 0, 4, 5, AVG)),
    "avg_same_lower_even": ("AveragePool", {"kernel_shape": [4, 2], "strides": [2, 2], "auto_pad": "SAME_LOWER"}, (4, 2, 2, 2, 2, 1, 4, 5, AVG)),
    "max_valid_3x3_s2": ("MaxPool", {"kernel_shape": [3, 3], "strides": [2, 2], "auto_pad": "VALID"}, (3, 3, 2, 2, 0, 0, 3, 4, MAX)),
    "avg_exclude_pad": ("AveragePool", {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1], "count_include_pad": 0},
                        (3, 3, 2, 2, 1, 1, 4, 5, AVG)),
    "avg_include_pad": ("AveragePool", {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1], "count_include_pad": 1},
                        (3, 3, 2, 2, 1, 1, 4, 5, AVG_PAD)),
    "max_ceil_mode_same_size": ("MaxPool", {"kernel_shape": [3, 3], "strides": [2, 2], "ceil_mode": 1}, (3, 3, 2, 2, 0, 0, 3, 4, MAX)),
    "avg_3x3_s3": ("AveragePool", {"kernel_shape": [3, 3], "strides": [3, 3]}, (3, 3, 3, 3, 0, 0, 2, 3, AVG)),
    "max_dilations_of_one": ("MaxPool", {"kernel_shape": [2, 2], "strides": [2, 2], "dilations": [1, 1], "storage_order": 0}, (2, 2, 2, 2, 0, 0, 3, 4, MAX)),
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_both_readers_give_the_stated_pool_record(case, base, tmp_path):
    op, attrs, (kh, kw, sh, sw, pt, pl, oh, ow, mode) = ACCEPTED[case]
    want, got = both_readers(pool_graph(base, op, attrs), base, tmp_path)
    same_tables_and_blob(want, got)
    assert [L.op for L in got.layers] == [mf.OP_CONV, mf.OP_POOL, mf.OP_PWCONV, mf.OP_GAP, mf.OP_DENSE]
    P = got.layers[1]
    stated = mf.Layer(mf.OP_POOL, mf.ACT_NONE, 1, mf.NO_TENSOR, 8, 8, kh, kw, sh, sw, pt, pl, 7, 9, oh, ow, 0, 0, 0, mode)
    assert P == stated, (P, stated)
    assert got.layers[0].act == mf.ACT_RELU and got.layers[2].act == mf.ACT_NONE          # the Relu in front stays on the stem
    assert (got.layers[2].in_h, got.layers[2].in_w, got.layers[2].in_tensor) == (oh, ow, 2)


REFUSED = {
    "dilation": ("MaxPool", {"kernel_shape": [2, 2], "dilations": [2, 1]}, {}, "dilation"),
    "storage_order": ("MaxPool", {"kernel_shape": [2, 2], "storage_order": 1}, {}, "storage_order"),
    "indices": ("MaxPool", {"kernel_shape": [2, 2]}, {"indices": True}, "Indices"),
    "ceil_mode_changes_size": ("AveragePool", {"kernel_shape": [2, 2], "strides": [2, 2], "ceil_mode": 1}, {}, "ceil_mode"),
    "window_in_the_padding": ("MaxPool", {"kernel_shape": [3, 3], "pads": [3, 0, 0, 0]}, {}, "in-image tap"),
    "window_past_the_image": ("AveragePool", {"kernel_shape": [2, 2], "strides": [4, 4], "pads": [0, 0, 3, 0]}, {}, "in-image tap"),
    "on_the_spectrogram": ("MaxPool", {"kernel_shape": [2, 2]}, {"on_spectrogram": True}, "spectrogram"),
    "activation_behind": ("MaxPool", {"kernel_shape": [2, 2]}, {"after": "Relu"}, "activation"),
    "batchnorm_behind": ("AveragePool", {"kernel_shape": [2, 2]}, {"after": "BatchNormalization"}, "BatchNormalization"),
    "no_kernel_shape": ("MaxPool", {"strides": [2, 2]}, {}, "kernel_shape"),
    "kernel_65": ("MaxPool", {"kernel_shape": [65, 1], "pads": [32, 0, 32, 0]}, {}, "kernel_shape"),
    "stride_17": ("AveragePool", {"kernel_shape": [2, 2], "strides": [17, 1]}, {}, "strides"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_both_readers_refuse_by_name(case, base, tmp_path):
    op, attrs, kw, reason = REFUSED[case]
    g = pool_graph(base, op, attrs, **kw)
    data = ox.dump(g)
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
    if case not in ("activation_behind", "batchnorm_behind"):
        assert op in msg and "the_pool" in msg, msg            # the operator and the node
    else:
        assert "Pool" in msg or "convolution" in msg, msg      # what the activation / normalisation follows


def test_an_activation_in_front_of_a_pool_stays_on_the_convolution(base):
    """Relu -> pool: the Relu is the convolution's, the pool record carries none (pool -> Relu: REFUSED["activation_behind"])."""
    g = pool_graph(base, "AveragePool", {"kernel_shape": [2, 2]})
    m = convert.model_from_graph(g, base)
    assert m.layers[1].op == mf.OP_POOL and m.layers[1].act == mf.ACT_NONE and m.layers[0].act == mf.ACT_RELU


@pytest.mark.parametrize("kind", ["cnn_pool", "pool0", "pool1", "pool2", "pool3", "pool4", "pool5"])
def test_model_to_onnx_round_trip_reproduces_the_records(kind, tmp_path):
    m = synth.build_model("cnn_pool", n_classes=40) if kind == "cnn_pool" else synth.build_model("pool_plan", plan=synth.random_pool_plan(int(kind[4:])))
    pools = [L for L in m.layers if L.op == mf.OP_POOL]
    assert len(pools) >= 3
    if kind != "cnn_pool":
        assert sorted(L.reserved for L in pools) == [0, 1, 2]
    data = convert.model_to_onnx(m)
    assert data == ox.dump(convert.graph_from_model(m))
    g = ox.load(data)
    assert sum(n.op_type in ("MaxPool", "AveragePool") for n in g.nodes) == len(pools)
    assert all(len(n.attrs["pads"]) == 4 for n in g.nodes if n.op_type in ("MaxPool", "AveragePool"))       # explicit pads
    back = convert.model_from_graph(g, m)
    same_tables_and_blob(m, back)
    # ... and through the library's reader, from the audio input (the front-end read off the graph): the same records and weights
    onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m.bhm")
    with open(onnx_path, "wb") as f:
        f.write(convert.model_to_onnx(m, frontend_spelling="stft"))
    L = _lib.load()
    assert L.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, L.bh_last_error()
    native = mf.read_model(out)
    assert len(native.layers) == len(m.layers)
    for i, (x, y) in enumerate(zip(m.layers, native.layers)):
        for f in RECORD[:-2]:
            assert getattr(x, f) == getattr(y, f), (i, f)
        nw = {mf.OP_CONV: x.kh * x.kw * x.cin * x.cout, mf.OP_DWCONV: x.kh * x.kw * x.cout, mf.OP_PWCONV: x.cin * x.cout, mf.OP_DENSE: x.cin * x.cout}.get(x.op, 0)
        assert m.blob[x.w_off:x.w_off + nw].tobytes() == native.blob[y.w_off:y.w_off + nw].tobytes(), i
        if x.op == mf.OP_POOL:
            assert (y.w_off, y.b_off) == (0, 0)
    # the float16 rewrite of the graph keeps its pools
    g16 = convert.graph_to_float16(convert.graph_from_model(m, frontend_spelling="stft"))
    m16 = convert.model_from_graph(g16, m, "spectrogram")
    assert [(L.op, L.reserved, L.kh, L.kw, L.out_h, L.out_w) for L in m16.layers] == [(L.op, L.reserved, L.kh, L.kw, L.out_h, L.out_w) for L in m.layers]


def test_random_pool_plans_hold_what_they_promise():
    """a pool directly behind an MBConv block, a pool in a shortcut (Add(conv, conv1x1(pool(x)))), non-square kernels, strides up to
    3 and every kind of padding, over the seeds the device tests run"""
    kernels, strides, pads = set(), set(), set()
    for seed in range(6):
        plan = synth.random_pool_plan(seed)
        assert plan == synth.random_pool_plan(seed)
        m = synth.build_model("pool_plan", plan=plan)
        behind_block = shortcut = False
        for i, L in enumerate(m.layers):
            if L.op != mf.OP_POOL:
                continue
            prev = m.layers[L.in_tensor - 1]
            if L.in_tensor == i and prev.op == mf.OP_PWCONV and m.layers[i - 2].op == mf.OP_DWCONV:
                behind_block = True
            readers = [M for M in m.layers if M.in_tensor == i + 1]
            if len(readers) == 1 and readers[0].op == mf.OP_PWCONV and any(M.in_tensor == L.in_tensor and M.op == mf.OP_CONV for M in m.layers):
                j = m.layers.index(readers[0])
                shortcut = shortcut or readers[0].res_tensor != mf.NO_TENSOR or any(M.res_tensor == j + 1 for M in m.layers)
            kernels.add((L.kh, L.kw)); strides.add((L.sh, L.sw))
        assert behind_block and shortcut, (seed, plan["items"])
        pads |= {it[6] if isinstance(it[6], str) else "explicit" for it in plan["items"] if it[0] == "pool"}
    assert any(kh != kw for kh, kw in kernels) and {k for kk in kernels for k in kk} == {2, 3, 5}
    assert {s for ss in strides for s in ss} == {1, 2, 3}
    assert pads >= {"valid", "explicit"} and pads & {"same", "same_lower"}


# ---- the validator, through the library's host-only loader ---------------------------------------------------------------------
def _load(path):
    """bh_plan_fused_blocks walks a model file on the host: load_model + validate_model; >= 0 = loaded"""
    L = _lib.load()
    rc = L.bh_plan_fused_blocks(path.encode(), 0, None, None, 0)
    return rc, L.bh_last_error().decode()


def _pooled_model():
    """stem -> 3x3 stride-1 average pool with pad 1 (the shape stays: a residual of the right size exists) -> head -> pool -> dense"""
    b = synth._Builder(np.random.default_rng(1))
    base = synth.build_model("mini")
    m = copy.deepcopy(base)
    b.chunks, b.off = [np.asarray(base.blob)], base.blob.size
    t, h, w = b.conv(0, 32, 115, 2, 8, 3, 2, mf.ACT_RELU, in_layout=1)
    t, h, w = b.pool(t, h, w, 8, 3, 3, 1, 1, mf.POOL_AVG, (1, 1, 1, 1))
    t = b.pwconv(t, h, w, 8, 16, mf.ACT_RELU)
    t = emb = b.gap(t, h, w, 16)
    b.dense(t, 16, 10)
    m.layers, m.blob, m.n_classes, m.embedding_dim, m.embedding_tensor = b.layers, np.concatenate(b.chunks), 10, 16, emb
    return m


BAD_RECORDS = {
    "mode_3": (dict(reserved=3), "mode"),
    "channel_change": (dict(cin=12), "channel"),
    "activation": (dict(act=mf.ACT_RELU), "activation"),
    "residual": (dict(res_tensor=1), "residual"),
    "pad_t_is_kh": (dict(pad_t=3), "window"),
    "pad_l_past_kw": (dict(pad_l=4), "window"),
    "last_row_past_the_image": (dict(sh=16, out_h=3), "window"),
    "planar_layout": (dict(in_layout=1), "planar"),
}


def test_a_valid_pool_container_loads(tmp_path):
    path = str(tmp_path / "ok.bhm")
    mf.write_model(path, _pooled_model())
    rc, msg = _load(path)
    assert rc >= 0, msg
    back = mf.read_model(path)
    assert back.layers[1].op == mf.OP_POOL and back.layers[1].reserved == mf.POOL_AVG
    for mode in (mf.POOL_MAX, mf.POOL_AVG_PAD):
        m = _pooled_model()
        m.layers[1].reserved = mode
        mf.write_model(path, m)
        assert _load(path)[0] >= 0 and mf.read_model(path).layers[1].reserved == mode


@pytest.mark.parametrize("case", sorted(BAD_RECORDS))
def test_the_validator_refuses_a_bad_pool_record(case, tmp_path):
    change, reason = BAD_RECORDS[case]
    m = _pooled_model()
    for k, v in change.items():
        setattr(m.layers[1], k, v)
    path = str(tmp_path / "bad.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and "pool" in msg and reason in msg, (rc, msg)


# ---- nothing changes for a model without a pool --------------------------------------------------------------------------------
def test_a_graph_without_a_pool_converts_to_the_same_bytes(tmp_path):
    """the library's container of a pool-free graph against the one convert.py + write_model give: the same file, byte for byte;
    and the reserved word of every record of a pool-free model is zero, as write_model always wrote it"""
    m = synth.build_model("mini")
    data = ox.dump(convert.graph_from_model(m))
    onnx_path, native, py = (str(tmp_path / n) for n in ("mini.onnx", "native.bhm", "py.bhm"))
    with open(onnx_path, "wb") as f:
        f.write(data)
    L = _lib.load()
    assert L.bh_onnx_to_bhm(onnx_path.encode(), native.encode()) == 0, L.bh_last_error()
    want = convert.model_from_graph(ox.load(data), m)
    mf.write_model(py, want)
    a, b = open(native, "rb").read(), open(py, "rb").read()
    n_l = len(want.layers)
    tables = mf.HEADER_SIZE + len(want.branches) * mf.BRANCH_SIZE
    assert a[tables:] == b[tables:]                                       # layer table, padding and blob
    same_tables_and_blob(want, mf.read_model(native))
    for i in range(n_l):
        rec = struct.unpack_from(mf.LAYER_FMT, b, tables + i * mf.LAYER_SIZE)
        assert rec[17] == 0 and b[tables + i * mf.LAYER_SIZE + struct.calcsize(mf.LAYER_FMT):tables + (i + 1) * mf.LAYER_SIZE] == bytes(mf.LAYER_SIZE - struct.calcsize(mf.LAYER_FMT))
    assert mf.Layer(mf.OP_GAP, 0, 1, mf.NO_TENSOR, 4, 4).reserved == 0
