"""OP_REDUCE = 13 (max / mean / max + mean over one image axis or both; the head of the PANNs audio CNNs) on the host: the container, the
validator and both .onnx readers -- csrc/onnx_conv.hpp through bh_onnx_to_bhm, and its twin convert.model_from_graph.

* both readers give the same records and the same blob, bit for bit, for every spelling of the head: keepdims 0 / 1, the axes as an
  attribute or as the opset-18 input, negative axes, GlobalMaxPool, either operand order of the max + mean Add, the ArgMax that
  torch.max leaves behind -- on hand-built graphs and on synth's reduce_plan models, as float32 and as float16 files;
* the .bhm round trip; every validate_model refusal of a code-13 record is hit by changing one field; 9, 11 and 14 stay unknown;
* every refusal the readers make is held to a word of its message, in both readers, and the refused graphs are one step from
  accepted ones; the decomposed LayerNorm chain keeps its refusals;
* cnn14_audio loads through both routes (before the op existed the .onnx route ended in the ReduceMean refusal and the .bhm route in
  "unknown layer op").
"""
import copy
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = ("op", "act", "in_tensor", "res_tensor", "cin", "cout", "kh", "kw", "sh", "sw", "pad_t", "pad_l", "in_h", "in_w", "out_h", "out_w",
          "in_layout", "reserved", "dil_h", "dil_w", "w_off", "b_off")
MAX, MEAN, MAXMEAN = mf.REDUCE_MAX, mf.REDUCE_MEAN, mf.REDUCE_MAXMEAN


@pytest.fixture(scope="module")
def base():
    return synth.build_model("mini")     # the two-branch mini front end: what a graph that starts at [N, 2, 32, 115] is given


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
    assert len(a.layers) == len(b.layers), ([L.op for L in a.layers], [L.op for L in b.layers])
    for i, (x, y) in enumerate(zip(a.layers, b.layers)):
        for f in RECORD:
            assert getattr(x, f) == getattr(y, f), (i, f, getattr(x, f), getattr(y, f))
    assert np.asarray(a.blob, "<f4").tobytes() == np.asarray(b.blob, "<f4").tobytes()
    assert (a.embedding_tensor, a.embedding_dim, a.n_classes, a.output_activation) == (b.embedding_tensor, b.embedding_dim, b.n_classes, b.output_activation)


class Case:
    """spectrogram [N, 2, 32, 115] -> Conv 4x4 stride 4 (C channels, an 8 x 28 image) -> Relu -> `head` -> Gemm -> Sigmoid"""

    def __init__(self, C=8, dtype=np.float32):
        self.rng = np.random.default_rng(7)
        self.g = ox.Graph(name="reduce_case", producer="tests")
        self.g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", 2, 32, 115]))
        self.C, self.k = C, 0
        self.x = self.node("Relu", [self.node("Conv", ["spectrogram", self.f32(C, 2, 4, 4), self.f32(C)], kernel_shape=[4, 4], strides=[4, 4], name="stem")])

    def f32(self, *shape, value=None, dtype=np.float32):
        self.k += 1
        name = f"c{self.k}"
        self.g.initializers[name] = (self.rng.standard_normal(shape) if value is None else np.asarray(value)).astype(dtype).reshape(shape)
        return name

    def node(self, op, ins, name=None, outs=None, **attrs):
        self.k += 1
        outs = outs or [f"v{self.k}"]
        self.g.nodes.append(ox.Node(op, list(ins), list(outs), attrs, name=name or f"{op.lower()}_{self.k}"))
        return outs[0]

    def red(self, op, x, axes, keep, as_input=False, name=None):
        if as_input:
            return self.node(op, [x, self.f32(len(axes), value=axes, dtype=np.int64)], name=name, keepdims=keep)
        return self.node(op, [x], name=name, axes=list(axes), keepdims=keep)

    def pair(self, x, axes, keep, as_input=False, swap=False, argmax=False, name="the_add"):
        mx = self.red("ReduceMax", x, axes, keep, as_input, name="the_max")
        if argmax:
            self.node("ArgMax", [x], name="the_leftover", axis=axes[0], keepdims=keep)
        mn = self.red("ReduceMean", x, axes, keep, as_input, name="the_mean")
        return self.node("Add", [mn, mx] if swap else [mx, mn], name=name)

    def finish(self, x, flatten=False, C=None):
        C = C or self.C
        if flatten:
            x = self.node("Flatten", [x], axis=1)
        y = self.node("Gemm", [x, self.f32(C, 10), self.f32(10)], outs=["logits"])
        self.node("Sigmoid", [y], outs=["probabilities"])
        self.g.outputs.append(ox.ValueInfo("probabilities", ox.FLOAT, ["N", 10]))
        return self.g


def _panns(c, keep=0, as_input=False, neg=False, swap=False, argmax=False):
    """x.mean(dim = 2) over the frequency axis, then torch.max(x, dim) + x.mean(dim) over time, as torch.onnx spells them"""
    f = c.red("ReduceMean", c.x, [-2 if neg else 2], keep, as_input, name="the_freq_mean")
    t = (-1 if neg else 3) if keep else (-1 if neg else 2)
    return c.finish(c.pair(f, [t], keep, as_input, swap, argmax), flatten=bool(keep))


# case -> (the graph's builder, the records behind the stem: (op, mode, kh, kw, out_h, out_w))
R = mf.OP_REDUCE
ACCEPTED = {
    "panns_keepdims_0": (lambda c: _panns(c), [(R, MEAN, 8, 1, 1, 28), (R, MAXMEAN, 1, 28, 1, 1)]),
    "panns_keepdims_1": (lambda c: _panns(c, keep=1), [(R, MEAN, 8, 1, 1, 28), (R, MAXMEAN, 1, 28, 1, 1)]),
    "panns_axes_as_input": (lambda c: _panns(c, as_input=True), [(R, MEAN, 8, 1, 1, 28), (R, MAXMEAN, 1, 28, 1, 1)]),
    "panns_axes_as_input_keepdims_1": (lambda c: _panns(c, keep=1, as_input=True), [(R, MEAN, 8, 1, 1, 28), (R, MAXMEAN, 1, 28, 1, 1)]),
    "panns_negative_axes": (lambda c: _panns(c, neg=True), [(R, MEAN, 8, 1, 1, 28), (R, MAXMEAN, 1, 28, 1, 1)]),
    "panns_negative_axes_keepdims_1": (lambda c: _panns(c, keep=1, neg=True), [(R, MEAN, 8, 1, 1, 28), (R, MAXMEAN, 1, 28, 1, 1)]),
    "panns_add_mean_first": (lambda c: _panns(c, swap=True), [(R, MEAN, 8, 1, 1, 28), (R, MAXMEAN, 1, 28, 1, 1)]),
    "panns_leftover_argmax": (lambda c: _panns(c, argmax=True), [(R, MEAN, 8, 1, 1, 28), (R, MAXMEAN, 1, 28, 1, 1)]),
    "panns_leftover_argmax_keepdims_1": (lambda c: _panns(c, keep=1, argmax=True, swap=True), [(R, MEAN, 8, 1, 1, 28), (R, MAXMEAN, 1, 28, 1, 1)]),
    "time_first": (lambda c: c.finish(c.pair(c.red("ReduceMean", c.x, [3], 0), [2], 0)), [(R, MEAN, 1, 28, 8, 1), (R, MAXMEAN, 8, 1, 1, 1)]),
    "global_max_pool": (lambda c: c.finish(c.node("GlobalMaxPool", [c.x]), flatten=True), [(R, MAX, 8, 28, 1, 1)]),
    "reduce_max_both_keepdims_0": (lambda c: c.finish(c.red("ReduceMax", c.x, [2, 3], 0)), [(R, MAX, 8, 28, 1, 1)]),
    "reduce_max_both_negative_swapped": (lambda c: c.finish(c.red("ReduceMax", c.x, [-1, -2], 1, True), flatten=True), [(R, MAX, 8, 28, 1, 1)]),
    "pair_over_both": (lambda c: c.finish(c.pair(c.x, [2, 3], 0)), [(R, MAXMEAN, 8, 28, 1, 1)]),
    "pair_over_both_keepdims_1": (lambda c: c.finish(c.pair(c.x, [2, 3], 1, swap=True), flatten=True), [(R, MAXMEAN, 8, 28, 1, 1)]),
    "mean_then_max": (lambda c: c.finish(c.red("ReduceMax", c.red("ReduceMean", c.x, [2], 0), [2], 0)), [(R, MEAN, 8, 1, 1, 28), (R, MAX, 1, 28, 1, 1)]),
    "mean_then_max_keepdims_1_squeezed": (lambda c: c.finish(c.node("Squeeze", [c.red("ReduceMax", c.red("ReduceMean", c.x, [2], 1), [3], 1)])),
                                          [(R, MEAN, 8, 1, 1, 28), (R, MAX, 1, 28, 1, 1)]),
    "rank_3_keepdims_1_then_flatten": (lambda c: c.finish(c.red("ReduceMax", c.red("ReduceMean", c.x, [2], 0), [-1], 1), flatten=True),
                                       [(R, MEAN, 8, 1, 1, 28), (R, MAX, 1, 28, 1, 1)]),
    "unsqueeze_behind_the_head": (lambda c: c.finish(c.node("Unsqueeze", [c.red("ReduceMax", c.x, [2, 3], 0), c.f32(1, value=[2], dtype=np.int64)]), flatten=True),
                                  [(R, MAX, 8, 28, 1, 1)]),
    "mean_over_both_stays_the_global_pool": (lambda c: c.finish(c.red("ReduceMean", c.x, [2, 3], 0)), [(mf.OP_GAP, 0, 8, 28, 1, 1)]),
}


@pytest.mark.parametrize("f16", (False, True), ids=("float32", "float16"))
@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_both_readers_give_the_same_records_and_blob(case, f16, base, tmp_path):
    build, records = ACCEPTED[case]
    g = build(Case())
    if f16:
        g = convert.graph_to_float16(g)
        assert all(a.dtype == np.float16 for a in g.initializers.values() if a.dtype.kind == "f")
    want, got = both_readers(g, base, tmp_path)
    same_tables_and_blob(want, got)
    assert [(L.op, L.reserved, L.kh, L.kw, L.out_h, L.out_w) for L in got.layers[1:-1]] == records
    assert got.layers[0].op == mf.OP_CONV and got.layers[-1].op == mf.OP_DENSE and got.layers[-1].in_tensor == len(got.layers) - 1
    for L in got.layers[1:-1]:
        assert (L.cin, L.cout, L.sh, L.sw, L.pad_t, L.pad_l, L.act, L.res_tensor, L.in_layout, L.w_off, L.b_off, L.dil_h, L.dil_w) == \
               (8, 8, 1, 1, 0, 0, 0, mf.NO_TENSOR, 0, 0, 0, 1, 1)
    assert got.embedding_tensor == len(got.layers) - 1 and got.embedding_dim == 8     # what leaves one pixel is the embedding
    assert got.output_activation == mf.OUT_SIGMOID


def _same_records_and_weights(m, got):
    assert len(got.layers) == len(m.layers)
    for i, (x, y) in enumerate(zip(m.layers, got.layers)):
        for f in RECORD[:-2]:
            assert getattr(x, f) == getattr(y, f), (i, f, getattr(x, f), getattr(y, f))
        k = {mf.OP_CONV: x.kh * x.kw * x.cin * x.cout, mf.OP_PWCONV: x.cin * x.cout, mf.OP_DENSE: x.cin * x.cout}.get(x.op, 0)
        assert m.blob[x.w_off:x.w_off + k].tobytes() == got.blob[y.w_off:y.w_off + k].tobytes(), (i, "weights")
        if k:
            assert m.blob[x.b_off:x.b_off + x.cout].tobytes() == got.blob[y.b_off:y.b_off + y.cout].tobytes(), (i, "bias")
    assert (got.embedding_tensor, got.embedding_dim, got.n_classes) == (m.embedding_tensor, m.embedding_dim, m.n_classes)


SYNTH_SPELLINGS = ("", "keep", "input", "neg", "input,neg,keep", "gmp,keep", "swap", "argmax", "keep,swap,argmax,input")


@pytest.mark.parametrize("seed", range(4))
def test_both_readers_give_the_synth_model_s_records(seed, tmp_path):
    """reduce_plan models from the audio input, in every spelling: the library's reader and convert.py's give the synth model's
    records and weights, and the same table and blob as each other -- bit for bit from the first layer's weights on (in front of them
    lies the mel matrix, which each reader recovers from the graph with code of its own that this op does not touch)"""
    m = synth.build_model("reduce_plan", seed=seed)
    assert m.reduce_spelling in ("", "keep")
    lib = _lib.load()
    for sp in (SYNTH_SPELLINGS if seed == 0 else (m.reduce_spelling, "keep,swap,argmax,input")):      # (every spelling on the PANNs pair)
        for f16 in ((False, True) if sp in ("", "keep,swap,argmax,input") else (False,)):
            g = convert.graph_from_model(m, frontend_spelling="stft", spell_reduce=sp)
            ops = [n.op_type for n in g.nodes]
            assert ("ArgMax" in ops) == ("argmax" in sp and any(L.op == R and L.reserved != MEAN for L in m.layers))
            if f16:
                g = convert.graph_to_float16(g)
            data = ox.dump(g)
            onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m.bhm")
            with open(onnx_path, "wb") as f:
                f.write(data)
            assert lib.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, (sp, lib.bh_last_error())
            got = mf.read_model(out)
            want = convert.model_from_graph(ox.load(data), None, sample_rate=m.sample_rate)
            assert got.layers == want.layers, sp
            first = got.layers[0].w_off
            assert got.blob[first:].tobytes() == want.blob[first:].tobytes() and got.blob.size == want.blob.size, sp
            assert (got.embedding_tensor, got.embedding_dim, got.output_activation) == (want.embedding_tensor, want.embedding_dim, want.output_activation)
            if not f16:
                _same_records_and_weights(m, got)
            else:
                assert [(L.op, L.reserved, L.kh, L.kw) for L in got.layers] == [(L.op, L.reserved, L.kh, L.kw) for L in m.layers]


def test_random_reduce_plans_hold_what_they_promise():
    heads, firsts, keeps = set(), set(), set()
    for seed in range(8):
        plan = synth.random_reduce_plan(seed)
        assert plan == synth.random_reduce_plan(seed)
        m = synth.build_model("reduce_plan", plan=plan)
        reds = [L for L in m.layers if L.op == R]
        want = {"panns": [MEAN, MAXMEAN], "global_max": [MAX], "mean_then_max": [MEAN, MAX], "maxmean_both": [MAXMEAN]}[plan["head"]]
        assert [L.reserved for L in reds] == want and m.embedding_tensor == m.layers.index(reds[-1]) + 1
        assert (reds[0].in_h, reds[0].in_w) == (8, 29) and (reds[-1].out_h, reds[-1].out_w) == (1, 1)
        if len(reds) == 2:
            assert (reds[0].kh, reds[0].kw) == ((8, 1) if plan["first"] == "h" else (1, 29))
            assert (reds[1].kh, reds[1].kw) == ((1, 29) if plan["first"] == "h" else (8, 1))
        assert [L.op for L in m.layers[-2:]] == [mf.OP_DENSE, mf.OP_DENSE] and m.layers[-2].act == mf.ACT_RELU
        heads.add(plan["head"]); firsts.add(plan["first"]); keeps.add(plan["keepdims"])
        assert m.macs_per_segment() == sum(L.out_h * L.out_w * L.kh * L.kw * L.cin * L.cout for L in m.layers if L.op in (mf.OP_CONV, mf.OP_DENSE))
    assert heads == set(synth.REDUCE_HEADS) and firsts == {"h", "w"} and keeps == {0, 1}
    assert {synth.random_reduce_plan(s)["head"] for s in range(4)} == set(synth.REDUCE_HEADS)
    big = synth.build_model("cnn14_audio", n_classes=40)
    assert [(L.op, L.reserved, L.kh, L.kw, L.in_h, L.in_w, L.cout) for L in big.layers[-4:-2]] == [(R, MEAN, 3, 1, 3, 16, 512), (R, MAXMEAN, 1, 16, 1, 16, 512)]
    assert [(L.op, L.act) for L in big.layers[-2:]] == [(mf.OP_DENSE, mf.ACT_RELU), (mf.OP_DENSE, mf.ACT_NONE)] and big.output_activation == mf.OUT_SIGMOID
    pool = synth.build_model("cnn_pool", n_classes=40)
    body = len(pool.layers) - 2
    assert pool.layers[:body] == big.layers[:body] and np.array_equal(pool.blob[:pool.layers[body - 1].b_off + 512], big.blob[:big.layers[body - 1].b_off + 512])


# ---- the container -----------------------------------------------------------------------------------------------------------------
def test_the_round_trip_and_code_13_in_the_file(tmp_path):
    for seed in range(4):
        m = synth.build_model("reduce_plan", seed=seed)
        path = str(tmp_path / "m.bhm")
        mf.write_model(path, m)
        back = mf.read_model(path)
        assert back.layers == m.layers and np.array_equal(back.blob, m.blob)
        raw = open(path, "rb").read()
        n_b, n_l = struct.unpack_from("<II", raw, 32)
        for i, L in enumerate(m.layers):
            rec = raw[mf.HEADER_SIZE + n_b * mf.BRANCH_SIZE + i * mf.LAYER_SIZE:][:mf.LAYER_SIZE]
            assert struct.unpack_from("<I", rec, 0)[0] == L.op and rec[88:] == bytes(40)
            if L.op == R:
                assert L.op == 13 and struct.unpack_from("<I", rec, 68)[0] == L.reserved <= 2 and struct.unpack_from("<QQ", rec, 72) == (0, 0)
        # .bhm -> .onnx -> .bhm through the library's reader and writer (bh_onnx_to_bhm), and that file through the validator
        onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m_native.bhm")
        with open(onnx_path, "wb") as f:
            f.write(convert.model_to_onnx(m, frontend_spelling="stft", spell_reduce=m.reduce_spelling))
        lib = _lib.load()
        assert lib.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, lib.bh_last_error()
        _same_records_and_weights(m, mf.read_model(out))
        assert _load(out)[0] >= 0
    assert (mf.OP_REDUCE, mf.REDUCE_MAX, mf.REDUCE_MEAN, mf.REDUCE_MAXMEAN) == (13, 0, 1, 2)


def test_existing_models_keep_their_records(tmp_path):
    """a model without the op is written, by either writer, as it always was: no code 13, and its global pool the OP_GAP record"""
    for kind in ("mini", "mini_se"):
        m = synth.build_model(kind)
        p = str(tmp_path / f"{kind}.bhm")
        mf.write_model(p, m)
        assert all(L.op != R for L in mf.read_model(p).layers) and any(L.op == mf.OP_GAP for L in m.layers)
        g = convert.graph_from_model(m)
        assert not any(n.op_type in ("ReduceMax", "ReduceMean", "GlobalMaxPool") for n in g.nodes)
        back = convert.model_from_graph(ox.load(ox.dump(g)), m)
        assert back.layers == m.layers and np.array_equal(back.blob, m.blob)


# ---- the validator -----------------------------------------------------------------------------------------------------------------
def _load(path):
    """bh_plan_fused_blocks walks a model file on the host: load_model + validate_model; >= 0 = loaded (the fused blocks' count)"""
    L = _lib.load()
    rc = L.bh_plan_fused_blocks(path.encode(), 0, None, None, 0)
    return rc, L.bh_last_error().decode()


def _twice_reduced():
    """stem -> conv -> MAXMEAN over both (tensor 3) -> MAX over both of the same map (tensor 4) -> dense: a record whose output has the
    size of an earlier tensor, so that a residual can be put on it"""
    b = synth._Builder(np.random.default_rng(3))
    base = synth.build_model("mini")
    br = [copy.deepcopy(x) for x in base.branches]
    for x in br:
        x.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(x.n_mels, x.n_bins, base.sample_rate, x.fmin, x.fmax))
    t, h, w = b.conv(0, 32, 115, 2, 8, 3, 2, mf.ACT_RELU, in_layout=1)
    x, h, w = b.conv(t, h, w, 8, 12, 3, 2, mf.ACT_RELU)
    b.reduce(x, h, w, 12, MAXMEAN)
    t, _, _ = b.reduce(x, h, w, 12, MAX)
    b.dense(t, 12, 10)
    return synth._finish(b, br, base.sample_rate, base.sample_count, 10, 12, t, mf.OUT_SIGMOID)


def _first(m, pred=lambda L: True):
    return next(L for L in m.layers if L.op == R and pred(L))


# case -> (the seed of the reduce_plan model or a builder, which record, the change -- a dict of fields or a callable --, the reason)
BAD_RECORDS = {
    "mode": (0, None, dict(reserved=3), "reduce layer with an unknown mode"),
    "changed_channels": (0, None, lambda L: setattr(L, "cin", L.cin + 4), "reduce layer that changes the channel count"),
    "activation": (0, None, dict(act=mf.ACT_RELU), "reduce layer with an activation"),
    "residual": (_twice_reduced, lambda L: L.reserved == MAX, dict(res_tensor=3), "reduce layer with a residual"),
    "planar_layout": (0, None, dict(in_layout=1), "reduce layer on the planar spectrogram (tensor 0)"),
    "stride": (0, None, dict(sw=2), "reduce layer with a stride or padding other than 1 / 0"),
    "padding": (0, None, dict(pad_t=1), "reduce layer with a stride or padding other than 1 / 0"),
    "window_not_the_axis": (0, None, lambda L: setattr(L, "kh" if L.kh > 1 else "kw", 3), "neither the whole axis nor 1"),
    "window_1x1": (0, None, dict(kh=1, kw=1), "1x1 window"),
    "changed_image": (0, None, lambda L: setattr(L, "out_w", L.out_w + 1), "output image is not its input image over its window"),
    "mean_over_both": (3, None, dict(reserved=MEAN), "OP_GAP is its one spelling"),
    "dilation": (0, None, dict(dil_h=2), "dilation on a reduce layer"),
}


@pytest.mark.parametrize("case", sorted(BAD_RECORDS))
def test_the_validator_refuses_a_bad_reduce_record(case, tmp_path):
    src, pred, change, reason = BAD_RECORDS[case]
    m = src() if callable(src) else synth.build_model("reduce_plan", seed=src)
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc >= 0, msg                                   # the model loads as it stands
    L = _first(m, pred or (lambda L: True))
    before = copy.copy(L)
    if callable(change):
        change(L)
    else:
        for k, v in change.items():
            setattr(L, k, v)
    assert sum(getattr(L, f) != getattr(before, f) for f in RECORD) == 1, case          # one field
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and reason in msg, (rc, msg)


def test_the_validator_refuses_six_channels_too_many_taps_and_the_unused_codes(tmp_path):
    path = str(tmp_path / "m.bhm")
    # C % 4 != 0: the whole stack at 6 channels
    m6 = synth.build_model("reduce_plan", plan=dict(synth.random_reduce_plan(0), width=6))
    mf.write_model(path, m6)
    rc, msg = _load(path)
    assert rc < 0 and "reduce layer over a channel count that is not a multiple of 4" in msg, msg
    # more than 65 536 taps: a 300 x 300 spectrogram, a stem that keeps the image and the max over both axes (over H alone, 300 taps, it loads)
    def wide(both):
        b = synth._Builder(np.random.default_rng(5))
        sr, n = 48000, 512 + 299 * 100
        br = mf.Branch(512, 100, 300, 300, 0.0, 3000.0, 1.23)
        br.mel_w_off = b.put(np.zeros((br.n_bins, br.n_mels), np.float32))
        t, h, w = b.conv(0, 300, 300, 1, 4, 3, 1, mf.ACT_RELU, in_layout=1)
        t, h, w = b.reduce(t, h, w, 4, MAX, over_h=True, over_w=both)
        if not both:
            t = b.gap(t, h, w, 4)
        b.dense(t, 4, 10)
        return synth._finish(b, [br], sr, n, 10, 4, t, mf.OUT_SIGMOID)
    mf.write_model(path, wide(False))
    rc, msg = _load(path)
    assert rc >= 0, msg
    mf.write_model(path, wide(True))
    rc, msg = _load(path)
    assert rc < 0 and "reduce layer over more than 65 536 taps" in msg, msg
    # 9, 11 and 14 stay unknown
    m = synth.build_model("reduce_plan", seed=0)
    for code in (9, 11, 14):
        m4 = copy.deepcopy(m)
        _first(m4).op = code
        mf.write_model(path, m4)
        rc, msg = _load(path)
        assert rc < 0 and "unknown layer op" in msg, (code, msg)


def test_no_matcher_takes_a_record_run_with_a_reduce(tmp_path):
    """a squeeze-excite gate whose pool is a reduce record is no gate launch and no fused block: the planner finds none in any
    precision, while the same stack with OP_GAP in that place has its block"""
    lib = _lib.load()
    m = synth.build_model("mini_se")
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    with_gap = [lib.bh_plan_fused_blocks(path.encode(), flags, None, None, 0) for flags in (0, 1, 2, 3)]
    assert min(with_gap) >= 0 and max(with_gap) >= 1, lib.bh_last_error()
    k = 0
    for L in m.layers:
        if L.op == mf.OP_GAP and L.in_h * L.in_w > 1 and any(M.op == mf.OP_SCALE for M in m.layers):
            nxt = m.layers[m.layers.index(L) + 1]
            if nxt.op == mf.OP_PWCONV:                    # a gate's squeeze
                L.op, L.reserved = R, MAXMEAN
                k += 1
    assert k >= 1
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc >= 0, msg
    for flags, before in zip((0, 1, 2, 3), with_gap):
        got = lib.bh_plan_fused_blocks(path.encode(), flags, None, None, 0)
        assert 0 <= got < max(before, 1), (flags, got, before)       # the gated blocks are fused no longer


# ---- what both readers refuse ------------------------------------------------------------------------------------------------------
def _refused(kind):
    c = Case()
    C = c.C
    if kind == "pair_over_different_axes":
        mx, mn = c.red("ReduceMax", c.x, [2], 1, name="the_max"), c.red("ReduceMean", c.x, [3], 1, name="the_mean")
        return c.finish(c.node("Add", [mx, mn], name="the_add"), flatten=True)
    if kind == "pair_of_different_keepdims":
        f = c.red("ReduceMean", c.x, [2], 1)
        mx, mn = c.red("ReduceMax", f, [3], 1, name="the_max"), c.red("ReduceMean", f, [3], 0, name="the_mean")
        return c.finish(c.node("Add", [mx, mn], name="the_add"), flatten=True)
    if kind == "pair_of_different_tensors":
        f = c.red("ReduceMean", c.x, [2], 1)
        mx, mn = c.red("ReduceMax", f, [3], 1, name="the_max"), c.red("ReduceMean", c.x, [2, 3], 1, name="the_mean")
        return c.finish(c.node("Add", [mx, mn], name="the_add"), flatten=True)
    if kind == "pair_of_two_maxima":
        mx, mn = c.red("ReduceMax", c.x, [2, 3], 0, name="the_max"), c.red("ReduceMax", c.x, [2, 3], 0, name="the_other")
        return c.finish(c.node("Add", [mx, mn], name="the_add"))
    if kind == "reduce_read_twice":
        y = c.pair(c.x, [2, 3], 0)
        c.node("Relu", [next(n.outputs[0] for n in c.g.nodes if n.name == "the_max")], name="a_second_reader")
        return c.finish(y)
    if kind == "conv_on_a_rank_3_tensor":
        f = c.red("ReduceMean", c.x, [2], 0)
        y = c.node("Conv", [f, c.f32(C, C, 1), c.f32(C)], name="the_conv", kernel_shape=[1])
        return c.finish(c.red("ReduceMax", y, [2], 0))
    if kind == "pool_on_a_rank_3_tensor":
        f = c.red("ReduceMean", c.x, [2], 0)
        return c.finish(c.red("ReduceMax", c.node("MaxPool", [f], name="the_pool", kernel_shape=[2]), [2], 0))
    if kind == "transpose_of_a_rank_3_tensor":
        f = c.red("ReduceMean", c.x, [2], 0)
        return c.finish(c.red("ReduceMax", c.node("Transpose", [f], name="the_transpose", perm=[0, 2, 1]), [1], 0))
    if kind == "flatten_of_a_rank_3_tensor_with_pixels_left":
        return c.finish(c.node("Flatten", [c.red("ReduceMean", c.x, [2], 0)], name="the_flatten", axis=1), C=C * 28)
    if kind == "reduce_over_axis_1":
        return c.finish(c.node("Flatten", [c.red("ReduceMax", c.x, [1], 0, name="the_max")], axis=1), C=8 * 28)
    if kind == "reduce_over_the_channels_of_a_rank_3_tensor":
        return c.finish(c.red("ReduceMax", c.red("ReduceMean", c.x, [2], 0), [1], 0, name="the_max"), C=28)
    if kind == "reduce_mean_over_axis_1":
        return c.finish(c.node("Flatten", [c.red("ReduceMean", c.x, [1], 1, name="the_mean")], axis=1), C=8 * 28)
    if kind == "reduce_on_a_view":
        v = c.node("Transpose", [c.x], perm=[0, 2, 3, 1])
        return c.finish(c.red("ReduceMax", v, [1, 2], 0, name="the_max"))
    if kind == "reduce_mean_over_the_last_axis_of_a_view":
        v = c.node("Transpose", [c.x], perm=[0, 2, 3, 1])
        return c.finish(c.node("Flatten", [c.red("ReduceMean", v, [-1], 1, name="the_mean")], axis=1), C=8 * 28)
    if kind == "reduce_on_tensor_0":
        f = c.red("ReduceMax", "spectrogram", [2], 1, name="the_max")
        return c.finish(c.node("GlobalAveragePool", [c.node("Conv", [f, c.f32(C, 2, 1, 1), c.f32(C)], kernel_shape=[1, 1])]), flatten=True)
    if kind == "reduce_sum":
        return c.finish(c.red("ReduceSum", c.x, [2, 3], 0, as_input=True, name="the_sum"))
    if kind == "reduce_min":
        return c.finish(c.red("ReduceMin", c.x, [2, 3], 0, name="the_min"))
    if kind == "reduce_l2":
        return c.finish(c.red("ReduceL2", c.x, [2, 3], 0, name="the_norm"))
    if kind == "activation_behind_a_reduce":
        return c.finish(c.node("Relu", [c.red("ReduceMax", c.x, [2, 3], 0)], name="the_relu"))
    if kind == "window_of_one_pixel":
        f = c.red("ReduceMean", c.x, [2], 1)
        return c.finish(c.red("ReduceMax", c.red("ReduceMax", f, [2], 1, name="the_second"), [3], 1), flatten=True)
    if kind == "avgmax_of_two_global_pools":
        a, b = c.node("GlobalAveragePool", [c.x]), c.node("GlobalMaxPool", [c.x])
        return c.finish(c.node("Add", [a, b], name="the_add"), flatten=True)
    if kind == "argmax_that_is_read":
        c.node("ArgMax", [c.x], name="the_argmax", outs=["idx"], axis=2, keepdims=0)
        c.g.outputs.append(ox.ValueInfo("idx", ox.INT64 if hasattr(ox, "INT64") else 7, ["N", 8, 28]))
        g = c.finish(c.red("ReduceMax", c.x, [2, 3], 0))
        g.outputs.reverse()
        return g
    if kind == "attention_pooling_ends_in_no_dense_layer":
        g = c.finish(c.red("ReduceMax", c.x, [2, 3], 0))
        del g.nodes[-2:]
        g.outputs[:] = [ox.ValueInfo(g.nodes[-1].outputs[0], ox.FLOAT, ["N", 8])]
        return g
    raise KeyError(kind)


# kind -> the words both refusals hold
REFUSED = {
    "pair_over_different_axes": ("the_add", "different axes"),
    "pair_of_different_keepdims": ("the_add", "keepdims"),
    "pair_of_different_tensors": ("the_add", "different tensors"),
    "pair_of_two_maxima": ("the_add", "one ReduceMax and one ReduceMean"),
    "reduce_read_twice": ("the_add", "another node reads too"),
    "conv_on_a_rank_3_tensor": ("Conv", "the_conv", "rank-3"),
    "pool_on_a_rank_3_tensor": ("MaxPool", "the_pool", "rank-3"),
    "transpose_of_a_rank_3_tensor": ("Transpose", "the_transpose", "rank-3"),
    "flatten_of_a_rank_3_tensor_with_pixels_left": ("Flatten", "1x28 map"),
    "reduce_over_axis_1": ("the_max", "axis 1", "never the batch or the channels"),
    "reduce_over_the_channels_of_a_rank_3_tensor": ("the_max", "axis 1", "rank-3"),
    "reduce_mean_over_axis_1": ("the_mean", "not the LayerNorm chain"),                   # today's refusal
    "reduce_on_a_view": ("ReduceMax", "the_max", "[N, H, W, C] view"),
    "reduce_mean_over_the_last_axis_of_a_view": ("the_mean", "not the LayerNorm chain"),  # today's refusal
    "reduce_on_tensor_0": ("the_max", "tensor 0"),
    "reduce_sum": ("unsupported operator ReduceSum", "the_sum"),
    "reduce_min": ("unsupported operator ReduceMin", "the_min"),
    "reduce_l2": ("unsupported operator ReduceL2", "the_norm"),
    "activation_behind_a_reduce": ("activation", "reduce layer carries no activation"),
    "window_of_one_pixel": ("the_second", "nothing to reduce"),
    "avgmax_of_two_global_pools": ("Add", "no convolution to fold the residual into"),   # today's refusal of every other Add
    "argmax_that_is_read": ("unsupported operator ArgMax", "the_argmax"),
    "attention_pooling_ends_in_no_dense_layer": ("the graph does not end in a dense layer",),
}


@pytest.mark.parametrize("kind", sorted(REFUSED))
def test_both_readers_refuse_by_name(kind, base, tmp_path):
    g = _refused(kind)
    data = ox.dump(g)
    with pytest.raises(convert.ConvertError) as e:
        convert.model_from_graph(ox.load(data), base)
    for word in REFUSED[kind]:
        assert word in str(e.value), (kind, word, str(e.value))
    onnx_path = str(tmp_path / "case.onnx")
    with open(onnx_path, "wb") as f:
        f.write(data)
    lib = _lib.load()
    rc = lib.bh_onnx_to_bhm(onnx_path.encode(), str(tmp_path / "case.bhm").encode())
    msg = lib.bh_last_error().decode()
    assert rc != 0, kind
    for word in REFUSED[kind]:
        assert word in msg, (kind, word, msg)


def test_the_layer_norm_chain_keeps_its_place(base, tmp_path):
    """ReduceMean -> Sub(x, mean) ... over the last axis of a view is still the decomposed LayerNorm, and with keepdims = 0 still refused
    as the chain it is; without the Sub the same ReduceMean over axis 3 of an NCHW map is a reduction over W"""
    def chain(c, x, keep=1):
        mu = c.node("ReduceMean", [x], name="the_mean", axes=[-1], keepdims=keep)
        d = c.node("Sub", [x, mu], name="the_sub")
        var = c.node("ReduceMean", [c.node("Pow", [d, c.f32(value=2.0)])], axes=[-1], keepdims=1)
        sd = c.node("Sqrt", [c.node("Add", [var, c.f32(value=1e-6)])])
        return c.node("Add", [c.node("Mul", [c.node("Div", [d, sd]), c.f32(c.C)]), c.f32(c.C)])
    c = Case()
    y = c.node("Transpose", [chain(c, c.node("Transpose", [c.x], perm=[0, 2, 3, 1]))], perm=[0, 3, 1, 2])
    want, got = both_readers(c.finish(c.red("ReduceMax", y, [2, 3], 0)), base, tmp_path)
    same_tables_and_blob(want, got)
    assert [L.op for L in got.layers] == [mf.OP_CONV, mf.OP_LNORM, R, mf.OP_DENSE]
    c = Case()
    y = c.node("Transpose", [chain(c, c.node("Transpose", [c.x], perm=[0, 2, 3, 1]), keep=0)], perm=[0, 3, 1, 2])
    g = c.finish(c.red("ReduceMax", y, [2, 3], 0))
    with pytest.raises(convert.ConvertError, match="keepdims = 0"):
        convert.model_from_graph(ox.load(ox.dump(g)), base)
    onnx_path = str(tmp_path / "keep0.onnx")
    with open(onnx_path, "wb") as f:
        f.write(ox.dump(g))
    lib = _lib.load()
    assert lib.bh_onnx_to_bhm(onnx_path.encode(), str(tmp_path / "keep0.bhm").encode()) != 0 and b"keepdims = 0" in lib.bh_last_error()
    c = Case()
    want, got = both_readers(c.finish(c.red("ReduceMax", c.red("ReduceMean", c.x, [-1], 1), [2, 3], 0)), base, tmp_path)
    same_tables_and_blob(want, got)
    assert [(L.op, L.reserved, L.kh, L.kw) for L in got.layers[1:3]] == [(R, MEAN, 1, 28), (R, MAX, 8, 1)]
    # a norm behind the reduce that leaves one pixel is the embedding, as behind the global pool
    c = Case()
    p = c.node("GlobalMaxPool", [c.x])
    y = c.node("LayerNormalization", [p, c.f32(c.C), c.f32(c.C)], axis=1, epsilon=1e-6)
    want, got = both_readers(c.finish(y, flatten=True), base, tmp_path)
    same_tables_and_blob(want, got)
    assert [L.op for L in got.layers] == [mf.OP_CONV, R, mf.OP_LNORM, mf.OP_DENSE] and got.embedding_tensor == 3


def test_the_refused_graphs_are_one_step_from_accepted_ones(base, tmp_path):
    """the same builder's well-formed graphs load through both readers (so each refusal above is about its one deviation)"""
    def ok(build):
        want, got = both_readers(build(Case()), base, tmp_path)
        same_tables_and_blob(want, got)
        return got
    # the pair over the same axis; the same keepdims; the same tensor; max + mean
    got = ok(lambda c: c.finish(c.node("Add", [c.red("ReduceMax", c.x, [2, 3], 1), c.red("ReduceMean", c.x, [2, 3], 1)]), flatten=True))
    assert [(L.op, L.reserved) for L in got.layers] == [(mf.OP_CONV, 0), (R, MAXMEAN), (mf.OP_DENSE, 0)]
    # the reduce read once; a reduce (not an activation) behind a reduce; two different axes in a row
    got = ok(lambda c: c.finish(c.red("ReduceMax", c.red("ReduceMean", c.x, [2], 1), [3], 1), flatten=True))
    assert [(L.op, L.reserved) for L in got.layers[1:3]] == [(R, MEAN), (R, MAX)]
    # further reductions, and Flatten once one pixel is left, read a rank-3 tensor
    got = ok(lambda c: c.finish(c.node("Flatten", [c.red("ReduceMax", c.red("ReduceMean", c.x, [2], 0), [2], 1)], axis=1)))
    assert [(L.op, L.reserved) for L in got.layers[1:3]] == [(R, MEAN), (R, MAX)]
    # a reduce of a feature map (not the spectrogram, not a view); a Conv on the rank-4 result of keepdims = 1
    got = ok(lambda c: c.finish(c.node("GlobalAveragePool", [c.node("Conv", [c.red("ReduceMax", c.x, [2], 1), c.f32(c.C, c.C, 1, 1), c.f32(c.C)], kernel_shape=[1, 1])]),
                                flatten=True))
    assert [L.op for L in got.layers] == [mf.OP_CONV, R, mf.OP_PWCONV, mf.OP_GAP, mf.OP_DENSE] and got.embedding_tensor == 4
    # an ArgMax nothing reads is ignored -- and counts as no reader of x
    got = ok(lambda c: (c.node("ArgMax", [c.x], name="the_argmax", outs=["idx"], axis=2, keepdims=0), c.finish(c.red("ReduceMax", c.x, [2, 3], 0)))[1])
    assert [(L.op, L.reserved) for L in got.layers] == [(mf.OP_CONV, 0), (R, MAX), (mf.OP_DENSE, 0)]
    # the reduce feeds a squeeze-excite gate like the global pool
    def gate(c):
        s = c.node("Conv", [c.node("GlobalMaxPool", [c.x]), c.f32(c.C, c.C, 1, 1), c.f32(c.C)], kernel_shape=[1, 1])
        y = c.node("Mul", [c.x, c.node("Sigmoid", [s])])
        return c.finish(c.node("GlobalAveragePool", [y]), flatten=True)
    got = ok(gate)
    assert [L.op for L in got.layers] == [mf.OP_CONV, R, mf.OP_PWCONV, mf.OP_SCALE, mf.OP_GAP, mf.OP_DENSE] and got.embedding_tensor == 5


# ---- fails without the feature -----------------------------------------------------------------------------------------------------
def test_cnn14_audio_loads_through_both_routes(tmp_path):
    """before this op existed the .onnx route ended in the ReduceMean refusal ("not the LayerNorm chain ... keepdims = 0") and the .bhm
    route in 'unknown layer op'"""
    lib = _lib.load()
    m = synth.build_model("cnn14_audio", n_classes=40)
    onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m_native.bhm")
    with open(onnx_path, "wb") as f:
        f.write(convert.model_to_onnx(m, frontend_spelling="stft"))
    g = ox.load(open(onnx_path, "rb").read())
    tail = [n.op_type for n in g.nodes][-8:]
    assert tail == ["ReduceMean", "ReduceMax", "ReduceMean", "Add", "Gemm", "Relu", "Gemm", "Sigmoid"], tail
    assert [n.attrs.get("keepdims") for n in g.nodes[-8:-5]] == [0, 0, 0] and [n.attrs.get("axes") for n in g.nodes[-8:-5]] == [[2], [2], [2]]
    assert lib.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, lib.bh_last_error()
    _same_records_and_weights(m, mf.read_model(out))
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc == 0, msg


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------
def test_mutated_reduce_files_are_refused_or_read_never_a_crash():
    """tools/fuzz_onnx_reader.py over reduce heads (every spelling, from the audio input) and containers with code-13 records, in child
    processes: every mutant loads or is refused"""
    env = dict(os.environ, FUZZ_REDUCE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_onnx_reader.py"), "160", "5"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-600:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("160 mutants, 0 bad batches"), r.stdout[-800:]
    assert "'0':" in last and "'-2':" in last, last
