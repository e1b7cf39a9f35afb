"""OP_BNACT = 14 (a folded BatchNormalization + activation on a tensor no convolution can take the norm into: DenseNet's relu(bn(cat(..))),
a pre-activation ResNet's relu(bn(sum))) on the host: the container, the validator and both .onnx readers -- csrc/onnx_conv.hpp through
bh_onnx_to_bhm, and its twin convert.model_from_graph.

* hand-written graphs -- BN + Relu behind a MaxPool, an AveragePool, a two-source Concat, a shuffle, a residual sum, an activated
  convolution and another such record, in front of the global pool; every activation spelling; a float16 file -- give the same records
  and the same blob bits in both readers, scale = gamma / sqrt(var + eps) and shift = beta - mean scale computed in float64;
* a bare BN behind those producers, a BN whose output an activation AND something else read, BN + Sigmoid and C % 4 != 0 keep the
  refusal the producer had before the op existed; a BN of a convolution output with other readers keeps its own;
* every validate_model refusal of a code-14 record is hit by changing one field; 9, 11 and 15 stay unknown; the .bhm round trip;
* a Concat over the growing list of earlier features reads to the records of the two-input spelling (prefix reuse), a list whose prefix
  is no whole earlier Concat falls back to the chain;
* graph_from_model -> model_from_graph round trips dense_plan seeds bit for bit; no matcher fuses across the op;
* dense_plan and densenet_audio load through both routes (before the op existed the .onnx route ended in a BatchNormalization refusal
  and the .bhm route in "unknown layer op").

forward64 below is the float64 yardstick of tests/test_bnact_gpu.py: tests/test_hardswish.py's layer (test_resact.py's position word,
test_pool_gpu.py's pools), tests/test_concat.py's gather and the op itself."""
import copy
import os
import struct

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O
from test_concat import gather
from test_hardswish import act64h, layer64h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = ("op", "act", "in_tensor", "res_tensor", "cin", "cout", "kh", "kw", "sh", "sw", "pad_t", "pad_l", "in_h", "in_w", "out_h", "out_w",
          "in_layout", "reserved", "dil_h", "dil_w", "w_off", "b_off")
B = mf.OP_BNACT
NONE = mf.NO_TENSOR


# ---- the yardstick: the model's logits in float64 ----------------------------------------------------------------------------------
def bnact64(X, scale, shift, act):
    """act(x scale + shift) in float64 on the f32 operands"""
    return act64h(np.asarray(X, np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64), act)


def layer64b(m, L, X, R):
    n = X.shape[0]
    if L.op == B:
        assert R is None
        return bnact64(X.reshape(n, L.out_h, L.out_w, L.cout), m.blob[L.w_off:L.w_off + L.cout], m.blob[L.b_off:L.b_off + L.cout], L.act)
    if L.op == mf.OP_CONCAT:          # res_tensor is the second input here, not a residual
        return gather(L, np.asarray(X, np.float64), None if R is None else np.asarray(R, np.float64), n)
    return layer64h(m, L, X, R)


def forward64(m, segs, tensors=False):
    """-> logits [n][n_classes] in float64 (tensors=True: every tensor, T[0] the spectrogram)"""
    spec, _ = O.frontend64(m, segs)
    T = [spec]
    for L in m.layers:
        T.append(layer64b(m, L, T[L.in_tensor], None if L.res_tensor == NONE else T[L.res_tensor]))
    return T if tensors else T[-1].reshape(segs.shape[0], -1)


# ---- hand-written graphs through both readers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return synth.build_model("mini")     # the two-branch mini front end: what a graph that starts at [N, 2, 32, 115] is given


def read_both(g, base, tmp_path):
    """-> (convert.py's model or its refusal, the library's model or its refusal)"""
    data = ox.dump(g)
    onnx_path, out = str(tmp_path / "case.onnx"), str(tmp_path / "case.bhm")
    with open(onnx_path, "wb") as f:
        f.write(data)
    try:
        want = convert.model_from_graph(ox.load(data), base)
    except convert.ConvertError as e:
        want = str(e)
    L = _lib.load()
    rc = L.bh_onnx_to_bhm(onnx_path.encode(), out.encode())
    return want, (mf.read_model(out) if rc == 0 else L.bh_last_error().decode())


def both_readers(g, base, tmp_path):
    want, got = read_both(g, base, tmp_path)
    assert not isinstance(want, str) and not isinstance(got, str), (want, got)
    assert len(want.layers) == len(got.layers), ([L.op for L in want.layers], [L.op for L in got.layers])
    for i, (x, y) in enumerate(zip(want.layers, got.layers)):
        for f in RECORD:
            assert getattr(x, f) == getattr(y, f), (i, f, getattr(x, f), getattr(y, f))
    assert np.asarray(want.blob, "<f4").tobytes() == np.asarray(got.blob, "<f4").tobytes()
    assert (want.embedding_tensor, want.embedding_dim, want.n_classes, want.output_activation) == \
           (got.embedding_tensor, got.embedding_dim, got.n_classes, got.output_activation)
    return got


def both_refuse(g, base, tmp_path, *words):
    want, got = read_both(g, base, tmp_path)
    assert isinstance(want, str) and isinstance(got, str), (want if isinstance(want, str) else "convert.py read it", got if isinstance(got, str) else "the library read it")
    for word in words:
        assert word in want and word in got, (word, want, got)


class Case:
    """spectrogram [N, 2, 32, 115] -> Conv 4x4 stride 4 (C channels, an 8 x 28 image) -> Relu = x; ... -> GlobalAveragePool -> Gemm -> Sigmoid"""

    def __init__(self, C=8):
        self.rng = np.random.default_rng(11)
        self.g = ox.Graph(name="bnact_case", producer="tests")
        self.g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", 2, 32, 115]))
        self.C, self.k = C, 0
        self.x = self.node("Relu", [self.conv("spectrogram", 2, C, 4, 4, name="stem")])

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

    def conv(self, x, cin, cout, k=1, s=1, name=None):
        pad = (k - 1) // 2 if s == 1 else 0
        return self.node("Conv", [x, self.f32(cout, cin, k, k), self.f32(cout)], name=name, kernel_shape=[k, k], strides=[s, s], pads=[pad] * 4)

    def bn(self, x, C=None, name="the_bn", eps=1e-5, **kw):
        C = C or self.C
        var = np.abs(self.rng.standard_normal(C)) + 0.5
        self.params = (self.f32(C), self.f32(C), self.f32(C), self.f32(C, value=var))
        attrs = {} if eps is None else {"epsilon": eps}
        return self.node("BatchNormalization", [x] + list(self.params), name=name, **attrs, **kw)

    def finish(self, x, C=None):
        C = C or self.C
        x = self.node("Flatten", [self.node("GlobalAveragePool", [x])], axis=1)
        y = self.node("Gemm", [x, self.f32(C, 10), self.f32(10)], outs=["logits"])
        self.node("Sigmoid", [y], outs=["probabilities"])
        self.g.outputs.append(ox.ValueInfo("probabilities", ox.FLOAT, ["N", 10]))
        return self.g


def _shuffle(c, x, C, groups=2, h=8, w=28):
    r5 = c.node("Reshape", [x, c.f32(5, value=[0, groups, C // groups, h, w], dtype=np.int64)])
    tr = c.node("Transpose", [r5], perm=[0, 2, 1, 3, 4])
    return c.node("Reshape", [tr, c.f32(4, value=[0, C, h, w], dtype=np.int64)])


def _producer(c, kind):
    """-> (the tensor the norm reads, its channels, the op of the record that produces it)"""
    C = c.C
    if kind == "maxpool":
        return c.node("MaxPool", [c.x], kernel_shape=[2, 2], strides=[2, 2]), C, mf.OP_POOL
    if kind == "avgpool":
        return c.node("AveragePool", [c.x], kernel_shape=[2, 2], strides=[2, 2]), C, mf.OP_POOL
    if kind == "concat":
        return c.node("Concat", [c.x, c.node("Relu", [c.conv(c.x, C, 12, 3)])], name="the_cat", axis=1), C + 12, mf.OP_CONCAT
    if kind == "shuffle":
        return _shuffle(c, c.node("Concat", [c.x, c.node("Relu", [c.conv(c.x, C, C, 3)])], axis=1), 2 * C), 2 * C, mf.OP_CONCAT
    if kind == "sum":
        return c.node("Add", [c.conv(c.x, C, C, 3), c.x], name="the_sum"), C, mf.OP_CONV
    if kind == "activated_conv":
        return c.x, C, mf.OP_CONV
    raise KeyError(kind)


PRODUCERS = ("maxpool", "avgpool", "concat", "shuffle", "sum", "activated_conv")
TODAY = {"maxpool": "BatchNormalization that does not follow a convolution directly", "avgpool": "BatchNormalization that does not follow a convolution directly",
         "concat": "directly after a Concat, Split, Slice or channel shuffle cannot be folded", "shuffle": "directly after a Concat, Split, Slice or channel shuffle cannot be folded",
         "sum": "BatchNormalization after a residual Add (BN(conv + x)) cannot be folded into the convolution",
         "activated_conv": "BatchNormalization that does not follow a convolution directly"}


def _folded(c, got_layer, blob, eps=1e-5):
    """the record's scale / shift against the float64 fold of the graph's parameters, rounded once"""
    ga, be, mu, var = (c.g.initializers[k].astype(np.float64) for k in c.params)
    scale = ga / np.sqrt(var + float(np.float32(eps)))
    shift = be - mu * scale
    n = got_layer.cout
    assert blob[got_layer.w_off:got_layer.w_off + n].tobytes() == scale.astype(np.float32).tobytes()
    assert blob[got_layer.b_off:got_layer.b_off + n].tobytes() == shift.astype(np.float32).tobytes()


@pytest.mark.parametrize("kind", PRODUCERS)
def test_bn_relu_behind_each_producer_is_one_record(kind, base, tmp_path):
    c = Case()
    x, C, op = _producer(c, kind)
    y = c.node("Relu", [c.bn(x, C)])
    got = both_readers(c.finish(c.conv(y, C, 16), 16), base, tmp_path)
    i = next(i for i, L in enumerate(got.layers) if L.op == B)
    L, P = got.layers[i], got.layers[got.layers[i].in_tensor - 1]
    assert P.op == op and (L.act, L.cin, L.cout, L.kh, L.kw, L.sh, L.sw, L.pad_t, L.pad_l, L.res_tensor, L.reserved, L.in_layout) == \
           (mf.ACT_RELU, C, C, 1, 1, 1, 1, 0, 0, NONE, 0, 0)
    assert (L.in_h, L.in_w) == (L.out_h, L.out_w) == (P.out_h, P.out_w) and sum(M.op == B for M in got.layers) == 1
    assert got.layers[i + 1].op == mf.OP_PWCONV and got.layers[i + 1].in_tensor == i + 1
    if kind == "sum":
        assert P.res_tensor == 1 and P.act == mf.ACT_NONE and P.reserved == 0
    if kind == "shuffle":
        assert P.reserved == 2
    _folded(c, L, got.blob)
    assert L.w_off % 16 == 0 and L.b_off % 16 == 0


def _spell(c, x, how):
    if how == "relu":
        return c.node("Relu", [x]), mf.ACT_RELU
    if how == "clip":
        return c.node("Clip", [x, c.f32(value=0.0), c.f32(value=6.0)]), mf.ACT_RELU6
    if how == "swish":
        return c.node("Mul", [x, c.node("Sigmoid", [x])]), mf.ACT_SWISH
    if how == "gelu_erf_chain":
        e = c.node("Erf", [c.node("Div", [x, c.f32(value=np.float32(convert.SQRT2))])])
        return c.node("Mul", [c.node("Mul", [x, c.node("Add", [e, c.f32(value=1.0)])]), c.f32(value=0.5)]), mf.ACT_GELU_ERF
    if how == "gelu":
        return c.node("Gelu", [x], approximate="none"), mf.ACT_GELU_ERF
    if how == "gelu_tanh":
        return c.node("Gelu", [x], approximate="tanh"), mf.ACT_GELU_TANH
    if how == "hardswish":
        return c.node("HardSwish", [x]), mf.ACT_HSWISH
    if how == "hardswish_chain":
        r6 = c.node("Clip", [c.node("Add", [x, c.f32(value=3.0)]), c.f32(value=0.0), c.f32(value=6.0)])
        return c.node("Div", [c.node("Mul", [x, r6]), c.f32(value=6.0)]), mf.ACT_HSWISH
    raise KeyError(how)


SPELLINGS = ("relu", "clip", "swish", "gelu_erf_chain", "gelu", "gelu_tanh", "hardswish", "hardswish_chain")


@pytest.mark.parametrize("how", SPELLINGS)
def test_every_activation_spelling_completes_the_record(how, base, tmp_path):
    c = Case()
    x, C, _ = _producer(c, "concat")
    y, act = _spell(c, c.bn(x, C), how)
    got = both_readers(c.finish(c.conv(y, C, 16), 16), base, tmp_path)
    recs = [L for L in got.layers if L.op == B]
    assert len(recs) == 1 and recs[0].act == act and act in mf.BNACT_ACTS
    _folded(c, recs[0], got.blob)


def test_a_float16_file_an_epsilon_by_default_and_a_record_behind_a_record(base, tmp_path):
    c = Case()
    x, C, _ = _producer(c, "maxpool")
    y = c.node("Relu", [c.bn(x, C, eps=None)])                           # the attribute's default, 1e-5 as an f32
    first = c.params
    z = c.node("Relu", [c.bn(y, C, name="the_second", eps=1e-3)])        # a norm + activation of a norm + activation
    g = c.finish(z)                                                      # ... in front of the global pool
    got = both_readers(g, base, tmp_path)
    assert [L.op for L in got.layers] == [mf.OP_CONV, mf.OP_POOL, B, B, mf.OP_GAP, mf.OP_DENSE] and got.embedding_tensor == 5
    _folded(c, got.layers[3], got.blob, 1e-3)
    c.params = first
    _folded(c, got.layers[2], got.blob)
    g16 = convert.graph_to_float16(g)
    assert all(a.dtype == np.float16 for a in g16.initializers.values() if a.dtype.kind == "f")
    got16 = both_readers(g16, base, tmp_path)
    assert [L.op for L in got16.layers] == [L.op for L in got.layers]
    ga, be, mu, var = (g16.initializers[k].astype(np.float64) for k in first)
    scale = (ga / np.sqrt(var + float(np.float32(1e-5)))).astype(np.float32)
    assert got16.blob[got16.layers[2].w_off:][:C].tobytes() == scale.tobytes()


# ---- what stays refused, in the words it had --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PRODUCERS)
def test_a_bare_bn_keeps_the_refusal_of_its_producer(kind, base, tmp_path):
    c = Case()
    x, C, _ = _producer(c, kind)
    both_refuse(c.finish(c.conv(c.bn(x, C), C, 16), 16), base, tmp_path, TODAY[kind])      # BN -> Conv: something other than an activation reads it
    c = Case()
    x, C, _ = _producer(c, kind)
    both_refuse(c.finish(c.bn(x, C), C), base, tmp_path, TODAY[kind])                       # BN -> GlobalAveragePool


@pytest.mark.parametrize("kind", ("maxpool", "concat", "sum"))
def test_a_bn_read_by_an_activation_and_by_something_else_is_refused(kind, base, tmp_path):
    c = Case()
    x, C, _ = _producer(c, kind)
    y = c.bn(x, C)
    a = c.node("Relu", [y])
    z = c.node("Concat", [a, y], axis=1)
    both_refuse(c.finish(c.conv(z, 2 * C, 16), 16), base, tmp_path, TODAY[kind])
    # ... and where the second reader comes first in the file
    c = Case()
    x, C, _ = _producer(c, kind)
    y = c.bn(x, C)
    p = c.node("MaxPool", [y], kernel_shape=[1, 1])
    a = c.node("Relu", [y])
    both_refuse(c.finish(c.conv(c.node("Concat", [a, p], axis=1), 2 * C, 16), 16), base, tmp_path, TODAY[kind])
    # a swish whose Sigmoid has a second reader is no activation spelling: the norm stays bare
    c = Case()
    x, C, _ = _producer(c, kind)
    y = c.bn(x, C)
    s = c.node("Sigmoid", [y])
    z = c.node("Concat", [c.node("Mul", [y, s]), s], axis=1)
    both_refuse(c.finish(c.conv(z, 2 * C, 16), 16), base, tmp_path, TODAY[kind])


@pytest.mark.parametrize("kind", ("avgpool", "concat", "sum"))
def test_bn_sigmoid_a_clip_that_is_not_relu6_and_six_channels_are_refused(kind, base, tmp_path):
    c = Case()
    x, C, _ = _producer(c, kind)
    both_refuse(c.finish(c.conv(c.node("Sigmoid", [c.bn(x, C)]), C, 16), 16), base, tmp_path, TODAY[kind])
    c = Case()
    x, C, _ = _producer(c, kind)
    both_refuse(c.finish(c.conv(c.node("HardSigmoid", [c.bn(x, C)], alpha=float(np.float32(1 / 6)), beta=0.5), C, 16), 16), base, tmp_path, TODAY[kind])
    c = Case()
    x, C, _ = _producer(c, kind)
    both_refuse(c.finish(c.conv(c.node("Clip", [c.bn(x, C), c.f32(value=0.0), c.f32(value=1.0)]), C, 16), 16), base, tmp_path, TODAY[kind])


def test_a_channel_count_that_is_no_multiple_of_4_keeps_today_s_refusal(base, tmp_path):
    for kind in ("maxpool", "sum", "activated_conv"):
        c = Case(C=6)
        x, C, _ = _producer(c, kind)
        both_refuse(c.finish(c.conv(c.node("Relu", [c.bn(x, C)]), C, 16), 16), base, tmp_path, TODAY[kind])
        c = Case(C=12)                                   # one step away: 12 channels load
        x, C, _ = _producer(c, kind)
        got = both_readers(c.finish(c.conv(c.node("Relu", [c.bn(x, C)]), C, 16), 16), base, tmp_path)
        assert sum(L.op == B for L in got.layers) == 1


def test_rule_a_is_what_it_was(base, tmp_path):
    """a BN behind a convolution without an activation or a residual folds into it, or is refused where the output has other readers"""
    c = Case()
    y = c.node("Relu", [c.bn(c.conv(c.x, c.C, 16, 3), 16)])
    got = both_readers(c.finish(y, 16), base, tmp_path)
    assert [(L.op, L.act) for L in got.layers] == [(mf.OP_CONV, mf.ACT_RELU), (mf.OP_CONV, mf.ACT_RELU), (mf.OP_GAP, 0), (mf.OP_DENSE, 0)]
    c = Case()
    t = c.conv(c.x, c.C, c.C, 3)
    y = c.node("Add", [c.conv(c.node("Relu", [c.bn(t)]), c.C, c.C), t])         # the skip is taken in front of the BN
    both_refuse(c.finish(y), base, tmp_path, "BatchNormalization of a convolution output that has other readers cannot be folded")
    # the stem-less pre-activation block: the stem convolution feeds the first block's norm and its identity skip directly
    c = Case()
    stem = c.conv("spectrogram", 2, 8, 4, 4, name="bare_stem")
    p = c.node("Relu", [c.bn(stem)])
    y = c.node("Add", [c.conv(p, 8, 8, 3), stem])
    both_refuse(c.finish(y), base, tmp_path, "BatchNormalization of a convolution output that has other readers cannot be folded")
    # a norm behind the global pool, a dense layer or a LayerNorm is no image tensor's: refused as it was
    c = Case()
    p = c.node("GlobalAveragePool", [c.x])
    y = c.node("Flatten", [c.node("Relu", [c.bn(p)])], axis=1)
    c.node("Sigmoid", [c.node("Gemm", [y, c.f32(8, 10), c.f32(10)], outs=["logits"])], outs=["probabilities"])
    c.g.outputs.append(ox.ValueInfo("probabilities", ox.FLOAT, ["N", 10]))
    both_refuse(c.g, base, tmp_path, "BatchNormalization that does not follow a convolution directly")
    # a bare activation behind a pool or a concat stays refused too
    c = Case()
    x, C, _ = _producer(c, "concat")
    both_refuse(c.finish(c.conv(c.node("Relu", [x]), C, 16), 16), base, tmp_path, "the record carries no activation")
    c = Case()
    x, C, _ = _producer(c, "maxpool")
    both_refuse(c.finish(c.conv(c.node("Relu", [x]), C, 16), 16), base, tmp_path, "a pool layer carries no activation")


# ---- Concat prefix reuse -----------------------------------------------------------------------------------------------------------
def _dense_block(c, spelling, layers=4, growth=12, bad=None):
    """a dense block on c.x: layer k reads relu(bn(cat(f0 .. fk))) -- 'list': Concat over the whole list; 'pair': Concat(previous, new)"""
    feats, cat, C = [c.x], c.x, c.C
    for k in range(layers):
        y = c.conv(c.node("Relu", [c.bn(cat, C, name=f"bn{k}")]), C, growth, 3)
        feats.append(y)
        if spelling == "pair":
            cat = c.node("Concat", [cat, y], axis=1)
        else:
            lst = list(feats)
            if bad == "reordered" and k == layers - 1:
                lst[0], lst[1] = lst[1], lst[0]
            if bad == "missing" and k == layers - 1:
                del lst[1]
            cat = c.node("Concat", lst, axis=1)
        C = sum((c.C if i == 0 else growth) for i in range(len(feats))) - (growth if bad == "missing" and k == layers - 1 else 0)
    return c.finish(c.conv(c.node("Relu", [c.bn(cat, C, name="tail")]), C, 16), 16)


def test_the_list_spelling_of_a_dense_block_reads_to_the_two_input_records(base, tmp_path):
    pair = both_readers(_dense_block(Case(), "pair"), base, tmp_path)
    lst = both_readers(_dense_block(Case(), "list"), base, tmp_path)
    assert pair.layers == lst.layers and pair.blob.tobytes() == lst.blob.tobytes()
    cats = [L for L in lst.layers if L.op == mf.OP_CONCAT]
    assert len(cats) == 4 and all(L.res_tensor != NONE for L in cats)                  # one two-source record a layer
    assert [L.cin for L in cats] == [8, 20, 32, 44] and all(L.cout - L.cin == 12 for L in cats)
    assert sum(L.op == B for L in lst.layers) == 5


@pytest.mark.parametrize("bad", ("reordered", "missing"))
def test_a_list_whose_prefix_is_no_whole_earlier_concat_is_the_chain(bad, base, tmp_path):
    got = both_readers(_dense_block(Case(), "list", bad=bad), base, tmp_path)
    cats = [L for L in got.layers if L.op == mf.OP_CONCAT]
    # three reused records and the last Concat's own left-to-right chain over its 5 (4) inputs
    assert len(cats) == 3 + (4 if bad == "reordered" else 3)
    last = cats[3:]
    assert last[-1].cout == (56 if bad == "reordered" else 44)
    first_src = got.layers[last[0].in_tensor - 1]
    assert first_src.op != mf.OP_CONCAT                                                # the chain starts from a feature, not from an earlier concat


def test_existing_concat_graphs_keep_their_records(base, tmp_path):
    """a three-input Concat with no earlier Concat of its first two inputs is the chain it was"""
    c = Case()
    a, b2 = c.node("Relu", [c.conv(c.x, 8, 8, 3)]), c.node("Relu", [c.conv(c.x, 8, 12)])
    got = both_readers(c.finish(c.conv(c.node("Concat", [c.x, a, b2], axis=1), 28, 16), 16), base, tmp_path)
    cats = [(L.in_tensor, L.res_tensor, L.cin, L.cout) for L in got.layers if L.op == mf.OP_CONCAT]
    assert cats == [(1, 2, 8, 16), (4, 3, 16, 28)]


# ---- synth's plans -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_dense_plans_round_trip_bit_for_bit(seed, tmp_path):
    plan = synth.random_dense_plan(seed)
    assert plan == synth.random_dense_plan(seed)
    m = synth.build_model("dense_plan", plan=plan)
    recs = [L for L in m.layers if L.op == B]
    assert len(recs) >= 8 and all(L.act == plan["act"] for L in recs)
    producers = {m.layers[L.in_tensor - 1].op for L in recs}
    assert {mf.OP_POOL, mf.OP_CONCAT} <= producers and (mf.OP_CONV in producers or mf.OP_PWCONV in producers)
    assert m.layers[-3].op == B and m.layers[-2].op == mf.OP_GAP
    for L in recs:
        s = m.blob[L.w_off:L.w_off + L.cout]
        assert (s == 0).any() and (s < 0).any() and np.abs(s).max() > 2.0
    assert m.macs_per_segment() == sum(L.out_h * L.out_w * L.kh * L.kw * (1 if L.op == mf.OP_DWCONV else L.cin) * L.cout
                                        for L in m.layers if L.op in (mf.OP_CONV, mf.OP_PWCONV, mf.OP_DWCONV, mf.OP_DENSE))
    lib = _lib.load()
    for sc in ("pair", "list"):
        g = convert.graph_from_model(m, spell_concat=sc)
        if sc == "list":
            assert max(len(n.inputs) for n in g.nodes if n.op_type == "Concat") >= 3
        bns = [n for n in g.nodes if n.op_type == "BatchNormalization"]
        assert len(bns) == len(recs) and all(n.attrs["epsilon"] == 0.0 for n in bns)
        back = convert.model_from_graph(ox.load(ox.dump(g)), m)
        assert back.layers == m.layers and back.blob.tobytes() == m.blob.tobytes(), sc
        # from the audio input, through the library's reader and convert.py's: the same table, the same bits from the first layer on
        data = convert.model_to_onnx(m, frontend_spelling="stft", spell_concat=sc)
        onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m.bhm")
        with open(onnx_path, "wb") as f:
            f.write(data)
        assert lib.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, lib.bh_last_error()
        got, want = mf.read_model(out), convert.model_from_graph(ox.load(data), None, sample_rate=m.sample_rate)
        assert got.layers == want.layers
        first = got.layers[0].w_off
        assert got.blob[first:].tobytes() == want.blob[first:].tobytes() and got.blob.size == want.blob.size
        for x, y in zip(m.layers, got.layers):
            assert all(getattr(x, f) == getattr(y, f) for f in RECORD[:-2])
            if x.op == B:
                assert m.blob[x.w_off:x.w_off + x.cout].tobytes() == got.blob[y.w_off:y.w_off + x.cout].tobytes()
                assert m.blob[x.b_off:x.b_off + x.cout].tobytes() == got.blob[y.b_off:y.b_off + x.cout].tobytes()


def test_the_plans_cover_every_activation_and_block():
    acts, kinds = set(), set()
    for seed in range(12):
        plan = synth.random_dense_plan(seed)
        acts.add(plan["act"])
        kinds |= {it[0] if it[0] != "preact" else it[:3] for it in plan["items"]}
    assert acts == set(mf.BNACT_ACTS)
    assert {"dense", "trans", "mb", ("preact", "basic", "identity"), ("preact", "bottleneck", "proj")} <= kinds
    assert any(it[:3] == ("preact", "bottleneck", "identity") for s in range(12) for it in synth.random_dense_plan(s)["items"])


# ---- the container and the validator -----------------------------------------------------------------------------------------------
def _load(path, flags=0):
    """bh_plan_fused_blocks walks a model file on the host: load_model + validate_model; >= 0 = loaded (the fused blocks' count)"""
    L = _lib.load()
    rc = L.bh_plan_fused_blocks(path.encode(), flags, None, None, 0)
    return rc, L.bh_last_error().decode()


def _blocks(path, flags=0):
    """-> the first layer of every fused block the planner finds in the file"""
    import ctypes as C
    L = _lib.load()
    cfgs, first = (C.c_int32 * 256)(), (C.c_int32 * 256)()
    rc = L.bh_plan_fused_blocks(path.encode(), flags, cfgs, first, 256)
    assert rc >= 0, L.bh_last_error()
    return [int(first[i]) for i in range(rc)]


def test_the_round_trip_and_code_14_in_the_file(tmp_path):
    m = synth.build_model("dense_plan", seed=1)
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    back = mf.read_model(path)
    assert back.layers == m.layers and np.array_equal(back.blob, m.blob)
    raw = open(path, "rb").read()
    n_b, n_l = struct.unpack_from("<II", raw, 32)
    for i, L in enumerate(m.layers):
        rec = raw[mf.HEADER_SIZE + n_b * mf.BRANCH_SIZE + i * mf.LAYER_SIZE:][:mf.LAYER_SIZE]
        assert struct.unpack_from("<I", rec, 0)[0] == L.op and rec[88:] == bytes(40)
        if L.op == B:
            assert L.op == 14 and struct.unpack_from("<I", rec, 68)[0] == 0 and struct.unpack_from("<QQ", rec, 72) == (L.w_off, L.b_off)
    assert _load(path)[0] >= 0
    assert mf.OP_BNACT == 14 and mf.BNACT_ACTS == (1, 2, 3, 4, 5, 7)


def _two_records():
    """stem -> pool (tensor 2) -> norm + activation (3) -> norm + activation (4) -> global pool -> dense: tensor 2 has the second record's size"""
    b = synth._Builder(np.random.default_rng(3))
    base = synth.build_model("mini")
    br = [copy.deepcopy(x) for x in base.branches]
    for x in br:
        x.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(x.n_mels, x.n_bins, base.sample_rate, x.fmin, x.fmax))
    t, h, w = b.conv(0, 32, 115, 2, 8, 3, 2, mf.ACT_RELU, in_layout=1)
    t, h, w = b.pool(t, h, w, 8, 2, 2, 2, 2, mf.POOL_MAX, "valid")
    t = b.bnact(t, h, w, 8, mf.ACT_RELU)
    t = b.bnact(t, h, w, 8, mf.ACT_SWISH)
    t = b.gap(t, h, w, 8)
    b.dense(t, 8, 10)
    return synth._finish(b, br, base.sample_rate, base.sample_count, 10, 8, t, mf.OUT_SIGMOID)


BAD_RECORDS = {
    "window": (dict(kh=3), "unknown layer op"),
    "window_w": (dict(kw=2), "unknown layer op: a norm + activation layer with a window other than 1x1"),
    "stride": (dict(sw=2), "norm + activation layer with a stride or padding other than 1 / 0"),
    "padding": (dict(pad_t=1), "norm + activation layer with a stride or padding other than 1 / 0"),
    "changed_image": (dict(out_h=7), "norm + activation layer whose output image is not its input image"),
    "changed_channels": (dict(cin=12), "norm + activation layer that changes the channel count"),
    "planar_layout": (dict(in_layout=1), "norm + activation layer on the planar spectrogram (tensor 0)"),
    "residual": (dict(res_tensor=2), "norm + activation layer with a residual"),
    "reserved": (dict(reserved=1), "norm + activation layer with a reserved word that is not 0"),
    "no_activation": (dict(act=mf.ACT_NONE), "norm + activation layer without an activation"),
    "sigmoid": (dict(act=mf.ACT_SIGMOID), "norm + activation layer with a gate activation"),
    "hard_sigmoid": (dict(act=mf.ACT_HSIGMOID), "norm + activation layer with a gate activation"),
    "unknown_activation": (dict(act=9), "norm + activation layer with an unknown activation"),
    "scale_outside": (dict(w_off=1 << 40), "norm + activation layer scale / shift outside the blob"),
    "shift_outside": (lambda L, m: setattr(L, "b_off", m.blob.size - 4), "norm + activation layer scale / shift outside the blob"),
    "scale_misaligned": (lambda L, m: setattr(L, "w_off", L.w_off + 2), "norm + activation layer scale / shift at an offset that is not a multiple of 4"),
    "shift_misaligned": (lambda L, m: setattr(L, "b_off", L.b_off - 3), "norm + activation layer scale / shift at an offset that is not a multiple of 4"),
    "dilation": (dict(dil_h=2), "dilation on a norm + activation layer"),
}


@pytest.mark.parametrize("case", sorted(BAD_RECORDS))
def test_the_validator_refuses_a_bad_record(case, tmp_path):
    change, reason = BAD_RECORDS[case]
    m = _two_records()
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc >= 0, msg                                   # the model loads as it stands
    L = m.layers[3]
    assert L.op == B
    before = copy.copy(L)
    if callable(change):
        change(L, m)
    else:
        for k, v in change.items():
            setattr(L, k, v)
    assert sum(getattr(L, f) != getattr(before, f) for f in RECORD) == 1, case          # one field
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and reason in msg, (rc, msg)


def test_six_channels_tensor_0_and_the_unused_codes(tmp_path):
    path = str(tmp_path / "m.bhm")
    m = _two_records()
    for L in m.layers[:5]:
        L.cout = 6
        if L.op != mf.OP_CONV:
            L.cin = 6
    m.layers[5].cin = 6
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and "norm + activation layer over a channel count that is not a multiple of 4" in msg, msg
    for code in (9, 11, 15):
        m = _two_records()
        m.layers[3].op = code
        mf.write_model(path, m)
        rc, msg = _load(path)
        assert rc < 0 and "unknown layer op" in msg, (code, msg)
    # every activation of the record's set loads
    for act in mf.BNACT_ACTS:
        m = _two_records()
        m.layers[3].act = act
        mf.write_model(path, m)
        assert _load(path)[0] >= 0, act


def test_no_matcher_fuses_across_a_norm_activation_layer(tmp_path):
    """expand -> depthwise -> project with a norm + activation record between two of them is no triple in any precision, while the same
    stack without the record is one: behind the expand convolution the record leaves depthwise -> project, a block of its own that starts
    behind it, and in front of the project convolution nothing.  A dense plan's only fused block is its MBConv item."""
    lib = _lib.load()

    def stack(where):
        b = synth._Builder(np.random.default_rng(4))
        base = synth.build_model("mini")
        br = [copy.deepcopy(x) for x in base.branches]
        for x in br:
            x.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(x.n_mels, x.n_bins, base.sample_rate, x.fmin, x.fmax))
        t, h, w = b.conv(0, 32, 115, 2, 16, 3, 2, mf.ACT_RELU6, in_layout=1)
        t = b.pwconv(t, h, w, 16, 64, mf.ACT_RELU6)
        if where == 1:
            t = b.bnact(t, h, w, 64, mf.ACT_RELU6)
        t, h, w = b.dwconv(t, h, w, 64, 3, 1, mf.ACT_RELU6)
        if where == 2:
            t = b.bnact(t, h, w, 64, mf.ACT_RELU6)
        t = b.pwconv(t, h, w, 64, 24, mf.ACT_NONE)
        t = b.gap(t, h, w, 24)
        b.dense(t, 24, 10)
        return synth._finish(b, br, base.sample_rate, base.sample_count, 10, 24, t, mf.OUT_SIGMOID)
    path = str(tmp_path / "m.bhm")
    for flags in (0, 1, 2, 3):
        mf.write_model(path, stack(0))
        assert _blocks(path, flags) == [1], flags                   # pw -> dw -> pw from the expand convolution on
        mf.write_model(path, stack(1))
        assert _blocks(path, flags) in ([], [3]), flags             # at most dw -> pw, behind the record (layer 2)
        mf.write_model(path, stack(2))
        assert _blocks(path, flags) == [], flags
    for seed in range(4):
        m = synth.build_model("dense_plan", seed=seed)
        mf.write_model(path, m)
        recs = {i for i, L in enumerate(m.layers) if L.op == B}
        for first in _blocks(path):
            run = m.layers[first:first + 3]
            assert [L.op for L in run] == [mf.OP_PWCONV, mf.OP_DWCONV, mf.OP_PWCONV] and not recs & set(range(first, first + 3)), (seed, first)


# ---- fails without the feature -----------------------------------------------------------------------------------------------------
def test_a_dense_plan_and_densenet_audio_load_through_both_routes(tmp_path):
    """before this op existed the .onnx route ended in a BatchNormalization refusal and the .bhm route in 'unknown layer op'"""
    lib = _lib.load()
    for m, sc in ((synth.build_model("dense_plan", seed=0), "pair"), (synth.build_model("densenet_audio", n_classes=40), "list")):
        onnx_path, out = str(tmp_path / "m.onnx"), str(tmp_path / "m_native.bhm")
        with open(onnx_path, "wb") as f:
            f.write(convert.model_to_onnx(m, frontend_spelling="stft", spell_concat=sc))
        assert lib.bh_onnx_to_bhm(onnx_path.encode(), out.encode()) == 0, lib.bh_last_error()
        got = mf.read_model(out)
        assert len(got.layers) == len(m.layers)
        for x, y in zip(m.layers, got.layers):
            assert all(getattr(x, f) == getattr(y, f) for f in RECORD[:-2])
        path = str(tmp_path / "m.bhm")
        mf.write_model(path, m)
        rc, msg = _load(path)
        assert rc >= 0, msg
    big = synth.build_model("densenet_audio", n_classes=40)
    recs = [L for L in big.layers if L.op == B]
    assert len(recs) == 58 + 3 + 1 and recs[-1].cout == 1024 and {L.act for L in recs} == {mf.ACT_RELU}
    assert sum(L.op == mf.OP_CONCAT for L in big.layers) == 58 and all(L.res_tensor != NONE for L in big.layers if L.op == mf.OP_CONCAT)


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------
def test_mutated_dense_files_are_refused_or_read_never_a_crash():
    """tools/fuzz_onnx_reader.py over dense plans (both concat spellings, from the audio input) and containers with code-14 records, in
    child processes: every mutant loads or is refused"""
    import subprocess
    import sys
    env = dict(os.environ, FUZZ_BNACT="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_onnx_reader.py"), "120", "5"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-600:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("120 mutants, 0 bad batches"), r.stdout[-800:]
