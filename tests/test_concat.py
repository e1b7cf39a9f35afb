"""Channel Concat, Split / Slice and the channel shuffle on the host side: the container's OP_CONCAT record, both ONNX readers, the
writer, the validator and the fusion planner.

* hand-written graphs -- a Fire module, a 4-way Inception module, both ShuffleNetV2 units, the Slice spelling, a float16 file -- go
  through the library's reader (bh_onnx_to_bhm) and through convert.py to the stated records, the same layer table and the same
  blob, bit for bit;
* forward64 -- tests/test_gconv.py's float64 forward with OP_CONCAT added (a gather: no arithmetic); the device tests
  (tests/test_concat_gpu.py) are held to it -- against a torch float64 composition (torch.cat, chunk / narrow, the
  reshape-transpose shuffle).  The plain-C oracle never sees such a model;
* convert.model_to_onnx -> either reader reproduces the records of the random multi-branch plans, and every plan holds what
  synth.random_branchy_plan promises;
* every refusal of the readers and of the validator (model.hpp validate_model, through the library's host-only loader) is checked by
  its message; op 9 stays unknown, op 10 loads;
* the planner (bh_plan_fused_blocks) does not fuse an expand -> depthwise -> project triple whose expand output a concat also reads;
* the records of a model without a concat are what they were.
"""
import copy
import ctypes as C
import hashlib

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O
from test_gconv import layer64g
from test_pool import RECORD, both_readers, same_tables_and_blob

NONE = mf.NO_TENSOR
I64_MAX = (1 << 63) - 1


# ---- the yardstick: the model's logits in float64 ----------------------------------------------------------------------------------
def gather(L, A, B, n):
    """An OP_CONCAT record on its source tensors (any dtype; no arithmetic): channels w_off .. w_off + cin - 1 of A, then channels
    b_off .. b_off + (cout - cin) - 1 of B, shuffled in L.reserved groups -> [n][out_h][out_w][cout]"""
    px = L.in_h * L.in_w
    cat = A.reshape(n, px, -1)[:, :, L.w_off:L.w_off + L.cin]
    assert cat.shape[2] == L.cin
    if B is not None:
        b = B.reshape(n, px, -1)[:, :, L.b_off:L.b_off + L.cout - L.cin]
        assert b.shape[2] == L.cout - L.cin
        cat = np.concatenate([cat, b], axis=2)
    if L.reserved > 1:
        c = np.arange(L.cout)
        cat = cat[:, :, (c % L.reserved) * (L.cout // L.reserved) + c // L.reserved]
    return np.ascontiguousarray(cat).reshape(n, L.out_h, L.out_w, L.cout)


def layer64c(m, L, X, R):
    if L.op == mf.OP_CONCAT:          # res_tensor is the second input here, not a residual
        return gather(L, np.asarray(X, np.float64), None if R is None else np.asarray(R, np.float64), X.shape[0])
    return layer64g(m, L, X, R)


def forward64(m, segs, tensors=False):
    """-> logits [n][n_classes] in float64 (tensors=True: every tensor, T[0] the spectrogram)"""
    spec, _ = O.frontend64(m, segs)
    T = [spec]
    for L in m.layers:
        T.append(layer64c(m, L, T[L.in_tensor], None if L.res_tensor == NONE else T[L.res_tensor]))
    return T if tensors else T[-1].reshape(segs.shape[0], -1)


# ---- hand-written graphs through both readers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return synth.build_model("mini")          # the two-branch 32 x 115 front-end: a graph that starts at the spectrogram


class Net:
    """spectrogram [N, 2, 32, 115] -> Conv 3x3 stride 2 SAME (a 16 x 58 image of `stem_c` channels) -> Relu = self.stem, tensor 1;
    then whatever the case adds; finish(): -> Conv 1x1 -> GlobalAveragePool -> Flatten -> Gemm"""

    def __init__(self, stem_c=16):
        self.rng = np.random.default_rng(17)
        self.g = ox.Graph(name="concat_case", producer="tests")
        self.g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", 2, 32, 115]))
        self.k = 0
        c0 = self._conv("spectrogram", 2, stem_c, 3, 3, {"strides": [2, 2], "auto_pad": "SAME_UPPER"}, "stem")
        self.stem = self.relu(c0)

    def f32(self, *s):
        return self.rng.standard_normal(s).astype(np.float32)

    def _conv(self, x, cin, cout, kh, kw, attrs, name=None, group=1):
        self.k += 1
        w, b, y = f"w{self.k}", f"b{self.k}", f"c{self.k}"
        self.g.initializers[w], self.g.initializers[b] = self.f32(cout, cin // group, kh, kw) * np.float32(0.3), self.f32(cout) * np.float32(0.1)
        a = {"kernel_shape": [kh, kw], "group": group}
        a.update(attrs)
        self.g.nodes.append(ox.Node("Conv", [x, w, b], [y], a, name=name or y))
        return y

    def relu(self, x):
        self.g.nodes.append(ox.Node("Relu", [x], [x + "_r"]))
        return x + "_r"

    def conv(self, x, cin, cout, kh=1, kw=1, stride=1, group=1, relu=True):
        y = self._conv(x, cin, cout, kh, kw, {"strides": [stride, stride], "pads": [kh // 2, kw // 2, kh // 2, kw // 2]}, group=group)
        return self.relu(y) if relu else y

    def node(self, op, ins, outs, attrs=None, name=""):
        self.g.nodes.append(ox.Node(op, list(ins), list(outs), dict(attrs or {}), name=name or outs[0]))
        return outs[0] if len(outs) == 1 else outs

    def ints(self, name, values, constant_node=False):
        if constant_node:
            self.g.nodes.append(ox.Node("Constant", [], [name], {"value": np.asarray(values, np.int64)}, name=name))
        else:
            self.g.initializers[name] = np.asarray(values, np.int64)
        return name

    def shuffle(self, x, groups, c, h=16, w=58, s5=None, s4=None, constant_node=False):
        self.node("Reshape", [x, self.ints(x + "_s5", s5 or [0, groups, c // groups, h, w], constant_node)], [x + "_5d"], name=x + "_shuffle")
        self.node("Transpose", [x + "_5d"], [x + "_tr"], {"perm": [0, 2, 1, 3, 4]})
        return self.node("Reshape", [x + "_tr", self.ints(x + "_s4", s4 or [0, c, h, w], constant_node)], [x + "_shuffled"])

    def finish(self, x, c):
        y = self._conv(x, c, 16, 1, 1, {}, "head")
        self.node("GlobalAveragePool", [y], ["gap"])
        self.node("Flatten", ["gap"], ["flat"], {"axis": 1})
        self.g.initializers["wd"], self.g.initializers["bd"] = self.f32(16, 10), self.f32(10)
        self.node("Gemm", ["flat", "wd", "bd"], ["logits"])
        self.g.outputs.append(ox.ValueInfo("logits", ox.FLOAT, ["N", 10]))
        return self.g


def fire(axis=1):
    n = Net()
    s = n.conv(n.stem, 16, 8)
    a, d = n.conv(s, 8, 16), n.conv(s, 8, 16, 3, 3)
    return n.finish(n.node("Concat", [a, d], ["cat"], {"axis": axis}, "the_concat"), 32)


def inception4():
    n = Net()
    b1 = n.conv(n.stem, 16, 8)
    b3 = n.conv(n.conv(n.stem, 16, 8), 8, 16, 3, 3)
    b7 = n.conv(n.conv(n.conv(n.stem, 16, 8), 8, 8, 1, 7), 8, 12, 7, 1)
    bp = n.conv(n.node("AveragePool", [n.stem], ["ap"], {"kernel_shape": [3, 3], "strides": [1, 1], "pads": [1, 1, 1, 1]}), 16, 4)
    return n.finish(n.node("Concat", [b1, b3, b7, bp], ["cat"], {"axis": -3}, "the_concat"), 40)


def shufflenet_basic(sizes="attribute", constant_node=False, s5=None, s4=None):
    """Split -> (x1 | 1x1 -> depthwise 3x3 -> 1x1 of x2) -> Concat -> shuffle"""
    n = Net()
    attrs, ins = {"axis": 1}, [n.stem]
    if sizes == "attribute":
        attrs["split"] = [8, 8]
    elif sizes == "input":
        ins.append(n.ints("sizes", [8, 8], constant_node))
    elif sizes == "num_outputs":
        attrs["num_outputs"] = 2
    x1, x2 = n.node("Split", ins, ["x1", "x2"], attrs, "the_split")
    y = n.conv(n.conv(n.conv(x2, 8, 8), 8, 8, 3, 3, group=8, relu=False), 8, 8)
    cat = n.node("Concat", [x1, y], ["cat"], {"axis": 1}, "the_concat")
    return n.finish(n.shuffle(cat, 2, 16, s5=s5, s4=s4, constant_node=constant_node), 16)


def shufflenet_down():
    """depthwise 3x3 stride 2 -> 1x1 | 1x1 -> depthwise 3x3 stride 2 -> 1x1, both of the stem; Concat -> shuffle on an 8 x 29 image"""
    n = Net()
    l = n.conv(n.conv(n.stem, 16, 16, 3, 3, stride=2, group=16, relu=False), 16, 12)
    r = n.conv(n.conv(n.conv(n.stem, 16, 12), 12, 12, 3, 3, stride=2, group=12, relu=False), 12, 12)
    cat = n.node("Concat", [l, r], ["cat"], {"axis": 1}, "the_concat")
    return n.finish(n.shuffle(cat, 2, 24, 8, 29, s5=[-1, 2, 12, 8, 29], s4=[0, -1, 8, 29], constant_node=True), 24)


def sliced(starts, ends, axes=(1,), steps=None, reader="conv"):
    """Slice of the stem -> a convolution (the slice is materialised) or a Concat with a convolution of the stem (it is folded)"""
    n = Net()
    ins = [n.stem, n.ints("starts", starts), n.ints("ends", ends), n.ints("axes", axes)] + ([n.ints("steps", steps)] if steps else [])
    x = n.node("Slice", ins, ["cut"], {}, "the_slice")
    if reader == "conv":
        return n.finish(n.conv(x, 8, 8), 8)
    y = n.conv(n.stem, 16, 8)
    return n.finish(n.node("Concat", [y, x], ["cat"], {"axis": 1}, "the_concat"), 16)


def _rec(in_t, res_t, cin, cout, w_off=0, b_off=0, groups=0, h=16, w=58):
    return mf.Layer(mf.OP_CONCAT, mf.ACT_NONE, in_t, res_t, cin, cout, 1, 1, 1, 1, 0, 0, h, w, h, w, 0, w_off, b_off, groups)


# case -> (graph, {layer index: the stated record}, the op of every layer)
CV, DW, PW, GAP, FC, CAT, POOL = mf.OP_CONV, mf.OP_DWCONV, mf.OP_PWCONV, mf.OP_GAP, mf.OP_DENSE, mf.OP_CONCAT, mf.OP_POOL
ACCEPTED = {
    # tensors: 1 stem, 2 squeeze, 3 expand 1x1, 4 expand 3x3 -> 5
    "fire": (fire, {4: _rec(3, 4, 16, 32)}, [CV, PW, PW, CV, CAT, PW, GAP, FC]),
    # 1 stem, 2 b1, 3-4 b3, 5-7 b7, 8 pool, 9 its 1x1; a left-to-right chain of three records: 8 + 16, 24 + 12, 36 + 4
    "inception4": (inception4, {9: _rec(2, 4, 8, 24), 10: _rec(10, 7, 24, 36), 11: _rec(11, 9, 36, 40)},
                   [CV, PW, PW, CV, PW, CV, CV, POOL, PW, CAT, CAT, CAT, PW, GAP, FC]),
    # x1 is a view of the stem folded into the Concat's window; x2 -- channels 8 .. 15 -- is materialised for its convolution
    # (tensor 2); 3-5 the branch; the shuffle is the Concat's only reader: its record's reserved word
    "shufflenet_basic": (shufflenet_basic, {1: _rec(1, NONE, 8, 8, w_off=8), 5: _rec(1, 5, 8, 16, groups=2)}, [CV, CAT, PW, DW, PW, CAT, PW, GAP, FC]),
    "split_sizes_from_an_initializer": (lambda: shufflenet_basic("input"), {1: _rec(1, NONE, 8, 8, w_off=8), 5: _rec(1, 5, 8, 16, groups=2)}, None),
    "split_sizes_from_a_constant_node": (lambda: shufflenet_basic("input", True), {1: _rec(1, NONE, 8, 8, w_off=8), 5: _rec(1, 5, 8, 16, groups=2)}, None),
    "split_num_outputs": (lambda: shufflenet_basic("num_outputs"), {1: _rec(1, NONE, 8, 8, w_off=8), 5: _rec(1, 5, 8, 16, groups=2)}, None),
    "split_equal_parts": (lambda: shufflenet_basic("none"), {1: _rec(1, NONE, 8, 8, w_off=8), 5: _rec(1, 5, 8, 16, groups=2)}, None),
    "shuffle_shapes_with_minus_one": (lambda: shufflenet_basic(s5=[0, 2, -1, 16, 58], s4=[0, -1, 16, 58]), {5: _rec(1, 5, 8, 16, groups=2)}, None),
    # 1 stem, 2-3 left, 4-6 right -> 7, shapes from Constant nodes with -1 entries
    "shufflenet_down": (shufflenet_down, {6: _rec(3, 6, 12, 24, groups=2, h=8, w=29)}, [CV, DW, PW, PW, DW, PW, CAT, PW, GAP, FC]),
    "slice_materialised": (lambda: sliced([8], [16]), {1: _rec(1, NONE, 8, 8, w_off=8)}, [CV, CAT, PW, PW, GAP, FC]),
    "slice_end_clamped": (lambda: sliced([8], [I64_MAX]), {1: _rec(1, NONE, 8, 8, w_off=8)}, None),
    "slice_negative_indices": (lambda: sliced([-12], [-4], axes=[-3], steps=[1]), {1: _rec(1, NONE, 8, 8, w_off=4)}, None),
    "slice_folded": (lambda: sliced([4], [12], reader="concat"), {2: _rec(2, 1, 8, 16, b_off=4)}, [CV, PW, CAT, PW, GAP, FC]),
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_both_readers_give_the_stated_records(case, base, tmp_path):
    make, stated, ops = ACCEPTED[case]
    want, got = both_readers(make(), base, tmp_path)
    same_tables_and_blob(want, got)
    if ops is not None:
        assert [L.op for L in got.layers] == ops
    for i, rec in stated.items():
        assert got.layers[i] == rec, (i, got.layers[i], rec)


def test_a_shuffle_that_is_not_the_concats_only_reader_is_a_record_of_its_own(base, tmp_path):
    """the Concat's output read by the shuffle AND by a convolution: the shuffle cannot ride on the Concat's record"""
    n = Net()
    a, d = n.conv(n.stem, 16, 8), n.conv(n.stem, 16, 8)
    cat = n.node("Concat", [a, d], ["cat"], {"axis": 1})
    sh = n.shuffle(cat, 4, 16)
    side = n.conv(cat, 16, 16)
    g = n.finish(n.node("Concat", [sh, side], ["both"], {"axis": 1}), 32)
    want, got = both_readers(g, base, tmp_path)
    same_tables_and_blob(want, got)
    assert got.layers[3] == _rec(2, 3, 8, 16) and got.layers[4] == _rec(4, NONE, 16, 16, groups=4) and got.layers[6] == _rec(5, 6, 16, 32)


def test_both_readers_read_a_float16_file_alike(base, tmp_path):
    for make in (fire, shufflenet_basic, shufflenet_down):
        g16 = convert.graph_to_float16(make())
        assert all(a.dtype == np.float16 for a in g16.initializers.values() if a.dtype.kind == "f")
        want, got = both_readers(g16, base, tmp_path)
        same_tables_and_blob(want, got)
        w32, _ = both_readers(make(), base, tmp_path)
        assert [(L.op, L.in_tensor, L.res_tensor, L.cin, L.cout, L.reserved) for L in got.layers] == \
               [(L.op, L.in_tensor, L.res_tensor, L.cin, L.cout, L.reserved) for L in w32.layers]


# ---- forward64 against torch -----------------------------------------------------------------------------------------------------------
def test_forward64_is_the_torch_composition():
    """every OP_CONCAT tensor of the random plans' float64 forward against torch.cat / narrow / chunk and the reshape-transpose
    shuffle of the same source tensors; and the operator chain of a ShuffleNetV2 unit -- chunk, cat, shuffle -- as torch spells it"""
    import torch
    seen = set()
    for seed in (0, 1):
        m = synth.build_model("branchy_plan", plan=synth.random_branchy_plan(seed))
        segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=3)
        T = forward64(m, segs, tensors=True)
        nchw = lambda t, L: torch.from_numpy(np.ascontiguousarray(np.asarray(T[t]).reshape(2, L.in_h, L.in_w, -1).transpose(0, 3, 1, 2)))
        for i, L in enumerate(m.layers):
            if L.op != CAT:
                continue
            a = nchw(L.in_tensor, L)
            if L.w_off == 0 and 2 * L.cin == a.shape[1]:
                parts = [torch.chunk(a, 2, dim=1)[0]]
            elif L.w_off == L.cin and 2 * L.cin == a.shape[1]:
                parts = [torch.chunk(a, 2, dim=1)[1]]
            else:
                parts = [a.narrow(1, L.w_off, L.cin)]
            if L.res_tensor != NONE:
                parts.append(nchw(L.res_tensor, L).narrow(1, L.b_off, L.cout - L.cin))
            y = torch.cat(parts, dim=1)
            if L.reserved > 1:
                y = y.reshape(2, L.reserved, L.cout // L.reserved, L.out_h, L.out_w).transpose(1, 2).reshape(2, L.cout, L.out_h, L.out_w)
            want = y.numpy().transpose(0, 2, 3, 1)
            assert T[i + 1].shape == want.shape and np.abs(T[i + 1] - want).max() <= 1e-12, (seed, i)
            seen.add((L.res_tensor != NONE, L.reserved > 1, L.w_off > 0))
        assert np.isfinite(T[-1]).all() and np.abs(T[-1]).max() > 0
    assert {(True, False, False), (True, True, False), (False, False, True), (False, True, False)} <= seen


# ---- the writer, and the random plans -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_model_to_onnx_round_trip_reproduces_the_records(seed, tmp_path):
    plan = synth.random_branchy_plan(seed)
    assert plan == synth.random_branchy_plan(seed)
    m = synth.build_model("branchy_plan", plan=plan)
    data = convert.model_to_onnx(m)
    g = ox.load(data)
    assert sum(n.op_type == "Concat" for n in g.nodes) >= 7 and sum(n.op_type == "Transpose" for n in g.nodes) == 3
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
        for f in (RECORD if x.op == CAT else RECORD[:-2]):
            assert getattr(x, f) == getattr(y, f), (i, f)
    # the float16 rewrite keeps the records
    m16 = convert.model_from_graph(convert.graph_to_float16(convert.graph_from_model(m)), m, "spectrogram")
    assert [(L.op, L.reserved, L.in_tensor, L.res_tensor) for L in m16.layers] == [(L.op, L.reserved, L.in_tensor, L.res_tensor) for L in m.layers]


def _fused_blocks(path, flags=0):
    L = _lib.load()
    cfgs, layers = (C.c_int32 * 256)(), (C.c_int32 * 256)()
    n = L.bh_plan_fused_blocks(path.encode(), flags, cfgs, layers, 256)
    assert n >= 0, L.bh_last_error()
    return [int(layers[k]) for k in range(n)]


@pytest.mark.parametrize("seed", range(6))
def test_random_branchy_plans_hold_what_they_promise(seed, tmp_path):
    m = synth.build_model("branchy_plan", plan=synth.random_branchy_plan(seed))
    path = str(tmp_path / "p.bhm")
    mf.write_model(path, m)
    fused = _fused_blocks(path)
    cats = [(i, L) for i, L in enumerate(m.layers) if L.op == CAT]
    reads = lambda L: [t for t in (L.in_tensor, L.res_tensor) if t != NONE]
    # an MBConv block that runs fused (expand at layer f, project at f + 2) feeds a concat
    assert any(f + 3 in reads(L) for f in fused for _, L in cats), (fused, [reads(L) for _, L in cats])
    # a concat feeds a fused MBConv block
    assert any(m.layers[f].in_tensor == i + 1 for f in fused for i, _ in cats)
    # a 4-way concat: a chain of three records, each reading the one before as its first source
    assert any(m.layers[i + 1].op == CAT and m.layers[i + 2].op == CAT and m.layers[i + 1].in_tensor == i + 1 and m.layers[i + 2].in_tensor == i + 2
               for i, _ in cats[:-2])
    # a view folded into a concat (a window narrower than its source), a materialised view, windows at non-zero offsets
    width = lambda t: m.layers[t - 1].cout
    assert any(L.res_tensor != NONE and L.cin < width(L.in_tensor) for _, L in cats)
    assert any(L.res_tensor == NONE and L.reserved <= 1 and L.cin < width(L.in_tensor) for _, L in cats)
    assert any(L.w_off > 0 for _, L in cats)
    # shuffles: on a Concat's record and as a record of its own
    assert any(L.res_tensor != NONE and L.reserved > 1 for _, L in cats) and any(L.res_tensor == NONE and L.reserved > 1 for _, L in cats)
    assert any(L.op == mf.OP_GCONV for L in m.layers) and any(L.kh != L.kw for L in m.layers if L.op == CV)


def test_shufflenet_audio_is_shufflenet_v2_x1_5():
    m = synth.build_model("shufflenet_audio", n_classes=50)
    cats = [L for L in m.layers if L.op == CAT]
    assert sorted({L.cout for L in cats if L.reserved == 2}) == [176, 352, 704] and sum(L.reserved == 2 for L in cats) == 16
    assert m.layers[0].cout == 24 and m.layers[-3].cout == 1024 and (m.spec_h, m.spec_w) == (96, 511)


# ---- refusals of the readers --------------------------------------------------------------------------------------------------------
def _bad_concat(kind):
    n = Net()
    a = n.conv(n.stem, 16, 8)
    if kind == "other_images":
        return n.finish(n.node("Concat", [a, n.conv(n.stem, 16, 8, 3, 3, stride=2)], ["cat"], {"axis": 1}, "the_concat"), 16)
    if kind == "constant_input":
        n.g.initializers["k"] = n.f32(1, 8, 16, 58)
        return n.finish(n.node("Concat", [a, "k"], ["cat"], {"axis": 1}, "the_concat"), 16)
    if kind == "off_path_input":
        return n.finish(n.node("Concat", [a, "nowhere"], ["cat"], {"axis": 1}, "the_concat"), 16)
    if kind == "spectrogram_input":
        n.node("Concat", ["spectrogram", "spectrogram"], ["cat0"], {"axis": 1}, "the_concat")
        return n.finish(a, 8)
    if kind == "width_6":
        return n.finish(n.node("Concat", [a, n.conv(n.stem, 16, 6)], ["cat"], {"axis": 1}, "the_concat"), 14)
    d = n.conv(n.stem, 16, 8)
    cat = n.node("Concat", [a, d], ["cat"], {"axis": 1}, "the_concat")
    if kind == "relu_behind":
        return n.finish(n.relu(cat), 16)
    if kind == "swish_behind":
        n.node("Sigmoid", [cat], ["sg"])
        return n.finish(n.node("Mul", [cat, "sg"], ["sw"]), 16)
    if kind == "batchnorm_behind":
        for k in "gbmv":
            n.g.initializers["bn_" + k] = np.abs(n.f32(16)) + np.float32(0.5)
        return n.finish(n.node("BatchNormalization", [cat, "bn_g", "bn_b", "bn_m", "bn_v"], ["bn"], {"epsilon": 1e-3}, "the_bn"), 16)
    if kind == "residual_into_it":
        return n.finish(n.node("Add", [cat, n.stem], ["sum"]), 16)
    if kind == "relu_behind_a_shuffle":
        return n.finish(n.relu(n.shuffle(cat, 2, 16)), 16)
    if kind == "computed_shape":
        n.node("Shape", [cat], ["shp"], {}, "the_shape")
        n.node("Reshape", [cat, "shp"], ["r5"], {}, "r5")
        n.node("Transpose", ["r5"], ["tr"], {"perm": [0, 2, 1, 3, 4]})
        return n.finish(n.node("Reshape", ["tr", n.ints("s4", [0, 16, 16, 58])], ["out"]), 16)
    if kind == "shuffle_of_other_shapes":
        return n.finish(n.shuffle(cat, 2, 16, s5=[0, 2, 8, 58, 16]), 16)
    if kind == "lone_transpose":
        return n.finish(n.node("Transpose", [cat], ["tr"], {"perm": [0, 1, 3, 2]}, "the_transpose"), 16)
    if kind == "lone_reshape":
        return n.finish(n.node("Reshape", [cat, n.ints("s", [0, 16, 58, 16])], ["rs"], {}, "the_reshape"), 16)
    raise ValueError(kind)


def _bad_split(kind):
    n = Net()
    if kind == "split_axis_2":
        x1, x2 = n.node("Split", [n.stem], ["x1", "x2"], {"axis": 2, "split": [8, 8]}, "the_split")
    elif kind == "split_parts_of_6_and_10":
        x1, x2 = n.node("Split", [n.stem], ["x1", "x2"], {"axis": 1, "split": [6, 10]}, "the_split")
        return n.finish(n.node("Concat", [n.conv(x1, 6, 6, relu=False), x2], ["cat"], {"axis": 1}), 16)
    elif kind == "split_sizes_do_not_add_up":
        x1, x2 = n.node("Split", [n.stem], ["x1", "x2"], {"axis": 1, "split": [8, 12]}, "the_split")
    elif kind == "relu_behind_a_split":
        x1, x2 = n.node("Split", [n.stem], ["x1", "x2"], {"axis": 1, "split": [8, 8]}, "the_split")
        x1 = n.relu(x1)
    return n.finish(n.node("Concat", [x1, n.conv(x2, 8, 8)], ["cat"], {"axis": 1}), 16)


REFUSED = {
    "concat_axis_2": (lambda: fire(axis=2), ("the_concat", "axis 2")),
    "concat_of_other_images": (lambda: _bad_concat("other_images"), ("the_concat", "different images")),
    "concat_with_a_constant": (lambda: _bad_concat("constant_input"), ("the_concat", "constant")),
    "concat_with_an_off_path_input": (lambda: _bad_concat("off_path_input"), ("the_concat", "not on the path")),
    "concat_of_the_spectrogram": (lambda: _bad_concat("spectrogram_input"), ("the_concat", "spectrogram")),
    "concat_of_6_channels": (lambda: _bad_concat("width_6"), ("the_concat", "not a multiple of 4", "58-channel")),
    "relu_behind_a_concat": (lambda: _bad_concat("relu_behind"), ("activation", "Concat")),
    "swish_behind_a_concat": (lambda: _bad_concat("swish_behind"), ("activation", "Concat")),
    "batchnorm_behind_a_concat": (lambda: _bad_concat("batchnorm_behind"), ("BatchNormalization", "the_bn", "Concat")),
    "residual_add_into_a_concat": (lambda: _bad_concat("residual_into_it"), ("no convolution to fold the residual into",)),
    "relu_behind_a_shuffle": (lambda: _bad_concat("relu_behind_a_shuffle"), ("activation", "shuffle")),
    "shuffle_with_a_computed_shape": (lambda: _bad_concat("computed_shape"), ("Shape",)),
    "shuffle_of_other_shapes": (lambda: _bad_concat("shuffle_of_other_shapes"), ("channel shuffle", "[N, g, C / g, H, W]")),
    "transpose_outside_the_pattern": (lambda: _bad_concat("lone_transpose"), ("Transpose",)),
    "reshape_outside_the_pattern": (lambda: _bad_concat("lone_reshape"), ("Reshape of a 16x58 map",)),
    "split_axis_2": (lambda: _bad_split("split_axis_2"), ("the_split", "axis 2")),
    "split_parts_of_6_and_10": (lambda: _bad_split("split_parts_of_6_and_10"), ("the_split", "not a multiple of 4")),
    "split_sizes_do_not_add_up": (lambda: _bad_split("split_sizes_do_not_add_up"), ("the_split", "add up")),
    "relu_behind_a_split": (lambda: _bad_split("relu_behind_a_split"), ("activation", "Split")),
    "slice_axis_2": (lambda: sliced([8], [16], axes=[2]), ("the_slice", "axis 2")),
    "slice_step_2": (lambda: sliced([0], [16], steps=[2]), ("the_slice", "step 2")),
    "slice_from_channel_2": (lambda: sliced([2], [10]), ("the_slice", "not a multiple of 4")),
    "slice_empty": (lambda: sliced([12], [4]), ("the_slice", "empty")),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_both_readers_refuse_by_name(case, base, tmp_path):
    make, reasons = REFUSED[case]
    data = ox.dump(make())
    with pytest.raises(convert.ConvertError) as e:
        convert.model_from_graph(ox.load(data), base)
    for reason in reasons:
        assert reason in str(e.value), str(e.value)
    onnx_path = str(tmp_path / "refused.onnx")
    with open(onnx_path, "wb") as f:
        f.write(data)
    L = _lib.load()
    assert L.bh_onnx_to_bhm(onnx_path.encode(), str(tmp_path / "refused.bhm").encode()) != 0
    msg = L.bh_last_error().decode()
    for reason in reasons:
        assert reason in msg, msg


# ---- the validator, through the library's host-only loader -------------------------------------------------------------------------
def _load(path):
    """bh_plan_fused_blocks walks a model file on the host: load_model + validate_model; >= 0 = loaded"""
    L = _lib.load()
    rc = L.bh_plan_fused_blocks(path.encode(), 0, None, None, 0)
    return rc, L.bh_last_error().decode()


def _concat_model(two=True, groups=0):
    """stem (32 channels, tensor 1) -> 1x1 to 24 (tensor 2) -> the record under test: channels 8 .. 23 of the stem and channels
    4 .. 11 of tensor 2 (or the stem's window alone) -> head -> pool -> dense"""
    b = synth._Builder(np.random.default_rng(1))
    base = synth.build_model("mini")
    m = copy.deepcopy(base)
    b.chunks, b.off = [np.asarray(base.blob)], base.blob.size
    s, h, w = b.conv(0, 32, 115, 2, 32, 3, 2, mf.ACT_RELU, in_layout=1)
    t = b.pwconv(s, h, w, 32, 24, mf.ACT_RELU)
    t, c = b.concat([(s, 8, 16), (t, 4, 8)] if two else [(s, 8, 16)], h, w, groups)
    t = b.pwconv(t, h, w, c, 16, mf.ACT_RELU)
    t = emb = b.gap(t, h, w, 16)
    b.dense(t, 16, 10)
    m.layers, m.blob, m.n_classes, m.embedding_dim, m.embedding_tensor = b.layers, np.concatenate(b.chunks), 10, 16, emb
    return m


BAD_RECORDS = {
    "offset_of_2": (True, dict(w_off=2), "multiple of 4"),
    "second_offset_of_6": (True, dict(b_off=6), "multiple of 4"),
    "length_of_6": (True, dict(cin=6, cout=14), "multiple of 4"),
    "window_past_the_first_source": (True, dict(w_off=20), "past its source"),
    "window_past_the_second_source": (True, dict(b_off=20), "past its source"),
    "huge_offset": (True, dict(w_off=1 << 62), "past its source"),
    "source_of_another_image": (True, dict(in_h=15, out_h=15), "whole images"),
    "sum_is_not_the_output": (False, dict(cout=24), "sum of its windows"),
    "no_channels_from_the_first_source": (True, dict(cin=0), "sum of its windows"),
    "nothing_from_the_second_source": (True, dict(cin=24), "sum of its windows"),
    "groups_do_not_divide": (True, dict(reserved=5), "does not divide"),
    "more_groups_than_channels": (True, dict(reserved=48), "does not divide"),
    "activation": (True, dict(act=mf.ACT_RELU), "activation"),
    "kernel_3": (True, dict(kh=3), "kernel, stride or padding"),
    "stride_2": (True, dict(sw=2), "kernel, stride or padding"),
    "padding": (True, dict(pad_t=1), "kernel, stride or padding"),
    "output_image_differs": (True, dict(out_w=57), "output image"),
    "first_source_is_the_spectrogram": (True, dict(in_tensor=0), "spectrogram"),
    "second_source_is_the_spectrogram": (True, dict(res_tensor=0), "spectrogram"),
    "planar_layout": (True, dict(in_layout=1), "spectrogram"),
}


def test_a_valid_concat_container_loads(tmp_path):
    path = str(tmp_path / "ok.bhm")
    for two, groups in ((True, 0), (True, 3), (False, 0), (False, 4), (True, 1), (True, 24)):
        m = _concat_model(two, groups)
        mf.write_model(path, m)
        rc, msg = _load(path)
        assert rc >= 0, msg
        back = mf.read_model(path)
        assert back.layers[2] == m.layers[2] and back.layers[2].op == mf.OP_CONCAT == 10
    # op 9 is still unknown, and so is 11
    m.layers[1].op = 9
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and "unknown layer op" in msg, msg
    m.layers[1].op = 11
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and "unknown layer op" in msg, msg


@pytest.mark.parametrize("case", sorted(BAD_RECORDS))
def test_the_validator_refuses_a_bad_concat_record(case, tmp_path):
    two, change, reason = BAD_RECORDS[case]
    m = _concat_model(two)
    for k, v in change.items():
        setattr(m.layers[2], k, v)
    path = str(tmp_path / "bad.bhm")
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc < 0 and reason in msg and "concat" in msg, (rc, msg)


# ---- the planner: a tensor a concat reads counts as read ---------------------------------------------------------------------------
def _triple_model(concat_reads_expand):
    """stem (16) -> 1x1 expand to 64 (tensor 2) -> depthwise 3x3 (3) -> 1x1 project to 16 (4) -> Concat of the project's output with
    16 channels of the expand output, or of the stem -> head"""
    b = synth._Builder(np.random.default_rng(2))
    base = synth.build_model("mini")
    m = copy.deepcopy(base)
    b.chunks, b.off = [np.asarray(base.blob)], base.blob.size
    s, h, w = b.conv(0, 32, 115, 2, 16, 3, 2, mf.ACT_GELU_ERF, in_layout=1)
    e = b.pwconv(s, h, w, 16, 64, mf.ACT_GELU_ERF)
    d, _, _ = b.dwconv(e, h, w, 64, 3, 1, mf.ACT_GELU_ERF)
    p = b.pwconv(d, h, w, 64, 16, mf.ACT_NONE)
    t, c = b.concat([(p, 0, 16), (e, 32, 16) if concat_reads_expand else (s, 0, 16)], h, w)
    t = b.pwconv(t, h, w, c, 16, mf.ACT_GELU_ERF)
    t = emb = b.gap(t, h, w, 16)
    b.dense(t, 16, 10)
    m.layers, m.blob, m.n_classes, m.embedding_dim, m.embedding_tensor = b.layers, np.concatenate(b.chunks), 10, 16, emb
    return m


def test_a_triple_whose_expand_output_a_concat_reads_is_not_fused(tmp_path):
    path = str(tmp_path / "t.bhm")
    mf.write_model(path, _triple_model(False))
    assert _fused_blocks(path) == [1]
    # (the depthwise and the project may still run as a block of their own behind the expand layer, whose tensor then exists)
    mf.write_model(path, _triple_model(True))
    assert 1 not in _fused_blocks(path)
    # ... nor one whose depthwise output a concat reads as its FIRST source
    m = _triple_model(False)
    m.layers[4].in_tensor, m.layers[4].res_tensor, m.layers[4].w_off = 3, 4, 16
    mf.write_model(path, m)
    rc, msg = _load(path)
    assert rc >= 0, msg
    assert _fused_blocks(path) == []


# ---- nothing changes for a model without a concat -----------------------------------------------------------------------------------
def test_the_records_of_mini_are_what_they_were(tmp_path):
    """synth's "mini": its container is, byte for byte, the one the builder wrote before it knew of concats (the digest below was
    taken then), and both readers still turn its graph back into it"""
    m = synth.build_model("mini")
    assert not any(L.op == CAT for L in m.layers)
    path = str(tmp_path / "mini.bhm")
    mf.write_model(path, m)
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == MINI_SHA256
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


MINI_SHA256 = "3018a6a2f9ed0ca55b25047b528a0fb9b50f25fcf132e284482f90cbaace87a1"


# ---- hostile files --------------------------------------------------------------------------------------------------------------------
def test_mutated_multi_branch_files_are_refused_or_read_never_a_crash():
    """tools/fuzz_onnx_reader.py on synth's multi-branch plans alone (FUZZ_BRANCHY: their graphs -- Concat and Slice nodes, the shuffle's
    Reshape / Transpose, int64 constants -- and their containers with OP_CONCAT records), in child processes: every mutant
    returns, read or refused"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_onnx_reader.py"), "300", "7"], capture_output=True, text=True,
                       env=dict(os.environ, FUZZ_BRANCHY="1"), timeout=600)
    assert r.returncode == 0, r.stderr[-600:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("300 mutants, 0 bad batches"), r.stdout[-800:]
    assert "'0':" in last and "'-2':" in last, last
