"""Float16 model files (the `fp16` variant the reference's installer picks whenever the inference device is a GPU) through both
readers, on the CPU.

Meaning, stated once: a float16 constant is the exact real number it encodes; Cast between floating types is the identity; the graph
is evaluated in the library's own arithmetic.  The library's C++ reader (csrc/onnx_graph.hpp, onnx_conv.hpp, through bh_onnx_to_bhm)
and the Python witness (birda_amd/onnx_io.py, convert.py) are held to each other by the rule of tests/test_onnx_native.py -- the same
layer table and the same weights, bit for bit -- and to `float32(float16(w))` of the model the file was written from.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_onnx_native import _native, _same_model, _weights  # noqa: E402  (the existing witness rule, not restated)


def _write(path, g):
    with open(path, "wb") as f:
        f.write(ox.dump(g))
    return path


def _rc(tmp_path, g_or_bytes, name):
    L = _lib.load()
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(g_or_bytes if isinstance(g_or_bytes, bytes) else ox.dump(g_or_bytes))
    return L.bh_onnx_to_bhm(p.encode(), (p + ".bhm").encode()), L.bh_last_error().decode()


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# ---- 1. the wire format -------------------------------------------------------------------------------------------------------
def test_every_float16_bit_pattern_round_trips_in_both_spellings(tmp_path):
    """raw_data (2 bytes an element) and int32_data (one bit pattern per entry) give the same array, and all 65 536 bit patterns
    decode to what numpy.float16 says: subnormals, +-0, inf, NaN (payload and sign kept)."""
    bits = np.arange(65536, dtype=np.uint16)
    want = bits.view(np.float16).reshape(256, 256)
    raw = ox._ser_tensor("t", want)
    name, a = ox._parse_tensor(raw)
    assert name == "t" and a.dtype == np.float16 and a.shape == (256, 256) and a.view(np.uint16).tobytes() == bits.tobytes()
    as_ints = (ox._f_varint(1, 256) + ox._f_varint(1, 256) + ox._f_varint(2, ox.FLOAT16) + ox._f_str(8, "t")
               + ox._f_bytes(5, b"".join(ox._enc_varint(int(b)) for b in bits)))
    _, b = ox._parse_tensor(as_ints)
    assert b.dtype == np.float16 and b.view(np.uint16).tobytes() == bits.tobytes()
    # through a whole file, with the element type of a ValueInfo honoured
    g = ox.Graph(nodes=[ox.Node("Identity", ["x"], ["y"])], initializers={"w": want}, inputs=[ox.ValueInfo("x", ox.FLOAT16, ["N", 3])],
                 outputs=[ox.ValueInfo("y", ox.FLOAT, ["N", 3])])
    h = ox.load(ox.dump(g))
    assert h.initializers["w"].view(np.uint16).tobytes() == bits.tobytes() and (h.inputs[0].elem_type, h.outputs[0].elem_type) == (ox.FLOAT16, ox.FLOAT)


def test_the_library_decodes_every_float16_bit_pattern_exactly(tmp_path):
    """The C++ decoder on all 65 536 patterns: a Gemm whose [256, 256] weight holds them (as raw_data and as int32_data) converts to
    a container whose blob carries float32(float16) of each, bit for bit -- NaN payloads included; a non-finite weight is treated as
    a non-finite float32 weight is (validate_model has no rule about weight values)."""
    bits = np.arange(65536, dtype=np.uint16)
    w = bits.view(np.float16).reshape(256, 256)
    want = w.astype(np.float32)

    def graph():
        g = ox.Graph(name="bits", producer="tests")
        g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", 2, 32, 115]))
        g.initializers["w0"] = np.full((256, 2, 3, 3), 0.25, np.float16)
        g.nodes.append(ox.Node("Conv", ["spectrogram", "w0"], ["c0"], {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1]}, name="c0"))
        g.nodes.append(ox.Node("GlobalAveragePool", ["c0"], ["p"]))
        g.nodes.append(ox.Node("Flatten", ["p"], ["f"], {"axis": 1}))
        g.initializers["w1"] = w
        g.nodes.append(ox.Node("MatMul", ["f", "w1"], ["y"]))
        g.outputs.append(ox.ValueInfo("y", ox.FLOAT, ["N", 256]))
        return g
    raw_path = _write(str(tmp_path / "raw.onnx"), graph())
    ser = ox._ser_tensor

    def as_int32_data(name, arr):
        arr = np.asarray(arr)
        if arr.dtype != np.float16:
            return ser(name, arr)
        out = b"".join(ox._f_varint(1, int(d)) for d in arr.shape) + ox._f_varint(2, ox.FLOAT16) + ox._f_str(8, name)
        return out + ox._f_bytes(5, b"".join(ox._enc_varint(int(b)) for b in arr.reshape(-1).view(np.uint16)))
    ox._ser_tensor = as_int32_data
    try:
        int_path = _write(str(tmp_path / "ints.onnx"), graph())
    finally:
        ox._ser_tensor = ser
    assert open(int_path, "rb").read() != open(raw_path, "rb").read()
    for p in (raw_path, int_path):
        assert np.array_equal(ox.load(open(p, "rb").read()).initializers["w1"].view(np.uint16), bits.reshape(256, 256))
        m = _native(p, p + ".bhm")
        L = m.layers[-1]
        got = np.asarray(m.blob[L.w_off:L.w_off + 65536])
        assert got.view(np.uint32).tobytes() == want.reshape(-1).view(np.uint32).tobytes(), p


# ---- 2. whole models through both converters -------------------------------------------------------------------------------------
def _fused_model(seed):
    return synth.build_model("custom", plan=synth.random_fused_plan(seed))


MODELS = {
    "birdnet_v30": lambda: synth.build_model("birdnet_v30"),
    "perch_v2_tiny": lambda: synth.build_model("perch_v2_tiny"),
    "birdnet_v24": lambda: synth.build_model("birdnet_v24", n_classes=600),      # (reduced class count: time)
    "fused0": lambda: _fused_model(0), "fused1": lambda: _fused_model(1), "fused2": lambda: _fused_model(2),
}


def _value_rounded(g, only=None):
    """the float32 graph `g` with its float constants rounded to float16 VALUES (element type unchanged)"""
    h = ox.Graph(list(g.nodes), dict(g.initializers), g.inputs, g.outputs, g.name, g.opset, g.producer)
    for k, a in g.initializers.items():
        if a.dtype == np.float32 and (only is None or k in only):
            h.initializers[k] = _f16(a)
    return h


def _same_layers(a, b):
    """the layer half of test_onnx_native._same_model: same table, same weights bit for bit"""
    for f in ("family", "sample_rate", "sample_count", "n_classes", "embedding_dim", "output_activation", "embedding_tensor", "spec_h", "spec_w"):
        assert getattr(a, f) == getattr(b, f), f
    assert len(a.layers) == len(b.layers)
    for i, (x, y) in enumerate(zip(a.layers, b.layers)):
        for f in ("op", "act", "in_tensor", "res_tensor", "cin", "cout", "kh", "kw", "sh", "sw", "pad_t", "pad_l", "in_h", "in_w", "out_h", "out_w", "in_layout"):
            assert getattr(x, f) == getattr(y, f), (i, f)
        (wa, ba), (wb, bb) = _weights(a, x), _weights(b, y)
        assert wa.tobytes() == wb.tobytes() and ba.tobytes() == bb.tobytes(), (i, "weights differ")


def _check_float16_file(tmp_path, m, frontend_spelling, form, folded_bn=()):
    g32 = convert.graph_from_model(m, frontend_spelling=frontend_spelling)
    g16 = convert.graph_to_float16(g32, frontend=form)
    casts = [n for n in g16.nodes if n.op_type == "Cast"]
    assert [v.elem_type for v in g16.inputs + g16.outputs] == [ox.FLOAT] * (len(g16.inputs) + len(g16.outputs))
    assert casts[0].inputs == [g16.inputs[0].name] and casts[0].attrs["to"] == ox.FLOAT16
    assert casts[-1].outputs == [g16.outputs[0].name] and casts[-1].attrs["to"] == ox.FLOAT
    kept32 = {k for k, a in g16.initializers.items() if a.dtype == np.float32}
    if frontend_spelling and form == "f32":
        assert kept32 and all(k.startswith("fe") for k in kept32) and len(casts) == 4
    else:
        assert not kept32 and len(casts) == 2
    data = ox.dump(g16)
    path = str(tmp_path / "m16.onnx")
    with open(path, "wb") as f:
        f.write(data)
    got = _native(path, str(tmp_path / "m16.bhm"))
    want = convert.model_from_graph(ox.load(data), m, "spectrogram" if frontend_spelling else None)
    if frontend_spelling and form == "f16":
        # the front-end of this file is NOT the manifest's (norm_eps 1e-6 is 1.0133e-6 in float16, the DFT rows are rounded): the
        # manifest-fed Python witness is held to the layer table and weights here, the front-end to its float32 twin below
        _same_layers(want, got)
    else:
        _same_model(want, got, frontend_exact=frontend_spelling is None)
    if frontend_spelling is None:      # nothing fitted anywhere: the two containers are the same bytes
        mf.write_model(str(tmp_path / "py16.bhm"), want)
        assert open(str(tmp_path / "py16.bhm"), "rb").read() == open(str(tmp_path / "m16.bhm"), "rb").read()
    # ... the layer table the float32 file of the same model gives (activations, residuals, gates in place)
    as32 = convert.model_from_graph(ox.load(ox.dump(g32)), m, "spectrogram" if frontend_spelling else None)
    assert [(L.op, L.act, L.res_tensor) for L in got.layers] == [(L.op, L.act, L.res_tensor) for L in as32.layers]
    assert got.output_activation == as32.output_activation and len(got.layers) == len(m.layers)
    for i, (a, b) in enumerate(zip(m.layers, got.layers)):
        if i in folded_bn:
            continue
        (wa, ba), (wb, bb) = _weights(m, a), _weights(got, b)
        assert np.array_equal(_f16(wa), wb) and np.array_equal(_f16(ba), bb), (i, "weights are not float32(float16(w32))")
    if frontend_spelling:
        # the recovered operator is the file's own, rounding included: the same records as the float32 graph whose front-end
        # constants were rounded in value only (none of them, with the front-end kept in float32)
        fe = {k for k in g32.initializers if k.startswith("fe")}
        ref = _native(_write(str(tmp_path / "ref32.onnx"), _value_rounded(g32, fe if form == "f16" else set())), str(tmp_path / "ref32.bhm"))
        assert np.float32(ref.norm_eps) == np.float32(got.norm_eps) and len(ref.branches) == len(got.branches) == len(m.branches)
        for x, y in zip(ref.branches, got.branches):
            for f in ("frame_length", "frame_step", "n_mels", "n_frames", "flags"):
                assert getattr(x, f) == getattr(y, f), f
            for f in ("fmin", "fmax", "mag_scale", "out_scale", "out_shift"):
                assert np.float32(getattr(x, f)) == np.float32(getattr(y, f)), f
            n = x.n_bins * x.n_mels
            assert ref.blob[x.mel_w_off:x.mel_w_off + n].tobytes() == got.blob[y.mel_w_off:y.mel_w_off + n].tobytes()
    return got


@pytest.mark.parametrize("form", ["f16", "f32"])
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_float16_files_convert_alike_in_both_readers(tmp_path, kind, form):
    """graph_to_float16 of each model's audio-input graph (the DFT spelled as a Conv1d, as the published file's), both `frontend`
    forms, through bh_onnx_to_bhm AND convert.model_from_graph: the same layer table and weights bit for bit, every layer's weights
    float32(float16(w32)) exactly, the front-end read off the float16 constants as off the same constants in float32."""
    _check_float16_file(tmp_path, MODELS[kind](), "conv1d", form)


@pytest.mark.parametrize("kind", ["birdnet_v30", "mini_se"])
def test_float16_files_that_start_at_the_spectrogram_give_the_same_container_bytes(tmp_path, kind):
    """(a graph that starts at the spectrogram takes its front-end from the family table in both readers: nothing is fitted, and
    the two containers are the same bytes)"""
    _check_float16_file(tmp_path, synth.build_model(kind), None, "f16")


@pytest.mark.parametrize("form", ["f16", "f32"])
@pytest.mark.parametrize("spelling", ["conv1d", "stft"])
def test_python_front_end_recovery_reads_a_float16_file_like_the_library(tmp_path, spelling, form):
    """convert.model_from_graph WITHOUT a manifest (the route of convert_file / tools/onnx_to_bhm.py --sample-rate): the front-end
    is read off the float16 graph by frontend_recover.py, the second witness of onnx_frontend.hpp -- the same branch records as
    the library's, at the bounds tests/test_onnx_frontend.py holds the two recoveries to on float32 files; the layers bit for bit."""
    m = synth.build_model("mini")
    g16 = convert.graph_to_float16(convert.graph_from_model(m, frontend_spelling=spelling), frontend=form)
    data = ox.dump(g16)
    path = str(tmp_path / "fe16.onnx")
    with open(path, "wb") as f:
        f.write(data)
    lib = _native(path, str(tmp_path / "fe16.bhm"))
    py = convert.model_from_graph(ox.load(data), None, sample_rate=m.sample_rate)
    _same_layers(py, lib)
    assert lib.norm_eps == pytest.approx(py.norm_eps, rel=1e-6)
    # the file's own epsilon: float16(1e-6) = 1.0133e-6 where the front-end constants are float16
    assert lib.norm_eps == pytest.approx(float(np.float16(m.norm_eps)) if form == "f16" else m.norm_eps, rel=1e-5)
    assert len(py.branches) == len(lib.branches) == len(m.branches)
    for a, b in zip(py.branches, lib.branches):
        assert (a.frame_length, a.frame_step, a.n_frames, a.n_mels, a.flags) == (b.frame_length, b.frame_step, b.n_frames, b.n_mels, b.flags)
        assert np.float32(a.mag_scale) == pytest.approx(np.float32(b.mag_scale), abs=1e-6) and a.out_scale == pytest.approx(b.out_scale, rel=1e-6)
        assert a.out_shift == pytest.approx(b.out_shift, rel=1e-6)
        n = a.n_bins * a.n_mels
        assert np.abs(np.asarray(py.blob[a.mel_w_off:a.mel_w_off + n]) - np.asarray(lib.blob[b.mel_w_off:b.mel_w_off + n])).max() < 1e-6


def _unfold_bn(g, rng, which):
    """BatchNormalization nodes behind the `which`-th convolutions (parameters of the graph's own element type, float32 here)"""
    convs = [n for n in g.nodes if n.op_type == "Conv" and not n.name.startswith("fe")]
    for q in which:
        conv = convs[q]
        cout = g.initializers[conv.inputs[1]].shape[0]
        names = []
        for k, v in (("g", rng.uniform(0.5, 1.5, cout)), ("b", rng.normal(0, 0.1, cout)), ("m", rng.normal(0, 0.1, cout)), ("v", rng.uniform(0.5, 2.0, cout))):
            g.initializers[f"bn{q}_{k}"] = v.astype(np.float32)
            names.append(f"bn{q}_{k}")
        i = g.nodes.index(conv)
        old = conv.outputs[0]
        conv.outputs[0] = old + "_prebn"
        g.nodes.insert(i + 1, ox.Node("BatchNormalization", [conv.outputs[0]] + names, [old], {"epsilon": 1e-3}, name=f"bn{q}"))


@pytest.mark.parametrize("form", ["f16", "f32"])
def test_float16_file_with_unfolded_batchnorm(tmp_path, form):
    """BatchNormalization left in the graph, its parameters float16 like everything else: folded in float64 from the exact values
    by both readers alike (weights bit for bit); the layers without one still carry float32(float16(w32))."""
    m = synth.build_model("mini_se")
    g32 = convert.graph_from_model(m, frontend_spelling="conv1d")
    _unfold_bn(g32, np.random.default_rng(5), (0, 2, 3))
    g16 = convert.graph_to_float16(g32, frontend=form)
    assert sum(n.op_type == "BatchNormalization" for n in g16.nodes) == 3 and g16.initializers["bn2_g"].dtype == np.float16
    data = ox.dump(g16)
    path = str(tmp_path / "bn16.onnx")
    with open(path, "wb") as f:
        f.write(data)
    got = _native(path, str(tmp_path / "bn16.bhm"))
    want = convert.model_from_graph(ox.load(data), m, "spectrogram")
    (_same_layers if form == "f16" else lambda a, b: _same_model(a, b, frontend_exact=False))(want, got)
    conv_layers = [i for i, L in enumerate(m.layers) if L.op in (mf.OP_CONV, mf.OP_DWCONV, mf.OP_PWCONV)]
    folded = {conv_layers[q] for q in (0, 2, 3)}
    n_off = 0
    for i, (a, b) in enumerate(zip(m.layers, got.layers)):
        (wa, ba), (wb, bb) = _weights(m, a), _weights(got, b)
        if i in folded:
            # float64 restatement of the fold from the float16 values
            q = (0, 2, 3)[sorted(folded).index(i)]
            gm, bt, mu, var = (g16.initializers[f"bn{q}_{k}"].astype(np.float64) for k in "gbmv")
            scale = gm / np.sqrt(var + float(np.float32(1e-3)))
            assert np.array_equal(wb.reshape(-1, a.cout), _f16(wa).reshape(-1, a.cout) * scale.astype(np.float32))
            assert np.array_equal(bb, ((_f16(ba).astype(np.float64) - mu) * scale + bt).astype(np.float32))
            n_off += int(not np.array_equal(_f16(wb), wb))
        else:
            assert np.array_equal(_f16(wa), wb) and np.array_equal(_f16(ba), bb), i
    assert n_off == 3          # a folded layer's weights are no longer float16 values


def test_a_cast_between_a_convolution_and_its_swish_does_not_break_the_fold(tmp_path):
    """Casts in the middle of the conv stack (float16 -> float32 -> float16 round a Sigmoid, as a mixed-precision exporter leaves
    them; a chain of two): the sole-consumer / pattern logic sees through them in both readers."""
    m = synth.build_model("mini_se")
    g = convert.graph_to_float16(convert.graph_from_model(m))
    k = next(i for i, n in enumerate(g.nodes) if n.op_type == "Sigmoid" and g.nodes[i + 1].op_type == "Mul")
    sig, mul = g.nodes[k], g.nodes[k + 1]
    x = sig.inputs[0]
    g.nodes[k:k + 2] = [ox.Node("Cast", [x], [x + "_c32"], {"to": ox.FLOAT}), ox.Node("Cast", [x + "_c32"], [x + "_c64"], {"to": ox.DOUBLE}),
                        ox.Node("Sigmoid", [x + "_c64"], [sig.outputs[0] + "_c"]), ox.Node("Cast", [sig.outputs[0] + "_c"], [sig.outputs[0]], {"to": ox.FLOAT16}),
                        mul]
    data = ox.dump(g)
    path = str(tmp_path / "casts.onnx")
    with open(path, "wb") as f:
        f.write(data)
    got = _native(path, str(tmp_path / "casts.bhm"))
    _same_model(convert.model_from_graph(ox.load(data), m), got)
    assert [(L.op, L.act, L.res_tensor) for L in got.layers] == [(L.op, L.act, L.res_tensor) for L in m.layers]


# ---- 3. an independent float64 reading ---------------------------------------------------------------------------------------
def test_hand_written_float16_graph_matches_an_independent_float64_evaluation(tmp_path):
    """What tests/test_convert.py does for the float32 route, for a float16 file: a graph written node by node here (stem, depthwise,
    residual 1x1, full 3x3 convolution with a residual, ReduceMean, MatMul + Add, Gemm; ReLU6 / swish / ReLU), converted by
    graph_to_float16, restated in torch float64 with the weights taken as float64(float16(w)), against the oracle on the container
    the library's reader writes, at that test's own 2e-5 max(1, max |want|)."""
    import torch
    import torch.nn.functional as F
    from oracle import oracle as O
    rng = np.random.default_rng(321)
    base = synth.build_model("mini")
    C0, H, W = len(base.branches), base.spec_h, base.spec_w
    g = ox.Graph(name="hand_written_f16", producer="tests")
    g.inputs.append(ox.ValueInfo("spectrogram", ox.FLOAT, ["N", C0, H, W]))
    P = {}

    def init(name, arr):
        g.initializers[name] = np.asarray(arr, np.float32)
        P[name] = torch.from_numpy(_f16(arr).astype(np.float64))
        return name
    oh, ow = -(-H // 2), -(-W // 2)
    ph, pw = max((oh - 1) * 2 + 3 - H, 0), max((ow - 1) * 2 + 3 - W, 0)
    pads = [ph // 2, pw // 2, ph - ph // 2, pw - pw // 2]
    init("w0", rng.normal(0, 0.3, (8, C0, 3, 3))); init("b0", rng.normal(0, 0.1, 8))
    g.nodes.append(ox.Node("Conv", ["spectrogram", "w0", "b0"], ["c0"], {"kernel_shape": [3, 3], "strides": [2, 2], "pads": pads}, name="c0"))
    g.nodes.append(ox.Node("Clip", ["c0", init("lo", 0.0), init("hi", 6.0)], ["a0"]))
    init("w1", rng.normal(0, 0.4, (8, 1, 3, 3))); init("b1", rng.normal(0, 0.1, 8))
    g.nodes.append(ox.Node("Conv", ["a0", "w1", "b1"], ["c1"], {"kernel_shape": [3, 3], "pads": [1, 1, 1, 1], "group": 8}, name="c1"))
    g.nodes.append(ox.Node("Sigmoid", ["c1"], ["s1"]))
    g.nodes.append(ox.Node("Mul", ["c1", "s1"], ["a1"]))
    init("w2", rng.normal(0, 0.3, (8, 8, 1, 1))); init("b2", rng.normal(0, 0.1, 8))
    g.nodes.append(ox.Node("Conv", ["a1", "w2", "b2"], ["c2"], {"kernel_shape": [1, 1]}, name="c2"))
    g.nodes.append(ox.Node("Add", ["c2", "a0"], ["r2"]))
    init("w3", rng.normal(0, 0.12, (8, 8, 3, 3))); init("b3", rng.normal(0, 0.1, 8))
    g.nodes.append(ox.Node("Conv", ["r2", "w3", "b3"], ["c3"], {"kernel_shape": [3, 3], "pads": [1, 1, 1, 1]}, name="c3"))
    g.nodes.append(ox.Node("Sigmoid", ["c3"], ["s3"]))
    g.nodes.append(ox.Node("Mul", ["c3", "s3"], ["a3"]))
    g.nodes.append(ox.Node("Add", ["a3", "r2"], ["r3"]))
    init("w4", rng.normal(0, 0.3, (16, 8, 1, 1))); init("b4", rng.normal(0, 0.1, 16))
    g.nodes.append(ox.Node("Conv", ["r3", "w4", "b4"], ["c4"], {"kernel_shape": [1, 1]}, name="c4"))
    g.nodes.append(ox.Node("Relu", ["c4"], ["a4"]))
    g.nodes.append(ox.Node("ReduceMean", ["a4"], ["p4"], {"axes": [2, 3], "keepdims": 1}))
    g.nodes.append(ox.Node("Flatten", ["p4"], ["f4"], {"axis": 1}))
    init("w5", rng.normal(0, 0.3, (16, 12))); init("b5", rng.normal(0, 0.1, 12))
    g.nodes.append(ox.Node("MatMul", ["f4", "w5"], ["m5"]))
    g.nodes.append(ox.Node("Add", ["m5", "b5"], ["d5"]))
    g.nodes.append(ox.Node("Relu", ["d5"], ["a5"]))
    init("w6", rng.normal(0, 0.5, (7, 12))); init("b6", rng.normal(0, 0.1, 7))
    g.nodes.append(ox.Node("Gemm", ["a5", "w6", "b6"], ["logits"], {"transB": 1}))
    g.outputs.append(ox.ValueInfo("logits", ox.FLOAT, ["N", 7]))

    g16 = convert.graph_to_float16(g)
    assert all(a.dtype == np.float16 for a in g16.initializers.values())
    path = _write(str(tmp_path / "hand16.onnx"), g16)
    m = _native(path, str(tmp_path / "hand16.bhm"))
    assert [L.op for L in m.layers] == [mf.OP_CONV, mf.OP_DWCONV, mf.OP_PWCONV, mf.OP_CONV, mf.OP_PWCONV, mf.OP_GAP, mf.OP_DENSE, mf.OP_DENSE]
    assert [L.act for L in m.layers[:5]] == [mf.ACT_RELU6, mf.ACT_SWISH, mf.ACT_NONE, mf.ACT_SWISH, mf.ACT_RELU]
    assert (m.layers[2].res_tensor, m.layers[3].res_tensor) == (1, 3)
    _same_model(convert.model_from_graph(ox.load(open(path, "rb").read()), base), m)     # (family-table front-end: bit for bit)
    pa = str(tmp_path / "base.bhm")
    mf.write_model(pa, base)
    segs = synth.synth_segments(3, base.sample_count, base.sample_rate, start=11)
    _, spec = O.OracleModel(pa).forward(segs, dump_tensor=0)
    xs = torch.from_numpy(spec.reshape(3, C0, H, W).astype(np.float64))
    a0 = torch.clamp(F.conv2d(F.pad(xs, (pads[1], pads[3], pads[0], pads[2])), P["w0"], P["b0"], stride=2), 0.0, 6.0)
    y = F.conv2d(a0, P["w1"], P["b1"], padding=1, groups=8)
    r2 = F.conv2d(y * torch.sigmoid(y), P["w2"], P["b2"]) + a0
    y = F.conv2d(r2, P["w3"], P["b3"], padding=1)
    r3 = y * torch.sigmoid(y) + r2
    f4 = F.relu(F.conv2d(r3, P["w4"], P["b4"])).mean((2, 3))
    want = (F.relu(f4 @ P["w5"] + P["b5"]) @ P["w6"].T + P["b6"]).numpy()
    got = O.OracleModel(str(tmp_path / "hand16.bhm")).forward(segs)
    err = float(np.abs(got - want).max())
    print(f"float16 hand-written graph: max |oracle - float64| = {err:.3e}, max |want| = {float(np.abs(want).max()):.3f}")
    assert err <= 2e-5 * max(1.0, float(np.abs(want).max())), err


@pytest.mark.parametrize("spell", ["div", "mul"])
def test_erf_gelu_constants_of_a_float16_file(tmp_path, spell):
    """f16(sqrt 2) = 1.4140625 and f16(1 / sqrt 2) = 0.70703125 from a float16 tensor are the erf-GELU spelling (compared exactly,
    no wider window); 1.4130 is not; the same constants in a float32 tensor keep today's behaviour (1.5e-4 from sqrt 2: outside the
    1e-4 window, not recognised; sqrt 2 itself recognised)."""
    L = _lib.load()
    m = synth.build_model("mini")
    assert any(Lr.act == mf.ACT_GELU_ERF for Lr in m.layers)

    def graph(const, dtype):
        g = convert.graph_from_model(m)
        if dtype == np.float16:
            g = convert.graph_to_float16(g)
        for n in g.nodes:
            if n.op_type == "Div" and n.inputs[1].endswith("_sqrt2"):
                if spell == "mul":
                    n.op_type = "Mul"
                g.initializers[n.inputs[1]] = np.asarray(const, dtype).reshape(())
        return g

    def outcome(const, dtype, name):
        g = graph(const, dtype)
        data = ox.dump(g)
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        rc, msg = L.bh_onnx_to_bhm(p.encode(), (p + ".bhm").encode()), L.bh_last_error().decode()
        try:
            py = convert.model_from_graph(ox.load(data), m)
        except convert.ConvertError as e:
            py = e
        if rc == 0:
            got = mf.read_model(p + ".bhm")
            assert not isinstance(py, Exception)
            assert [Lr.act for Lr in got.layers] == [Lr.act for Lr in m.layers] == [Lr.act for Lr in py.layers]
            return True
        assert rc == -2 and isinstance(py, convert.ConvertError), (rc, msg, py)
        return False
    exact = np.sqrt(2.0) if spell == "div" else 1.0 / np.sqrt(2.0)
    r16 = float(np.float16(exact))
    assert r16 == (1.4140625 if spell == "div" else 0.70703125)
    assert outcome(r16, np.float16, "f16_ok.onnx")
    off = 1.4130 if spell == "div" else 1.0 / 1.4130
    assert float(np.float16(off)) != r16 and abs(float(np.float16(off)) - exact) > 1e-4
    assert not outcome(off, np.float16, "f16_off.onnx")
    assert not outcome(float(np.nextafter(np.float16(r16), np.float16(2.0))), np.float16, "f16_next.onnx")     # one float16 ulp beside it
    assert outcome(exact, np.float32, "f32_ok.onnx")
    # (today's float32 rule, unchanged: within 1e-4 of the exact value.  1.4140625 is 1.5e-4 from sqrt 2 -- outside; 0.70703125 is
    # 7.6e-5 from 1 / sqrt 2 -- inside)
    assert outcome(r16, np.float32, "f32_rounded.onnx") == (abs(r16 - exact) < 1e-4) == (spell == "mul")


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause(tmp_path):
    m = synth.build_model("mini")

    def both(g, what, name, py_error=(convert.ConvertError, ValueError)):
        data = g if isinstance(g, bytes) else ox.dump(g)
        rc, msg = _rc(tmp_path, data, name)
        assert rc == -2 and what in msg, (name, rc, msg)
        with pytest.raises(py_error, match=what):
            convert.model_from_graph(ox.load(data), m)

    # a float16 graph input (the C ABI feeds float32; rounding the audio to 11 bits is not done silently), and output
    g = convert.graph_to_float16(convert.graph_from_model(m))
    g.inputs[0] = ox.ValueInfo(g.inputs[0].name, ox.FLOAT16, g.inputs[0].shape)
    both(g, "is float16", "in16.onnx")
    g = convert.graph_to_float16(convert.graph_from_model(m))
    g.outputs[0] = ox.ValueInfo(g.outputs[0].name, ox.FLOAT16, g.outputs[0].shape)
    both(g, "is float16", "out16.onnx")
    # Cast to int8 on the path
    g = convert.graph_to_float16(convert.graph_from_model(m))
    next(n for n in g.nodes if n.op_type == "Cast").attrs["to"] = 3
    both(g, "int8", "cast8.onnx")
    # raw_data of odd size / an int32_data entry above 0xFFFF / a bfloat16 initializer where a weight is expected
    ser = ox._ser_tensor
    g = convert.graph_to_float16(convert.graph_from_model(m))
    wname = next(n for n in g.nodes if n.op_type == "Conv").inputs[1]

    def dumped(tensor_bytes):
        def patched(name, arr):
            return tensor_bytes(name, np.asarray(arr)) if name == wname else ser(name, arr)
        ox._ser_tensor = patched
        try:
            return ox.dump(g)
        finally:
            ox._ser_tensor = ser

    def header(name, arr, dtype):
        return b"".join(ox._f_varint(1, int(d)) for d in arr.shape) + ox._f_varint(2, dtype) + ox._f_str(8, name)
    both(dumped(lambda n, a: header(n, a, ox.FLOAT16) + ox._f_bytes(9, a.tobytes()[:-1])), "raw_data size", "odd.onnx")
    both(dumped(lambda n, a: header(n, a, ox.FLOAT16) + ox._f_bytes(5, b"".join(ox._enc_varint(0x10000 if i == 5 else int(b))
                                                                               for i, b in enumerate(a.reshape(-1).view(np.uint16))))),
         "above 0xFFFF", "big.onnx")
    both(dumped(lambda n, a: header(n, a, ox.BFLOAT16) + ox._f_bytes(9, a.tobytes())), "bfloat16", "bf16.onnx")


def test_mutated_float16_files_are_refused_or_read_never_a_crash():
    """tests/test_reader_fuzz.py's loop and budget on float16 seed files (tools/fuzz_onnx_reader.py with FUZZ_F16=1: the same four
    front-end spellings, converted by graph_to_float16 in both forms)."""
    env = dict(os.environ, FUZZ_F16="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_onnx_reader.py"), "240", "3"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-600:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("240 mutants, 0 bad batches"), r.stdout[-800:]
    assert "'0':" in last and "'-2':" in last, last


# ---- 5. which weight matrices run two-term products (host only) -----------------------------------------------------------------
def test_two_term_eligibility_is_read_off_the_values():
    """bh_debug_w16_two_terms, the answer of the routine that builds the operand planes at create: a matrix of f16 values
    qualifies; one weight off by one float32 ulp does not; a matrix whose largest weight forces a power-of-two pre-scale that pushes
    its smallest f16 value below the f16 subnormal grid does not.  The rule reads values, not the file's element type."""
    import ctypes as C
    L = _lib.load()
    rng = np.random.default_rng(17)

    def two_terms(W):
        W = np.ascontiguousarray(W, np.float32)
        rc = L.bh_debug_w16_two_terms(W.ctypes.data_as(C.c_void_p), W.shape[0], W.shape[1])
        assert rc in (0, 1), (rc, L.bh_last_error())
        return bool(rc)
    W32 = (rng.standard_normal((96, 40)) * np.sqrt(2.0 / 96)).astype(np.float32)
    W = _f16(W32)
    assert not two_terms(W32) and two_terms(W)
    assert two_terms(np.zeros((32, 16), np.float32)) and two_terms(-W)
    off = W.copy()
    off[37, 11] = np.nextafter(off[37, 11], np.float32(4.0))           # one float32 ulp
    assert not two_terms(off)
    # f16 subnormals qualify as long as the pre-scale lifts them (the largest weight below 2^14: the scale is >= 1) ...
    small = W.copy()
    small[5, 3] = np.float32(3 * 2.0 ** -24)
    assert float(np.float16(small[5, 3])) == float(small[5, 3]) and two_terms(small)
    # ... and not once a large weight turns the pre-scale into a division: 40 000 -> scale 2^-2, and 3 * 2^-24 is no longer on
    # the grid (the planes would hold 2^-24 for it, with the rest in the lo plane)
    # (on weights of a known range, 0.25 .. 1, so that the one small weight is what decides)
    big = _f16(rng.uniform(0.25, 1.0, (96, 40)) * rng.choice([-1.0, 1.0], (96, 40)))
    big[5, 3] = np.float32(3 * 2.0 ** -24)
    assert two_terms(big)
    big[0, 0] = np.float32(40000.0)
    assert float(np.float16(big[0, 0])) == 40000.0 and not two_terms(big)
    big[5, 3] = np.float32(4 * 2.0 ** -24)                             # a multiple of 4 x 2^-24 survives the same pre-scale
    assert two_terms(big)
