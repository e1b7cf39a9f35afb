"""Full k x k convolutions past the stem, host side: the residual Add of a Fused-MBConv block folded by both ONNX readers, the
Fused-MBConv stages of the model generator (`birdnet_v30_v2l`, `random_fused_plan`).  No device needed."""
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth

# a quarter-second segment, one mel branch, a stem and then full convolutions: 3x3 stride 1 with the block input added back
# (expand ratio 1), a 3x3 stride 2 expand + 1x1 project, and an MBConv stage behind them
FUSED_PLAN = {"sr": 48000, "n": 12000, "branches": [(512, 100, 32, 0.0, 3000.0)], "stem": 16,
              "stages": [(1, 3, 1, 16, 2, True), (4, 3, 2, 24, 1, True), (4, 3, 2, 32, 1)], "head": 64, "classes": 30,
              "act": mf.ACT_SWISH}


def _native(onnx_path, out_path):
    L = _lib.load()
    rc = L.bh_onnx_to_bhm(onnx_path.encode(), out_path.encode())
    if rc != 0:
        raise RuntimeError(f"rc {rc}: {L.bh_last_error().decode()}")
    return mf.read_model(out_path)


def _weights(m, L):
    nw = {mf.OP_CONV: L.kh * L.kw * L.cin * L.cout, mf.OP_DWCONV: L.kh * L.kw * L.cout, mf.OP_PWCONV: L.cin * L.cout,
          mf.OP_DENSE: L.cin * L.cout}.get(L.op, 0)
    return m.blob[L.w_off:L.w_off + nw].tobytes(), m.blob[L.b_off:L.b_off + (L.cout if nw else 0)].tobytes()


FIELDS = ("op", "act", "in_tensor", "res_tensor", "cin", "cout", "kh", "kw", "sh", "sw", "pad_t", "pad_l", "in_h", "in_w", "out_h",
          "out_w", "in_layout")


def test_both_readers_fold_the_residual_add_of_a_full_convolution(tmp_path):
    """Conv 3x3 -> Swish -> Add(x): one OP_CONV layer with res_tensor set, in the Python reader and the library's, and the two
    containers are the same model (the one the graph was written from)."""
    m = synth.build_model("custom", plan=FUSED_PLAN)
    full = [i for i, L in enumerate(m.layers) if L.op == mf.OP_CONV and L.in_layout == 0]
    assert [m.layers[i].res_tensor != mf.NO_TENSOR for i in full] == [True, True, False]   # both 16 -> 16 blocks add their input
    g = convert.graph_from_model(m, frontend_spelling="stft")     # (an audio-input graph: the library reads its front-end off it)
    assert sum(n.op_type == "Add" for n in g.nodes) >= 2
    data = ox.dump(g)
    onnx_path = str(tmp_path / "fused.onnx")
    with open(onnx_path, "wb") as f:
        f.write(data)
    py = convert.model_from_graph(ox.load(data), m, "spectrogram")
    nat = _native(onnx_path, str(tmp_path / "fused.bhm"))
    for got in (py, nat):
        assert len(got.layers) == len(m.layers)
        for i, (x, y) in enumerate(zip(m.layers, got.layers)):
            for f in FIELDS:
                assert getattr(x, f) == getattr(y, f), (i, f)
            assert _weights(m, x) == _weights(got, y), (i, "weights differ")
    r = py.layers[full[1]]
    assert r.op == mf.OP_CONV and r.res_tensor == full[1] and r.act == mf.ACT_SWISH


def test_an_add_on_the_stem_is_still_refused(tmp_path):
    """The NCHW stem never takes a residual (its kernel has none): an Add onto it is refused by both readers, by name."""
    plan = dict(FUSED_PLAN, stem=4, branches=[(512, 100, 32, 0.0, 3000.0)] * 4, stem_stride=1)
    m = synth.build_model("custom", plan=plan)
    assert m.layers[0].op == mf.OP_CONV and m.layers[0].in_layout == 1 and m.layers[0].cin == m.layers[0].cout == 4
    m.layers[0].res_tensor = 0          # stem(x) + x: the spectrogram and the stem output have the same shape here
    g = convert.graph_from_model(m)
    data = ox.dump(g)
    with pytest.raises(convert.ConvertError, match="no convolution to fold the residual into"):
        convert.model_from_graph(ox.load(data), m)


def test_v2l_has_efficientnetv2_l_census():
    m = synth.build_model("birdnet_v30_v2l")
    assert (m.sample_rate, m.sample_count, m.n_classes, m.embedding_dim, m.output_activation) == (32000, 160000, 11560, 1280, mf.OUT_NONE)
    assert len(m.branches) == 1 and m.branches[0].n_mels == 128
    full = [L for L in m.layers if L.op == mf.OP_CONV and L.in_layout == 0]
    # fused stages: 4 x (3x3 32 -> 32 + x), 7 x 3x3 expand to 4x (first stride 2), 7 more; then 10 + 19 + 25 + 7 MBConv blocks
    assert len(full) == 4 + 7 + 7
    assert sum(L.res_tensor != mf.NO_TENSOR for L in full) == 4
    assert sum(1 for L in m.layers if L.op == mf.OP_DWCONV) == 10 + 19 + 25 + 7
    assert sum(1 for L in m.layers if L.op == mf.OP_SCALE) == 10 + 19 + 25 + 7     # squeeze-excite on the MBConv stages only
    assert all(L.act == mf.ACT_SWISH for L in full)
    nparam = 0
    flops = flops_full = 0
    for L in m.layers:
        px = L.out_h * L.out_w
        nw = {mf.OP_CONV: L.kh * L.kw * L.cin * L.cout, mf.OP_DWCONV: L.kh * L.kw * L.cout, mf.OP_PWCONV: L.cin * L.cout,
              mf.OP_DENSE: L.cin * L.cout}.get(L.op, 0)
        nparam += nw + (L.cout if nw else 0)
        f = 2 * px * nw
        flops += f
        if L.op == mf.OP_CONV:
            flops_full += f
    assert 131e6 < nparam < 133e6, nparam
    assert 31.4e9 < flops < 31.8e9, flops
    assert 12.8e9 < flops_full < 13.0e9, flops_full
    assert any(L.kh == 3 and L.cin == 64 and L.cout == 256 and (L.in_h, L.in_w) == (32, 125) for L in full)


def test_random_fused_plan_is_deterministic_and_leaves_random_plan_alone():
    for seed in range(10):
        for big in (False, True):
            a, b, base = synth.random_fused_plan(seed, big), synth.random_fused_plan(seed, big), synth.random_plan(seed, big)
            assert a == b
            nf = sum(1 for st in a["stages"] if len(st) > 5 and st[5])
            assert 1 <= nf <= 3
            assert all(len(st) == 6 and st[5] for st in a["stages"][:nf])
            assert [tuple(st[:5]) for st in a["stages"]] == [tuple(st) for st in base["stages"]]
            assert {k: v for k, v in a.items() if k != "stages"} == {k: v for k, v in base.items() if k != "stages"}
    m1 = synth.build_model("custom", plan=synth.random_fused_plan(3))
    m2 = synth.build_model("custom", plan=synth.random_fused_plan(3))
    assert m1.blob.tobytes() == m2.blob.tobytes()
    assert any(L.op == mf.OP_CONV and L.in_layout == 0 for L in m1.layers)


def test_five_element_stages_build_what_they_did():
    """A stage tuple without the sixth element (or with it False) is MBConv, as before."""
    plan = dict(FUSED_PLAN, stages=[tuple(st[:5]) for st in FUSED_PLAN["stages"]])
    plan_f = dict(FUSED_PLAN, stages=[tuple(st[:5]) + (False,) for st in FUSED_PLAN["stages"]])
    a, b = synth.build_model("custom", plan=plan), synth.build_model("custom", plan=plan_f)
    assert a.blob.tobytes() == b.blob.tobytes()
    assert not any(L.op == mf.OP_CONV and L.in_layout == 0 for L in a.layers)
