"""MobileNetV3's activations, hard swish (mf.ACT_HSWISH = 7) and hard sigmoid (mf.ACT_HSIGMOID = 8), on the CPU side: the file
format, both ONNX readers and the synthetic models.

    hswish(x) = x min(max(x + 3, 0), 6) / 6            hsigmoid(x) = min(max(x / 6 + 1/2, 0), 1)

* every spelling -- the HardSwish operator, HardSigmoid(alpha 1/6, beta 1/2) * x, and the decomposed chain Add(x, 3) -> Clip(0, 6)
  -> Mul(., x) -> Mul(., 1/6) in either operand order, with the scaling first, with Div(., 6), with float16 constants and with a
  Cast inside the fold; the gate as HardSigmoid and as the chain without the Mul(., x) -- is read by the library's reader
  (bh_onnx_to_bhm) and by convert.py into the same container, which is the model that was written (act == 7 / 8 where it put them);
* the refusals, by message, in both readers: HardSigmoid with the ONNX default alpha = 0.2 (Keras's function), a HardSigmoid inside
  the graph that is neither . * x nor a gate, a decomposed chain whose inner tensor has a second reader (it does not fold, and the
  bare Add is then refused by the rule it met before), HardSwish straight after a Concat record;
* a file with Clip(0, 6), Sigmoid * x and a residual Add (tests/test_convert.py's hand-written graph) reads to the records it read
  before;
* codes 7 and 8 round-trip through modelfile.py, and the library's loader takes the file;
* the gate's clamp: written as comparisons a NaN stays a NaN, written with fmin / fmax it becomes 0 -- evaluated in numpy, the
  reason tests/test_hardswish_gpu.py's NaN case can fail at all;
* forward64h, the float64 forward the GPU tests hold the logits to (tests/test_resact.py's layer walk with the two functions, the
  squeeze-excite scale included), against a torch float64 composition of one block.

* the fused block kernel's fourth family: bh_mb_config_families() == 4, bh_mb_config_name still ends at 3 n_base, the _ex form names
  4 n_base entries, family 3 is family 0's list with the ACT field changed, bh_debug_mbconv_plan with act = 7 answers indices of
  [3 n_base, 4 n_base) on every case of tests/test_mbconv_block.py's catalogue and what it answered before for acts 2 / 3 / 4, and
  the planner fuses every hard-swish block of the synthetic models on a family-3 entry."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O
from test_onnx_native import _same_model
from test_resact import AFTER, GEMM_OPS, layer64

HSWISH, HSIGMOID = 7, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
def hswish64(x):
    x = np.asarray(x, np.float64)
    return x * np.minimum(np.maximum(x + 3.0, 0.0), 6.0) / 6.0


def hsigmoid64(x):
    x = np.asarray(x, np.float64)
    return np.minimum(np.maximum(x / 6.0 + 0.5, 0.0), 1.0)


def act64h(v, act):
    """oracle.act64 with the two codes the plain-C oracle does not know"""
    return hswish64(v) if act == HSWISH else hsigmoid64(v) if act == HSIGMOID else O.act64(v, act)


def layer64h(m, L, X, R):
    """tests/test_resact.py's layer64 (the linear part: the record with its activation taken off), the activation where the record
    puts it -- act(conv + b) + R, or act(conv + b + R) -- and OP_SCALE: the feature map times its [n][C] gate"""
    if L.op == mf.OP_SCALE:
        n = X.shape[0]
        return X.reshape(n, L.out_h, L.out_w, L.cout) * np.asarray(R, np.float64).reshape(n, 1, 1, L.cout)
    after = L.op in GEMM_OPS and L.reserved == AFTER
    lin = dataclasses.replace(L, act=mf.ACT_NONE, reserved=0 if L.op in GEMM_OPS else L.reserved)
    pre = layer64(m, lin, X, None)
    if R is None:
        return act64h(pre, L.act)
    r = np.asarray(R, np.float64).reshape(pre.shape)
    return act64h(pre + r, L.act) if after else act64h(pre, L.act) + r


def forward64h(m, segs, tensors=False):
    spec, _ = O.frontend64(m, segs)
    T = [spec]
    for L in m.layers:
        T.append(layer64h(m, L, T[L.in_tensor], None if L.res_tensor == mf.NO_TENSOR else T[L.res_tensor]))
    return T if tensors else T[-1].reshape(segs.shape[0], -1)


def test_the_two_functions_at_their_corners():
    x = np.array([-np.inf, -7.5, -3.0, -1.5, 0.0, 1.5, 3.0, 7.5])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(hswish64(x)[1:], [0.0, 0.0, -0.375, 0.0, 1.125, 3.0, 7.5]) and np.isnan(hswish64(x)[0])
    assert np.array_equal(hsigmoid64(x), [0.0, 0.0, 0.0, 0.25, 0.5, 0.75, 1.0, 1.0])
    assert hswish64(np.inf) == np.inf
    # the slopes the GPU tolerances carry: max |hswish'| = 1.5 (at +-3 from inside), hsigmoid' = 1/6
    t = np.linspace(-3, 3, 6001)
    assert np.max(np.abs(np.diff(hswish64(t)) / np.diff(t))) <= 1.5 and np.max(np.abs(np.diff(hsigmoid64(t)) / np.diff(t))) <= 1 / 6 + 1e-12


def test_forward64h_is_the_torch_float64_composition():
    import torch
    import torch.nn.functional as F
    plan = synth.random_mnv3_plan(1)
    assert plan["se"]
    m = synth.build_model("mnv3_plan", plan=plan)
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=3)
    T = forward64h(m, segs, tensors=True)
    # the second block (expand -> depthwise -> gate -> project): layers 3 .. 9 behind the stem and the no-expand block
    i0 = next(i for i, L in enumerate(m.layers) if L.op == mf.OP_PWCONV and L.act == HSWISH)
    E, D, Gp, G1, G2, S, P = m.layers[i0:i0 + 7]
    assert [L.op for L in (E, D, Gp, G1, G2, S, P)] == [mf.OP_PWCONV, mf.OP_DWCONV, mf.OP_GAP, mf.OP_PWCONV, mf.OP_PWCONV, mf.OP_SCALE, mf.OP_PWCONV]
    assert (D.act, G1.act, G2.act) == (HSWISH, mf.ACT_RELU, HSIGMOID)
    w = lambda L, k: torch.from_numpy(np.asarray(m.blob[L.w_off:L.w_off + k], np.float64))
    b = lambda L: torch.from_numpy(np.asarray(m.blob[L.b_off:L.b_off + L.cout], np.float64))
    hs = lambda v: v * torch.clamp(v + 3, 0, 6) / 6
    x = torch.from_numpy(T[E.in_tensor]).permute(0, 3, 1, 2)
    e = hs(F.conv2d(x, w(E, E.cin * E.cout).reshape(E.cin, E.cout).T[:, :, None, None], b(E)))
    pb, pr = (D.out_h - 1) * D.sh + D.kh - D.in_h - D.pad_t, (D.out_w - 1) * D.sw + D.kw - D.in_w - D.pad_l
    d = hs(F.conv2d(F.pad(e, (D.pad_l, max(pr, 0), D.pad_t, max(pb, 0))), w(D, D.kh * D.kw * D.cout).reshape(D.kh, D.kw, D.cout).permute(2, 0, 1)[:, None],
                    b(D), stride=D.sh, groups=D.cout))
    g = d.mean(dim=(2, 3))
    g = torch.relu(g @ w(G1, G1.cin * G1.cout).reshape(G1.cin, G1.cout) + b(G1))
    g = torch.clamp((g @ w(G2, G2.cin * G2.cout).reshape(G2.cin, G2.cout) + b(G2)) / 6 + 0.5, 0, 1)
    y = F.conv2d(d * g[:, :, None, None], w(P, P.cin * P.cout).reshape(P.cin, P.cout).T[:, :, None, None], b(P))
    if P.res_tensor != mf.NO_TENSOR:
        y = y + torch.from_numpy(T[P.res_tensor]).permute(0, 3, 1, 2)
    want = y.permute(0, 2, 3, 1).numpy()
    assert np.abs(T[i0 + 7] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


# ---- the gate's clamp keeps a NaN ---------------------------------------------------------------------------------------------------
def test_a_clamp_of_comparisons_keeps_a_nan_and_fmin_fmax_do_not():
    """kernels.hpp bh_hsigmoid_keep_nan against the fminf / fmaxf spelling, in float32 numpy (np.fmin / np.fmax are C's fminf /
    fmaxf: they return the other operand for a NaN)"""
    v = np.array([np.nan, -9.0, -1.5, 0.0, 1.5, 9.0], np.float32)
    t = v * np.float32(1.0 / 6.0) + np.float32(0.5)
    with np.errstate(invalid="ignore"):
        keep = np.where(t < 0, np.float32(0), np.where(t > 1, np.float32(1), t))
    launder = np.fmin(np.fmax(t, np.float32(0)), np.float32(1))
    assert np.isnan(keep[0]) and not np.isnan(launder[0]) and launder[0] in (0.0, 1.0)
    assert np.array_equal(keep[1:], launder[1:]) and np.array_equal(keep[1:], hsigmoid64(v[1:]).astype(np.float32))


# ---- both readers, spelling for spelling ---------------------------------------------------------------------------------------------
SPELLINGS = ["op", "hsigmoid", "hsigmoid:swap", "hsigmoid:cast", "decomposed", "decomposed:swap", "decomposed:scale_first", "decomposed:div",
             "decomposed:div,scale_first,swap", "decomposed:f16", "decomposed:f16,div", "decomposed:cast", "decomposed:cast,scale_first,f16"]


def _native(data, path):
    L = _lib.load()
    with open(path, "wb") as f:
        f.write(data)
    rc = L.bh_onnx_to_bhm(path.encode(), (path + ".bhm").encode())
    return (rc, L.bh_last_error().decode()) if rc else (0, mf.read_model(path + ".bhm"))


def _key(L):
    return (L.op, L.act, L.reserved, L.in_tensor, L.res_tensor, L.cin, L.cout, L.kh, L.kw, L.sh, L.sw, L.pad_t, L.pad_l, L.out_h, L.out_w)


@pytest.mark.parametrize("spelling", SPELLINGS)
@pytest.mark.parametrize("seed", [0, 1])
def test_every_spelling_reads_to_the_model_that_was_written(seed, spelling, tmp_path):
    """seed 0: no gates; seed 1: a hard-sigmoid gate in every block.  Both readers from the audio input (the one-branch spectrogram is
    in no family table): the same container, record for record and weight for weight, and the records of the model written."""
    m = synth.build_model("mnv3_plan", plan=synth.random_mnv3_plan(seed))
    acts = [L.act for L in m.layers]
    assert HSWISH in acts and (HSIGMOID in acts) == bool(seed) and m.layers[-2].op == mf.OP_DENSE and m.layers[-2].act == HSWISH
    data = convert.model_to_onnx(m, frontend_spelling="stft", spell_hswish=spelling)
    ops = {n.op_type for n in ox.load(data).nodes}
    assert ("HardSwish" in ops) == (spelling == "op") and ("HardSigmoid" in ops) == (not spelling.startswith("decomposed") and (seed == 1 or spelling != "op"))
    want = convert.model_from_graph(ox.load(data), None, sample_rate=m.sample_rate)
    rc, got = _native(data, str(tmp_path / "m.onnx"))
    assert rc == 0, got
    _same_model(want, got, frontend_exact=False)
    assert [_key(L) for L in got.layers] == [_key(L) for L in m.layers]


def test_mobilenetv3_audio_reads_back_with_its_relu_blocks(tmp_path):
    m = synth.build_model("mobilenetv3_audio", n_classes=24)
    dws = [L for L in m.layers if L.op == mf.OP_DWCONV]
    assert [L.act for L in dws] == [mf.ACT_RELU] * 6 + [HSWISH] * 9 and sum(L.act == HSIGMOID for L in m.layers) == 8
    assert [L.cout for L in dws] == [16, 64, 72, 72, 120, 120, 240, 200, 184, 184, 480, 672, 672, 960, 960]
    rc, got = _native(convert.model_to_onnx(m, frontend_spelling="stft", spell_hswish="hsigmoid"), str(tmp_path / "l.onnx"))
    assert rc == 0, got
    assert [_key(L) for L in got.layers] == [_key(L) for L in m.layers]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _gated_graph(seed=1):
    m = synth.build_model("mnv3_plan", plan=synth.random_mnv3_plan(seed))
    return m, convert.graph_from_model(m, frontend_spelling="stft", spell_hswish="hsigmoid")


def _both_refuse(g, what, tmp_path, name, also=()):
    data = ox.dump(g)
    with pytest.raises(convert.ConvertError) as e:
        convert.model_from_graph(ox.load(data), None, sample_rate=48000)
    rc, msg = _native(data, str(tmp_path / name))
    assert rc == -2, (rc, msg)
    for w in (what,) + tuple(also):
        assert w in str(e.value), (w, str(e.value))
        assert w in msg, (w, msg)


def test_the_keras_hard_sigmoid_is_refused_by_name_with_its_values(tmp_path):
    m, g = _gated_graph()
    gate = next(n for n in g.nodes if n.op_type == "HardSigmoid" and n.outputs[0].endswith("_hsig") and not any(
        n.outputs[0] in q.inputs and n.inputs[0] in q.inputs for q in g.nodes))
    gate.attrs.clear()                        # the ONNX defaults: alpha = 0.2, beta = 0.5
    _both_refuse(g, "alpha = 0.2, beta = 0.5", tmp_path, "keras.onnx", also=("HardSigmoid", "Keras"))
    # ... and inside HardSigmoid * x as well: the fold does not take it
    m, g = _gated_graph(0)
    next(n for n in g.nodes if n.op_type == "HardSigmoid").attrs["alpha"] = 0.2
    _both_refuse(g, "alpha = 0.2, beta = 0.5", tmp_path, "keras_mul.onnx")
    m, g = _gated_graph(0)
    next(n for n in g.nodes if n.op_type == "HardSigmoid").attrs["beta"] = 0.25
    _both_refuse(g, "beta = 0.25", tmp_path, "beta.onnx")


def test_a_hard_sigmoid_on_a_feature_map_is_refused(tmp_path):
    """HardSigmoid(x) read by a convolution: neither . * x nor a gate (in both spellings of the function)"""
    for spelling in ("hsigmoid", "decomposed"):
        m = synth.build_model("mnv3_plan", plan=synth.random_mnv3_plan(0))
        g = convert.graph_from_model(m, frontend_spelling="stft", spell_hswish=spelling)
        # the first hard swish behind a 1x1 convolution: drop its Mul(., x), the next node reads the gate function itself
        mul = next(n for n in g.nodes if n.op_type == "Mul" and n.outputs[0].endswith("_hswish" if spelling == "hsigmoid" else "_hsx"))
        inner = next(x for x in mul.inputs if x.endswith("_hsig") or x.endswith("_r6"))
        g.nodes.remove(mul)
        for n in g.nodes:
            n.inputs[:] = [inner if x == mul.outputs[0] else x for x in n.inputs]
        _both_refuse(g, "HardSigmoid inside the graph that is neither HardSigmoid * x nor a squeeze-excite gate", tmp_path, spelling + "_map.onnx")


def test_a_chain_whose_inner_tensor_has_a_second_reader_does_not_fold(tmp_path):
    """the Clip's output read by a second node: no hard swish; the Add(x, 3) then meets the rule a bare Add met before"""
    m = synth.build_model("mnv3_plan", plan=synth.random_mnv3_plan(0))
    for spelling, inner_end in (("decomposed", "_r6"), ("decomposed", "_p3"), ("hsigmoid", "_hsig")):
        g = convert.graph_from_model(m, frontend_spelling="stft", spell_hswish=spelling)
        inner = next(n.outputs[0] for n in g.nodes if n.outputs[0].endswith(inner_end))
        g.nodes.append(ox.Node("Relu", [inner], ["second_reader"]))
        what = "HardSigmoid inside the graph" if spelling == "hsigmoid" else "operands are not both activations on the path"
        _both_refuse(g, what, tmp_path, f"second_{inner_end}.onnx")


def test_hard_swish_straight_after_a_concat_record_is_refused(tmp_path):
    m = synth.build_model("branchy_plan", plan=synth.random_branchy_plan(0))
    g = convert.graph_from_model(m, frontend_spelling="stft")
    cat = next(n for n in g.nodes if n.op_type == "Concat" and n.outputs[0] != "spectrogram" and not n.outputs[0].startswith("fe"))
    for op in ("HardSwish", "HardSigmoid"):
        g2 = ox.load(ox.dump(g))
        i = next(k for k, n in enumerate(g2.nodes) if n.outputs == cat.outputs)
        attrs = {} if op == "HardSwish" else {"alpha": float(np.float32(1 / 6)), "beta": 0.5}
        if op == "HardSigmoid":     # HardSigmoid * x: the fold's other spelling
            g2.nodes.insert(i + 1, ox.Node("Mul", [cat.outputs[0], "cat_gate"], ["cat_act"]))
        g2.nodes.insert(i + 1, ox.Node(op, [cat.outputs[0]], ["cat_act" if op == "HardSwish" else "cat_gate"], attrs))
        for n in g2.nodes[i + (2 if op == "HardSwish" else 3):]:
            n.inputs[:] = ["cat_act" if x == cat.outputs[0] else x for x in n.inputs]
        _both_refuse(g2, "directly after a Concat, Split, Slice or channel shuffle", tmp_path, op + "_concat.onnx")


# ---- files that loaded before read as before ------------------------------------------------------------------------------------------
def test_clip_and_a_residual_add_read_as_before(tmp_path):
    from test_convert import hand_written_graph
    g, _, _, base = hand_written_graph()
    data = ox.dump(g)
    want = convert.model_from_graph(ox.load(data), base)
    rc, got = _native(data, str(tmp_path / "hand.onnx"))
    assert rc == 0, got
    _same_model(want, got)
    assert [L.act for L in got.layers[:4]] == [mf.ACT_RELU6, mf.ACT_SWISH, mf.ACT_NONE, mf.ACT_RELU] and got.layers[2].res_tensor == 1
    # Add(x, 3) with no Clip behind it, and Clip(0, 6) with no Add(., 3) in front, stay what they were
    for kind in ("mini", "mini_se"):
        m = synth.build_model(kind, act=mf.ACT_RELU6)
        d2 = convert.model_to_onnx(m)
        rc, got = _native(d2, str(tmp_path / (kind + ".onnx")))
        assert rc == 0 and [_key(L) for L in got.layers] == [_key(L) for L in m.layers]
        assert [_key(L) for L in convert.model_from_graph(ox.load(d2), m).layers] == [_key(L) for L in m.layers]


# ---- the container ------------------------------------------------------------------------------------------------------------------
def test_codes_7_and_8_round_trip_through_the_container(tmp_path):
    assert (mf.ACT_HSWISH, mf.ACT_HSIGMOID) == (7, 8) and mf.ACT_SIGMOID == 6
    m = synth.build_model("mnv3_plan", plan=synth.random_mnv3_plan(1))
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    back = mf.read_model(path)
    assert [_key(L) for L in back.layers] == [_key(L) for L in m.layers] and {7, 8} <= {L.act for L in back.layers}
    assert back.blob.tobytes() == m.blob.tobytes()
    # the library's host-only planner loads the file: validate_model takes the codes
    L = _lib.load()
    assert L.bh_plan_fused_blocks(path.encode(), 0, None, None, 0) >= 0, L.bh_last_error()


# ---- the fused block kernel's fourth family -----------------------------------------------------------------------------------------
def names_ex():
    """every configuration bh_mb_config_name_ex names, in index order"""
    L = _lib.load()
    out = []
    while True:
        buf = C.create_string_buffer(128)
        if L.bh_mb_config_name_ex(len(out), buf, 128) <= 0:
            return out
        out.append(buf.value.decode())


def family3_rows():
    """The rows of the hard-swish family as tests/test_mbconv_block.py's table() holds the other three: family 0's live rows with
    ACT = 7, the full index base + 3 n_base and the name bh_mb_config_name_ex gives that index."""
    import test_mbconv_block as CAT
    ex = names_ex()
    rows = []
    for r in CAT.table():
        if r["ACT"] == 4:
            ci = r["base"] + 3 * r["nbase"]
            rows.append(dict(r, ACT=HSWISH, ci=ci, name=ex[ci]))
    return rows


def family3_cases(r3):
    """the catalogue's cases of the family-0 twin of the row, with the activation code swapped"""
    import test_mbconv_block as CAT
    r0 = next(r for r in CAT.table() if r["ACT"] == 4 and r["base"] == r3["base"])
    out = []
    for c in CAT.cases_for(r0):
        shape = list(c["shape"])
        shape[11] = HSWISH
        out.append(dict(c, shape=shape))
    return out


def test_the_index_space_keeps_its_first_three_families_where_they_were():
    import test_mbconv_block as CAT
    L = _lib.load()
    assert L.bh_mb_config_families() == 4
    buf = C.create_string_buffer(128)
    old = []
    while L.bh_mb_config_name(len(old), buf, 128) > 0:
        old.append(buf.value.decode())
    ex = names_ex()
    assert len(old) % 3 == 0 and len(ex) % 4 == 0
    n_base = len(old) // 3
    assert len(ex) == 4 * n_base and ex[:3 * n_base] == old
    assert L.bh_mb_config_name(3 * n_base, buf, 128) <= 0 and L.bh_mb_config_name(4 * n_base - 1, buf, 128) <= 0 and L.bh_mb_config_name_ex(4 * n_base, buf, 128) <= 0
    # family 3 is family 0's list with the ACT field (the eighteenth) changed and nothing else
    for a, b in zip(ex[:n_base], ex[3 * n_base:]):
        fa, fb = a.split(","), b.split(",")
        assert fa[:17] + fa[18:] == fb[:17] + fb[18:] and fa[17] in ("0", "4") and fb[17] == ("7" if fa[0] != "0" else fb[17]), (a, b)
    assert all(r["nbase"] == n_base for r in CAT.table())


def test_the_planner_puts_hard_swish_blocks_on_family_3_and_the_others_where_they_were():
    import test_mbconv_block as CAT
    rows = family3_rows()
    n_base = rows[0]["nbase"]
    assert len(rows) == sum(r["ACT"] == 4 for r in CAT.table())
    n = 0
    for r3 in rows:
        cs = family3_cases(r3)
        assert cs, r3["base"]
        for c in cs:
            rc, rec, name = CAT.plan(c["shape"], r3["base"])
            assert rc == 0 and rec[0] == r3["ci"] and 3 * n_base <= rec[0] < 4 * n_base, (r3["base"], rc, rec[0], c["shape"])
            assert name == "mbconv<%s,%d>" % (r3["name"], c["se"]), (name, r3["name"])
            n += 1
    print("family 3: %d rows, %d cases" % (len(rows), n))
    # acts 2 / 3 / 4: every row's first case still plans to the row's own index (tests/test_mbconv_block.py holds all of them)
    for r in CAT.table():
        c = CAT.cases_for(r)[0]
        rc, rec, name = CAT.plan(c["shape"], r["base"])
        assert rc == 0 and rec[0] == r["ci"] < 3 * n_base and name == "mbconv<%s,%d>" % (r["name"], c["se"]), (r["base"], r["ACT"])


def hard_swish_blocks(m):
    """first layers of the model's hard-swish inverted-residual blocks: the expand 1x1 in front of a hard-swish depthwise layer, or
    that layer itself where there is no expand convolution"""
    out = []
    for i, L in enumerate(m.layers):
        if L.op == mf.OP_DWCONV and L.act == HSWISH:
            E = m.layers[i - 1]
            out.append(i - 1 if (E.op == mf.OP_PWCONV and E.act == HSWISH and L.in_tensor == i) else i)
    return out


@pytest.mark.parametrize("which", [0, 1, 3, "large"])
def test_every_hard_swish_block_is_planned_fused_on_family_3(which, tmp_path):
    """the host-only planner on the models tests/test_hardswish_gpu.py runs, split f16: every hard-swish block is a fused block on an
    index of [3 n_base, 4 n_base); mobilenetv3_audio's ReLU blocks stay with the layer kernels (no ReLU family)"""
    L = _lib.load()
    n_base = len(names_ex()) // 4
    m = synth.build_model("mobilenetv3_audio", n_classes=40) if which == "large" else synth.build_model("mnv3_plan", plan=synth.random_mnv3_plan(which))
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    cfgs, layers = (C.c_int32 * 256)(), (C.c_int32 * 256)()
    n = L.bh_plan_fused_blocks(path.encode(), 0, cfgs, layers, 256)
    assert n > 0, L.bh_last_error()
    firsts = {int(layers[k]) for k in range(n)}
    assert all(3 * n_base <= int(cfgs[k]) < 4 * n_base for k in range(n)), [int(cfgs[k]) for k in range(n)]
    want = hard_swish_blocks(m)
    assert want and set(want) <= firsts, (want, sorted(firsts))
    relu = [i for i, a in enumerate(m.layers) if a.op == mf.OP_DWCONV and a.act == mf.ACT_RELU]
    assert (which != "large") or (len(relu) == 6 and not ({i for i in relu} | {i - 1 for i in relu}) & firsts)


# ---- the compressed code objects ---------------------------------------------------------------------------------------------------
def compressed_code_objects(tmp_path):
    """The gfx950 code objects of the units the Makefile builds with --offload-compress (the layer GEMMs and the hard-swish family),
    unbundled from libbirda_hip.so's .hip_fatbin: a compressed bundle starts with 'CCOB', a version, the method and its own length."""
    import re
    import struct
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [llvm + "/" + t for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not all(os.path.exists(t) for t in tools):
        return None
    fat = str(tmp_path / "fat.bin")
    subprocess.run([tools[0], "--dump-section", ".hip_fatbin=" + fat, os.path.join(ROOT, "birda_amd", "libbirda_hip.so")], check=True, capture_output=True, timeout=120)
    data = open(fat, "rb").read()
    out = []
    for m in re.finditer(b"CCOB", data):
        a = m.start()
        ver = struct.unpack_from("<H", data, a + 4)[0]
        if a % 8 or ver not in (2, 3):
            continue
        size = struct.unpack_from("<Q" if ver == 3 else "<I", data, a + 8)[0]
        piece, code = str(tmp_path / f"ccob{len(out)}.bin"), str(tmp_path / f"ccob{len(out)}.o")
        open(piece, "wb").write(data[a:a + size])
        subprocess.run([tools[1], "--unbundle", "--type=o", "--input=" + piece, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + code],
                       check=True, capture_output=True, timeout=120)
        out.append(subprocess.run([tools[2], "-d", code], check=True, capture_output=True, text=True, timeout=900).stdout)
    return out


def test_the_compressed_code_objects_hold_to_the_library_s_rules(tmp_path):
    """tests/test_abi_and_host.py reads the bundles it finds by the plain bundle magic; the four compressed ones are read here and held
    to the same rule (no packed-f32 instruction selects operand halves with op_sel: -- DESIGN.md section 3).  They are the hard-swish
    family (its kernels carry the FMA with the clamp modifier that the hard swish compiles to) and the layer GEMMs."""
    import re
    texts = compressed_code_objects(tmp_path)
    if texts is None:
        pytest.skip("ROCm llvm tools not available")
    assert len(texts) == 4, len(texts)
    for k, text in enumerate(texts):
        bad = [l.strip() for l in text.splitlines() if re.search(r"v_pk_(add|mul|fma)_f32\b.*\bop_sel:\[", l)]
        assert not bad, (k, bad[:3])
    family = [t for t in texts if "mbconv_kernel" in t]
    assert len(family) == 3 and all(len(re.findall(r"v_fma_f32 .* clamp", t)) > 100 for t in family)
    assert sum("pw_gemm16s_kernel" in t for t in texts) == 1
