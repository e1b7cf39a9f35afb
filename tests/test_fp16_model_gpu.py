"""Float16 model files on the device, and the two-term GEMM kernels they run (kernels_conv.hip TERMS == 2: hi hi, lo hi on compact
planes, for weight matrices made of f16 values).

Kernel level, through the debug entry points with terms = 2, on the shape tables of tests/test_layer_gemm_gpu.py and
tests/test_gated_gemm_gpu.py with W rounded to f16 values: every output element (a) meets the SAME bound as terms 3 there --
tau = 4e-7 max(1, sqrt(K / 1024)) on 1.2 (|A||W| + |b|) + |R|, plus eps_act; derived, not measured: x_lo w is kept and w_lo is
exactly zero, so no product term is dropped that three terms keep -- and (b) equals the terms = 3 result on the same operands as a
number, element for element (== on finite values; the sign of a zero may differ).  Model level: float16 files created on the .onnx
route against the oracle on the converted container, the weight summary, two-term against BH_FLAG_FULL_PLANES classifiers.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gated_gemm_gpu as TG  # noqa: E402
import test_layer_gemm_gpu as TL  # noqa: E402  (shape tables, operand generators and bounds: imported, not restated)

pytestmark = pytest.mark.gpu

LOGIT_RTOL = 2e-5
REACHED2 = set()


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def _same_numbers(a, b, what):
    assert np.isfinite(a).all() and np.isfinite(b).all(), what
    if not (a == b).all():
        i = np.unravel_index(np.argmax(a != b), a.shape)
        pytest.fail(f"{what}: {int((a != b).sum())} of {a.size} elements differ between terms 2 and terms 3, first at {i}: {a[i]!r} != {b[i]!r}")


# ---- 6. kernel level ------------------------------------------------------------------------------------------------------------
def _conv_params2():
    out = []
    for i, case in enumerate(TL.CONV_CASES):
        act = TL.ACTS16[(i + 2) % 4]
        out.append(pytest.param(case, act, id=f"{case[0]}-{O.ACT_NAMES[act]}"))
    res = TL._conv_case("res_96to96", 2, 10, 12, 96, 96, 3, 3, residual=True)
    for act in TL.ACTS16:
        out.append(pytest.param(res, act, id=f"res_96to96-{O.ACT_NAMES[act]}"))
    return out


_CONV_REF = {}


def _conv_ref16(case):
    name, n_seg, shape, residual = case
    if name not in _CONV_REF:
        in_h, in_w, oh, ow, cin, cout, kh, kw, sh, sw, pt, pl = shape
        rng = np.random.default_rng(sum(shape) * 7 + n_seg)
        M = n_seg * oh * ow
        X, W, b, R = TL._operands(rng, (n_seg, in_h, in_w, cin), kh * kw * cin, cout, residual, M)
        W = _f16(W).reshape(kh, kw, cin, cout)
        pre, A = O.conv_nhwc64(X, W.astype(np.float64), b, sh, sw, pt, pl, oh, ow)
        bound = np.abs(A) @ np.abs(W.reshape(-1, cout).astype(np.float64)) + np.abs(b.astype(np.float64))
        _CONV_REF[name] = (X, W, b, R, pre, bound)
    return _CONV_REF[name]


@pytest.mark.parametrize("case,act", _conv_params2())
def test_conv16_two_terms(case, act):
    name, n_seg, shape, residual = case
    X, W, b, R, pre, bound = _conv_ref16(case)
    got, kname = TL._conv(X, W, b, R, shape, act, 2)
    REACHED2.add(kname)
    assert kname.startswith("conv_gemm16_kernel<2,"), kname
    TL._check(got, kname, pre, bound, R, act, 3, shape[6] * shape[7] * shape[4], name)     # terms 3's bound
    three, k3 = TL._conv(X, W, b, R, shape, act, 3)
    assert k3.startswith("conv_gemm16_kernel<3,"), k3
    _same_numbers(got, three, name)


def _pw_params2():
    return [pytest.param(mkn, TL.ACTS16[(i + 2) % 4], id="M%d_K%d_N%d" % mkn + f"-{O.ACT_NAMES[TL.ACTS16[(i + 2) % 4]]}") for i, mkn in enumerate(TL.PW16)]


@pytest.mark.parametrize("mkn,act", _pw_params2())
def test_layer_gemm_two_terms(mkn, act):
    M, K, N = mkn
    rng = np.random.default_rng(M * 7 + K * 131 + N)
    A, W, b, R = TL._operands(rng, (M, K), K, N, (M + N) % 2 == 0, M)
    W = _f16(W)
    got, kname = TL._layer(A, W, b, R, act, 2)
    REACHED2.add(kname)
    assert re.match(r"pw_gemm16\w*_kernel<2,", kname), kname
    pre = O.gemm64(A, W, b)
    bound = np.abs(A.astype(np.float64)) @ np.abs(W.astype(np.float64)) + np.abs(b.astype(np.float64))
    TL._check(got, kname, pre, bound, R, act, 3, K, "pw two terms")
    three, k3 = TL._layer(A, W, b, R, act, 3)
    assert k3 == kname.replace("<2,", "<3,"), (kname, k3)      # the same kernel family and tile at either terms
    _same_numbers(got, three, mkn)


def _head_params2():
    return [pytest.param(case, TL.HEAD_ACTS[(i + 2) % 3], id="P%d_n%d_K%d_N%d" % case + f"-{O.ACT_NAMES[TL.HEAD_ACTS[(i + 2) % 3]]}")
            for i, case in enumerate(TL.HEAD)]


@pytest.mark.parametrize("case,act", _head_params2())
def test_head_pool_two_terms(case, act):
    P, n_seg, K, N = case
    rng = np.random.default_rng(P * 1000 + n_seg * 10 + K + N)
    A, W, b, _ = TL._operands(rng, (n_seg * P, K), K, N, False, n_seg * P)
    W = _f16(W)
    got, kname = TL._layer(A, W, b, None, act, 2, pool_rows=P)
    REACHED2.add(kname)
    assert kname.startswith("head_gap16_kernel<") and ",T=2," in kname, kname
    TL._check_head(got, kname, A, W, b, P, act, 3, "head two terms")
    three, k3 = TL._layer(A, W, b, None, act, 3, pool_rows=P)
    assert k3 == kname.replace(",T=2,", ",T=3,")
    _same_numbers(got, three, case)


def test_every_epilogue_of_every_two_term_family():
    """Every activation instantiation of the skinny / streaming / staged (NTB 2, 4, 8) GEMMs and of the head kernel (PT / SW 3 / 2 and
    5 / 1, CT 2 and 8) on two terms, against three terms on the same operands: the same numbers."""
    rng = np.random.default_rng(31)
    for (M, K, N) in ((16, 64, 132), (40, 64, 132), (300, 32, 20), (3000, 32, 1000), (6151, 32, 1024)):
        A, W, b, R = TL._operands(rng, (M, K), K, N, True, M)
        W = _f16(W)
        for act in TL.ACTS16:
            two, k2 = TL._layer(A, W, b, R, act, 2)
            three, k3 = TL._layer(A, W, b, R, act, 3)
            REACHED2.add(k2)
            assert k2.replace("<2,", "<3,") == k3, (k2, k3)
            _same_numbers(two, three, (M, K, N, act))
    for (P, n_seg) in ((16, 8), (16, 100), (49, 5), (49, 100)):
        A, W, b, _ = TL._operands(rng, (n_seg * P, 64), 64, 128, False, n_seg * P)
        W = _f16(W)
        for act in TL.HEAD_ACTS:
            two, k2 = TL._layer(A, W, b, None, act, 2, pool_rows=P)
            three, k3 = TL._layer(A, W, b, None, act, 3, pool_rows=P)
            REACHED2.add(k2)
            assert k2.replace(",T=2,", ",T=3,") == k3, (k2, k3)
            _same_numbers(two, three, (P, n_seg, act))


def _gated(A, gate, W, bias, R, P, terms, blocked, want_name=False):
    lib = _lib.load()
    out = TG._run(lib, A, gate, W, bias, R, P, terms, blocked)
    buf = C.create_string_buffer(160)
    lib.bh_debug_last_gated_kernel(buf, 160)
    name = buf.value.decode()
    if terms == 2:
        REACHED2.add(name)
    return (out, name) if want_name else out


def _gated_instantiations():
    """(n_seg, rows per segment, K, N, blocked, the instantiation launch_pw_gemm16_gated must pick at terms 2): every TERMS == 2
    instantiation behind that launcher -- the streaming kernel (N <= 48, 4 096 rows and more: NT 1 .. 3, SHALLOW for K <= 32), the
    row-streaming kernel (NT 4 .. 15; from 40 960 rows for NT >= 10; NHWC and blocked rows by turns; K % 32 != 0) and the staged
    tiles (NTB 6 / 8 / 10 by the padding of N, NHWC and blocked rows), the piece arithmetic of compact planes differing per NT"""
    out = []
    for nt in (1, 2, 3):
        for K in (24, 72):
            out.append((5, 1000, K, 16 * nt, 0, f"pw_gemm16_thin_kernel<2,NT={nt},SHALLOW={'true' if K <= 32 else 'false'}>"))
    for nt in range(4, 16):
        rb, pf = (3, 3) if nt <= 7 else (2, 4) if nt <= 9 else (2, 3)
        out.append((17 if nt < 10 else 161, 256, 80, 16 * nt, nt % 2 if nt >= 6 else 0, f"pw_gemm16_wide_kernel<2,NT={nt},RB={rb},PF={pf}>"))
    for ntb, N in ((6, 96), (8, 128), (10, 160)):
        for blocked in (0, 1):
            out.append((16, 64, 80, N, blocked, f"pw_gemm16s_kernel<2,NONE,GATE,NTB={ntb},BLK={'true' if blocked else 'false'}>"))
    return out


GATED2 = _gated_instantiations()


@pytest.mark.parametrize("case", GATED2, ids=lambda c: c[5])
def test_every_gated_two_term_instantiation(case):
    n_seg, P, K, N, blocked, want = case
    A, gate, W, bias, R = TG._operands(K * 131 + N, n_seg, P, K, N, True)
    W = _f16(W)
    ref, bound = TG._reference(A, gate, W, bias, R, P)
    two, name = _gated(A, gate, W, bias, R, P, 2, blocked, want_name=True)
    assert name == want, (name, want)
    err = np.abs(two - ref) / bound
    assert np.isfinite(two).all() and err.max() <= 4e-7, (case, float(err.max()))
    three, name3 = _gated(A, gate, W, bias, R, P, 3, blocked, want_name=True)
    assert name3 == want.replace("<2,", "<3,"), (name3, want)          # the same kernel and tile at either terms
    _same_numbers(two, three, case)


REACHED1 = set()


@pytest.mark.parametrize("case", GATED2, ids=lambda c: c[5].replace("<2,", "<1,"))
def test_every_gated_plain_f16_instantiation(case):
    """The same 24 shapes on plain f16 (terms 1), W as it is: the instantiation by name, and every element within 1.5e-3 of
    sum |a g||w| + |b| + |R| -- tests/test_gated_gemm_gpu.py's figure for terms 1."""
    n_seg, P, K, N, blocked, want = case
    A, gate, W, bias, R = TG._operands(K * 131 + N, n_seg, P, K, N, True)
    ref, bound = TG._reference(A, gate, W, bias, R, P)
    one, name = _gated(A, gate, W, bias, R, P, 1, blocked, want_name=True)
    REACHED1.add(name)
    assert name == want.replace("<2,", "<1,"), (name, want)
    err = np.abs(one - ref) / bound
    assert np.isfinite(one).all() and err.max() <= 1.5e-3, (case, float(err.max()))


def test_every_gated_plain_f16_kernel_was_reached():
    """(keep behind test_every_gated_plain_f16_instantiation: it reads what that ran)"""
    if len(REACHED1) < 2:
        pytest.skip("reads the kernels test_every_gated_plain_f16_instantiation ran: run the module whole")
    want = {c[5].replace("<2,", "<1,") for c in GATED2}
    assert len(want) == 24 and REACHED1 == want, sorted(want ^ REACHED1)


@pytest.mark.parametrize("shape", TG.SHAPES, ids=lambda s: "n%d_P%d_K%d_N%d_r%d_b%d" % s)
def test_gated_gemm_two_terms(shape):
    """Every kernel behind launch_pw_gemm16_gated (streaming, row-streaming over NHWC and blocked rows, staged tiles) on two terms:
    test_gated_gemm_gpu's own bound for three terms (4e-7 of sum |a g||w| + |b| + |R|), and the three-term numbers."""
    n_seg, P, K, N, residual, blocked = shape
    A, gate, W, bias, R = TG._operands(K * 131 + N, n_seg, P, K, N, residual)
    W = _f16(W)
    ref, bound = TG._reference(A, gate, W, bias, R, P)
    two = _gated(A, gate, W, bias, R, P, 2, blocked)
    err = np.abs(two - ref) / bound
    assert np.isfinite(two).all() and err.max() <= 4e-7, (shape, float(err.max()))
    _same_numbers(two, _gated(A, gate, W, bias, R, P, 3, blocked), shape)


def test_launches_of_different_sizes_give_the_same_bits_on_two_terms():
    """What tests/test_layer_gemm_gpu.py and tests/test_gated_gemm_gpu.py hold for terms 1 and 3: five pointwise kernels, the conv's
    launch size, the head kernel's column tile, a gated row's kernel -- one set of bits."""
    rng = np.random.default_rng(9)
    M, K, N = 6151, 320, 1024
    A, W, b, R = TL._operands(rng, (M, K), K, N, True, M)
    W = _f16(W)
    outs = {}
    for m in (16, 48, 256, 3000, 6151):
        got, kname = TL._layer(A[:m].copy(), W, b, R[:m].copy(), O.ACT_GELU_ERF, 2)
        REACHED2.add(kname)
        outs[kname] = got[:16]
    assert len(outs) == 5, sorted(outs)
    first = next(iter(outs.values()))
    for kname, o in outs.items():
        assert np.array_equal(o, first), kname
    case = next(c for c in TL.CONV_CASES if c[0] == "37seg_17x23_36to100")
    X, Wc, bc, Rc, _, _ = _conv_ref16(case)
    rows = case[2][2] * case[2][3]
    big, _ = TL._conv(X, Wc, bc, Rc, case[2], O.ACT_GELU_ERF, 2)
    one, _ = TL._conv(X[:1].copy(), Wc, bc, Rc[:rows].copy(), case[2], O.ACT_GELU_ERF, 2)
    assert np.array_equal(big[:rows], one)
    for P in (16, 49):
        A, W, b, _ = TL._operands(rng, (100 * P, 320), 320, 1280, False, 100 * P)
        W = _f16(W)
        big, kb = TL._layer(A, W, b, None, O.ACT_GELU_ERF, 2, pool_rows=P)
        few, kf = TL._layer(A[:32 * P].copy(), W, b, None, O.ACT_GELU_ERF, 2, pool_rows=P)
        assert kb.endswith("CT=8>") and kf.endswith("CT=2>"), (kb, kf)
        assert np.array_equal(big[:32], few), P
    for (n_seg, P, K, N) in ((650, 64, 336, 232), (20, 256, 816, 136), (6, 1008, 24, 24)):
        A, gate, W, bias, R = TG._operands(7 * K + N, n_seg, P, K, N, True)
        W = _f16(W)
        few = max(1, 2048 // P)
        for blocked in ((0, 1) if (K % 16 == 0 and P % 16 == 0 and 6 <= -(-N // 16) <= 15) else (0,)):
            big = _gated(A, gate, W, bias, R, P, 2, blocked)
            small = _gated(A[:few * P].copy(), gate[:few].copy(), W, bias, R[:few * P].copy(), P, 2, blocked)
            assert np.array_equal(big[:few * P], small), (n_seg, P, K, N, blocked)


def test_two_terms_are_refused_for_weights_that_are_not_f16_values():
    lib = _lib.load()
    rng = np.random.default_rng(2)
    A, W, b, _ = TL._operands(rng, (64, 64), 64, 128, False, 64)
    out = np.empty((64, 128), np.float32)
    p = TL._p
    assert lib.bh_debug_layer_gemm(0, p(A), p(W), p(b), None, p(out), 64, 64, 128, 0, O.ACT_NONE, 2, None, 0) == -6
    assert b"f16 values" in lib.bh_last_error()
    assert lib.bh_debug_layer_gemm(0, p(A), p(_f16(W)), p(b), None, p(out), 64, 64, 128, 0, O.ACT_NONE, 2, None, 0) == 0
    out4 = np.empty((4, 128), np.float32)
    assert lib.bh_debug_layer_gemm(0, p(A), p(W), p(b), None, p(out4), 64, 64, 128, 16, O.ACT_GELU_ERF, 2, None, 0) == -6
    shape = np.asarray((6, 6, 6, 6, 8, 8, 3, 3, 1, 1, 1, 1), np.int32)
    X = rng.standard_normal((1, 6, 6, 8)).astype(np.float32)
    Wc = rng.standard_normal((3, 3, 8, 8)).astype(np.float32)
    outc = np.empty((36, 8), np.float32)
    assert lib.bh_debug_conv_gemm(0, p(X), p(Wc), p(b), None, p(outc), 1, p(shape), O.ACT_NONE, 2, None, 0) == -6
    assert lib.bh_debug_conv_gemm(0, p(X), p(_f16(Wc)), p(b), None, p(outc), 1, p(shape), O.ACT_NONE, 2, None, 0) == 0
    g = rng.uniform(0, 1, (4, 64)).astype(np.float32)
    assert lib.bh_debug_gated_gemm(0, p(A), p(g), p(W), p(b), None, p(out), 64, 64, 128, 16, 2, 0) == -6
    assert lib.bh_debug_gated_gemm(0, p(A), p(g), p(_f16(W)), p(b), None, p(out), 64, 64, 128, 16, 2, 0) == 0


def test_every_two_term_kernel_was_reached():
    """(keep behind the kernel-level tests: it reads what they ran)"""
    if not REACHED2:
        pytest.skip("reads the kernels the module's other tests ran: run the module whole")
    want = [f"conv_gemm16_kernel<2,{a}>" for a in ("NONE", "GELU", "SWISH", "RELU6")]
    for a in ("NONE", "GELU", "SWISH", "RELU6"):
        want += [f"pw_gemm16_skinny_kernel<2,{a}>", f"pw_gemm16_kernel<2,{a}>"] + [f"pw_gemm16s_kernel<2,{a},NTB={b}>" for b in (2, 4, 8)]
    for a in ("GELU", "SWISH", "RELU6"):
        want += [f"head_gap16_kernel<PT={pt},SW={sw},T=2,{a},CT={ct}>" for pt, sw in ((3, 2), (5, 1)) for ct in (2, 8)]
    want += [c[5] for c in GATED2]           # the 24 instantiations behind launch_pw_gemm16_gated
    assert len(set(want)) == 36 + 24
    missing = [w for w in want if w not in REACHED2]
    assert not missing, (missing, sorted(REACHED2))


# ---- 7. model level -------------------------------------------------------------------------------------------------------------
def _unfold_bn(g, rng, which):
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


def _files(tmp_path, kind):
    """-> (model, float32 .onnx, float16 .onnx, the container bh_onnx_to_bhm writes from the float16 file)"""
    bn = kind == "bn"
    if kind.startswith("fused"):
        m = synth.build_model("custom", plan=synth.random_fused_plan(int(kind[5:])))
    else:
        m = synth.build_model("mini_hg" if bn else kind)
    g32 = convert.graph_from_model(m, frontend_spelling="conv1d")
    if bn:      # BatchNormalization left in the graph behind every convolution outside the front-end
        n_conv = sum(1 for n in g32.nodes if n.op_type == "Conv" and not n.name.startswith("fe"))
        _unfold_bn(g32, np.random.default_rng(5), range(n_conv))
    p32, p16, bhm = (str(tmp_path / f"{kind}{s}") for s in ("_32.onnx", "_16.onnx", "_16.bhm"))
    with open(p32, "wb") as f:
        f.write(ox.dump(g32))
    with open(p16, "wb") as f:
        f.write(ox.dump(convert.graph_to_float16(g32, frontend="f32" if kind in ("fused1", "perch_v2_tiny") else "f16")))
    L = _lib.load()
    assert L.bh_onnx_to_bhm(p16.encode(), bhm.encode()) == 0, L.bh_last_error()
    return m, p32, p16, bhm


def _logits(path, segs, n_max, **kw):
    from birda_amd.classifier import BirdClassifier
    clf = BirdClassifier(path, None, **kw)
    ctx = clf.create_batch_context(n_max)
    out = clf.predict_logits(ctx, segs)
    info = (clf.weight_summary(), clf.layer_terms(), clf.fused_blocks())
    ctx.close(); clf.close()
    return out, info


@pytest.mark.parametrize("kind", ["birdnet_v30", "perch_v2_tiny", "birdnet_v24", "fused0", "fused1", "fused2", "bn"])
def test_float16_file_on_the_device(tmp_path, kind):
    m, p32, p16, bhm = _files(tmp_path, kind)
    conv = mf.read_model(bhm)
    segs = synth.synth_segments(300, m.sample_count, m.sample_rate, start=41)
    ref = O.OracleModel(bhm).forward(segs[:3])
    scale = max(1.0, float(np.abs(ref).max()))
    n_blocks = sum(1 for L in m.layers if L.op == mf.OP_DWCONV)
    for prec in ("f32", "f16x3", "auto"):
        got, (ws, terms, fused) = _logits(p16, segs[:3], 4, precision=prec)
        err = float(np.abs(got - ref).max())
        print(f"{kind} {prec}: max |dlogit| {err:.3e} of {scale:.3f}; {ws}")
        assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale, (kind, prec, err, scale)
        assert ws["float16_file"] == 1 and len(fused) == len(_logits_fused_ref(m, p32, prec)), (kind, prec)
        if kind != "bn":
            assert len(fused) == n_blocks, (kind, prec, len(fused), n_blocks)       # every MBConv block still fused
        if prec == "f32":
            assert ws["two_term_layers"] == 0 and ws["gemm_layers"] == 0 and not any(terms)
            continue
        # the rule, restated on the container's values: a layer with operand planes runs two terms iff its weights are f16 values
        want2 = []
        for i, L in enumerate(conv.layers):
            if terms[i] == 0:
                continue
            nw = {mf.OP_CONV: L.kh * L.kw * L.cin * L.cout, mf.OP_PWCONV: L.cin * L.cout, mf.OP_DENSE: L.cin * L.cout}[L.op]
            w = np.asarray(conv.blob[L.w_off:L.w_off + nw])
            want2.append(bool(np.array_equal(_f16(w), w)))
            assert terms[i] == (2 if want2[-1] else 3), (kind, i, terms[i])
        assert ws["gemm_layers"] == len(want2) >= 2 and ws["two_term_layers"] == sum(want2)
        if kind == "bn":
            assert 0 < sum(want2) < len(want2), want2            # the folded layers stay on three terms, the dense layer takes two
        else:
            assert all(want2)
    # two terms against full planes: plane bytes, and the same numbers at 3, 80 and 300 segments
    two, (ws2, t2, _) = _logits(p16, segs, 300, precision="auto")
    full, (ws3, t3, _) = _logits(p16, segs, 300, precision="auto", full_planes=True)
    assert ws3["two_term_layers"] == 0 and ws3["gemm_layers"] == ws2["gemm_layers"] and 2 not in t3
    assert ws3["plane_bytes"] - ws2["plane_bytes"] == ws2["two_term_plane_bytes"]        # half of the full planes of those layers
    _same_numbers(two, full, (kind, 300))
    for n in (3, 80):
        a, _ = _logits(p16, segs[:n], n, precision="auto")
        b, _ = _logits(p16, segs[:n], n, precision="auto", full_planes=True)
        _same_numbers(a, b, (kind, n))
        assert np.array_equal(a, two[:n]), (kind, n)            # and a segment's bits do not depend on the launch
    # the float32 parent (He-normal weights, not f16 values): no two-term layer, and bit for bit what BH_FLAG_FULL_PLANES gives
    a, (wsa, ta, _) = _logits(p32, segs[:80], 80, precision="auto")
    b, _ = _logits(p32, segs[:80], 80, precision="auto", full_planes=True)
    assert wsa["float16_file"] == 0 and wsa["two_term_layers"] == 0 and 2 not in ta
    assert a.tobytes() == b.tobytes()


def _logits_fused_ref(m, p32, prec):
    """the fused blocks of the float32 parent under the same precision (what the float16 file must still fuse)"""
    from birda_amd.classifier import BirdClassifier
    clf = BirdClassifier(p32, None, precision=prec)
    out = clf.fused_blocks()
    clf.close()
    return out


def test_a_float32_container_of_f16_values_qualifies_too(tmp_path):
    """The rule reads values, not the file's element type: the BHM1 container converted from a float16 file (an f32 blob whose values
    happen to be f16 values) runs two terms wherever the .onnx does, and gives the same logits."""
    m, p32, p16, bhm = _files(tmp_path, "mini_hg")
    segs = synth.synth_segments(5, m.sample_count, m.sample_rate, start=3)
    a, (wsa, ta, _) = _logits(p16, segs, 8, precision="auto")
    b, (wsb, tb, _) = _logits(bhm, segs, 8, precision="auto")
    assert wsa["float16_file"] == 1 and wsb["float16_file"] == 0
    assert ta == tb and wsb["two_term_layers"] == wsa["two_term_layers"] == wsa["gemm_layers"] > 0
    assert a.tobytes() == b.tobytes()


def test_v2l_in_float16_end_to_end(tmp_path):
    m, p32, p16, bhm = _files(tmp_path, "birdnet_v30_v2l")
    os.remove(p32)
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=9)
    ref = O.OracleModel(bhm).forward(segs)
    scale = max(1.0, float(np.abs(ref).max()))
    got, (ws, terms, fused) = _logits(p16, segs, 2, precision="auto")
    err = float(np.abs(got - ref).max())
    print(f"birdnet_v30_v2l float16: max |dlogit| {err:.3e} of {scale:.3f}; {ws}; {len(fused)} fused blocks")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale, (err, scale)
    assert ws["float16_file"] == 1 and ws["two_term_layers"] == ws["gemm_layers"] > 10 and 3 not in terms


# ---- 8. the small-call path -----------------------------------------------------------------------------------------------------
def test_one_segment_under_low_latency_takes_the_two_term_skinny_kernel(tmp_path):
    from birda_amd.classifier import BirdClassifier
    m, p32, p16, bhm = _files(tmp_path, "birdnet_v30")
    segs = synth.synth_segments(1, m.sample_count, m.sample_rate, start=13)
    ref = O.OracleModel(bhm).forward(segs)
    scale = max(1.0, float(np.abs(ref).max()))
    clf = BirdClassifier(p16, None, precision="auto", low_latency=True)
    ctx = clf.create_batch_context(1)
    got = clf.predict_logits(ctx, segs)
    dense = len(m.layers) - 1
    name = clf.layer_kernel(dense)
    ctx.close(); clf.close()
    assert name.startswith("pw_gemm16_skinny_kernel<2,"), name
    assert float(np.abs(got - ref).max()) <= LOGIT_RTOL * scale
