"""Full k x k convolutions past the stem on the device (kernels_conv.hip conv_gemm_kernel / conv_gemm16_kernel: implicit GEMM on
the MFMA), held to the plain-C oracle.

* a shape sweep of small models with one mid-network full convolution: kernels 1x3 / 3x1 / 3 / 5 / 7 and non-square, strides 1 / 2
  per axis, odd images with SAME (asymmetric) and VALID padding, 4 .. 96 input and 4 .. 384 output channels, with and without the
  residual, GELU / swish / ReLU6 / ReLU / none -- in f32, f16x3, auto (fp32 tolerance) and f16, bit-identical across launches of
  3, 80 and 300 segments;
* a full convolution's own output tensor against the oracle's;
* birdnet_v30_v2l (EfficientNetV2-L: three Fused-MBConv stages) end to end;
* a launch whose largest full-convolution tensor is past 2^31 bytes;
* seeded random_fused_plan models through the .onnx route;
* f16 overflow inside a full convolution's output: BH_ERR_NONFINITE under f16x3, the oracle's logits under auto;
* a residual on a layer whose kernel cannot add one (depthwise) is refused at create.
"""
import copy

import numpy as np
import pytest

from birda_amd import convert, modelfile as mf, onnx_io as ox, synth

pytestmark = pytest.mark.gpu

LOGIT_RTOL = 2e-5          # tests/test_parity_gpu.py: max |dlogit| <= 2e-5 max(1, max |logit|) in the f32-grade modes
F16_LOGIT_RTOL = 3e-3      # plain f16 operands
PRECISIONS = (("f32", LOGIT_RTOL), ("f16x3", LOGIT_RTOL), ("auto", LOGIT_RTOL), ("f16", F16_LOGIT_RTOL))


def _pad(n, k, s, same):
    if not same:
        return (n - k) // s + 1, 0
    out = -(-n // s)
    return out, max((out - 1) * s + k - n, 0) // 2


def conv_model(kh, kw, sh, sw, same, cin, cout, act, res, stem_stride=1, seed=5):
    """The mini front-end (one 32-mel branch, 115 frames), a 3x3 NCHW stem to `cin` channels, the full convolution under test
    (with the stem output added back when `res`), a 1x1 head, the pool and a dense layer"""
    rng = np.random.default_rng(seed)
    b = synth._Builder(rng)
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    t, h, w = b.conv(0, br.n_mels, br.n_frames, 1, cin, 3, stem_stride, mf.ACT_GELU_ERF, in_layout=1)
    oh, pt = _pad(h, kh, sh, same)
    ow, pl = _pad(w, kw, sw, same)
    wt = b.he((kh, kw, cin, cout), kh * kw * cin) * np.float32(0.5 if res else 1.0)
    L = mf.Layer(mf.OP_CONV, act, t, t if res else mf.NO_TENSOR, cin, cout, kh, kw, sh, sw, pt, pl, h, w, oh, ow, 0,
                 b.put(wt), b.put(b.bias(cout)))
    t = b.add(L)
    t = b.pwconv(t, oh, ow, cout, 64, mf.ACT_GELU_ERF)
    t = b.gap(t, oh, ow, 64)
    emb = t
    b.dense(t, 64, 30, gain=1.5)
    return mf.Model(0, sr, n, n / sr, 30, 64, mf.OUT_SIGMOID, emb, br.n_mels, br.n_frames, 1e-6, [br], b.layers,
                    np.concatenate(b.chunks))


#        kh kw sh sw same  cin cout act                res
SHAPES = [(1, 3, 1, 1, True, 4, 4, mf.ACT_GELU_ERF, True),
          (3, 1, 2, 1, True, 12, 20, mf.ACT_SWISH, False),
          (3, 3, 1, 1, True, 24, 24, mf.ACT_RELU6, True),
          (3, 3, 2, 2, True, 32, 64, mf.ACT_NONE, False),
          (3, 3, 1, 1, True, 64, 256, mf.ACT_SWISH, False),
          (5, 5, 1, 1, False, 64, 64, mf.ACT_SWISH, False),
          (5, 5, 2, 2, True, 96, 256, mf.ACT_GELU_ERF, False),
          (7, 7, 1, 1, True, 32, 32, mf.ACT_GELU_ERF, True),
          (7, 7, 2, 2, False, 12, 384, mf.ACT_RELU6, False),
          (3, 5, 1, 2, True, 4, 20, mf.ACT_NONE, False),
          (1, 1, 2, 2, False, 24, 64, mf.ACT_RELU, False),
          (3, 3, 1, 1, True, 96, 96, mf.ACT_SWISH, True),
          (5, 3, 2, 1, False, 20, 4, mf.ACT_GELU_ERF, False)]


def _ids(s):
    return f"k{s[0]}x{s[1]}_s{s[2]}{s[3]}_{'same' if s[4] else 'valid'}_{s[5]}to{s[6]}_a{s[7]}{'_res' if s[8] else ''}"


@pytest.mark.parametrize("shape", SHAPES, ids=[_ids(s) for s in SHAPES])
def test_full_convolution_shape_sweep_matches_oracle(shape, tmp_path, oracle_lib):
    from birda_amd.classifier import BirdClassifier
    m = conv_model(*shape, stem_stride=2 if shape[5] >= 64 else 1)
    path = str(tmp_path / "conv.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=21)
    segs[2] *= np.float32(0.01)
    ref = oracle_lib.OracleModel(path).forward(segs)
    scale = max(1.0, float(np.abs(ref).max()))
    for prec, tol in PRECISIONS:
        clf = BirdClassifier(path, None, precision=prec)
        first = None
        for n in (3, 80, 300):
            ctx = clf.create_batch_context(n)
            ctx.set_sub_slices(1)
            got = clf.predict_logits(ctx, np.ascontiguousarray(segs[np.arange(n) % 3]))
            ctx.close()
            if first is None:
                first = got
                err = float(np.abs(got - ref).max())
                print(f"{_ids(shape)} {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f}")
                assert np.isfinite(got).all() and err <= tol * scale, (prec, err)
            else:
                assert all((got[i] == first[i % 3]).all() for i in range(n)), (prec, n)
        clf.close()


def test_full_convolution_output_tensor_matches_oracle(tmp_path, oracle_lib, monkeypatch):
    """read_tensor on the full convolution's output (the f32 kernel: BIRDA_HIP_KEEP_TENSORS contexts) against dump_tensor"""
    from birda_amd.classifier import BirdClassifier
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    for shape in (SHAPES[4], SHAPES[7], SHAPES[9]):
        m = conv_model(*shape)
        path = str(tmp_path / "conv.bhm")
        mf.write_model(path, m)
        segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=3)
        clf = BirdClassifier(path, None, precision="f32")
        ctx = clf.create_batch_context(2)
        clf.predict_logits(ctx, segs)
        om = oracle_lib.OracleModel(path)
        for t in (1, 2):      # the stem's output (the convolution's input) and the convolution's
            ref = om.forward(segs, dump_tensor=t)[1]
            got = clf.read_tensor(ctx, t, 2)
            scale = max(1.0, float(np.abs(ref).max()))
            d = float(np.abs(got - ref).max())
            print(f"{_ids(shape)} tensor {t}: max|d| = {d:.3e} of {scale:.2f}")
            assert np.isfinite(got).all() and d <= 1e-4 * scale, (t, d)
        ctx.close(); clf.close()


def test_birdnet_v30_v2l_matches_oracle(oracle_lib, tmp_path):
    """EfficientNetV2-L on the v3.0 contract: 18 full convolutions in three Fused-MBConv stages, then 61 MBConv blocks with
    squeeze-excite, 54 of which run fused (the seven of the 640-channel stage are past the widest tile entries, as in
    birdnet_v30_sized).  Probabilities and embeddings against the oracle; bit-identical across launch sizes."""
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("birdnet_v30_v2l")
    path = str(tmp_path / "v30_v2l.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=15)
    ref, ref_emb = oracle_lib.OracleModel(path).forward(segs, want_embeddings=True)
    assert ref.min() >= 0.0 and ref.max() <= 1.0
    for prec in ("f16x3", "auto", "f32"):
        clf = BirdClassifier(path, None, top_k=5, min_confidence=0.0, precision=prec)
        blocks = clf.fused_blocks()
        print(f"v3.0 V2-L {prec}: {len(blocks)} of 61 MBConv blocks fused, {2 * clf.info.macs_per_segment / 1e9:.2f} GFLOP per segment")
        assert len(blocks) >= (54 if prec != "f32" else 40), (prec, len(blocks))
        ctx = clf.create_batch_context(2)
        got, emb = clf.predict_logits(ctx, segs, want_embeddings=True)
        err = float(np.abs(got - ref).max())
        escale = max(1.0, float(np.abs(ref_emb).max()))
        eerr = float(np.abs(emb - ref_emb).max())
        print(f"v3.0 V2-L {prec}: max |dp| = {err:.3e}, embeddings {eerr / escale:.3e} of their scale")
        assert np.isfinite(got).all() and err <= LOGIT_RTOL and eerr <= LOGIT_RTOL * escale, (prec, err, eerr)
        big = clf.create_batch_context(40)
        gb = clf.predict_logits(big, np.ascontiguousarray(np.tile(segs, (20, 1))))
        assert all((gb[i] == got[i % 2]).all() for i in range(40)), prec
        big.close()
        ctx.close(); clf.close()


def test_full_convolution_tensor_past_2_gib_keeps_a_segments_bits(tmp_path):
    """A 64 -> 256 convolution on a 32 x 115 image: 3.8 MB per segment, 600 segments in one launch = 2.26 GB, past 2^31 bytes.
    Every row bit-identical to the same segment in a launch of 3."""
    from birda_amd.classifier import BirdClassifier
    m = conv_model(3, 3, 1, 1, True, 64, 256, mf.ACT_SWISH, False)
    L = m.layers[1]
    n_big = 600
    assert n_big * L.out_h * L.out_w * L.cout * 4 > 2 ** 31
    path = str(tmp_path / "big.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=60)
    for prec in ("f16x3", "f32"):
        clf = BirdClassifier(path, None, precision=prec)
        ctx = clf.create_batch_context(3)
        small = clf.predict_logits(ctx, segs)
        ctx.close()
        ctx = clf.create_batch_context(n_big)
        ctx.set_sub_slices(1)
        got = clf.predict_logits(ctx, np.ascontiguousarray(np.tile(segs, (n_big // 3, 1))))
        ctx.close(); clf.close()
        assert np.isfinite(got).all()
        bad = [i for i in range(n_big) if not (got[i] == small[i % 3]).all()]
        assert not bad, (prec, bad[:5], len(bad))


@pytest.mark.parametrize("seed", range(9))
def test_random_fused_plans_on_the_onnx_route_match_oracle(seed, tmp_path, oracle_lib):
    """random_fused_plan: random_plan with its first one to three stages Fused-MBConv, written as `.onnx` (the residual Add of the
    expand-ratio-1 fused blocks onto a full convolution) and created from it; every MBConv block fused in f16x3"""
    from birda_amd.classifier import BirdClassifier
    plan = synth.random_fused_plan(seed)
    m = synth.build_model("custom", plan=plan)
    bhm, onnx = str(tmp_path / "p.bhm"), str(tmp_path / "p.onnx")
    mf.write_model(bhm, m)
    with open(onnx, "wb") as f:
        f.write(ox.dump(convert.graph_from_model(m, frontend_spelling="stft")))
    n_mb = sum(1 for L in m.layers if L.op == mf.OP_DWCONV)
    assert any(L.op == mf.OP_CONV and L.in_layout == 0 for L in m.layers)
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=5)
    ref = oracle_lib.OracleModel(bhm).forward(segs)
    scale = max(1.0, float(np.abs(ref).max()))
    for prec in ("f16x3", "f32"):
        clf = BirdClassifier(onnx, None, precision=prec)
        if prec == "f16x3":
            assert len(clf.fused_blocks()) == n_mb, (clf.fused_blocks(), n_mb)
        ctx = clf.create_batch_context(3)
        got = clf.predict_logits(ctx, segs)
        ctx.close(); clf.close()
        err = float(np.abs(got - ref).max())
        print(f"fused plan {seed} {plan['stages']} {prec}: max|dlogit| = {err:.3e} of {scale:.2f}")
        assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale, (prec, err)


def test_f16_overflow_in_a_full_convolution_is_marked(tmp_path, oracle_lib):
    """The full convolution's weights and bias times 2^20 (a linear layer: its output, ~1e6, is past 65 504) and the 1x1 layer
    that reads it divided by 2^20: the same function in f32 arithmetic.  f16x3 cannot represent the tensor -- BH_ERR_NONFINITE;
    auto re-runs the rows on the f32 kernels and gives the oracle's logits."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    m0 = conv_model(3, 3, 1, 1, True, 32, 64, mf.ACT_NONE, False)
    m = copy.deepcopy(m0)
    blob = m.blob.copy()
    C, P = m.layers[1], m.layers[2]
    s = np.float32(2.0 ** 20)
    blob[C.w_off:C.w_off + C.kh * C.kw * C.cin * C.cout] *= s
    blob[C.b_off:C.b_off + C.cout] *= s
    blob[P.w_off:P.w_off + P.cin * P.cout] /= s
    m.blob = blob
    p0, path = str(tmp_path / "base.bhm"), str(tmp_path / "overflow.bhm")
    mf.write_model(p0, m0)
    mf.write_model(path, m)
    segs = synth.synth_segments(4, m.sample_count, m.sample_rate, start=8)
    ref = oracle_lib.OracleModel(path).forward(segs)
    scale = max(1.0, float(np.abs(ref).max()))
    assert np.abs(ref - oracle_lib.OracleModel(p0).forward(segs)).max() <= 1e-5 * scale
    clf = BirdClassifier(path, None, precision="f16x3")
    ctx = clf.create_batch_context(4)
    with pytest.raises(BirdaHipError) as e:
        clf.predict_batch_with_context(ctx, list(segs))
    assert e.value.code == -8
    ctx.close(); clf.close()
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(4)
    got = clf.predict_logits(ctx, segs)
    assert clf.fallback_segments() > 0
    err = float(np.abs(got - ref).max())
    print(f"overflow, auto: max|dlogit| = {err:.3e}, {clf.fallback_segments()} segments re-run")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    ctx.close(); clf.close()


def test_residual_on_a_depthwise_layer_is_refused_at_create(tmp_path):
    """A BHM whose depthwise layer (outside any fused block) carries a residual: the layer kernel has no residual, and create
    refuses the model by name instead of dropping the Add."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("mini")
    i = next(i for i, L in enumerate(m.layers) if L.op == mf.OP_DWCONV and L.sh == 1 and L.in_tensor > 0
             and m.layers[L.in_tensor - 1].cout == L.cout)
    m.layers[i].res_tensor = m.layers[i].in_tensor       # dw(x) + x: the same shape
    path = str(tmp_path / "dwres.bhm")
    mf.write_model(path, m)
    for prec in ("auto", "f32"):
        with pytest.raises(BirdaHipError) as e:
            BirdClassifier(path, None, precision=prec)
        assert "residual on a depthwise layer" in str(e.value), str(e.value)
