"""Norm + activation layers (OP_BNACT) on the device.

bnact_kernel through bh_debug_bnact (include/birda_hip_bnact_debug.h), every output element against float64 on the f32 operands.  With
v = x scale + shift in float64 and y = act(v):

    ReLU, ReLU6      |got - y| <= 2^-24 |v| (1 + 2^-20)                        one FMA rounding; the clamps are exact
    the others       |got - y| <= 1.5 * 2^-24 |v| + _eps_act(v, act)           1.5: the largest slope among them (hard swish's); _eps_act is
                                                                               tests/test_layer_gemm_gpu.py's allowance for the function itself
    hard swish       ... + 3 * 2^-24 |y|                                        its three roundings

at C in {4, 20, 64, 2208} x 1 and 35 pixels, and at C = 4 x 524 288 + 37 pixels -- one past the launcher's grid cap of 2 048 x 256
threads, the grid-stride loop's second trip --, for every activation of the record's set.  A NaN element makes exactly its own output
NaN, +inf under ReLU with a positive scale stays +inf, -inf gives 0, inf times a zero scale NaN; the guard bands stay and every element
is written (the entry point's own check); a pixel's bits are the same at 1, 3 and 64 segments; what the record refuses the entry refuses.

At model level synth's dense_plan seeds (every activation) run in auto, f32, f16x3 and f16 through the .onnx route -- the concats as the
growing list -- and the .bhm route to the same bits (the container the library's reader writes of that file, held to synth's records and
weights field for field; synth's own container runs too, to the tolerance), within LOGIT_RTOL (F16_LOGIT_RTOL in f16) of tests/test_bnact.py's forward64; for one
seed every tensor of a keep-tensors context is held to the float64 forward's, and every norm + activation tensor to the kernel's own
bound on its input tensor read back.  An f16 overflow in front of a norm + activation layer ends in BH_ERR_NONFINITE (f16x3) and is
re-run on the f32 kernels (auto), which the provider status records.

Measured on the MI355X, worst err / tolerance (every test prints its own): see DESIGN.md, "Norm + activation layers"."""
import copy
import ctypes as C

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from test_bnact import B, RECORD, _blocks, bnact64, forward64
from test_layer_gemm_gpu import _eps_act
from test_resact_gpu import BH_ERR_NONFINITE, F16_LOGIT_RTOL, LOGIT_RTOL

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
BH_ERR_INVALID, BH_ERR_UNSUPPORTED = -1, -6
U = 2.0 ** -24
KERNEL = "bnact_kernel"
GRID_CAP_THREADS = 2048 * 256                     # launch_bnact: at most eight workgroups of 256 threads a CU's worth of a 256-CU chip
SHAPES = [(c, p) for c in (4, 20, 64, 2208) for p in (1, 35)] + [(4, GRID_CAP_THREADS + 37)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_bnact(X, scale, shift, act, expect=0):
    lib = _lib.load()
    n, C_ = X.shape
    out = np.empty((n, C_), np.float32)
    name = C.create_string_buffer(b"untouched", 128)
    rc = lib.bh_debug_bnact(0, _p(X), _p(scale), _p(shift), act, _p(out), n, C_, name, 128)
    if expect:
        assert rc == expect and name.value == b"untouched", (rc, lib.bh_last_error())
        return None, lib.bh_last_error().decode()
    assert rc == 0, (rc, lib.bh_last_error())
    assert not (out.view(np.uint32) == UNWRITTEN).any(), "elements never written"       # (the guards are checked by the entry itself)
    return out, name.value.decode()


def operands(C_, pixels, seed=0):
    rng = np.random.default_rng(1000 * C_ + pixels % 1000 + seed)
    X = (3.0 * rng.standard_normal((pixels, C_))).astype(np.float32)
    scale = (1.0 + 0.5 * rng.standard_normal(C_)).astype(np.float32)
    i0, i1, i2 = (int(v) for v in rng.choice(C_, 3, replace=False))
    scale[i0] = 0.0
    scale[i1] = -abs(scale[i1]) - np.float32(0.5)
    scale[i2] = np.float32(40.0)
    shift = rng.standard_normal(C_).astype(np.float32)
    return X, scale, shift


def tolerance(v, y, act):
    """the bound of the module's docstring, element by element"""
    if act in (mf.ACT_RELU, mf.ACT_RELU6):
        return U * np.abs(v) * (1.0 + 2.0 ** -20)
    tol = 1.5 * U * np.abs(v) + _eps_act(v, act)
    return tol + 3.0 * U * np.abs(y) if act == mf.ACT_HSWISH else tol


@pytest.mark.parametrize("act", mf.BNACT_ACTS)
@pytest.mark.parametrize("C_,pixels", SHAPES)
def test_bnact_against_float64(C_, pixels, act):
    X, scale, shift = operands(C_, pixels)
    got, name = run_bnact(X, scale, shift, act)
    assert name == KERNEL, name
    v = X.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)
    ref = bnact64(X, scale, shift, act)
    tol = tolerance(v, ref, act)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    share = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"bnact C {C_} pixels {pixels} act {act} {name}: worst err / tol {share:.3f}")
    if share > 1.0:
        i = np.unravel_index(np.argmax(err / np.maximum(tol, 1e-300)), err.shape)
        pytest.fail(f"C {C_} pixels {pixels} act {act}: {int((err > tol).sum())} of {err.size} elements off, worst at {i}: got {got[i]!r} want {ref[i]!r}, "
                    f"err {err[i]:.3e} > tol {tol[i]:.3e}")


@pytest.mark.parametrize("act", mf.BNACT_ACTS)
def test_non_finite_elements_stay_where_they_are(act):
    C_ = 20
    X, scale, shift = operands(C_, 35)
    scale[:] = np.abs(scale) + np.float32(0.25)             # positive scales ...
    scale[7] = 0.0                                         # ... and one exact zero
    scale[9] = np.float32(-1.5)
    clean, _ = run_bnact(X, scale, shift, act)
    Xn = X.copy()
    Xn[3, 5] = np.nan
    Xn[10, 2] = np.inf
    Xn[11, 4] = -np.inf
    Xn[12, 7] = np.inf                                     # inf * 0
    Xn[13, 9] = np.inf                                     # a negative scale: -inf
    Xn[34, C_ - 1] = np.nan
    got, _ = run_bnact(Xn, scale, shift, act)
    touched = np.zeros(X.shape, bool)
    for i in ((3, 5), (10, 2), (11, 4), (12, 7), (13, 9), (34, C_ - 1)):
        touched[i] = True
    assert (got.view(np.uint32)[~touched] == clean.view(np.uint32)[~touched]).all()      # no other element
    assert np.isnan(got[3, 5]) and np.isnan(got[34, C_ - 1]) and np.isnan(got[12, 7])
    top = np.float32(6.0) if act == mf.ACT_RELU6 else np.float32(np.inf)
    assert got[10, 2] == top, got[10, 2]                   # act(+inf) = +inf (ReLU6: its upper limit)
    assert got[11, 4] == 0.0 and got[13, 9] == 0.0         # act(-inf) = 0


def test_a_pixel_does_not_depend_on_its_launch():
    """35 pixels a segment: 3 and 64 segments made of one repeated equal the one, bit for bit, with ReLU and with swish"""
    for C_ in (20, 2208):
        X, scale, shift = operands(C_, 35)
        for act in (mf.ACT_RELU, mf.ACT_SWISH):
            one, _ = run_bnact(X, scale, shift, act)
            for n in (3, 64):
                big, _ = run_bnact(np.ascontiguousarray(np.tile(X, (n, 1))), scale, shift, act)
                assert (big.view(np.uint32).reshape(n, 35, C_) == one.view(np.uint32)).all(), (C_, act, n)
            assert not np.array_equal(one[0], one[1])


def test_the_entry_refuses_what_the_record_refuses():
    ones, zeros = np.ones(8, np.float32), np.zeros(8, np.float32)
    X = np.zeros((3, 8), np.float32)
    for act in (mf.ACT_NONE, mf.ACT_SIGMOID, mf.ACT_HSIGMOID, 9, -1):
        _, msg = run_bnact(X, ones, zeros, act, expect=BH_ERR_INVALID)
        assert "activation" in msg, msg
    for C_ in (6, 65540):
        _, msg = run_bnact(np.zeros((1, C_), np.float32), np.ones(C_, np.float32), np.zeros(C_, np.float32), mf.ACT_RELU, expect=BH_ERR_UNSUPPORTED)
        assert "not built" in msg, msg


# ---------------------------------------------------------------------------------------------------------------------------
# the product path
# ---------------------------------------------------------------------------------------------------------------------------
def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


SEEDS = (0, 1, 3, 5, 7, 9)           # ReLU, ReLU6, swish, GELU (erf), GELU (tanh), hard swish
_PLAN_REF = {}


def _plan(seed):
    """-> (model, segments, float64 tensors): computed once, shared by the tests below"""
    if seed not in _PLAN_REF:
        m = synth.build_model("dense_plan", plan=synth.random_dense_plan(seed))
        segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=5 + seed)
        segs[2] *= np.float32(0.01)
        _PLAN_REF[seed] = (m, segs, forward64(m, segs, tensors=True))
    return _PLAN_REF[seed]


def _names(clf, m, what):
    for i, L in enumerate(m.layers):
        if L.op == B:
            assert clf.layer_kernel(i) == KERNEL, (what, i, clf.layer_kernel(i))


@pytest.mark.parametrize("seed", SEEDS)
def test_dense_plans_on_both_routes(seed, tmp_path):
    from birda_amd.classifier import BirdClassifier
    m, segs, T = _plan(seed)
    ref = T[-1].reshape(3, -1)
    scale = max(1.0, float(np.abs(ref).max()))
    # the .onnx route: the concats as the growing list; the .bhm route: the container the library's reader writes of that file -- the same
    # records and the same front end, so the same bits -- and synth's own container, written by modelfile.py without either reader: its
    # records and weights are the file's, field for field and bit for bit, its mel matrix differs in the last bit (each reader recovers
    # it from the graph), so it is held to the tolerance, not to the bits
    onnx = _write(str(tmp_path / "d.onnx"), convert.model_to_onnx(m, frontend_spelling="stft", spell_concat="list"))
    bhm, own = str(tmp_path / "d.bhm"), str(tmp_path / "own.bhm")
    assert _lib.load().bh_onnx_to_bhm(onnx.encode(), bhm.encode()) == 0, _lib.load().bh_last_error()
    read = mf.read_model(bhm)
    assert len(read.layers) == len(m.layers)
    for i, (x, y) in enumerate(zip(m.layers, read.layers)):
        assert all(getattr(x, f) == getattr(y, f) for f in RECORD[:-2]), (i, x, y)
        nw = {mf.OP_CONV: x.kh * x.kw * x.cin * x.cout, mf.OP_DWCONV: x.kh * x.kw * x.cout, mf.OP_PWCONV: x.cin * x.cout, mf.OP_DENSE: x.cin * x.cout, B: x.cout}.get(x.op, 0)
        assert m.blob[x.w_off:x.w_off + nw].tobytes() == read.blob[y.w_off:y.w_off + nw].tobytes(), (i, "weights")
        if nw:
            assert m.blob[x.b_off:x.b_off + x.cout].tobytes() == read.blob[y.b_off:y.b_off + x.cout].tobytes(), (i, "bias")
    mf.write_model(own, m)
    for prec, tol in (("auto", LOGIT_RTOL), ("f32", LOGIT_RTOL), ("f16x3", LOGIT_RTOL), ("f16", F16_LOGIT_RTOL)):
        first = None
        for route, path in (("onnx", onnx), ("bhm", bhm), ("own", own)):
            clf = BirdClassifier(path, None, precision=prec)
            ctx = clf.create_batch_context(3)
            got = clf.predict_logits(ctx, segs)
            ctx.close()
            if first is None:
                first = got
                err = float(np.abs(got - ref).max())
                print(f"dense plan {seed} (act {m.layers[-3].act}) {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (tol * scale):.3f})")
                assert np.isfinite(got).all() and err <= tol * scale, (prec, err, scale)
            elif route == "own":
                err = float(np.abs(got - ref).max())
                print(f"dense plan {seed} {prec}, synth's container: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (tol * scale):.3f})")
                assert np.isfinite(got).all() and err <= tol * scale, (prec, err, scale)
            else:
                assert (got.view(np.uint32) == first.view(np.uint32)).all(), (prec, route)
            _names(clf, m, (seed, prec, route))
            clf.close()


def test_every_tensor_of_a_dense_plan(tmp_path, monkeypatch):
    """BIRDA_HIP_KEEP_TENSORS, f32: every tensor outside a fused block, read back, is within LOGIT_RTOL of its own scale of the float64
    forward's; every norm + activation tensor is bnact64 of its INPUT tensor read back the same way, under the kernel's own bound"""
    from birda_amd.classifier import BirdClassifier
    m, segs, T = _plan(3)
    path = str(tmp_path / "k.bhm")
    mf.write_model(path, m)
    inner = {f + k for flags in (0, 1, 2, 3) for f in _blocks(path, flags) for k in (1, 2)}     # the outputs of a fused block's first two layers
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    clf = BirdClassifier(path, None, precision="f32")
    ctx = clf.create_batch_context(3)
    clf.predict_logits(ctx, segs)
    worst_t, worst_k = 0.0, 0.0
    for i, L in enumerate(m.layers):
        if i + 1 in inner:
            continue
        Y = clf.read_tensor(ctx, i + 1, 3).astype(np.float64)
        want = np.asarray(T[i + 1]).reshape(3, -1)
        share = float(np.abs(Y - want).max()) / (LOGIT_RTOL * max(1.0, float(np.abs(want).max())))
        worst_t = max(worst_t, share)
        assert share <= 1.0, (i, L.op, share)
        if L.op == B and L.in_tensor not in inner:
            X = clf.read_tensor(ctx, L.in_tensor, 3).reshape(-1, L.cout)
            sc, sh = m.blob[L.w_off:L.w_off + L.cout], m.blob[L.b_off:L.b_off + L.cout]
            v = X.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)
            ref = bnact64(X, sc, sh, L.act)
            k = float(np.max(np.abs(Y.reshape(ref.shape) - ref) / np.maximum(tolerance(v, ref, L.act), 1e-300)))
            worst_k = max(worst_k, k)
            assert k <= 1.0, (i, k)
    print(f"dense plan 3, kept tensors: worst tensor err / (LOGIT_RTOL scale) {worst_t:.3f}; worst norm + activation err / tol {worst_k:.3f}")
    ctx.close(); clf.close()


def test_f16_overflow_in_front_of_a_norm_activation_layer_reaches_the_logits(tmp_path):
    """tests/test_convnext_gpu.py's recipe with a norm + activation layer behind it: a LINEAR convolution whose weights and bias carry 2^20
    (its output is past 65 504) in front of a convolution whose weights carry 2^-20 -- the same function in f32 arithmetic.  The split-f16
    kernel cannot represent its operand, and the non-finite values it writes must pass THROUGH relu(x scale + shift) to the logits: f16x3
    ends in BH_ERR_NONFINITE, auto re-runs the rows on the f32 kernels and says so in the provider status."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    b = synth._Builder(np.random.default_rng(13))
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    t1, h, w = b.conv(0, br.n_mels, br.n_frames, 1, 72, 3, 2, mf.ACT_GELU_ERF, in_layout=1)
    t2, h, w = b.conv(t1, h, w, 72, 72, 3, 1, mf.ACT_NONE)
    t3, h, w = b.conv(t2, h, w, 72, 72, 3, 1, mf.ACT_NONE, res=t1, gain=0.5)        # a residual sum: what a pre-activation block hands on
    t = b.bnact(t3, h, w, 72, mf.ACT_RELU)
    t = b.pwconv(t, h, w, 72, 64, mf.ACT_GELU_ERF)
    t = emb = b.gap(t, h, w, 64)
    b.dense(t, 64, 30, gain=1.5)
    m0 = mf.Model(0, sr, n, n / sr, 30, 64, mf.OUT_SIGMOID, emb, br.n_mels, br.n_frames, 1e-6, [br], b.layers, np.concatenate(b.chunks))
    m = copy.deepcopy(m0)
    blob = m.blob.copy()
    Lin, Nx = m.layers[1], m.layers[2]
    s = np.float32(2.0 ** 20)
    blob[Lin.w_off:Lin.w_off + Lin.kh * Lin.kw * Lin.cin * Lin.cout] *= s
    blob[Lin.b_off:Lin.b_off + Lin.cout] *= s
    blob[Nx.w_off:Nx.w_off + Nx.kh * Nx.kw * Nx.cin * Nx.cout] /= s
    m.blob = blob
    path = str(tmp_path / "overflow.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(4, m.sample_count, m.sample_rate, start=8)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    assert np.abs(ref - forward64(m0, segs)).max() <= 1e-9 * scale
    clf = BirdClassifier(path, None, precision="f16x3")
    ctx = clf.create_batch_context(4)
    with pytest.raises(BirdaHipError) as e:
        clf.predict_batch_with_context(ctx, list(segs))
    assert e.value.code == BH_ERR_NONFINITE
    assert clf.layer_kernel(2).startswith("conv_gemm16_kernel<3,NONE"), clf.layer_kernel(2)
    assert clf.layer_kernel(3) == KERNEL
    ctx.close(); clf.close()
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(4)
    got = clf.predict_logits(ctx, segs)
    assert clf.fallback_segments() > 0 and b"f32 kernels" in clf.provider_status().fallback_reason
    err = float(np.abs(got - ref).max())
    print(f"overflow in front of a norm + activation layer, auto: max|dlogit| = {err:.3e} of {scale:.2f}, {clf.fallback_segments()} segments re-run")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    ctx.close(); clf.close()


def test_densenet_audio_runs_and_matches_float64(tmp_path):
    """synth's timing model at 40 classes, two segments in auto, from its list-spelled .onnx file: finite logits at LOGIT_RTOL of the
    float64 forward, bnact_kernel at every one of its 62 norm + activation layers and a two-source concat a dense layer"""
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("densenet_audio", n_classes=40)
    path = _write(str(tmp_path / "densenet.onnx"), convert.model_to_onnx(m, frontend_spelling="stft", spell_concat="list"))
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=2)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(2)
    got = clf.predict_logits(ctx, segs)
    ctx.close()
    err = float(np.abs(got - ref).max())
    print(f"densenet_audio auto: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    _names(clf, m, "densenet_audio")
    clf.close()
