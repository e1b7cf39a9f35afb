"""The float64 references tests/test_layer_gemm_gpu.py holds the layer kernels to (oracle/oracle.py: im2col_nhwc, conv_nhwc64,
gemm64, head_pool64, act64), held in turn to PyTorch on the CPU in float64 -- so that a wrong reference cannot let a wrong kernel
pass.  The convolution is checked over random shapes with asymmetric padding, a bottom / right padding larger than the kernel and a
negative one (a crop), against F.conv2d on the F.pad-ed NCHW input."""
import math

import numpy as np
import pytest

from oracle import oracle as O

torch = pytest.importorskip("torch")
F = torch.nn.functional


def _torch_conv(X, W, bias, sh, sw, pad_t, pad_l, out_h, out_w):
    n, in_h, in_w, cin = X.shape
    kh, kw, _, cout = W.shape
    pad_b = (out_h - 1) * sh + kh - in_h - pad_t
    pad_r = (out_w - 1) * sw + kw - in_w - pad_l
    x = F.pad(torch.from_numpy(X).permute(0, 3, 1, 2), (pad_l, pad_r, pad_t, pad_b))
    y = F.conv2d(x, torch.from_numpy(W).permute(3, 2, 0, 1), torch.from_numpy(bias), stride=(sh, sw))
    assert tuple(y.shape) == (n, cout, out_h, out_w)
    return y.permute(0, 2, 3, 1).reshape(-1, cout).numpy()


def _shapes():
    rng = np.random.default_rng(11)
    out = [  # (n, in_h, in_w, cin, cout, kh, kw, sh, sw, pad_t, pad_l, out_h, out_w)
        (2, 6, 9, 4, 3, 3, 3, 2, 2, 0, 0, 3, 5),      # stride-2 SAME: pad_t 0, pad_b 1
        (1, 2, 3, 5, 2, 7, 7, 1, 1, 3, 3, 2, 3),      # the kernel larger than the image
        (3, 5, 5, 2, 4, 4, 4, 1, 1, 3, 0, 5, 2),      # even kernel, pad_t 3, pad_r negative (a crop)
        (1, 4, 1, 3, 2, 3, 3, 1, 1, 3, 1, 4, 1),      # a one-pixel-wide image; a whole row of taps above it
        (1, 7, 6, 2, 2, 2, 2, 2, 2, 0, 0, 3, 3),      # 2x2 s2 VALID (pad_b = -1: the last row is cropped)
    ]
    for _ in range(20):
        kh, kw = (int(v) for v in rng.integers(1, 8, 2))
        sh, sw = (int(v) for v in rng.integers(1, 3, 2))
        in_h, in_w = (int(v) for v in rng.integers(1, 12, 2))
        pad_t, pad_l = int(rng.integers(0, kh + 2)), int(rng.integers(0, kw + 2))
        out_h = max(1, (in_h + pad_t + int(rng.integers(-2, kh + 2)) - kh) // sh + 1)
        out_w = max(1, (in_w + pad_l + int(rng.integers(-2, kw + 2)) - kw) // sw + 1)
        out.append((int(rng.integers(1, 4)), in_h, in_w, int(rng.integers(1, 6)), int(rng.integers(1, 5)), kh, kw, sh, sw,
                    pad_t, pad_l, out_h, out_w))
    return out


@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: "n%d_%dx%d_c%d-%d_k%dx%d_s%dx%d_p%d,%d_o%dx%d" % s)
def test_conv_reference_matches_torch(shape):
    n, in_h, in_w, cin, cout, kh, kw, sh, sw, pad_t, pad_l, out_h, out_w = shape
    pad_b = (out_h - 1) * sh + kh - in_h - pad_t
    pad_r = (out_w - 1) * sw + kw - in_w - pad_l
    if in_h + pad_t + pad_b < kh or in_w + pad_l + pad_r < kw or -pad_b >= in_h or -pad_r >= in_w:
        pytest.skip("F.pad / F.conv2d cannot express this crop")   # (the shapes below avoid it; kept honest if _shapes changes)
    rng = np.random.default_rng(sum(shape))
    X = rng.standard_normal((n, in_h, in_w, cin))
    W = rng.standard_normal((kh, kw, cin, cout))
    b = rng.standard_normal(cout)
    pre, A = O.conv_nhwc64(X, W, b, sh, sw, pad_t, pad_l, out_h, out_w)
    assert A.shape == (n * out_h * out_w, kh * kw * cin)
    np.testing.assert_allclose(pre, _torch_conv(X, W, b, sh, sw, pad_t, pad_l, out_h, out_w), rtol=1e-12, atol=1e-12)


def test_conv_reference_pads_by_hand():
    """One element of a 3x3 stride-2 SAME output worked out by hand: the bottom-right output's taps past the image are zero."""
    X = np.arange(1, 1 + 4 * 4 * 1, dtype=np.float64).reshape(1, 4, 4, 1)
    W = np.ones((3, 3, 1, 1))
    pre, _ = O.conv_nhwc64(X, W, np.zeros(1), 2, 2, 0, 0, 2, 2)    # SAME at stride 2 on 4x4: pad_t 0, pad_b 1
    assert pre[3, 0] == X[0, 2:4, 2:4, 0].sum()
    assert pre[0, 0] == X[0, 0:3, 0:3, 0].sum()


def test_gemm_and_pool_references():
    rng = np.random.default_rng(3)
    A, W, b = rng.standard_normal((30, 7)), rng.standard_normal((7, 5)), rng.standard_normal(5)
    ref = torch.addmm(torch.from_numpy(b), torch.from_numpy(A), torch.from_numpy(W)).numpy()
    np.testing.assert_allclose(O.gemm64(A, W, b), ref, rtol=1e-13, atol=1e-13)
    v = rng.standard_normal((6 * 5, 4))
    want = F.adaptive_avg_pool2d(torch.from_numpy(v).reshape(6, 5, 4).permute(0, 2, 1).unsqueeze(-1), 1).reshape(6, 4).numpy()
    np.testing.assert_allclose(O.head_pool64(v, 5), want, rtol=1e-14, atol=1e-15)


def _act_points():
    grid = np.linspace(-16.0, 16.0, 4097)
    mags = np.logspace(-30, 30, 121)
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38])
    edges = np.array([np.nextafter(np.float32(6), np.float32(0)), 6.0, np.nextafter(np.float32(6), np.float32(7))], np.float64)
    return np.concatenate([grid, mags, -mags, tiny, edges])


@pytest.mark.parametrize("act", [O.ACT_NONE, O.ACT_RELU, O.ACT_RELU6, O.ACT_SWISH, O.ACT_GELU_ERF, O.ACT_GELU_TANH, O.ACT_SIGMOID],
                         ids=lambda a: O.ACT_NAMES[a])
def test_activation_references_match_torch(act):
    v = _act_points()
    t = torch.from_numpy(v)
    want = {O.ACT_NONE: lambda x: x.clone(), O.ACT_RELU: F.relu, O.ACT_RELU6: F.relu6, O.ACT_SWISH: F.silu,
            O.ACT_GELU_ERF: F.gelu, O.ACT_GELU_TANH: lambda x: F.gelu(x, approximate="tanh"), O.ACT_SIGMOID: torch.sigmoid}[act](t).numpy()
    got = O.act64(v, act)
    assert got.dtype == np.float64 and np.isfinite(got).all()
    # relative to max(|v|, 1): the scale the device tolerances are stated at; tiny arguments compared absolutely as well
    err = np.abs(got - want) / np.maximum(np.abs(v), 1.0)
    assert err.max() <= 1e-14, (O.ACT_NAMES[act], float(v[np.argmax(err)]), float(err.max()))
    if act in (O.ACT_NONE, O.ACT_RELU, O.ACT_RELU6):
        assert np.array_equal(got, want)


def test_gelu_reference_points():
    """Textbook values, independent of both libraries: GELU(1) = Phi(1), GELU(-1) = -Phi(-1), swish(1) = 1 / (1 + e^-1)."""
    phi1 = 0.5 * (1.0 + math.erf(1.0 / math.sqrt(2.0)))
    assert abs(O.act64(1.0, O.ACT_GELU_ERF) - 0.8413447460685429) < 1e-15 and abs(phi1 - 0.8413447460685429) < 1e-15
    assert abs(O.act64(-1.0, O.ACT_GELU_ERF) + 0.15865525393145707) < 1e-15
    assert abs(O.act64(1.0, O.ACT_SWISH) - 1.0 / (1.0 + math.exp(-1.0))) < 1e-16
    assert O.act64(-1e30, O.ACT_SWISH) == 0.0 and O.act64(1e30, O.ACT_GELU_TANH) == 1e30


# ---------------------------------------------------------------------------------------------------------------------------
# the fused MBConv block's reference (O.mbconv64: tests/test_mbconv_block_gpu.py holds mbconv_kernel to it)
# ---------------------------------------------------------------------------------------------------------------------------
def _torch_act(v, act):
    if act == O.ACT_RELU6:
        return torch.clamp(v, 0.0, 6.0)
    if act == O.ACT_SWISH:
        return v * torch.sigmoid(v)
    assert act == O.ACT_GELU_ERF
    return F.gelu(v)


def _torch_mbconv(X, We, be, Wd, bd, Wp, bp, R, ks, st, pad_t, pad_l, out_h, out_w, act, noexp, gate, stem):
    t = torch.from_numpy
    if stem is not None:
        k, s, spt, spl, H, W = stem
        c = X.shape[1]
        pad_b, pad_r = (H - 1) * s + k - X.shape[2] - spt, (W - 1) * s + k - X.shape[3] - spl
        w = t(We).reshape(k, k, c, -1).permute(3, 2, 0, 1)
        e = _torch_act(F.conv2d(F.pad(t(X), (spl, pad_r, spt, pad_b)), w, t(be), stride=s), act)
    elif noexp:
        e = t(X).permute(0, 3, 1, 2)
    else:
        e = _torch_act(F.conv2d(t(X).permute(0, 3, 1, 2), t(We).T[:, :, None, None], t(be)), act)
    cexp = e.shape[1]
    pad_b, pad_r = (out_h - 1) * st + ks - e.shape[2] - pad_t, (out_w - 1) * st + ks - e.shape[3] - pad_l
    wd = t(Wd).reshape(ks, ks, cexp).permute(2, 0, 1)[:, None]
    d = _torch_act(F.conv2d(F.pad(e, (pad_l, pad_r, pad_t, pad_b)), wd, t(bd), stride=st, groups=cexp), act)
    dsum = d.sum(dim=(2, 3))
    dg = d if gate is None else d * t(gate)[:, :, None, None]
    y = F.conv2d(dg, t(Wp).T[:, :, None, None], t(bp)).permute(0, 2, 3, 1)
    if R is not None:
        y = y + t(R)
    return e.permute(0, 2, 3, 1).numpy(), d.permute(0, 2, 3, 1).numpy(), y.numpy(), dsum.numpy()


MB_REF_CASES = [  # (form, n, H, W, Cin, Cexp, Cout, ks, st, pad_t, pad_l, Ho, Wo, residual)
    ("plain", 2, 7, 9, 8, 24, 12, 3, 1, 1, 1, 7, 9, True),
    ("plain", 1, 8, 10, 4, 12, 20, 3, 2, 0, 0, 4, 5, False),        # stride-2 SAME on an even image: pad_t 0, pad_b 1
    ("plain", 3, 9, 11, 12, 20, 8, 5, 2, 2, 2, 5, 6, False),        # 5x5 stride 2 on an odd image
    ("plain", 1, 5, 6, 4, 8, 8, 5, 1, 2, 2, 5, 6, True),
    ("noexp", 2, 6, 7, 16, 16, 8, 3, 1, 1, 1, 6, 7, True),
    ("gated", 2, 6, 7, 16, 16, 12, 3, 1, 1, 1, 6, 7, False),
    ("gated", 3, 7, 7, 8, 8, 8, 5, 2, 1, 1, 3, 3, True),            # stride 2, pad_b = 0 by TF's SAME rule on 7 rows of 5x5 taps
    ("stem1", 2, 0, 0, 1, 16, 8, 3, 1, 1, 1, 0, 0, False),
    ("stem2", 2, 0, 0, 2, 12, 8, 3, 1, 1, 1, 0, 0, False),
    ("stem3", 1, 0, 0, 3, 8, 4, 3, 2, 0, 0, 0, 0, False),
]


@pytest.mark.parametrize("act", [O.ACT_GELU_ERF, O.ACT_SWISH, O.ACT_RELU6], ids=lambda a: O.ACT_NAMES[a])
@pytest.mark.parametrize("case", MB_REF_CASES, ids=lambda c: "%s_n%d_%dx%d_%d-%d-%d_k%ds%d_p%d,%d_o%dx%d_r%d" % c)
def test_mbconv_reference_matches_torch(case, act):
    form, n, H, W, Cin, Cexp, Cout, ks, st, pad_t, pad_l, Ho, Wo, residual = case
    rng = np.random.default_rng(1000 * MB_REF_CASES.index(case) + act)
    stem = None
    if form.startswith("stem"):
        c, sh, sw, ss = Cin, 11, 14, 2                    # an 11x14 spectrogram, stem stride 2 with TF's SAME padding (pad_t 1)
        H, W = -(-sh // ss), -(-sw // ss)
        spt, spl = max((H - 1) * ss + 3 - sh, 0) // 2, max((W - 1) * ss + 3 - sw, 0) // 2
        stem = (3, ss, spt, spl, H, W)
        X = rng.standard_normal((n, c, sh, sw))
        Cin = 9 * c
        Ho, Wo = -(-H // st), -(-W // st)
    else:
        X = rng.standard_normal((n, H, W, Cin))
    noexp = form in ("noexp", "gated")
    We, be = rng.standard_normal((Cin, Cexp)) * 0.3, rng.standard_normal(Cexp)
    Wd, bd = rng.standard_normal((ks * ks, Cexp)) * 0.4, rng.standard_normal(Cexp) * 3
    Wp, bp = rng.standard_normal((Cexp, Cout)) * 0.3, rng.standard_normal(Cout)
    R = rng.standard_normal((n, Ho, Wo, Cout)) if residual else None
    gate = rng.uniform(0.0, 1.0, (n, Cexp)) if form == "gated" else None
    got = O.mbconv64(X, We, be, Wd, bd, Wp, bp, R, ks, st, pad_t, pad_l, Ho, Wo, act, noexp=noexp, gate=gate, stem=stem)
    e, d, y, dsum = _torch_mbconv(X, We, be, Wd, bd, Wp, bp, R, ks, st, pad_t, pad_l, Ho, Wo, act, noexp, gate, stem)
    for name, a, b in (("E", got["E"], e), ("D", got["D"], d), ("Y", got["Y"], y), ("Dsum", got["Dsum"], dsum)):
        assert a.shape == b.shape, name
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12, err_msg=name)


def test_depthwise_reference_by_hand():
    """A 3x3 stride-2 depthwise output worked out by hand, SAME on 4x4 (pad_t 0, pad_b 1): taps past the image are zero, and tap
    (dy, dx) is row dy * 3 + dx of Wd."""
    E = np.arange(1, 17, dtype=np.float64).reshape(1, 4, 4, 1)
    Wd = np.arange(1, 10, dtype=np.float64).reshape(9, 1)
    out = O.depthwise64(E, Wd, 3, 2, 0, 0, 2, 2)
    assert out[0, 0, 0, 0] == sum(E[0, dy, dx, 0] * Wd[dy * 3 + dx, 0] for dy in range(3) for dx in range(3))
    assert out[0, 1, 1, 0] == sum(E[0, 2 + dy, 2 + dx, 0] * Wd[dy * 3 + dx, 0] for dy in range(2) for dx in range(2))
