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
