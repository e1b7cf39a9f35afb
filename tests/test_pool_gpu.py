"""MaxPool / AveragePool on the device (kernels_pool.hip pool_kernel<MODE, K>), held to float64.

The plain-C oracle has no pool, so the reference is written here from the definition (pool64): a window's taps are the pixels of the
image it covers; max is their maximum, NaN if any of them is; the average is their sum over the count -- the taps in the image
(mode 1, count_include_pad = 0) or kh * kw (mode 2).

* element by element through bh_debug_pool: all three modes, launches of 1, 3 and 5 segments, on shapes that drop the last row, hang
  past the image, exceed it, are one pixel wide, stride past the kernel, are not square.  Max is EXACT (== as numbers) on inputs
  with +-inf, -0, subnormals and 1e30; a NaN reaches exactly the windows that cover it; an average meets the forward bound of an
  f32 sequential sum and one division, |got - ref| <= n u S / count + u |ref| (n taps summed, S = sum |x| over them, u = 2^-24);
  no element keeps the 0x7fc0beef payload; the kernel's name is the mode's instantiation; refused shapes are refused;
* launches past the resident grid repeat the rows of a 3-segment launch bit for bit;
* through the product path, on synth.random_pool_plan models written as `.onnx`: every pool's own output tensor against pool64 of
  the device's own input tensor, logits against a float64 forward composed of oracle.oracle's float64 helpers and pool64, the same
  bits at 3 / 80 / 300 segments, every MBConv block still fused, and the same model as a float16 file;
* a pool whose input passes 2^32 bytes; an f16 overflow in front of a MaxPool still ends in BH_ERR_NONFINITE (f16x3) and in the
  float64 logits (auto).
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
UNWRITTEN = 0x7fc0beef
BH_ERR_UNSUPPORTED, BH_ERR_NONFINITE = -6, -8
LOGIT_RTOL = 2e-5          # tests/test_full_conv_gpu.py: max |dlogit| <= 2e-5 max(1, max |logit|) in the f32-grade modes
F16_LOGIT_RTOL = 3e-3      # plain f16 operands
PRECISIONS = (("f32", LOGIT_RTOL), ("f16x3", LOGIT_RTOL), ("auto", LOGIT_RTOL), ("f16", F16_LOGIT_RTOL))
MODE_NAMES = ("MAX", "AVG", "AVG_PAD")


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def pool64(X, geom, mode):
    """X [n][in_h][in_w][c] -> dict(ref [n][out_h][out_w][c] float64, taps [1][out_h][out_w][1]: the window's pixels inside the
    image, S: sum |x| over them, count: the divisor).  geom = (in_h, in_w, out_h, out_w, c, kh, kw, sh, sw, pad_t, pad_l)."""
    in_h, in_w, out_h, out_w, c, kh, kw, sh, sw, pt, pl = geom
    X = np.asarray(X, np.float64).reshape(-1, in_h, in_w, c)
    Hp, Wp = max((out_h - 1) * sh + kh, pt + in_h), max((out_w - 1) * sw + kw, pl + in_w)

    def windows(A, fill):
        P = np.full((A.shape[0], Hp, Wp, A.shape[3]), fill, np.float64)
        P[:, pt:pt + in_h, pl:pl + in_w] = A
        return [P[:, ky:ky + (out_h - 1) * sh + 1:sh, kx:kx + (out_w - 1) * sw + 1:sw] for ky in range(kh) for kx in range(kw)]

    taps = sum(windows(np.ones((1, in_h, in_w, 1)), 0.0))
    assert taps.min() >= 1
    if mode == 0:
        with np.errstate(invalid="ignore"):
            return {"ref": functools.reduce(np.maximum, windows(X, -np.inf)), "taps": taps}       # (np.maximum propagates NaN)
    count = taps if mode == 1 else float(kh * kw)
    return {"ref": sum(windows(X, 0.0)) / count, "taps": taps, "S": sum(windows(np.abs(X), 0.0)), "count": count}


def check_pool(got, X, geom, mode, what):
    r = pool64(X, geom, mode)
    ref = r["ref"]
    got = np.asarray(got).reshape(ref.shape)
    assert not (got.view(np.uint32) == UNWRITTEN).any(), (what, "elements never written")
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), (what, "NaN pattern", int(np.isnan(got).sum()), int(nan.sum()))
    if mode == 0:
        bad = ~nan & ~(got.astype(np.float64) == ref)
        assert not bad.any(), (what, int(bad.sum()), got[bad][:4], ref[bad][:4])
        return 0.0
    err = np.abs(got.astype(np.float64) - ref)
    bound = r["taps"] * U * r["S"] / r["count"] + U * np.abs(ref)
    bad = ~nan & ~(err <= bound)
    assert not bad.any(), (what, int(bad.sum()), err[bad][:4], bound[bad][:4])
    pos = ~nan & (bound > 0)
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def run_pool(X, geom, mode, n_seg):
    lib = _lib.load()
    in_h, in_w, out_h, out_w, c = geom[:5]
    X = np.ascontiguousarray(X, np.float32)
    assert X.size == n_seg * in_h * in_w * c
    Y = np.empty((n_seg, out_h, out_w, c), np.float32)
    name = C.create_string_buffer(128)
    sh = np.asarray(geom, np.int32)
    rc = lib.bh_debug_pool(0, _p(X), _p(Y), n_seg, _p(sh), mode, name, 128)
    assert rc == 0, (rc, lib.bh_last_error())
    return Y, name.value.decode()


# in_h, in_w, out_h, out_w, c, kh, kw, sh, sw, pad_t, pad_l
SHAPES = {
    "8x10x4_k2_s2": (8, 10, 4, 5, 4, 2, 2, 2, 2, 0, 0),
    "7x9x12_k2_s2_drop_last": (7, 9, 3, 4, 12, 2, 2, 2, 2, 0, 0),
    "7x9x12_k2_s2_same_upper_hanging": (7, 9, 4, 5, 12, 2, 2, 2, 2, 0, 0),
    "7x9x20_k3_s2_p1": (7, 9, 4, 5, 20, 3, 3, 2, 2, 1, 1),
    "7x9x36_k3_s1_p1": (7, 9, 7, 9, 36, 3, 3, 1, 1, 1, 1),
    "5x5x8_k7_s1_p3_kernel_past_image": (5, 5, 5, 5, 8, 7, 7, 1, 1, 3, 3),
    "6x1x4_k3x1_one_pixel_wide": (6, 1, 6, 1, 4, 3, 1, 1, 1, 1, 0),
    "9x11x68_k2_s3_stride_past_kernel": (9, 11, 3, 4, 68, 2, 2, 3, 3, 0, 0),
    "6x10x260_k5x3_s21_p20": (6, 10, 3, 8, 260, 5, 3, 2, 1, 2, 0),
    "4x4x4_k4_window_is_image": (4, 4, 1, 1, 4, 4, 4, 1, 1, 0, 0),
}


def _inputs(geom, n_seg, mode, seed):
    in_h, in_w, _, _, c = geom[:5]
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n_seg, in_h, in_w, c)) * 10.0 ** rng.integers(-3, 4, (n_seg, in_h, in_w, c))).astype(np.float32)
    if mode == 0:      # what a comparison must get right: infinities, the two zeros, subnormals, a huge value
        special = np.array([np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-39, -3e-41, 1e30, -1e30], np.float32)
        where = rng.random(X.shape) < 0.35
        X[where] = special[rng.integers(0, special.size, int(where.sum()))]
    return X


@pytest.mark.parametrize("mode", (0, 1, 2), ids=MODE_NAMES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_element_against_float64(shape, mode):
    geom = SHAPES[shape]
    for n_seg in (1, 3, 5):
        X = _inputs(geom, n_seg, mode, 100 * mode + n_seg)
        Y, name = run_pool(X, geom, mode, n_seg)
        worst = check_pool(Y, X, geom, mode, (shape, mode, n_seg))
        print(f"{shape} {MODE_NAMES[mode]} n {n_seg}: {name}" + (f", worst error / bound {worst:.3f}" if mode else ", exact"))
        assert name == f"pool_kernel<{MODE_NAMES[mode]}>", name


@pytest.mark.parametrize("mode", (0, 1, 2), ids=MODE_NAMES)
@pytest.mark.parametrize("shape", ["7x9x12_k2_s2_same_upper_hanging", "7x9x20_k3_s2_p1", "6x10x260_k5x3_s21_p20"])
def test_a_nan_reaches_exactly_the_windows_that_cover_it(shape, mode):
    """one NaN in an interior pixel, one in a corner pixel and one in the last pixel of the image -- which, in the SAME_UPPER shape,
    only windows that hang past the image reach --, each in a channel of its own"""
    geom = SHAPES[shape]
    in_h, in_w, out_h, out_w, c = geom[:5]
    X = _inputs(geom, 3, 1, 77)
    X[0, in_h // 2, in_w // 2, 1] = np.nan
    X[1, 0, 0, 2] = np.nan
    X[2, in_h - 1, in_w - 1, 3] = np.nan
    X[1, in_h - 1, in_w - 1, c - 1] = np.nan
    Y, _ = run_pool(X, geom, mode, 3)
    ref = pool64(X, geom, mode)["ref"]
    assert 4 <= int(np.isnan(ref).sum()) < ref.size // 4
    assert np.isnan(ref[2, out_h - 1, out_w - 1, 3]) and np.isnan(ref[1, 0, 0, 2]) and not np.isnan(ref[0, 0, 0, 1])
    check_pool(Y, X, geom, mode, (shape, mode, "NaN"))


def test_refused_shapes_are_refused():
    lib = _lib.load()
    z, out = np.zeros(1 << 16, np.float32), np.empty(1 << 16, np.float32)

    def pool(geom, mode):
        return lib.bh_debug_pool(0, _p(z), _p(out), 1, _p(np.asarray(geom, np.int32)), mode, None, 0)

    ok = (7, 9, 4, 5, 8, 3, 3, 2, 2, 1, 1)
    assert pool(ok, 0) == 0 and pool(ok, 2) == 0
    assert pool(ok, 3) == BH_ERR_UNSUPPORTED and pool(ok, -1) == BH_ERR_UNSUPPORTED                  # no such mode
    assert pool((7, 9, 4, 5, 6, 3, 3, 2, 2, 1, 1), 0) == BH_ERR_UNSUPPORTED                          # c = 6
    assert b"debug_pool" in lib.bh_last_error()
    assert pool((7, 9, 4, 5, 8, 3, 3, 2, 2, 3, 1), 1) == BH_ERR_UNSUPPORTED                          # pad_t = kh
    assert pool((7, 9, 4, 5, 8, 3, 3, 2, 2, 1, 3), 1) == BH_ERR_UNSUPPORTED                          # pad_l = kw
    assert pool((7, 9, 5, 5, 8, 3, 3, 2, 2, 1, 1), 0) == BH_ERR_UNSUPPORTED                          # the fifth row of windows starts at row 7
    assert pool((7, 9, 4, 6, 8, 3, 3, 2, 2, 1, 1), 0) == BH_ERR_UNSUPPORTED                          # the sixth column at column 9
    assert pool((7, 9, 0, 5, 8, 3, 3, 2, 2, 1, 1), 0) == BH_ERR_UNSUPPORTED                          # no output rows
    assert pool((7, 9, 4, 5, 8, 65, 3, 2, 2, 1, 1), 0) == BH_ERR_UNSUPPORTED                         # kernel 65
    assert pool((7, 9, 1, 1, 8, 3, 3, 17, 2, 1, 1), 0) == BH_ERR_UNSUPPORTED                         # stride 17


@pytest.mark.parametrize("mode", (0, 1, 2), ids=MODE_NAMES)
def test_launches_past_the_resident_grid_repeat_a_small_launch(mode):
    """the 7 x 9 x 36 shape at 300 segments (665 workgroups) and at 1 000 (567 000 elements for the 524 288 threads of the largest
    grid launch_pool makes: the grid-stride loop's second trip): every row is the row of the 3-segment launch it repeats"""
    geom = SHAPES["7x9x36_k3_s1_p1"]
    X = _inputs(geom, 3, mode, 9)
    small, _ = run_pool(X, geom, mode, 3)
    check_pool(small, X, geom, mode, ("small", mode))
    for n in (300, 1000):
        big, _ = run_pool(np.ascontiguousarray(X[np.arange(n) % 3]), geom, mode, n)
        assert not (big.view(np.uint32) == UNWRITTEN).any()
        assert (big.view(np.uint32) == small.view(np.uint32)[np.arange(n) % 3]).all(), (mode, n)


# ---- the product path --------------------------------------------------------------------------------------------------------------
def _geom(L):
    return (L.in_h, L.in_w, L.out_h, L.out_w, L.cout, L.kh, L.kw, L.sh, L.sw, L.pad_t, L.pad_l)


def forward64(m, segs):
    """The model's logits in float64: oracle.oracle's helpers layer by layer, pool64 for OP_POOL.  -> [n][n_classes]"""
    n = segs.shape[0]
    spec, _ = O.frontend64(m, segs)
    T = [spec]
    for L in m.layers:
        X = T[L.in_tensor]
        w = lambda k: np.asarray(m.blob[L.w_off:L.w_off + k], np.float64)
        bias = np.asarray(m.blob[L.b_off:L.b_off + L.cout], np.float64)
        if L.op == mf.OP_CONV and L.in_layout == 1:
            assert L.kh == L.kw and L.sh == L.sw
            rows = O.stem_rows64(X, L.kh, L.sh, L.pad_t, L.pad_l, L.out_h, L.out_w)
            Y = O.act64(O.gemm64(rows.reshape(-1, rows.shape[-1]), w(L.kh * L.kw * L.cin * L.cout).reshape(-1, L.cout), bias), L.act)
        elif L.op == mf.OP_CONV:
            Y = O.act64(O.conv_nhwc64(X, w(L.kh * L.kw * L.cin * L.cout).reshape(L.kh, L.kw, L.cin, L.cout), bias, L.sh, L.sw, L.pad_t, L.pad_l, L.out_h, L.out_w)[0], L.act)
        elif L.op == mf.OP_DWCONV:
            assert L.kh == L.kw and L.sh == L.sw
            Y = O.act64(O.depthwise64(X, w(L.kh * L.kw * L.cout).reshape(L.kh * L.kw, L.cout), L.kh, L.sh, L.pad_t, L.pad_l, L.out_h, L.out_w) + bias, L.act)
        elif L.op in (mf.OP_PWCONV, mf.OP_DENSE):
            Y = O.act64(O.gemm64(X.reshape(-1, L.cin), w(L.cin * L.cout).reshape(L.cin, L.cout), bias), L.act)
        elif L.op == mf.OP_GAP:
            Y = X.reshape(n, -1, L.cout).mean(axis=1)
        elif L.op == mf.OP_POOL:
            Y = pool64(X, _geom(L), L.reserved)["ref"]
        else:
            raise AssertionError(L.op)
        Y = Y.reshape(n, L.out_h, L.out_w, L.cout)
        if L.res_tensor != mf.NO_TENSOR:
            Y = Y + T[L.res_tensor]
        T.append(Y)
    return T[-1].reshape(n, -1)


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def _mb_layers(m):
    """the depthwise layer of every MBConv block, and that of the block whose project convolution a pool reads directly"""
    dws = [i for i, L in enumerate(m.layers) if L.op == mf.OP_DWCONV]
    front = [i - 2 for i, L in enumerate(m.layers) if L.op == mf.OP_POOL and L.in_tensor == i and i >= 2 and m.layers[i - 1].op == mf.OP_PWCONV
             and m.layers[i - 2].op == mf.OP_DWCONV]
    return dws, front


@pytest.mark.parametrize("seed", range(6))
def test_random_pool_plans_on_the_onnx_route(seed, tmp_path, monkeypatch):
    from birda_amd.classifier import BirdClassifier
    from test_arena_plan_gpu import PATH_FUSED, PATH_INNER, arena_plan
    plan = synth.random_pool_plan(seed)
    m = synth.build_model("pool_plan", plan=plan)
    onnx = _write(str(tmp_path / "p.onnx"), convert.model_to_onnx(m, frontend_spelling="stft"))
    pools = [i for i, L in enumerate(m.layers) if L.op == mf.OP_POOL]
    assert sorted(m.layers[i].reserved for i in pools) == [0, 1, 2]
    dws, front = _mb_layers(m)
    assert dws and front
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=5 + seed)
    segs[2] *= np.float32(0.01)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    # (b), (c), (d): logits, launch sizes, fused blocks, per precision
    for prec, tol in PRECISIONS:
        clf = BirdClassifier(onnx, None, precision=prec)
        first = None
        for n in (3, 80, 300):
            ctx = clf.create_batch_context(n)
            ctx.set_sub_slices(1)
            got = clf.predict_logits(ctx, np.ascontiguousarray(segs[np.arange(n) % 3]))
            if first is None:
                first = got
                err = float(np.abs(got - ref).max())
                print(f"pool plan {seed} {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f}  {plan['items']}")
                assert np.isfinite(got).all() and err <= tol * scale, (prec, err, scale)
                tags = arena_plan(clf, ctx, 0)[2]
                assert all(tags[i] not in (PATH_FUSED, PATH_INNER) for i in pools), (prec, tags, pools)         # no pool is inside a block
                if prec != "f32":      # (the f32 tile entries do not cover every block shape: tests/test_full_conv_gpu.py)
                    assert all(tags[d] in (PATH_FUSED, PATH_INNER) for d in dws), (prec, tags, dws)             # every MBConv block runs fused
                    assert all(tags[d] in (PATH_FUSED, PATH_INNER) for d in front), (prec, tags, front)         # the one in front of a pool too
            else:
                assert (got.view(np.uint32) == first.view(np.uint32)[np.arange(n) % 3]).all(), (prec, n)
            ctx.close()
        clf.close()
    # (a): every pool's own output against the float64 pool of the device's own input, layer by layer in f32
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    clf = BirdClassifier(onnx, None, precision="f32")
    ctx = clf.create_batch_context(3)
    clf.predict_logits(ctx, segs)
    for i in pools:
        L = m.layers[i]
        X, Y = clf.read_tensor(ctx, L.in_tensor, 3), clf.read_tensor(ctx, i + 1, 3)
        assert np.isfinite(X).all() and X.shape[1] == L.in_h * L.in_w * L.cout
        worst = check_pool(Y, X, _geom(L), L.reserved, (seed, i))
        print(f"pool plan {seed} layer {i} {MODE_NAMES[L.reserved]} {L.kh}x{L.kw}/{L.sh}x{L.sw} {L.in_h}x{L.in_w}x{L.cout} -> {L.out_h}x{L.out_w}: "
              + (f"worst error / bound {worst:.3f}" if L.reserved else "exact"))
    ctx.close(); clf.close()


@pytest.mark.parametrize("seed", range(6))
def test_random_pool_plan_as_a_float16_file(seed, tmp_path):
    """graph_to_float16 of the same graph: loads, keeps its pools, and meets the float64 forward of the container convert.py makes
    of it (its weights are the file's float16 values); the container the library's own reader writes holds the same records and
    the same blob, bit for bit"""
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("pool_plan", plan=synth.random_pool_plan(seed))
    g16 = convert.graph_to_float16(convert.graph_from_model(m, frontend_spelling="conv1d"))
    from birda_amd import onnx_io as ox
    p16, bhm = _write(str(tmp_path / "p16.onnx"), ox.dump(g16)), str(tmp_path / "p16.bhm")
    L = _lib.load()
    assert L.bh_onnx_to_bhm(p16.encode(), bhm.encode()) == 0, L.bh_last_error()
    conv = mf.read_model(bhm)
    assert [(a.op, a.reserved, a.kh, a.kw, a.pad_t, a.pad_l, a.out_h, a.out_w) for a in conv.layers] == \
           [(a.op, a.reserved, a.kh, a.kw, a.pad_t, a.pad_l, a.out_h, a.out_w) for a in m.layers]
    # ... and the weights are convert.py's reading of the same file, bit for bit: float32(float16(w)) of the model's
    want = convert.model_from_graph(ox.load(ox.dump(g16)), None, sample_rate=m.sample_rate)
    n_w = {mf.OP_CONV: lambda a: a.kh * a.kw * a.cin * a.cout, mf.OP_DWCONV: lambda a: a.kh * a.kw * a.cout,
           mf.OP_PWCONV: lambda a: a.cin * a.cout, mf.OP_DENSE: lambda a: a.cin * a.cout}
    assert [(a.op, a.reserved, a.act, a.res_tensor) for a in want.layers] == [(a.op, a.reserved, a.act, a.res_tensor) for a in conv.layers]
    for a, b, c in zip(want.layers, conv.layers, m.layers):
        if a.op in n_w:
            k = n_w[a.op](a)
            wa, wb, wc = want.blob[a.w_off:a.w_off + k], conv.blob[b.w_off:b.w_off + k], m.blob[c.w_off:c.w_off + k]
            assert (wa.view(np.uint32) == wb.view(np.uint32)).all() and (wa == wc.astype(np.float16).astype(np.float32)).all()
            assert (want.blob[a.b_off:a.b_off + a.cout].view(np.uint32) == conv.blob[b.b_off:b.b_off + b.cout].view(np.uint32)).all()
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=31)
    ref = forward64(conv, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    for prec, tol in PRECISIONS:
        clf = BirdClassifier(p16, None, precision=prec)
        assert clf.weight_summary()["float16_file"] == 1
        ctx = clf.create_batch_context(3)
        got = clf.predict_logits(ctx, segs)
        ctx.close(); clf.close()
        err = float(np.abs(got - ref).max())
        print(f"pool plan {seed} float16 file {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f}")
        assert np.isfinite(got).all() and err <= tol * scale, (prec, err, scale)


def pool_model(cstem, mode, head=32, conv=None):
    """The mini front-end (one 32-mel branch, 115 frames), a 3x3 NCHW stem to `cstem` channels [, a 3x3 convolution to `conv`
    channels], a 2x2 stride-2 pool, a 1x1 head, the global pool and a dense layer"""
    b = synth._Builder(np.random.default_rng(11))
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    t, h, w = b.conv(0, br.n_mels, br.n_frames, 1, cstem, 3, 1, mf.ACT_GELU_ERF, in_layout=1)
    c = cstem
    if conv:
        t, h, w = b.conv(t, h, w, c, conv, 3, 1, mf.ACT_NONE)
        c = conv
    t, h, w = b.pool(t, h, w, c, 2, 2, 2, 2, mode, "same")
    t = b.pwconv(t, h, w, c, head, mf.ACT_GELU_ERF)
    t = emb = b.gap(t, h, w, head)
    b.dense(t, head, 30, gain=1.5)
    return mf.Model(0, sr, n, n / sr, 30, head, mf.OUT_SIGMOID, emb, br.n_mels, br.n_frames, 1e-6, [br], b.layers, np.concatenate(b.chunks))


def test_pool_input_past_4_gib_keeps_a_segments_bits(tmp_path):
    """A 256-channel stem on the 32 x 115 image: 3.77 MB a segment in front of the pool; 1 140 segments in one launch is the
    smallest count whose pool input passes 2^32 bytes.  Every row bit-identical to the same segment in a launch of 3."""
    from birda_amd.classifier import BirdClassifier
    m = pool_model(256, mf.POOL_MAX)
    P = m.layers[1]
    assert P.op == mf.OP_POOL
    per_seg = P.in_h * P.in_w * P.cout * 4
    n_big = 2 ** 32 // per_seg + 1
    assert (n_big - 1) * per_seg <= 2 ** 32 < n_big * per_seg and n_big == 1140
    path = str(tmp_path / "big.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=60)
    clf = BirdClassifier(path, None, precision="f32")
    ctx = clf.create_batch_context(3)
    small = clf.predict_logits(ctx, segs)
    ctx.close()
    ctx = clf.create_batch_context(n_big)
    ctx.set_sub_slices(1)
    got = clf.predict_logits(ctx, np.ascontiguousarray(np.tile(segs, (n_big // 3, 1))))
    ctx.close(); clf.close()
    assert np.isfinite(got).all()
    bad = [i for i in range(n_big) if not (got[i] == small[i % 3]).all()]
    assert not bad, (bad[:5], len(bad))


def test_f16_overflow_in_front_of_a_max_pool_is_not_laundered(tmp_path):
    """The convolution's weights and bias times 2^20 (a linear layer: its output, ~1e6, is past 65 504), the MaxPool behind it, and
    the 1x1 layer that reads the pool divided by 2^20: the same function in f32 arithmetic (max commutes with a positive scale).
    f16x3 cannot represent the pooled tensor -- BH_ERR_NONFINITE, the pool has passed the values on --; auto re-runs the rows on
    the f32 kernels and gives the float64 logits."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    m0 = pool_model(32, mf.POOL_MAX, head=64, conv=64)
    m = copy.deepcopy(m0)
    blob = m.blob.copy()
    Cv, Pl, Pw = m.layers[1], m.layers[2], m.layers[3]
    assert Cv.op == mf.OP_CONV and Pl.op == mf.OP_POOL and Pl.reserved == mf.POOL_MAX and Pw.op == mf.OP_PWCONV
    s = np.float32(2.0 ** 20)
    blob[Cv.w_off:Cv.w_off + Cv.kh * Cv.kw * Cv.cin * Cv.cout] *= s
    blob[Cv.b_off:Cv.b_off + Cv.cout] *= s
    blob[Pw.w_off:Pw.w_off + Pw.cin * Pw.cout] /= s
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
    ctx.close(); clf.close()
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(4)
    got = clf.predict_logits(ctx, segs)
    assert clf.fallback_segments() > 0
    err = float(np.abs(got - ref).max())
    print(f"overflow in front of a MaxPool, auto: max|dlogit| = {err:.3e} of {scale:.2f}, {clf.fallback_segments()} segments re-run")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    ctx.close(); clf.close()


def test_cnn_pool_runs_and_matches_float64_on_its_pools(tmp_path, monkeypatch):
    """synth's timing model (conv + pool stages on the v2.4 front-end), one segment: its four pools against pool64 of their inputs"""
    from birda_amd.classifier import BirdClassifier
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    m = synth.build_model("cnn_pool", n_classes=40)
    path = str(tmp_path / "cnn_pool.bhm")
    mf.write_model(path, m)
    pools = [i for i, L in enumerate(m.layers) if L.op == mf.OP_POOL]
    assert [m.layers[i].reserved for i in pools] == [mf.POOL_MAX, mf.POOL_AVG, mf.POOL_MAX, mf.POOL_AVG]
    assert [m.layers[i].cout for i in pools] == [32, 64, 128, 256]
    segs = synth.synth_segments(1, m.sample_count, m.sample_rate, start=2)
    clf = BirdClassifier(path, None, precision="f32")
    ctx = clf.create_batch_context(1)
    got = clf.predict_logits(ctx, segs)
    assert np.isfinite(got).all()
    for i in pools:
        L = m.layers[i]
        check_pool(clf.read_tensor(ctx, i + 1, 1), clf.read_tensor(ctx, L.in_tensor, 1), _geom(L), L.reserved, ("cnn_pool", i))
    ctx.close(); clf.close()
