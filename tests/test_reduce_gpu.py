"""Max, mean and max + mean over one image axis or both on the device (kernels_reduce.hip reduce_kernel<MODE, G>), held to float64.

The plain-C oracle has no such layer, so the reference is written here from the definition (reduce64): the window is the whole image
along each reduced axis; max is its maximum, NaN if any tap is; the mean is the sum over the count; max + mean is their sum.

* element by element through bh_debug_reduce: all three modes, launches of 1, 3 and 5 segments, C = 4 / 12 / 68 / 260 / 2048, reduced
  extents 2, 3, 63 / 64 / 65, 511 and each side of the two thresholds of reduce_split (32 taps, 4096 kept float4s a
  segment), windows over H, over W and over both, a one-pixel-wide image, one kept pixel, an image of one pixel along the kept axis.
  MAX is EXACT (== as numbers) on inputs with +-inf, +-0, subnormals and +-1e30.  MEAN over R taps meets the first-order bound of an
  f32 sum in ANY order plus the scaling, |got - ref| <= (R - 1) u S / R + 2 u |ref| (S = sum |x| over the window, u = 2^-24; the 2
  covers a reciprocal multiply as well as a division); MAXMEAN that bound plus u |max + mean| for the final add.  The bounds are
  derived, not measured; the worst error / bound share is printed per shape.  No element keeps the 0x7fc0beef payload; the name is
  the mode's instantiation with the lanes the shape alone decides; refused shapes are refused; a NaN reaches exactly the outputs whose
  window covers it;
* launches past the resident grid repeat the rows of a 3-segment launch bit for bit, in both forms (1 and 8 lanes);
* through the product path, on synth.random_reduce_plan models written as `.onnx` and the float16 file of one: every reduce layer's own
  output tensor against reduce64 of the device's own input tensor, logits against a float64 forward composed of oracle.oracle's
  float64 helpers and reduce64, the same bits at 3 / 80 / 300 segments;
* an f16 overflow in front of a MAX reduce still ends in BH_ERR_NONFINITE (f16x3) and in the float64 logits (auto).
"""
import copy
import ctypes as C

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
UNWRITTEN = 0x7fc0beef
BH_ERR_INVALID, BH_ERR_UNSUPPORTED, BH_ERR_NONFINITE = -1, -6, -8
LOGIT_RTOL = 2e-5          # tests/test_pool_gpu.py: max |dlogit| <= 2e-5 max(1, max |logit|) in the f32-grade modes
F16_LOGIT_RTOL = 3e-3      # plain f16 operands
PRECISIONS = (("f32", LOGIT_RTOL), ("f16x3", LOGIT_RTOL), ("auto", LOGIT_RTOL), ("f16", F16_LOGIT_RTOL))
MAX, MEAN, MAXMEAN = mf.REDUCE_MAX, mf.REDUCE_MEAN, mf.REDUCE_MAXMEAN
MODE_NAMES = ("MAX", "MEAN", "MAXMEAN")


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def reduce64(X, geom, mode):
    """X [n][in_h][in_w][c] -> dict(ref [n][out_h][out_w][c] float64, S: sum |x| over the window, R: its taps).
    geom = (in_h, in_w, out_h, out_w, c, kh, kw)."""
    in_h, in_w, out_h, out_w, c, kh, kw = geom
    assert kh in (1, in_h) and kw in (1, in_w) and kh * kw > 1 and (out_h, out_w) == (in_h // kh, in_w // kw)
    X = np.asarray(X, np.float64).reshape(-1, in_h, in_w, c)
    axes = tuple(a for a, k in ((1, kh), (2, kw)) if k > 1)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = X.max(axis=axes, keepdims=True)                         # (np.max propagates NaN)
        mean = X.sum(axis=axes, keepdims=True) / float(kh * kw)
        ref = mx if mode == MAX else mean if mode == MEAN else mx + mean
    return {"ref": ref, "S": np.abs(X).sum(axis=axes, keepdims=True), "R": kh * kw}


def check_reduce(got, X, geom, mode, what):
    """-> the worst error / bound share (0 for MAX, which is exact)"""
    r = reduce64(X, geom, mode)
    ref = r["ref"]
    got = np.asarray(got).reshape(ref.shape)
    assert not (got.view(np.uint32) == UNWRITTEN).any(), (what, "elements never written")
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), (what, "NaN pattern", int(np.isnan(got).sum()), int(nan.sum()))
    if mode == MAX:
        bad = ~nan & ~(got.astype(np.float64) == ref)
        assert not bad.any(), (what, int(bad.sum()), got[bad][:4], ref[bad][:4])
        return 0.0
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref)
        if mode == MEAN:
            bound = (r["R"] - 1) * U * r["S"] / r["R"] + 2 * U * np.abs(ref)
        else:
            mean = reduce64(X, geom, MEAN)["ref"]
            bound = (r["R"] - 1) * U * r["S"] / r["R"] + 2 * U * np.abs(mean) + U * np.abs(ref)
    fin = ~nan & np.isfinite(ref)
    assert (got[~nan & ~fin].astype(np.float64) == ref[~nan & ~fin]).all(), (what, "infinities")
    bad = fin & ~(err <= bound)
    assert not bad.any(), (what, int(bad.sum()), err[bad][:4], bound[bad][:4])
    pos = fin & (bound > 0)
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def run_reduce(X, geom, mode, n_seg, split=0):
    lib = _lib.load()
    in_h, in_w, out_h, out_w, c = geom[:5]
    X = np.ascontiguousarray(X, np.float32)
    assert X.size == n_seg * in_h * in_w * c
    Y = np.empty((n_seg, out_h, out_w, c), np.float32)
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_reduce(0, _p(X), _p(Y), n_seg, _p(np.asarray(geom, np.int32)), mode, split, name, 128)
    assert rc == 0, (rc, lib.bh_last_error())
    return Y, name.value.decode()


def lanes(geom):
    """kernels.hpp reduce_split, restated: the lanes that share one output float4, from the shape alone"""
    in_h, in_w, out_h, out_w, c, kh, kw = geom
    R, kept4 = kh * kw, out_h * out_w * (c // 4)
    return 8 if R >= 32 and kept4 < 4096 else 1


def is_gap(geom, mode):
    return mode == MEAN and geom[5] > 1 and geom[6] > 1


# in_h, in_w, out_h, out_w, c, kh, kw
SHAPES = {
    "h2_of_2x5x4": (2, 5, 1, 5, 4, 2, 1),
    "w3_of_4x3x12": (4, 3, 4, 1, 12, 1, 3),
    "both_3x3x68_one_kept_pixel": (3, 3, 1, 1, 68, 3, 3),
    "h63_of_63x3x260": (63, 3, 1, 3, 260, 63, 1),
    "w64_of_2x64x12": (2, 64, 2, 1, 12, 1, 64),
    "h65_one_pixel_wide": (65, 1, 1, 1, 4, 65, 1),
    "w511_of_1x511x64_one_row": (1, 511, 1, 1, 64, 1, 511),
    "h511_of_511x2x12": (511, 2, 1, 2, 12, 511, 1),
    "both_8x32x2048": (8, 32, 1, 1, 2048, 8, 32),
    "w31_below_the_split": (3, 31, 3, 1, 8, 1, 31),
    "w32_at_the_split": (3, 32, 3, 1, 8, 1, 32),
    "w33_above_the_split": (3, 33, 3, 1, 8, 1, 33),
    "both_15x17_255_taps": (15, 17, 1, 1, 4, 15, 17),
    "both_16x16_256_taps": (16, 16, 1, 1, 4, 16, 16),
    "h257_of_257x2x4": (257, 2, 1, 2, 4, 257, 1),
    "w32_kept_4095": (3, 32, 3, 1, 5460, 1, 32),
    "w32_kept_4096": (4, 32, 4, 1, 4096, 1, 32),
    "w32_kept_4097": (17, 32, 17, 1, 964, 1, 32),
    "h40_of_40x7x20": (40, 7, 1, 7, 20, 40, 1),
}


def test_the_shapes_stand_on_each_side_of_every_threshold():
    got = {k: lanes(g) for k, g in SHAPES.items()}
    assert (got["w31_below_the_split"], got["w32_at_the_split"], got["w33_above_the_split"]) == (1, 8, 8)
    assert (got["w32_kept_4095"], got["w32_kept_4096"], got["w32_kept_4097"]) == (8, 1, 1)
    assert (got["w511_of_1x511x64_one_row"], got["both_8x32x2048"], got["h63_of_63x3x260"], got["h2_of_2x5x4"]) == (8, 8, 8, 1)
    assert {g[4] for g in SHAPES.values()} >= {4, 12, 68, 260, 2048} and {g[5] * g[6] for g in SHAPES.values()} >= {2, 3, 63, 64, 65, 511}


def _inputs(geom, n_seg, mode, seed):
    in_h, in_w, _, _, c = geom[:5]
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n_seg, in_h, in_w, c)) * 10.0 ** rng.integers(-3, 4, (n_seg, in_h, in_w, c))).astype(np.float32)
    if mode == MAX:      # what a comparison must get right: infinities, the two zeros, subnormals, huge values
        special = np.array([np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-39, -3e-41, 1e30, -1e30], np.float32)
        where = rng.random(X.shape) < 0.35
        X[where] = special[rng.integers(0, special.size, int(where.sum()))]
        X[0, :, :, 0] = -np.inf                        # a window of nothing but -inf
        if c > 4:
            X[0, :, :, 5] = np.float32(-0.0)
    return X


@pytest.mark.parametrize("mode", (MAX, MEAN, MAXMEAN), ids=MODE_NAMES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_element_against_float64(shape, mode):
    geom = SHAPES[shape]
    if is_gap(geom, mode):
        lib = _lib.load()
        z = np.zeros(int(np.prod(geom[:2])) * geom[4], np.float32)
        assert lib.bh_debug_reduce(0, _p(z), _p(z.copy()), 1, _p(np.asarray(geom, np.int32)), mode, 0, None, 0) == BH_ERR_UNSUPPORTED   # the global pool's
        return
    for n_seg in (1, 3, 5):
        X = _inputs(geom, n_seg, mode, 100 * mode + n_seg)
        Y, name = run_reduce(X, geom, mode, n_seg)
        worst = check_reduce(Y, X, geom, mode, (shape, mode, n_seg))
        print(f"{shape} {MODE_NAMES[mode]} n {n_seg}: {name}" + (f", worst error / bound {worst:.3f}" if mode else ", exact"))
        assert name == f"reduce_kernel<{MODE_NAMES[mode]},{lanes(geom)}>", name


@pytest.mark.parametrize("mode", (MAX, MAXMEAN), ids=("MAX", "MAXMEAN"))
def test_maxmean_reads_a_window_salted_with_specials_like_max(mode):
    """+-inf, +-0, subnormals and +-1e30 in front of MAXMEAN too: where the window's sum is finite the bound holds, where it is not
    the result is the float64 one (inf, or NaN from inf - inf), exactly"""
    geom = SHAPES["h40_of_40x7x20"]
    X = _inputs(geom, 3, MAX, 5)
    Y, _ = run_reduce(X, geom, mode, 3)
    check_reduce(Y, X, geom, mode, ("specials", mode))


NAN_SHAPES = {"h": (7, 9, 1, 9, 12, 7, 1), "w": (7, 9, 7, 1, 12, 1, 9), "both": (7, 9, 1, 1, 12, 7, 9), "h_split_8": (40, 6, 1, 6, 8, 40, 1),
              "w_split_long": (3, 300, 3, 1, 8, 1, 300)}


@pytest.mark.parametrize("shape,mode", [(k, md) for k in sorted(NAN_SHAPES) for md in (MAX, MEAN, MAXMEAN) if not is_gap(NAN_SHAPES[k], md)],
                         ids=lambda v: MODE_NAMES[v] if isinstance(v, int) else v)
def test_a_nan_reaches_exactly_the_outputs_whose_window_covers_it(shape, mode):
    """one NaN in an interior pixel, one in a corner pixel and one in the last pixel of the image, each in a channel of its own (and
    an inf beside them); the mean over both axes is the global average pool's record, not this kernel's"""
    geom = NAN_SHAPES[shape]
    in_h, in_w, out_h, out_w, c = geom[:5]
    X = _inputs(geom, 3, MEAN, 77)
    X[0, in_h // 2, in_w // 2, 1] = np.nan
    X[1, 0, 0, 2] = np.nan
    X[2, in_h - 1, in_w - 1, 3] = np.nan
    X[1, in_h - 1, in_w - 1, c - 1] = np.inf
    Y, _ = run_reduce(X, geom, mode, 3)
    ref = reduce64(X, geom, mode)["ref"]
    assert int(np.isnan(ref).sum()) == 3 and int(np.isinf(ref).sum()) == 1
    assert np.isnan(ref[2, out_h - 1, out_w - 1, 3]) and np.isnan(ref[1, 0, 0, 2]) and not np.isnan(ref[0, 0, 0, 2])
    check_reduce(Y, X, geom, mode, (shape, mode, "NaN"))


def test_refused_shapes_are_refused():
    lib = _lib.load()
    z, out = np.zeros(1 << 16, np.float32), np.empty(1 << 16, np.float32)

    def red(geom, mode, split=0):
        return lib.bh_debug_reduce(0, _p(z), _p(out), 1, _p(np.asarray(geom, np.int32)), mode, split, None, 0)

    ok = (7, 9, 1, 9, 8, 7, 1)
    assert red(ok, MAX) == 0 and red(ok, MEAN) == 0 and red(ok, MAXMEAN) == 0 and red(ok, MAX, 8) == 0
    assert red(ok, 3) == BH_ERR_UNSUPPORTED and red(ok, -1) == BH_ERR_UNSUPPORTED                 # no such mode
    assert b"debug_reduce" in lib.bh_last_error() and b"not built" in lib.bh_last_error()
    assert red((7, 9, 1, 9, 6, 7, 1), MAX) == BH_ERR_UNSUPPORTED                                   # c = 6
    assert red((7, 9, 7, 9, 8, 1, 1), MAX) == BH_ERR_UNSUPPORTED                                   # a 1x1 window
    assert red((7, 9, 2, 9, 8, 3, 1), MAX) == BH_ERR_UNSUPPORTED                                   # a window that is not the whole axis
    assert red((7, 9, 7, 9, 8, 7, 1), MAX) == BH_ERR_UNSUPPORTED                                   # an output image that is not in / window
    assert red((7, 9, 1, 1, 8, 7, 9), MEAN) == BH_ERR_UNSUPPORTED                                  # the mean over both axes: OP_GAP's
    assert red((7, 9, 1, 1, 8, 7, 9), MAX) == 0 and red((7, 9, 1, 1, 8, 7, 9), MAXMEAN) == 0
    assert red((300, 300, 1, 1, 4, 300, 300), MAX) == BH_ERR_UNSUPPORTED                           # 90 000 taps
    assert red(ok, MAX, 4) == BH_ERR_INVALID and red(ok, MAX, 64) == BH_ERR_INVALID                # no such form


@pytest.mark.parametrize("mode", (MAX, MEAN, MAXMEAN), ids=MODE_NAMES)
@pytest.mark.parametrize("shape,n_big", [((4, 40, 1, 40, 68, 4, 1), 800), ((12, 40, 12, 1, 36, 1, 40), 1000)], ids=("1_lane", "8_lanes"))
def test_launches_past_the_resident_grid_repeat_a_small_launch(shape, n_big, mode):
    """2 048 workgroups of 256 / G items are the largest grid: 544 000 items for its 524 288 (G = 1) and 108 000 for 65 536 (8) take
    the grid-stride loop's second trip; every row is the row of the 3-segment launch it repeats"""
    G = lanes(shape)
    assert n_big * shape[2] * shape[3] * (shape[4] // 4) > 2048 * (256 // G)
    X = _inputs(shape, 3, mode, 9)
    small, name = run_reduce(X, shape, mode, 3)
    check_reduce(small, X, shape, mode, ("small", mode))
    big, name_big = run_reduce(np.ascontiguousarray(X[np.arange(n_big) % 3]), shape, mode, n_big)
    assert name == name_big == f"reduce_kernel<{MODE_NAMES[mode]},{G}>"
    assert not (big.view(np.uint32) == UNWRITTEN).any()
    assert (big.view(np.uint32) == small.view(np.uint32)[np.arange(n_big) % 3]).all(), (mode, n_big)


def test_a_forced_form_meets_the_same_bounds():
    """the split argument of the diagnostic entry (what the timing tool compares): each form on a shape the launcher gives another"""
    geom = SHAPES["w64_of_2x64x12"]
    for mode in (MAX, MEAN, MAXMEAN):
        X = _inputs(geom, 3, mode, 31 + mode)
        for split in (1, 8):
            Y, name = run_reduce(X, geom, mode, 3, split)
            assert name == f"reduce_kernel<{MODE_NAMES[mode]},{split}>"
            check_reduce(Y, X, geom, mode, ("forced", mode, split))


# ---- the product path --------------------------------------------------------------------------------------------------------------
def _geom(L):
    return (L.in_h, L.in_w, L.out_h, L.out_w, L.cout, L.kh, L.kw)


def forward64(m, segs):
    """The model's logits in float64: oracle.oracle's helpers layer by layer, reduce64 for OP_REDUCE (and test_pool_gpu's pool64 for
    OP_POOL).  -> [n][n_classes]"""
    from test_pool_gpu import pool64
    n = segs.shape[0]
    spec, _ = O.frontend64(m, segs)
    T = [spec]
    for L in m.layers:
        X = T[L.in_tensor]
        w = lambda k: np.asarray(m.blob[L.w_off:L.w_off + k], np.float64)
        bias = np.asarray(m.blob[L.b_off:L.b_off + L.cout], np.float64)
        if L.op == mf.OP_CONV and L.in_layout == 1:
            rows = O.stem_rows64(X, L.kh, L.sh, L.pad_t, L.pad_l, L.out_h, L.out_w)
            Y = O.act64(O.gemm64(rows.reshape(-1, rows.shape[-1]), w(L.kh * L.kw * L.cin * L.cout).reshape(-1, L.cout), bias), L.act)
        elif L.op == mf.OP_CONV:
            Y = O.act64(O.conv_nhwc64(X, w(L.kh * L.kw * L.cin * L.cout).reshape(L.kh, L.kw, L.cin, L.cout), bias, L.sh, L.sw, L.pad_t, L.pad_l, L.out_h, L.out_w)[0], L.act)
        elif L.op in (mf.OP_PWCONV, mf.OP_DENSE):
            Y = O.act64(O.gemm64(X.reshape(-1, L.cin), w(L.cin * L.cout).reshape(L.cin, L.cout), bias), L.act)
        elif L.op == mf.OP_GAP:
            Y = X.reshape(n, -1, L.cout).mean(axis=1)
        elif L.op == mf.OP_POOL:
            Y = pool64(X, (L.in_h, L.in_w, L.out_h, L.out_w, L.cout, L.kh, L.kw, L.sh, L.sw, L.pad_t, L.pad_l), L.reserved)["ref"]
        elif L.op == mf.OP_REDUCE:
            Y = reduce64(X, _geom(L), L.reserved)["ref"]
        else:
            raise AssertionError(L.op)
        assert L.res_tensor == mf.NO_TENSOR
        T.append(Y.reshape(n, L.out_h, L.out_w, L.cout))
    return T[-1].reshape(n, -1)


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


@pytest.mark.parametrize("seed", range(4))
def test_random_reduce_plans_on_the_onnx_route(seed, tmp_path, monkeypatch):
    from birda_amd.classifier import BirdClassifier
    plan = synth.random_reduce_plan(seed)
    m = synth.build_model("reduce_plan", plan=plan)
    onnx = _write(str(tmp_path / "r.onnx"), convert.model_to_onnx(m, frontend_spelling="stft", spell_reduce=m.reduce_spelling))
    reduces = [i for i, L in enumerate(m.layers) if L.op == mf.OP_REDUCE]
    assert reduces and plan["head"] == synth.REDUCE_HEADS[seed]
    segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=5 + seed)
    segs[2] *= np.float32(0.01)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
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
                print(f"reduce plan {seed} {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f}  {plan}")
                assert np.isfinite(got).all() and err <= tol * scale, (prec, err, scale)
                for i in reduces:
                    L = m.layers[i]
                    assert clf.layer_kernel(i) == f"reduce_kernel<{MODE_NAMES[L.reserved]},{lanes(_geom(L))}>", (i, clf.layer_kernel(i))
            else:
                assert (got.view(np.uint32) == first.view(np.uint32)[np.arange(n) % 3]).all(), (prec, n)
            ctx.close()
        clf.close()
    # every reduce layer's own output against reduce64 of the device's own input, layer by layer in f32
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    clf = BirdClassifier(onnx, None, precision="f32")
    ctx = clf.create_batch_context(3)
    clf.predict_logits(ctx, segs)
    for i in reduces:
        L = m.layers[i]
        X, Y = clf.read_tensor(ctx, L.in_tensor, 3), clf.read_tensor(ctx, i + 1, 3)
        assert np.isfinite(X).all() and X.shape[1] == L.in_h * L.in_w * L.cout
        worst = check_reduce(Y, X, _geom(L), L.reserved, (seed, i))
        print(f"reduce plan {seed} layer {i} {MODE_NAMES[L.reserved]} {L.kh}x{L.kw} of {L.in_h}x{L.in_w}x{L.cout}: "
              + (f"worst error / bound {worst:.3f}" if L.reserved else "exact"))
    ctx.close(); clf.close()


def test_a_reduce_plan_as_a_float16_file(tmp_path):
    """graph_to_float16 of the PANNs-pair model's graph: loads, keeps its reduce records, and meets the float64 forward of the container
    the library's own reader writes of it (its weights are the file's float16 values)"""
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("reduce_plan", plan=synth.random_reduce_plan(0))
    g16 = convert.graph_to_float16(convert.graph_from_model(m, frontend_spelling="conv1d", spell_reduce=m.reduce_spelling))
    p16, bhm = _write(str(tmp_path / "r16.onnx"), ox.dump(g16)), str(tmp_path / "r16.bhm")
    L = _lib.load()
    assert L.bh_onnx_to_bhm(p16.encode(), bhm.encode()) == 0, L.bh_last_error()
    conv = mf.read_model(bhm)
    key = lambda a: (a.op, a.reserved, a.kh, a.kw, a.in_h, a.in_w, a.out_h, a.out_w, a.act)
    assert [key(a) for a in conv.layers] == [key(a) for a in m.layers]
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
        print(f"reduce plan 0 float16 file {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f}")
        assert np.isfinite(got).all() and err <= tol * scale, (prec, err, scale)


def reduce_model(cstem, conv, head=64):
    """The mini front-end (one 32-mel branch, 115 frames), a 3x3 NCHW stem to `cstem` channels, a 3x3 convolution to `conv` channels
    without an activation, the MAX over the frequency axis, a 1x1 head, the global pool and a dense layer"""
    b = synth._Builder(np.random.default_rng(11))
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    t, h, w = b.conv(0, br.n_mels, br.n_frames, 1, cstem, 3, 1, mf.ACT_GELU_ERF, in_layout=1)
    t, h, w = b.conv(t, h, w, cstem, conv, 3, 1, mf.ACT_NONE)
    t, h, w = b.reduce(t, h, w, conv, mf.REDUCE_MAX, over_h=True, over_w=False)
    t = b.pwconv(t, h, w, conv, head, mf.ACT_GELU_ERF)
    t = emb = b.gap(t, h, w, head)
    b.dense(t, head, 30, gain=1.5)
    return mf.Model(0, sr, n, n / sr, 30, head, mf.OUT_SIGMOID, emb, br.n_mels, br.n_frames, 1e-6, [br], b.layers, np.concatenate(b.chunks))


def test_f16_overflow_in_front_of_a_max_reduce_is_not_laundered(tmp_path):
    """The convolution's weights and bias times 2^20 (a linear layer: its output, ~1e6, is past 65 504), the MAX reduce behind it, and
    the 1x1 layer that reads the reduce divided by 2^20: the same function in f32 arithmetic (max commutes with a positive scale).
    f16x3 cannot represent the reduced tensor -- BH_ERR_NONFINITE, the reduce has passed the values on --; auto re-runs the rows on
    the f32 kernels and gives the float64 logits."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    m0 = reduce_model(32, 64)
    m = copy.deepcopy(m0)
    blob = m.blob.copy()
    Cv, Rd, Pw = m.layers[1], m.layers[2], m.layers[3]
    assert Cv.op == mf.OP_CONV and Rd.op == mf.OP_REDUCE and Rd.reserved == MAX and Pw.op == mf.OP_PWCONV
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
    print(f"overflow in front of a MAX reduce, auto: max|dlogit| = {err:.3e} of {scale:.2f}, {clf.fallback_segments()} segments re-run")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    ctx.close(); clf.close()


def test_cnn14_audio_runs_and_matches_float64_on_its_reduces(tmp_path, monkeypatch):
    """synth's timing model (the cnn_pool body under the PANNs head), one segment: its two reduce layers against reduce64 of their inputs"""
    from birda_amd.classifier import BirdClassifier
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    m = synth.build_model("cnn14_audio", n_classes=40)
    path = str(tmp_path / "cnn14.bhm")
    mf.write_model(path, m)
    reduces = [i for i, L in enumerate(m.layers) if L.op == mf.OP_REDUCE]
    assert [m.layers[i].reserved for i in reduces] == [MEAN, MAXMEAN] and m.embedding_tensor == reduces[1] + 1
    segs = synth.synth_segments(1, m.sample_count, m.sample_rate, start=2)
    clf = BirdClassifier(path, None, precision="f32")
    ctx = clf.create_batch_context(1)
    got = clf.predict_logits(ctx, segs)
    assert np.isfinite(got).all()
    for i in reduces:
        L = m.layers[i]
        check_reduce(clf.read_tensor(ctx, i + 1, 1), clf.read_tensor(ctx, L.in_tensor, 1), _geom(L), L.reserved, ("cnn14_audio", i))
    ctx.close(); clf.close()
