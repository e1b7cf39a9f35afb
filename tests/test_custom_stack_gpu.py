"""The dense stack of api_custom.hip (cc_build / cc_upload_rows / cc_run) held to float64, element by element.

The stack serves bh_custom_classifier_predict_batch, the bat two-stage path and the geomodel range filter.
`bh_debug_custom_logits` (include/birda_hip_custom_debug.h) returns the last layer's activated output for host rows through the
same upload and launches, with the name of the last GEMM.

The inequality is that of tests/test_layer_gemm_gpu.py for the f32 GEMM (its `_tau` with terms 0 and its `_eps_act`), layer by
layer in float64.  A layer on the device's own input A obeys

    |got - act(A W + b)| <= own(A) = tau(K) 1.2 (|A| |W| + |b|) + eps_act(pre).

Only the last layer is read back, so the stack is held end to end: with r_i the float64 activations and E_i the bound on the
device's activations, |A| <= |r_{i-1}| + E_{i-1} and an activation of slope at most lip (1 for none / ReLU, 1/4 for the sigmoid)
give

    E_0 = 0,   E_i = lip_i (E_{i-1} |W_i|) + own_i(|r_{i-1}| + E_{i-1}),

the sum of the per-layer bounds pushed through |W| (eps_act taken at |pre| + the carried error).  A one-layer stack is the layer
test's inequality itself.

Shapes: the smallest that reach each branch of cc_build (rows re-laid to ld = align4(out), the first layer's K zero-padded to
k0, the copy taken for a weight offset that is not a multiple of 4), of cc_upload_rows (the 2-D upload) and of launch_pw_gemm
(K below, at and not a multiple of 32, a partial 16-column tile, several pick_nt choices, BM = 64 and BM = 128).

Worst error / bound on the MI355X: 3 -> 5 0.339, 6 -> 4 -> 1 0.027, 33 -> 64 -> 33 0.017, 36 -> 260 -> 30 0.057, 100 -> 4 -> 257 0.283,
1024 -> 64 -> 30 0.030, 36 -> 64 -> 4 -> 5 0.003, 3 841 rows of 36 -> 64 -> 257 0.082; two-stage f32 0.023, f16x3 / auto 0.041, re-run
rows 0.029; range filter 0.029.
"""
import ctypes as C
import math
import struct

import numpy as np
import pytest

from oracle import oracle as O
from test_layer_gemm_gpu import _eps_act, _tau

pytestmark = pytest.mark.gpu

WORST = {}
ACT = {"none": O.ACT_NONE, "relu": O.ACT_RELU, "sigmoid": O.ACT_SIGMOID}
LIP = {O.ACT_NONE: 1.0, O.ACT_RELU: 1.0, O.ACT_SIGMOID: 0.25}


def make_stack(dims, acts, seed, out_act=0):
    from birda_amd import modelfile as mf
    rng = np.random.default_rng(seed)
    layers = []
    for i, a in enumerate(acts):
        w = (rng.standard_normal((dims[i], dims[i + 1])) * math.sqrt(2.0 / dims[i])).astype(np.float32)
        b = rng.standard_normal(dims[i + 1]).astype(np.float32)
        layers.append(mf.CustomLayer(w, b, ACT[a]))
    return mf.CustomClassifierModel(dims[0], out_act, layers)


def stack64(model, x):
    """-> (float64 output of the stack, the end-to-end bound E) for rows x (f32 values)"""
    r = np.asarray(x, np.float32).astype(np.float64)
    E = np.zeros_like(r)
    for i, L in enumerate(model.layers):
        W, b = L.w.astype(np.float64), L.b.astype(np.float64)
        K = -(-W.shape[0] // 4) * 4 if i == 0 else W.shape[0]                   # (the first layer runs on k0 zero-padded columns)
        pre = r @ W + b
        carried = E @ np.abs(W)
        own = _tau(0, K) * 1.2 * ((np.abs(r) + E) @ np.abs(W) + np.abs(b)) + _eps_act(np.abs(pre) + carried, L.act)
        r, E = O.act64(pre, L.act), LIP[L.act] * carried + own
    return r, E


def debug_logits(cc, x):
    from birda_amd import _lib
    L = _lib.load()
    x = np.ascontiguousarray(x, np.float32).reshape(-1, cc.input_dim())
    out = np.full((x.shape[0], cc.num_classes()), np.float32(np.nan))
    name = C.create_string_buffer(128)
    _lib.check(L.bh_debug_custom_logits(cc._h, x.ctypes.data, x.shape[0], out.ctypes.data, name, 128))
    return out, name.value.decode()


def hold(tag, got, model, x, rows=None):
    ref, E = stack64(model, x)
    if rows is not None:
        got, ref, E = got[rows], ref[rows], E[rows]
    assert np.isfinite(got).all(), (tag, "non-finite output")
    err = np.abs(got.astype(np.float64) - ref)
    WORST[tag.split(":")[0]] = max(WORST.get(tag.split(":")[0], 0.0), float((err / E).max()))
    if (err > E).any():
        i = np.unravel_index(np.argmax(err / E), err.shape)
        pytest.fail(f"{tag}: {int((err > E).sum())} of {err.size} elements off, worst at {i}: got {got[i]!r} want {ref[i]!r}, err {err[i]:.3e} > bound {E[i]:.3e}")


def inputs(rng, n, k):
    return (rng.standard_normal((n, k)) * rng.uniform(0.2, 3.0, k)).astype(np.float32)


def open_cc(tmp_path, model, name="stack.bhc"):
    from birda_amd import modelfile as mf
    from birda_amd.classifier import CustomClassifier
    path = str(tmp_path / name)
    mf.write_custom_classifier(path, model)
    return CustomClassifier(path, None)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# input widths 3, 6, 33, 36, 100, 1024; hidden 4, 64, 260; outputs 1, 5, 30, 33, 257; none / ReLU / sigmoid
STACKS = [((3, 5), ("none",)), ((6, 4, 1), ("relu", "sigmoid")), ((33, 64, 33), ("sigmoid", "none")), ((36, 260, 30), ("relu", "none")),
          ((100, 4, 257), ("none", "relu")), ((1024, 64, 30), ("relu", "sigmoid")), ((36, 64, 4, 5), ("sigmoid", "relu", "sigmoid"))]


@pytest.mark.parametrize("dims,acts", STACKS, ids=["-".join(map(str, d)) for d, _ in STACKS])
def test_stack_matches_float64(tmp_path, dims, acts):
    """1, 7, 65 and 129 rows (one 64-row tile, a partial one, two, and one row past two), ascending and then 7 again: the buffers
    grow between the calls."""
    model = make_stack(dims, acts, seed=sum(dims))
    cc = open_cc(tmp_path, model)
    rng = np.random.default_rng(dims[0])
    names = set()
    try:
        assert cc.input_dim() == dims[0] and cc.num_classes() == dims[-1]
        for n in (1, 7, 65, 129, 7):
            x = inputs(rng, n, dims[0])
            got, name = debug_logits(cc, x)
            names.add(name)
            hold(f"stack {dims}: {n} rows {name}", got, model, x)
        assert all(s.startswith("pw_gemm_kernel<BM=64,NT=") for s in names), names
    finally:
        print(f"custom stack {dims} {acts}: {sorted(names)}, worst error / bound {WORST.get(f'stack {dims}', 0.0):.3f}")
        cc.close()


def test_the_wide_tile_branch_and_the_buffers(tmp_path):
    """36 -> 64 -> 257: pick_nt(257) is 1 (17 column tiles), so 3841 rows are the fewest with 31 x 17 >= 512 blocks of 128 rows:
    BM = 128 there, BM = 64 at 3840.  Three rows, then the large count, then the same three rows: the two small results are
    bit-equal; every row of the large call is bit-equal to its row in a three-row call (a row's sum does not depend on the tile
    it sat in, and nothing of an earlier, larger call is left in the buffers)."""
    dims = (36, 64, 257)
    model = make_stack(dims, ("relu", "none"), seed=11)
    cc = open_cc(tmp_path, model)
    rng = np.random.default_rng(12)
    try:
        big = inputs(rng, 3841, 36)
        first, name3 = debug_logits(cc, big[:3])
        assert name3 == "pw_gemm_kernel<BM=64,NT=1>"
        got, name = debug_logits(cc, big)
        assert name == "pw_gemm_kernel<BM=128,NT=1>", name
        hold(f"wide: 3841 rows {name}", got, model, big)
        again, _ = debug_logits(cc, big[:3])
        assert np.array_equal(bits(first), bits(again)) and np.array_equal(bits(first), bits(got[:3]))
        below, name = debug_logits(cc, big[:3840])
        assert name == "pw_gemm_kernel<BM=64,NT=1>" and np.array_equal(bits(below), bits(got[:3840]))
        for r0 in range(0, 3841, 3):
            part, _ = debug_logits(cc, big[r0:r0 + 3])
            assert np.array_equal(bits(part), bits(got[r0:r0 + 3])), r0
        # the ranking entry point on the same buffers: a small batch after the large one
        res = cc.predict_batch(big[:3])
        assert [p.index for p in res[1].predictions][:5] == np.argsort(-got[1].astype(np.float64), kind="stable")[:5].tolist()
    finally:
        print(f"custom stack wide: worst error / bound {WORST.get('wide', 0.0):.3f}")
        cc.close()


def test_a_weight_offset_that_is_not_a_multiple_of_four(tmp_path):
    """A container packed by hand (modelfile's formats) whose second layer's weights start at float 1 (mod 4): modelfile's own
    writer aligns every chunk to 16 floats, so cc_build's copy for `w_off % 4 != 0` never ran.  The reader accepts the file; the
    stack matches."""
    from birda_amd import modelfile as mf
    from birda_amd.classifier import CustomClassifier
    model = make_stack((8, 4, 8), ("relu", "none"), seed=21)             # (ld == out and no K padding: only the offset asks for the copy)
    l0, l1 = model.layers
    chunks, offs, off = [], [], 0
    for arr, align in ((l0.w, 16), (l0.b, 16), (l1.w, None), (l1.b, 1)):
        if align is None:
            pad = (1 - off) % 4 or 4                                     # w_off = 1 (mod 4)
        else:
            pad = (-off) % align
        chunks.append(np.full(pad, 1e30, np.float32)); off += pad       # (padding a wrong offset would read shows up)
        offs.append(off); chunks.append(arr.ravel()); off += arr.size
    assert offs[2] % 4 == 1
    blob = np.concatenate(chunks).astype("<f4")
    recs = [struct.pack(mf.CUSTOM_LAYER_FMT, 8, 4, l0.act, 0, offs[0], offs[1]), struct.pack(mf.CUSTOM_LAYER_FMT, 4, 8, l1.act, 0, offs[2], offs[3])]
    path = str(tmp_path / "odd.bhc")
    with open(path, "wb") as f:
        f.write(struct.pack(mf.CUSTOM_HEADER_FMT, mf.CUSTOM_MAGIC, 1, 8, 2, 8, 0, 256, blob.size).ljust(64, b"\0"))
        f.write(b"".join(recs).ljust(256 - 64, b"\0"))
        f.write(blob.tobytes())
    cc = CustomClassifier(path, None)
    ref = open_cc(tmp_path, model, "aligned.bhc")
    try:
        x = inputs(np.random.default_rng(22), 7, 8)
        got, name = debug_logits(cc, x)
        hold(f"odd offset: {name}", got, model, x)
        assert np.array_equal(bits(got), bits(debug_logits(ref, x)[0]))   # the aligned file: the same bits
    finally:
        cc.close(); ref.close()


def test_rows_are_isolated(tmp_path):
    """One input row of 1e30 leaves every other row's bits unchanged (its own overflows); 1e30 under a zero weight row changes
    nothing at all; a NaN in one row reaches that row only."""
    model = make_stack((36, 64, 33), ("none", "none"), seed=31)
    model.layers[0].w[5, :] = 0.0
    cc = open_cc(tmp_path, model)
    try:
        x = inputs(np.random.default_rng(32), 65, 36)
        base, _ = debug_logits(cc, x)
        hold("isolation: base", base, model, x)
        others = np.arange(65) != 17
        huge = x.copy(); huge[17, :] = 1e30
        got, _ = debug_logits(cc, huge)
        assert np.array_equal(bits(got[others]), bits(base[others])) and np.abs(got[17]).max() > 1e25
        zero = x.copy(); zero[17, 5] = 1e30                              # 1e30 * 0: nothing
        got, _ = debug_logits(cc, zero)
        assert np.array_equal(bits(got[others]), bits(base[others]))
        hold("isolation: 1e30 under a zero weight row", got, model, zero, rows=[17])
        nan = x.copy(); nan[17, 3] = np.nan
        got, _ = debug_logits(cc, nan)
        assert np.array_equal(bits(got[others]), bits(base[others])) and np.isnan(got[17]).all()
    finally:
        cc.close()


# ---------------------------------------------------------------------------------------------------------------
# the two-stage path and the range filter
# ---------------------------------------------------------------------------------------------------------------
def test_two_stage_logits_match_float64_on_the_backbones_embeddings(model_dir, tmp_path):
    """f32 / f16x3 / auto backbones, a context smaller than the batch: logits_out is the stack applied to the embeddings that
    predict_logits(..., want_embeddings=True) returns, under the bound."""
    from birda_amd import synth
    from birda_amd.classifier import BirdClassifier
    path, labels, m, _ = model_dir["mini_b0"]
    model = synth.build_custom_classifier(m.embedding_dim, 30, (64,))
    cc = open_cc(tmp_path, model)
    segs = synth.synth_segments(7, m.sample_count, m.sample_rate, start=3)
    try:
        for prec in ("f32", "f16x3", "auto"):
            clf = BirdClassifier(path, labels, precision=prec)
            ctx = clf.create_batch_context(4)
            try:
                _, got = clf.predict_batch_two_stage(ctx, cc, list(segs), want_logits=True)
                _, emb = clf.predict_logits(ctx, segs, want_embeddings=True)
                hold(f"two-stage {prec}: 7 rows", got, model, emb)
            finally:
                ctx.close(); clf.close()
    finally:
        print(f"two-stage: worst error / bound { {k: round(v, 3) for k, v in WORST.items() if k.startswith('two-stage')} }")
        cc.close()


def test_two_stage_rows_rerun_on_f32_reach_the_stack_repaired(tmp_path):
    """BH_FLAG_AUTO on a model whose rows leave the f16 range (tests/test_multi_gpu.py builds it so): the rows settled on the f32
    kernels reach cc_run through the arena's embedding tensor.  Every row under the bound against the embeddings the auto
    classifier reports; the re-run rows -- those whose reported embedding is the f32 classifier's, bit for bit -- against the f32
    classifier's."""
    from birda_amd import modelfile as mf, synth
    from birda_amd.classifier import BirdClassifier
    from test_parity_gpu import _rescale_trunk
    m = synth.build_model("mini_b0")
    m2, _ = _rescale_trunk(m, [2.0 ** 14])
    path = str(tmp_path / "overflow.bhm")
    mf.write_model(path, m2)
    model = synth.build_custom_classifier(m.embedding_dim, 30, (64,))
    cc = open_cc(tmp_path, model)
    segs = synth.synth_segments(12, m.sample_count, m.sample_rate, start=40)
    auto = BirdClassifier(path, None, precision="auto")
    f32 = BirdClassifier(path, None, precision="f32")
    ctx, ctx32 = auto.create_batch_context(5), f32.create_batch_context(5)
    try:
        _, got = auto.predict_batch_two_stage(ctx, cc, list(segs), want_logits=True)
        assert auto.fallback_segments() > 0
        _, emb = auto.predict_logits(ctx, segs, want_embeddings=True)
        _, emb32 = f32.predict_logits(ctx32, segs, want_embeddings=True)
        assert np.isfinite(emb).all() and np.isfinite(emb32).all()
        hold("two-stage overflow: all rows", got, model, emb)
        rerun = [i for i in range(12) if np.array_equal(bits(emb[i]), bits(emb32[i]))]
        assert 0 < len(rerun), "no row came back from the f32 kernels"
        hold("two-stage overflow: re-run rows", got, model, emb32, rows=rerun)
        print(f"two-stage overflow: {len(rerun)} of 12 rows re-run, worst error / bound {WORST['two-stage overflow']:.3f}")
    finally:
        ctx.close(); ctx32.close(); auto.close(); f32.close(); cc.close()


def test_range_filter_scores_match_float64(tmp_path):
    """RangeFilter on a 3 -> 16 -> 257 stack (the three inputs zero-padded to four, one row through the 2-D upload) over twelve
    (latitude, longitude, week) points: every score against float64; the kept list is exactly score >= threshold on the
    returned f32 scores."""
    from birda_amd import modelfile as mf
    from birda_amd.classifier import RangeFilter
    model = make_stack((3, 16, 257), ("relu", "sigmoid"), seed=41)
    model.layers[0].w *= np.float32(0.02)                                # (latitudes and longitudes are of order 100)
    path, labels = str(tmp_path / "geo.bhc"), str(tmp_path / "geo.txt")
    mf.write_custom_classifier(path, model)
    open(labels, "w").write("".join(f"Genus species{i}_Name {i}\n" for i in range(257)))
    thr = 0.3
    rf = RangeFilter(path, labels, threshold=thr)
    try:
        assert rf.num_species() == 257
        rng = np.random.default_rng(42)
        kept_total = 0
        for k in range(12):
            lat, lon, week = float(rng.uniform(-90, 90)), float(rng.uniform(-180, 180)), float(rng.integers(1, 49))
            scores, kept = rf.predict_week(lat, lon, week)
            hold("range filter: scores", scores[None, :], model, np.asarray([[lat, lon, week]], np.float32))
            assert kept.tolist() == np.flatnonzero(scores >= np.float32(thr)).tolist(), k
            kept_total += kept.size
        assert 0 < kept_total < 12 * 257
        print(f"range filter: worst error / bound {WORST['range filter']:.3f}")
    finally:
        rf.close()
