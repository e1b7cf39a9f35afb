"""Channel concatenation, channel windows and the channel shuffle (OP_CONCAT) on the device: the two instantiations behind
launch_concat -- concat_kernel<PLAIN> and concat_kernel<SHUFFLE> -- alone through bh_debug_concat, and inside models through
bh_classifier_create.

The launch is a copy, so the kernel tests have no tolerance: every output element is compared AS A 32-BIT INTEGER with the gather
numpy makes of the same operands.  The operands are random 32-bit patterns (all of NaN space, subnormals, -0, inf); every source
value outside its window is a poison payload that must not occur in the output.  The shapes are the smallest that reach every path:
one to four sources, windows at offsets, lengths of one 16-byte group up to 65, a group count whose C / g is no multiple of 4, group
boundaries inside the sources, 1 x 1, 5 x 7 and 9 x 11 images in one and three segments, and one launch past the launcher's
workgroup cap, where the grid-stride loop takes a second trip.  Offsets beyond 2^32 bytes are not run (8 GB of operands): the 64-bit
arithmetic of concat_at and of the loop index is held by reading kernels_concat.hip only.

The product path: random multi-branch plans on the .onnx route against the float64 forward of tests/test_concat.py at the
LOGIT_RTOL / F16_LOGIT_RTOL of tests/test_resact_gpu.py, every concat tensor of a keep-tensors context against the gather of its
sources read back the same way, logits that do not depend on the launch size (the arena plan), the one-launch chain step of an
N-way Concat against the record-by-record schedule (the same bits), and the non-finite contract.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from birda_amd import _lib, convert, modelfile as mf, onnx_io as ox, synth
from test_concat import forward64, gather
from test_resact_gpu import BH_ERR_NONFINITE, F16_LOGIT_RTOL, LOGIT_RTOL

pytestmark = pytest.mark.gpu

UNWRITTEN, GUARD, POISON = 0x7fc0beef, 0x7fc00000, 0xffd0d0d0
PLAIN, SHUFFLE = "concat_kernel<PLAIN>", "concat_kernel<SHUFFLE>"
UNSUPPORTED, INVALID = -6, -1
REACHED = set()
IMAGES = ((1, 1), (5, 7), (9, 11))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _concat(X, h, w, groups, windows, n_seg, expect=0):
    """X: the sources [n_seg][h][w][total] as uint32; windows: [(total, off, len)] -> (Y [n_seg][h][w][C] as uint32, kernel name)"""
    lib = _lib.load()
    ctot = sum(ln for _, _, ln in windows)
    out = np.empty((n_seg, h, w, max(ctot, 1)), np.uint32)
    shape = np.asarray([h, w, groups] + [v for win in windows for v in win], np.int32)
    ptrs = (C.c_void_p * 4)(*[x.ctypes.data for x in X] + [None] * (4 - len(X)))
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_concat(0, ptrs, len(X), _p(out), n_seg, _p(shape), name, 128)
    if expect:
        assert rc == expect, (rc, lib.bh_last_error())
        return None, lib.bh_last_error().decode()
    assert rc == 0, (rc, lib.bh_last_error())
    REACHED.add(name.value.decode())
    return out, name.value.decode()


def _sources(rng, h, w, windows, n_seg):
    """random 32-bit patterns inside the windows, POISON outside"""
    X = []
    for total, off, ln in windows:
        x = np.full((n_seg, h, w, total), POISON, np.uint32)
        v = rng.integers(0, 1 << 32, (n_seg, h, w, ln), dtype=np.uint64).astype(np.uint32)
        v[np.isin(v, (UNWRITTEN, GUARD, POISON))] = 0x80000000        # (-0: the three marker values stay markers)
        x[..., off:off + ln] = v
        X.append(x)
    return X


def _want(X, windows, groups):
    cat = np.concatenate([x[..., off:off + ln] for x, (_, off, ln) in zip(X, windows)], axis=-1)
    if groups > 1:
        ctot = cat.shape[-1]
        c = np.arange(ctot)
        cat = cat[..., (c % groups) * (ctot // groups) + c // groups]
    return cat


def _hold(windows, groups, images=IMAGES, segments=(1, 3), seed=0):
    rng = np.random.default_rng(1000 * seed + 31 * sum(sum(win) for win in windows) + groups)
    for h, w in images:
        for n_seg in segments:
            X = _sources(rng, h, w, windows, n_seg)
            got, name = _concat(X, h, w, groups, windows, n_seg)
            assert name == (SHUFFLE if groups > 1 else PLAIN), name
            want = _want(X, windows, groups)
            assert not (got == UNWRITTEN).any(), "elements never written"
            assert not (got == POISON).any(), "a channel outside a window was read"
            assert not (got == GUARD).any(), "a guard band was read"
            bad = got != want
            assert not bad.any(), (windows, groups, (h, w), n_seg, int(bad.sum()), np.argwhere(bad)[0])
            # the patterns really are arbitrary: NaNs with payloads, subnormals and negative values all travel
            if got.size >= 4096:
                f = got.view(np.float32)
                assert np.isnan(f).any() and ((got & 0x7f800000) == 0).any() and (got >> 31).any()


whole = lambda *lens: [(ln, 0, ln) for ln in lens]
PLAIN_CASES = {
    "4+4": whole(4, 4), "4+8": whole(4, 8), "8+4": whole(8, 4), "12+20": whole(12, 20), "64+4": whole(64, 4), "4+260": whole(4, 260),
    "8of16from4+12of24from12": [(16, 4, 8), (24, 12, 12)],
    "first_half+second_half": [(32, 0, 16), (32, 16, 16)],
    "second_half+first_half": [(16, 8, 8), (16, 0, 8)],
    "slice_8of16from4": [(16, 4, 8)], "slice_12of24from12": [(24, 12, 12)], "slice_first_half": [(16, 0, 8)], "slice_second_half": [(16, 8, 8)],
    "whole_copy": whole(20),
    "three": [(8, 0, 8), (16, 4, 8), (12, 0, 12)],
    "four": [(4, 0, 4), (24, 12, 12), (8, 0, 8), (20, 4, 16)],
}


@pytest.mark.parametrize("case", sorted(PLAIN_CASES))
def test_plain_concat_is_the_gather_bit_for_bit(case):
    _hold(PLAIN_CASES[case], 0)
    _hold(PLAIN_CASES[case], 1, images=((5, 7),), segments=(3,))          # one group: no shuffle either


SHUFFLE_CASES = [(8, 2), (12, 2), (12, 3), (24, 2), (24, 3), (24, 4), (40, 8), (48, 2), (48, 3), (48, 4), (48, 8)]


@pytest.mark.parametrize("ctot,groups", SHUFFLE_CASES)
def test_shuffle_is_reshape_transpose_reshape_bit_for_bit(ctot, groups):
    _hold(whole(ctot), groups)                                             # a whole-tensor shuffle with no second source
    _hold([(ctot // 2 // 4 * 4 + 8, 4, ctot // 2 // 4 * 4), (ctot, 0, ctot - ctot // 2 // 4 * 4)], groups)     # two windows, the first at an offset
    # the formula is the operator chain: Reshape [g, C / g] -> Transpose -> Reshape
    c = np.arange(ctot)
    assert ((c % groups) * (ctot // groups) + c // groups == c.reshape(groups, ctot // groups).T.reshape(-1)).all()


def test_shuffle_whose_group_boundaries_fall_inside_the_sources():
    _hold(whole(8, 16), 3)                 # C = 24, C / g = 8: group 1 = channels 8 .. 15 starts at the seam, group 2 lies inside B ...
    _hold(whole(16, 8), 3)                 # ... and here group 1 straddles the seam
    _hold([(8, 0, 8), (16, 4, 8), (12, 0, 12), (12, 4, 8)], 4)       # four sources, C = 36, C / g = 9: groups end inside every source
    _hold([(8, 0, 8), (16, 4, 8), (12, 0, 12)], 7)                   # three sources, C = 28, C / g = 4


def test_a_launch_past_the_workgroup_cap_takes_a_second_trip():
    """3 segments of 32 x 43 x 512: 528 384 groups of 16 bytes, more than the launcher's 2 048 workgroups x 256 threads = 524 288, so
    the first 4 096 threads take a second trip of the grid-stride loop; plain and shuffled"""
    h, w, ctot, n_seg = 32, 43, 512, 3
    assert n_seg * h * w * (ctot // 4) == 528384 > 256 * 8 * 256 == 524288
    _hold([(256, 0, 256), (384, 128, 256)], 0, images=((h, w),), segments=(n_seg,))
    _hold([(256, 0, 256), (384, 128, 256)], 2, images=((h, w),), segments=(n_seg,))


def test_the_entry_refuses_what_has_no_kernel():
    rng = np.random.default_rng(5)
    ok = [(16, 4, 8), (8, 0, 8)]
    X = _sources(rng, 5, 7, ok, 1)
    for windows, groups in (([(16, 2, 8), (8, 0, 8)], 0),        # an offset that is no multiple of 4
                            ([(16, 4, 6), (8, 0, 8)], 0),        # a length that is no multiple of 4
                            ([(16, 12, 8), (8, 0, 8)], 0),       # a window past its source
                            ([(16, 4, 0), (8, 0, 8)], 0),        # an empty window
                            ([(16, 4, 8), (8, 0, 8)], 3),        # 16 % 3
                            ([(16, 4, 8), (8, 0, 8)], 32),       # more groups than channels
                            ([(16, 4, 8), (8, 0, 8)], -1)):
        _, msg = _concat(X, 5, 7, groups, windows, 1, expect=UNSUPPORTED)
        assert "concat" in msg, msg
    _, msg = _concat(X, 5, 7, 0, [(18, 4, 8), (8, 0, 8)], 1, expect=UNSUPPORTED)     # a source of 18 channels
    assert "multiple of 4" in msg, msg
    lib = _lib.load()
    out = np.empty(16, np.uint32)
    shape = np.asarray([1, 1, 0] + [4, 0, 4] * 5, np.int32)
    ptrs = (C.c_void_p * 5)(*[X[0].ctypes.data] * 5)
    assert lib.bh_debug_concat(0, ptrs, 5, _p(out), 1, _p(shape), None, 0) == INVALID      # five sources
    assert lib.bh_debug_concat(0, ptrs, 0, _p(out), 1, _p(shape), None, 0) == INVALID


# ---- the product path ---------------------------------------------------------------------------------------------------------------
def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def _concats(m):
    return [i for i, L in enumerate(m.layers) if L.op == mf.OP_CONCAT]


def _check_concat_kernels(clf, m, what):
    for i in _concats(m):
        assert clf.layer_kernel(i) == (SHUFFLE if m.layers[i].reserved > 1 else PLAIN), (what, i, clf.layer_kernel(i))


_PLAN_REF = {}


def _plan(seed):
    """-> (model, segments, float64 logits): computed once, shared by the tests below"""
    if seed not in _PLAN_REF:
        m = synth.build_model("branchy_plan", plan=synth.random_branchy_plan(seed))
        segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=5 + seed)
        segs[2] *= np.float32(0.01)
        _PLAN_REF[seed] = (m, segs, forward64(m, segs))
    return _PLAN_REF[seed]


@pytest.mark.parametrize("seed", range(6))
def test_random_branchy_plans_on_the_onnx_route(seed, tmp_path):
    from birda_amd.classifier import BirdClassifier
    m, segs, ref = _plan(seed)
    assert len(_concats(m)) >= 10
    path = _write(str(tmp_path / "x.onnx"), convert.model_to_onnx(m, frontend_spelling="stft"))
    scale = max(1.0, float(np.abs(ref).max()))
    for prec, tol in [("f32", LOGIT_RTOL), ("f16x3", LOGIT_RTOL), ("auto", LOGIT_RTOL)] + ([("f16", F16_LOGIT_RTOL)] if seed == 1 else []):
        clf = BirdClassifier(path, None, precision=prec)
        ctx = clf.create_batch_context(3)
        got = clf.predict_logits(ctx, segs)
        err = float(np.abs(got - ref).max())
        print(f"branchy plan {seed} {prec}: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (tol * scale):.3f})")
        assert np.isfinite(got).all() and err <= tol * scale, (prec, err, scale)
        _check_concat_kernels(clf, m, (seed, prec))
        ctx.close(); clf.close()


def test_a_float16_file_with_concats(tmp_path):
    """the float16 rewrite of a plan's graph: the reference is the float64 forward of the container the library's own reader makes
    of it (its weights are the file's float16 values)"""
    from birda_amd.classifier import BirdClassifier
    m, segs, _ = _plan(2)
    p16 = _write(str(tmp_path / "x16.onnx"), ox.dump(convert.graph_to_float16(convert.graph_from_model(m, frontend_spelling="conv1d"))))
    bhm = str(tmp_path / "x16.bhm")
    L = _lib.load()
    assert L.bh_onnx_to_bhm(p16.encode(), bhm.encode()) == 0, L.bh_last_error()
    m16 = mf.read_model(bhm)
    assert [(a.op, a.act, a.reserved, a.in_tensor, a.res_tensor) for a in m16.layers] == [(a.op, a.act, a.reserved, a.in_tensor, a.res_tensor) for a in m.layers]
    ref = forward64(m16, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    clf = BirdClassifier(p16, None, precision="auto")
    assert clf.weight_summary()["float16_file"]
    ctx = clf.create_batch_context(3)
    got = clf.predict_logits(ctx, segs)
    err = float(np.abs(got - ref).max())
    print(f"float16 file, auto: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    _check_concat_kernels(clf, m16, "float16 file")
    ctx.close(); clf.close()


def test_shufflenet_audio_runs_and_matches_float64(tmp_path):
    """synth's timing model, two segments in auto: finite logits at LOGIT_RTOL of the float64 forward"""
    from birda_amd.classifier import BirdClassifier
    m = synth.build_model("shufflenet_audio", n_classes=40)
    assert len(_concats(m)) == 16 + 13 and sum(m.layers[i].reserved == 2 for i in _concats(m)) == 16
    path = str(tmp_path / "shufflenet.bhm")
    mf.write_model(path, m)
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=2)
    ref = forward64(m, segs)
    scale = max(1.0, float(np.abs(ref).max()))
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(2)
    got = clf.predict_logits(ctx, segs)
    ctx.close()
    err = float(np.abs(got - ref).max())
    print(f"shufflenet_audio auto: max|dlogit| = {err:.3e} of scale {scale:.2f} (share {err / (LOGIT_RTOL * scale):.3f})")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    _check_concat_kernels(clf, m, "shufflenet_audio")
    clf.close()


def test_every_concat_tensor_is_the_gather_of_its_sources_in_a_model(tmp_path, monkeypatch):
    """BIRDA_HIP_KEEP_TENSORS, f32: every concat record's tensor, read back, equals bit for bit the gather of its source tensors read
    back the same way"""
    from birda_amd.classifier import BirdClassifier
    m, segs, _ = _plan(3)
    path = str(tmp_path / "k.bhm")
    mf.write_model(path, m)
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    clf = BirdClassifier(path, None, precision="f32")
    ctx = clf.create_batch_context(3)
    clf.predict_logits(ctx, segs)
    seen = set()
    for i in _concats(m):
        Lr = m.layers[i]
        A = clf.read_tensor(ctx, Lr.in_tensor, 3).view(np.uint32)
        B = None if Lr.res_tensor == mf.NO_TENSOR else clf.read_tensor(ctx, Lr.res_tensor, 3).view(np.uint32)
        Y = clf.read_tensor(ctx, i + 1, 3).view(np.uint32)
        want = gather(Lr, A, B, 3)
        assert (Y.reshape(want.shape) == want).all(), i
        assert clf.layer_kernel(i) == (SHUFFLE if Lr.reserved > 1 else PLAIN)
        seen.add((B is not None, Lr.reserved > 1, Lr.w_off > 0))
    assert {(True, False, False), (True, True, False), (False, False, True), (False, True, False)} <= seen, seen
    ctx.close(); clf.close()


def test_logits_do_not_depend_on_the_launch_size(tmp_path):
    """One plan at 3, 80 and 600 segments in ordinary contexts: a segment's logits are the same bits in all three -- a concat output
    planned over a source that is still live would show here (at 600 segments the arena is reused hardest)"""
    from birda_amd.classifier import BirdClassifier
    m, segs, ref = _plan(4)
    path = str(tmp_path / "a.bhm")
    mf.write_model(path, m)
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(3)
    first = clf.predict_logits(ctx, segs)
    ctx.close()
    assert np.abs(first - ref).max() <= LOGIT_RTOL * max(1.0, float(np.abs(ref).max()))
    for n in (80, 600):
        ctx = clf.create_batch_context(n)
        ctx.set_sub_slices(1)
        pick = np.arange(n) % 3
        got = clf.predict_logits(ctx, np.ascontiguousarray(segs[pick]))
        assert (got.view(np.uint32) == first.view(np.uint32)[pick]).all(), n
        ctx.close()
    clf.close()


def six_way_model():
    """The mini front-end, a 3x3 stride-2 stem to 16 channels, six 1x1 branches of 8 / 12 / 4 / 8 / 16 / 8 channels of it, their 6-way
    Concat (five records) shuffled in 4 groups, a 1x1 head, the global pool and a dense layer"""
    b = synth._Builder(np.random.default_rng(21))
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    s, h, w = b.conv(0, br.n_mels, br.n_frames, 1, 16, 3, 2, mf.ACT_GELU_ERF, in_layout=1)
    widths = (8, 12, 4, 8, 16, 8)
    parts = [(b.pwconv(s, h, w, 16, c, mf.ACT_GELU_ERF), 0, c) for c in widths]
    t, c = b.concat(parts, h, w, 4)
    t = b.pwconv(t, h, w, c, 32, mf.ACT_GELU_ERF)
    t = emb = b.gap(t, h, w, 32)
    b.dense(t, 32, 20, gain=1.5)
    return mf.Model(0, sr, n, n / sr, 20, 32, mf.OUT_SIGMOID, emb, br.n_mels, br.n_frames, 1e-6, [br], b.layers, np.concatenate(b.chunks))


PATH_LAYER, PATH_INNER, PATH_CONCAT = 0, 5, 6          # include/birda_hip_audit.h


@pytest.mark.parametrize("which", ["six_way", "plan_0", "plan_1"])
def test_the_chain_step_and_the_record_by_record_schedule_give_the_same_bits(which, tmp_path, monkeypatch):
    """An N-way Concat is one step of an ordinary context's schedule (BH_PATH_CONCAT on its first record, the others inside it, their
    tensors without bytes; more than four leaves: several steps) and N - 1 launches in a keep-tensors context.  BH_FLAG_F32 and
    BIRDA_HIP_KEEP_FUSED: every other layer runs the same kernel in both, so the logits are the same bits."""
    from birda_amd.classifier import BirdClassifier
    from test_arena_plan_gpu import arena_plan
    if which == "six_way":
        m = six_way_model()
        segs = synth.synth_segments(3, m.sample_count, m.sample_rate, start=4)
        ref = forward64(m, segs)
    else:
        m, segs, ref = _plan(int(which[-1]))
    path = str(tmp_path / "c.bhm")
    mf.write_model(path, m)
    clf = BirdClassifier(path, None, precision="f32")
    ctx = clf.create_batch_context(3)
    got = clf.predict_logits(ctx, segs)
    assert np.abs(got - ref).max() <= LOGIT_RTOL * max(1.0, float(np.abs(ref).max()))
    _check_concat_kernels_of_chains(clf, m)
    _, sizes, tags = arena_plan(clf, ctx, 0)
    cats = _concats(m)
    chained = [i for i in cats if tags[i] == PATH_CONCAT]
    assert chained and all(tags[i] in (PATH_LAYER, PATH_CONCAT, PATH_INNER) for i in cats)
    for i in chained:
        k = i + 1
        while k < len(m.layers) and tags[k] == PATH_INNER and m.layers[k].op == mf.OP_CONCAT:
            assert m.layers[k].in_tensor == k and sizes[k] == 0, (k, sizes[k])        # the record in front: read whole, its tensor without bytes
            k += 1
        leaves = (1 if m.layers[i].res_tensor == mf.NO_TENSOR else 2) + (k - i - 1)
        assert 2 <= k - i and leaves <= 4, (i, k, leaves)
    if which == "six_way":        # 2 + 1 + 1 leaves, then the step's output + 1 + 1: [CONCAT, INNER, INNER, CONCAT, INNER]
        assert [tags[i] for i in cats] == [PATH_CONCAT, PATH_INNER, PATH_INNER, PATH_CONCAT, PATH_INNER]
    else:                         # the 4-way Inception module is one step of three records
        assert any(tags[i:i + 3] == [PATH_CONCAT, PATH_INNER, PATH_INNER] for i in cats)
    ctx.close()
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    monkeypatch.setenv("BIRDA_HIP_KEEP_FUSED", "1")
    ctx = clf.create_batch_context(3)
    by_record = clf.predict_logits(ctx, segs)
    _, _, tags_keep = arena_plan(clf, ctx, 0)
    assert all(tags_keep[i] == PATH_LAYER for i in cats)
    assert (by_record.view(np.uint32) == got.view(np.uint32)).all()
    ctx.close(); clf.close()


def _check_concat_kernels_of_chains(clf, m):
    """every record of a chain names the one launch's instantiation: the last record's"""
    for i in _concats(m):
        assert clf.layer_kernel(i) in (PLAIN, SHUFFLE), (i, clf.layer_kernel(i))


def overflow_model():
    """The mini front-end, a 3x3 stride-2 stem to 32 channels, a LINEAR 1x1 layer 32 -> 32, a second linear 1x1 layer 32 -> 32, a
    Concat of the second half of its output behind the stem's first half, shuffled in 4 groups, a 1x1 head, the global pool and a
    dense layer"""
    b = synth._Builder(np.random.default_rng(13))
    sr, n = 48000, 12000
    br = mf.Branch(512, 100, 32, (n - 512) // 100 + 1, 0.0, 3000.0, 1.23)
    br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(br.n_mels, br.n_bins, sr, br.fmin, br.fmax))
    br.out_scale, br.out_shift = 0.8, -0.4
    s, h, w = b.conv(0, br.n_mels, br.n_frames, 1, 32, 3, 2, mf.ACT_GELU_ERF, in_layout=1)
    t = b.pwconv(s, h, w, 32, 32, mf.ACT_NONE)
    t = b.pwconv(t, h, w, 32, 32, mf.ACT_NONE)
    t, c = b.concat([(s, 0, 16), (t, 16, 16)], h, w, 4)
    t = b.pwconv(t, h, w, c, 64, mf.ACT_GELU_ERF)
    t = emb = b.gap(t, h, w, 64)
    b.dense(t, 64, 30, gain=1.5)
    return mf.Model(0, sr, n, n / sr, 30, 64, mf.OUT_SIGMOID, emb, br.n_mels, br.n_frames, 1e-6, [br], b.layers, np.concatenate(b.chunks))


def test_f16_overflow_in_front_of_a_concat_is_not_laundered(tmp_path):
    """The first linear layer's weights and bias times 2^20 (its output, ~1e6, is past 65 504) and the second's weights divided by
    2^20: the same function in f32 arithmetic.  The split-f16 GEMM of the second layer cannot represent its operand; the NaN / inf it
    computes must pass the concat -- f16x3 ends in BH_ERR_NONFINITE --, and auto re-runs the rows on the f32 kernels."""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    m0 = overflow_model()
    m = copy.deepcopy(m0)
    blob = m.blob.copy()
    L1, L2, Cc = m.layers[1], m.layers[2], m.layers[3]
    assert L1.act == L2.act == mf.ACT_NONE and L1.op == L2.op == mf.OP_PWCONV and Cc.op == mf.OP_CONCAT and Cc.reserved == 4
    s = np.float32(2.0 ** 20)
    blob[L1.w_off:L1.w_off + L1.cin * L1.cout] *= s
    blob[L1.b_off:L1.b_off + L1.cout] *= s
    blob[L2.w_off:L2.w_off + L2.cin * L2.cout] /= s
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
    assert clf.layer_kernel(3) == SHUFFLE, clf.layer_kernel(3)
    ctx.close(); clf.close()
    clf = BirdClassifier(path, None, precision="auto")
    ctx = clf.create_batch_context(4)
    got = clf.predict_logits(ctx, segs)
    assert clf.fallback_segments() > 0
    err = float(np.abs(got - ref).max())
    print(f"overflow in front of a concat, auto: max|dlogit| = {err:.3e} of {scale:.2f}, {clf.fallback_segments()} segments re-run")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale
    ctx.close(); clf.close()


# ---- both instantiations were reached (keep last: it reads what the tests above ran) -------------------------------------------------
def test_both_instantiations_were_reached():
    """Run with the module, it reads what the tests above launched; alone or under -k it launches what is missing itself."""
    for groups, name in ((0, PLAIN), (2, SHUFFLE)):
        if name not in REACHED:
            _hold(whole(8, 8), groups, images=((5, 7),), segments=(1,))
    assert REACHED == {PLAIN, SHUFFLE}, sorted(REACHED)
