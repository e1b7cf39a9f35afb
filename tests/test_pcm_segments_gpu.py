"""The device PCM front end on the MI355X: what segment_pcm_kernel<FMT> wrote for the last slice of a bh_predict_pcm / _rows /
_fd_rows / _at call (read back with bh_debug_read_segments, include/birda_hip_pcm_debug.h) against tests/test_pcm_segments.py
segments_ref, every sample as a uint32 -- no tolerance; a NaN that went through a channel mix: isnan on both sides.  The
catalogue, the reference and their CPU checks are in that module.

Each case goes through the entry point a caller uses, on an ordinary context (lanes on), twice: the case's stream, then a shorter
stream of other samples on the same context.  Cases with sub-slices repeat the first call under set_sub_slices(1 / 2 / 5 / 0).
On the resampling route the raw rows (which 1) are held to the reference at the source-rate length, and the model-rate rows
(which 0) to bh_resample_device run by the test on those same raw rows: bit for bit, no resampler tolerance of its own.

The library changes this module was shown to fail on are listed in DESIGN.md section 3."""
import os
import sys
import time

import numpy as np
import pytest

from birda_amd import modelfile as mf

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_pcm_segments as P                                      # noqa: E402  (the catalogue and the reference)

pytestmark = pytest.mark.gpu

BH_ERR_INVALID, BH_ERR_UNSUPPORTED = -1, -6
FD_OFFSET = 4099                     # odd, past a page
RAN = {}                             # case id -> samples compared
T0 = time.time()


@pytest.fixture(scope="module")
def clfs(tmp_path_factory):
    """sample_count -> a classifier on the token model of that segment length, created on first use"""
    from birda_amd.classifier import BirdClassifier
    d = tmp_path_factory.mktemp("pcm_models")
    made = {}

    def get(S):
        if S not in made:
            path = str(d / f"pcm_{S}.bhm")
            mf.write_model(path, P.case_model(S))
            made[S] = BirdClassifier(path, None, top_k=3, min_confidence=0.0)
        return made[S]
    yield get
    for clf in made.values():
        clf.close()


def _threads():
    env = os.environ.get("BIRDA_HIP_COPY_THREADS")
    return max(1, int(env)) if env else max(1, min(8, (os.cpu_count() or 2) // 2))


def _describe(c, run, f, got, want, ok, what):
    bad = np.argwhere(~ok)
    r, j = (int(v) for v in bad[0])
    last, fb = f["last"], f["frame_bytes"]
    frame = last["starts"][r] + j
    where = f"frame {frame} (past the stream's {f['n_frames']} frames: the pad)"
    if frame < f["n_frames"]:
        rel = (frame - last["f0"]) * fb
        piece, worker = P.share_of(rel, last["bytes"], _threads() if last["workers"] else 1)
        where = (f"stream byte {frame * fb} (frame {frame}), byte {rel} of the slice's span [{last['f0']}, {last['f1']}) of {last['bytes']} bytes "
                 f"({last['route']}): piece {piece} of {last['pieces']}, worker share {worker}")
    return (f"{c['id']} run {run} {what}: {len(bad)} of {ok.size} samples differ, first at [row {r}, sample {j}] (segment {last['b0'] + r}): got "
            f"0x{int(got.view(np.uint32)[r, j]):08x} want 0x{int(want.view(np.uint32)[r, j]):08x}, from {where}")


def _call(clf, ctx, c, run, tmp_path, route=None):
    """-> (results, starts the call reported or None)"""
    from birda_amd import _lib
    f = P.facts(c, run)
    raw = P.case_stream(c, run)
    route = route or c["route"]
    if c["call"] == "at":
        return clf.predict_pcm_at(ctx, raw, c["fmt"], c["channels"], c["rate"], f["starts"]), None
    if route == "fd":
        path = str(tmp_path / f"{c['id']}_{run}.pcm")
        with open(path, "wb") as fh:                 # other bytes before and after the stream
            fh.write((bytes(range(256)) * (FD_OFFSET // 256 + 1))[:FD_OFFSET])
            fh.write(raw.tobytes())
            fh.write(b"\xa5" * 64)
        fd = os.open(path, os.O_RDONLY)
        try:
            return clf.predict_pcm_fd(ctx, fd, FD_OFFSET, c["fmt"], f["n_frames"], c["channels"], c["rate"], c["overlap"])
        finally:
            os.close(fd)
    if route == "pinned":
        L = _lib.load()
        buf = raw.copy()
        _lib.check(L.bh_host_register(buf.ctypes.data, buf.nbytes))
        try:
            return clf.predict_pcm(ctx, buf, c["fmt"], c["channels"], c["rate"], c["overlap"])
        finally:
            _lib.check(L.bh_host_unregister(buf.ctypes.data))
    return clf.predict_pcm(ctx, raw, c["fmt"], c["channels"], c["rate"], c["overlap"])


def _hold(clf, ctx, c, run, what):
    """the rows the call left behind against the reference; -> samples compared"""
    want, f = P.case_reference(c, run)
    rows, seg, mixed = want.shape[0], f["seg"], c["channels"] > 1
    got = clf.read_segments(ctx, 1 if f["resampling"] else 0, rows, seg)
    ok = P.same_bits(got, want, mixed)
    if not ok.all():
        pytest.fail(_describe(c, run, f, got, want, ok, what))
    if f["resampling"]:
        import torch
        S = c["S"]
        got0 = clf.read_segments(ctx, 0, rows, S)
        d_in = torch.from_numpy(want).cuda()
        d_out = torch.full((rows, S), 7.0, device="cuda")
        clf.resample_device(ctx, d_in.data_ptr(), seg, seg, c["rate"], P.MODEL_RATE, d_out.data_ptr(), S, S, rows)
        ctx.synchronize()
        want0 = d_out.cpu().numpy()
        ok0 = got0.view(np.uint32) == want0.view(np.uint32)
        assert ok0.all(), (c["id"], run, what, "model-rate rows differ from bh_resample_device on the same raw rows", int((~ok0).sum()),
                           [int(v) for v in np.argwhere(~ok0)[0]])
    return got.size


def run_case(c, clfs, tmp_path):
    from birda_amd._lib import BirdaHipError
    clf = clfs(c["S"])
    clf.trim()                                       # no parked context: the context below holds exactly c["cap"] segments
    ctx = clf.create_batch_context(c["cap"])
    compared = 0
    try:
        for run in (0, 1):
            f = P.facts(c, run)
            for ss in ((None,) + c["sub_slices"]) if run == 0 else (None,):
                if ss is not None:
                    ctx.set_sub_slices(ss)
                what = "" if ss is None else f"set_sub_slices({ss})"
                try:
                    _res, starts = _call(clf, ctx, c, run, tmp_path)
                    if starts is not None:
                        assert starts == f["starts"], (c["id"], run, what)        # held to the oracle's in the CPU module
                    assert len(_res) == len(f["starts"])
                except BirdaHipError:
                    if not c["nonfinite"]:           # the return code of a stream with inf / NaN stays with the tests of that contract
                        raise
                compared += _hold(clf, ctx, c, run, what)
        if "sub_slices" in c["tags"] and not P.facts(c)["resampling"]:
            from birda_amd import _lib
            assert _lib.load().bh_batch_context_lane_fallbacks(ctx._h) == 0, (c["id"], "the sub-slices did not run on lanes")
    finally:
        ctx.set_sub_slices(0)
        ctx.close()
        clf.trim()
    RAN[c["id"]] = compared


@pytest.mark.parametrize("c", P.CASES, ids=P.CASE_IDS)
def test_segments_equal_the_reference_bit_for_bit(c, clfs, tmp_path):
    run_case(c, clfs, tmp_path)


def _rows(res):
    return [[(p.index, p.confidence) for p in r.predictions] for r in res]


@pytest.mark.parametrize("cid", ["pinned_s16_ch2", "pinned_s24_ch1_16388"])
def test_staged_pinned_and_fd_routes_agree(cid, clfs, tmp_path):
    """the same bytes handed over pageable, pinned and by file descriptor: the same starts and the same (index, confidence) rows"""
    c = P.BY_ID[cid]
    clf = clfs(c["S"])
    clf.trim()
    ctx = clf.create_batch_context(c["cap"])
    try:
        out = {route: _call(clf, ctx, c, 0, tmp_path, route) for route in ("staged", "pinned", "fd")}
    finally:
        ctx.close()
        clf.trim()
    want_starts = P.facts(c)["starts"]
    for route, (res, starts) in out.items():
        assert starts == want_starts, route
        assert _rows(res) == _rows(out["staged"][0]) and len(res) == len(want_starts), route


UNSTAGED = [c for c in P.CASES if c["route"] == "staged" and c["call"] == "stream" and any(s["route"] == "unstaged" for s in P.facts(c)["slices"])]


@pytest.mark.parametrize("c", UNSTAGED, ids=[c["id"] for c in UNSTAGED])
def test_fd_route_refuses_exactly_the_unstaged_slices(c, clfs, tmp_path):
    """a slice larger than the staging buffer cannot be read into it: BH_ERR_UNSUPPORTED, by return code"""
    from birda_amd._lib import BirdaHipError
    clf = clfs(c["S"])
    clf.trim()
    ctx = clf.create_batch_context(c["cap"])
    try:
        with pytest.raises(BirdaHipError) as e:
            _call(clf, ctx, c, 0, tmp_path, "fd")
        assert e.value.code == BH_ERR_UNSUPPORTED and "staging buffer" in str(e.value), str(e.value)
    finally:
        ctx.close()
        clf.trim()


def test_unstaged_cases_cover_every_kernel():
    assert {c["fmt"] for c in UNSTAGED if "unstaged" in c["tags"]} == set(P.BYTES)


def test_pcm_at_refuses_by_return_code(clfs):
    from birda_amd._lib import BirdaHipError
    c = P.BY_ID["at_repeated_s16_ch2"]
    clf = clfs(c["S"])
    ctx = clf.create_batch_context(4)
    raw, n = P.case_stream(c, 0), c["n_frames"][0]
    try:
        for starts in ([0, 10, 9], [0, n], [n + 5], [5, 5, 4]):
            with pytest.raises(BirdaHipError) as e:
                clf.predict_pcm_at(ctx, raw, c["fmt"], c["channels"], c["rate"], starts)
            assert e.value.code == BH_ERR_INVALID, (starts, str(e.value))
        assert len(clf.predict_pcm_at(ctx, raw, c["fmt"], c["channels"], c["rate"], [0, n - 1])) == 2
    finally:
        ctx.close()


def test_read_segments_refuses_by_return_code(clfs):
    from birda_amd._lib import BirdaHipError
    c = P.BY_ID["resample_44100_cap3_s16_ch1"]
    clf = clfs(c["S"])
    clf.trim()
    ctx = clf.create_batch_context(3)
    S, seg = c["S"], P.facts(c)["seg"]

    def refused(which, rows, row_floats, word):
        with pytest.raises(BirdaHipError) as e:
            clf.read_segments(ctx, which, rows, row_floats)
        assert e.value.code == BH_ERR_INVALID and word in str(e.value), str(e.value)
    try:
        refused(1, 1, seg, "no resampling call")                 # the raw buffer was never allocated
        refused(0, 4, S, "rows")
        refused(0, 0, S, "rows")
        refused(0, 3, S - 4, "floats")
        refused(2, 1, S, "which")
        clf.predict_pcm(ctx, P.case_stream(c, 0), c["fmt"], c["channels"], c["rate"], 0)
        refused(1, 4, seg, "rows")
        refused(1, 2, seg + 1, "raw rows")
        assert clf.read_segments(ctx, 1, 2, seg).shape == (2, seg) and clf.read_segments(ctx, 0, 3, S).shape == (3, S)
    finally:
        ctx.close()
        clf.trim()


def test_every_case_ran(clfs, tmp_path):
    """(Run on its own, this test first runs whatever the tests above have not.)"""
    for c in P.CASES:
        if c["id"] not in RAN:
            run_case(c, clfs, tmp_path)
    assert set(RAN) == set(P.CASE_IDS)
    fmts = {c["fmt"] for c in P.CASES}
    assert fmts == set(P.BYTES)                                   # all four segment_pcm_kernel instantiations
    print(f"\n{len(RAN)} cases, {sum(RAN.values())} samples compared as bits; module wall time {time.time() - T0:.1f} s")
