"""The device PCM front end (kernels_frontend.hip segment_pcm_kernel<FMT> and the slice logic of api.hip predict_pcm16_core): its
reference, the catalogue tests/test_pcm_segments_gpu.py runs, and everything about both that needs no GPU.

The stage is exact by construction -- a division by 2^15 or 2^31 is exact, the mix is a sequential f32 sum and one correctly
rounded division (reference src/audio/decode.rs:353-411, oracle/birda_oracle.c bo_pcm16_to_mono / bo_pcm32_to_mono /
bo_f32_to_mono) -- so the GPU module compares every sample as a uint32 and takes no tolerance; a NaN that went through a channel
mix (whose payload the adder may rewrite) is the one exception: isnan on both sides.

Here, on the CPU:
  * segments_ref, in NumPy float32, equals the C oracle (mono conversion, then bo_segmenter_next for the windows and starts) bit
    for bit on every case, and stays within (C + 1) 2^-24 sum_c |s_c / norm| / C of a float64 evaluation of (sum_c s_c / norm) / C:
    one rounding per int32 -> f32 conversion (C of them, u |s_c| each), one per addition (C - 1, each at most u sum|s_c|), one for
    the division (u |sum| / C).  Derived, not measured; it guards the reference against a restating mistake.
  * every case IS the edge its tags claim, by the library's formulas restated (facts below: the slices, their spans and routes,
    the pieces, the kernel's grid, the sub-slice threshold);
  * every mutant of the reference (MUTANTS) changes at least one sample the GPU module compares, in every case of the family it
    applies to -- a condition on the catalogue's data.

Each case is two calls on one context: run 0 is the case, run 1 a shorter stream of other samples whose tail is padded, so
anything the first call left behind (the upload buffer, the rows, the pad) would show in the second."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frontend as F                                          # noqa: E402  (fe_model: one cheap branch and the token network)

U = 2.0 ** -24
MODEL_RATE = 48000
PIECE = 8 << 20                     # predict_pcm16_core's upload pieces
SHARE_ALIGN = 4096                  # ... and what a gather worker's share of a piece is rounded up to
WORKERS_FROM = 1 << 20              # staged slices from this many bytes are gathered by several threads
SUB_SLICES_FROM = 256               # slices from this many segments are cut into sub-slices
BYTES = {"s16": 2, "s24": 3, "s32": 4, "f32": 4}
NORM = {"s16": 32768.0, "s24": 2147483648.0, "s32": 2147483648.0, "f32": 1.0}
NAN_A, NAN_B = 0x7FC00001, 0xFFC12345                              # quiet NaNs, two payloads

# the values the issue lists, as the stream holds them; each list ends on a value that is not zero (the pad mutant must see it)
EXTREMES = {
    "s16": np.array([0, 1, -1, 32767, -32768], np.int16).view(np.uint8).reshape(-1, 2),
    "s24": np.array([[0x01, 0x00, 0x00], [0xFF, 0xFF, 0xFF], [0xFF, 0xFF, 0x7F], [0x00, 0x00, 0x80]], np.uint8),
    "s32": np.array([-1, 16777217, 16777219, 2147483647, -2147483648], np.int32).view(np.uint8).reshape(-1, 4),
    "f32": np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x007FFFFF, 0x80000001], np.uint32).view(np.uint8).reshape(-1, 4),
    # a stream that holds these is refused or answered by the model as the existing tests of that contract say; its samples are
    # held all the same (single-slice cases only: a call that ends early leaves an earlier slice's rows behind)
    "f32_nonfinite": np.array([0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, NAN_A, NAN_B, 0x00000001], np.uint32).view(np.uint8).reshape(-1, 4),
}


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def _samples(raw, fmt, n_frames, channels, mut=None):
    """-> [n_frames][channels] float32, each sample scaled as the decoder scales it"""
    raw = np.frombuffer(raw, np.uint8) if not isinstance(raw, np.ndarray) else raw.reshape(-1).view(np.uint8)
    b = raw[: n_frames * channels * BYTES[fmt]].reshape(n_frames * channels, BYTES[fmt])
    if mut == "bytes_swapped":
        b = b[:, ::-1]
    b = np.ascontiguousarray(b)
    if fmt == "s16":
        return (b.view("<i2").astype(np.float32) / np.float32(32767.0 if mut == "div_32767" else 32768.0)).reshape(n_frames, channels)
    if fmt == "f32":
        return b.view("<f4").reshape(n_frames, channels)
    if fmt == "s24":
        b0, b1, b2 = (b[:, i].astype(np.uint32) for i in range(3))
        if mut == "s24_unsigned":            # the 24 bits taken as unsigned, widened without wrapping into the sign
            v = ((b0 | b1 << 8 | b2 << 16).astype(np.int64) << 8).astype(np.float32)
        elif mut == "s24_shift0":            # sign-extended but not widened
            v = ((b0 << 8 | b1 << 16 | b2 << 24).view(np.int32) >> 8).astype(np.float32)
        else:
            v = (b0 << 8 | b1 << 16 | b2 << 24).view(np.int32).astype(np.float32)      # int32 -> f32: round to nearest even
    else:
        v = b.view("<i4").astype(np.float32)
    return (v / np.float32(2147483648.0)).reshape(n_frames, channels)


def mono_ref(raw, fmt, n_frames, channels, mut=None):
    """-> [n_frames] float32: the sample itself, or ((+0 + s_0) + s_1 + ...) / float(channels), one f32 rounding each"""
    if mut == "no_channel_stride" and channels > 1:      # sample c of frame f read at f + c instead of f * channels + c
        flat = _samples(raw, fmt, n_frames * channels, 1)[:, 0]
        x = np.stack([flat[c: c + n_frames] for c in range(channels)], axis=1)
    else:
        x = _samples(raw, fmt, n_frames, channels, mut)
    if channels == 1:
        return x[:, 0].copy()
    if mut == "channel0_only":
        return x[:, 0].copy()
    acc = np.zeros(n_frames, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(channels):
            acc = acc + x[:, c]
        return acc / np.float32(2.0 if mut == "div_2" else channels)


def segments_ref(raw_bytes, fmt, n_frames, channels, starts, seg_len, mut=None):
    """-> float32 [len(starts)][seg_len]: row i = the mono stream from frame starts[i], +0.0 at and past n_frames"""
    mono = mono_ref(raw_bytes, fmt, n_frames, channels, mut)
    out = np.zeros((len(starts), seg_len), np.float32)
    for i, s in enumerate(starts):
        s = int(s) + (1 if mut == "start_plus_1" else 0)
        take = max(0, min(seg_len, n_frames - s))
        out[i, :take] = mono[s: s + take]
        if mut == "pad_last_sample" and take < seg_len:
            out[i, take:] = mono[n_frames - 1]
        if mut == "window_short" and take > 0:        # one sample fewer than the window holds
            out[i, take - 1] = 0.0
    return out


def same_bits(a, b, mixed):
    """a, b float32 of one shape -> bool array: equal as uint32, or -- where mixed (a channel mix ran) -- both NaN"""
    eq = a.view(np.uint32) == b.view(np.uint32)
    return eq | (np.isnan(a) & np.isnan(b)) if mixed else eq


# mutant -> the family it applies to
MUTANTS = {
    "div_32767": lambda c: c["fmt"] == "s16",
    "s24_unsigned": lambda c: c["fmt"] == "s24",
    "s24_shift0": lambda c: c["fmt"] == "s24",
    "bytes_swapped": lambda c: True,
    "channel0_only": lambda c: c["channels"] > 1,
    "div_2": lambda c: c["channels"] > 2,
    "no_channel_stride": lambda c: c["channels"] > 1,
    "start_plus_1": lambda c: True,
    "pad_last_sample": lambda c: True,
    "window_short": lambda c: True,
}


# ---------------------------------------------------------------------------------------------------------------------------
# the library's formulas, restated
# ---------------------------------------------------------------------------------------------------------------------------
def seg_starts(n_frames, seg, ovl):
    """bh_segment_starts (StreamingDecoder::next_segment, decode.rs:150-202)"""
    out, pos = [], 0
    while pos < n_frames:
        take = min(seg, n_frames - pos)
        out.append(pos)
        if take <= ovl:
            break
        pos += take - ovl
    return out


def src_len(n, rate):
    """a model-rate length at the source rate: ceil(n x rate / model rate) in double (processor.rs:67-82)"""
    return n if rate == MODEL_RATE else int(np.ceil(float(n) * rate / MODEL_RATE))


def facts(c, run=0):
    """What predict_pcm16_core does with run `run` of case c: the segment length and starts at the source rate, the slices with
    their frame spans, bytes, route and pieces, and the kernel's grid."""
    fb = BYTES[c["fmt"]] * c["channels"]
    n_frames = c["n_frames"][run]
    seg = src_len(c["S"], c["rate"])
    starts = list(c["starts"][run]) if c["call"] == "at" else seg_starts(n_frames, seg, src_len(c["overlap"], c["rate"]))
    stage_cap = c["cap"] * c["S"] * 4
    slices = []
    for b0 in range(0, len(starts), c["cap"]):
        st = starts[b0: b0 + c["cap"]]
        f0, f1 = st[0], min(n_frames, st[-1] + seg)
        nbytes = (f1 - f0) * fb
        staged = c["route"] != "pinned" and nbytes <= stage_cap
        slices.append(dict(b0=b0, starts=st, f0=f0, f1=f1, bytes=nbytes, staged=staged,
                           route="pinned" if c["route"] == "pinned" else (c["route"] if staged else "unstaged"),
                           pieces=-(-nbytes // PIECE) if (staged or c["route"] == "pinned") else 1,
                           workers=staged and nbytes >= WORKERS_FROM))
    blocks = min(-(-seg // 256), 64)
    return dict(frame_bytes=fb, n_frames=n_frames, seg=seg, starts=starts, slices=slices, last=slices[-1], blocks=blocks,
                passes=-(-seg // (blocks * 256)), resampling=c["rate"] != MODEL_RATE)


def share_of(offset, nbytes, n_threads):
    """(piece, worker) whose share holds byte `offset` of a slice span of nbytes (gather_part)"""
    j = offset // PIECE
    ln = min(PIECE, nbytes - j * PIECE)
    share = (-(-ln // n_threads) + SHARE_ALIGN - 1) & ~(SHARE_ALIGN - 1)
    return j, (offset - j * PIECE) // share


# ---------------------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------------------
def case(cid, tags, fmt, channels, S=132, cap=3, n_frames=None, n_frames2=None, overlap=0, rate=MODEL_RATE, route="staged",
         call="stream", starts=None, starts2=None, sub_slices=(), nonfinite=False):
    """n_frames / n_frames2: the two runs' streams (run 1 defaults to a shorter one with a padded tail); overlap in model-rate
    samples; route: how the stream is handed over -- "staged" (pageable), "pinned", "fd"; a slice larger than the staging buffer
    goes unstaged whatever the route says (facts); call "stream" | "at" (starts / starts2: the two runs' starts);
    sub_slices: set_sub_slices values run 0 is repeated with"""
    seg = src_len(S, rate)
    if n_frames2 is None:
        n_frames2 = max(1, n_frames - seg - seg // 3 - 1)
        if n_frames2 % seg == 0:
            n_frames2 -= 1
    if call == "at" and starts2 is None:
        starts2 = [s for s in starts if s < n_frames2][:-1] + [n_frames2 - 2]
    return dict(id=cid, tags=tuple(tags), fmt=fmt, channels=channels, S=S, cap=cap, n_frames=(n_frames, n_frames2), overlap=overlap,
                rate=rate, route=route, call=call, starts=(starts, starts2), sub_slices=tuple(sub_slices), nonfinite=nonfinite)


def _cases():
    c = []
    fmts = ("s16", "s24", "s32", "f32")
    # every format x 1, 2, 3, 8 channels, through slices of 3 with 7, 8, 9 segments (a last slice of 1, 2, 3 rows at f0 > 0) and
    # streams that end on, one before and one past a segment's end; frames of up to 32 bytes, so their full slices go unstaged
    k = 0
    for fmt in fmts:
        for ch in (1, 2, 3, 8):
            nseg, end = 7 + k % 3, (0, -1, 1)[(k // 3) % 3]
            n = (nseg if end <= 0 else nseg - 1) * 132 + end
            tags = [f"fmt_{fmt}", f"ch{ch}", f"last_rows_{(nseg - 1) % 3 + 1}", "f0_positive", {0: "end_exact", -1: "end_minus_1", 1: "end_plus_1"}[end]]
            c.append(case(f"{fmt}_ch{ch}_slices", tags, fmt, ch, n_frames=n))
            k += 1
    # the same formats staged whatever the frame size: a capacity that holds the whole stream's bytes, one slice, f0 = 0
    for fmt in fmts:
        for ch in (2, 3, 8):
            if BYTES[fmt] * ch > 4:
                c.append(case(f"{fmt}_ch{ch}_staged", [f"fmt_{fmt}", f"ch{ch}", "staged", "f0_zero", "one_slice"], fmt, ch,
                              cap=-(-5 * BYTES[fmt] * ch // 4), n_frames=5 * 132 - 7))
    # the kernel's grid: min(ceil(seg / 256), 64) blocks of 256 in a grid-stride loop
    for S, tag, fmt, ch in ((16384, "grid_one_full_pass", "s16", 1), (16388, "grid_second_pass_of_4", "s24", 1), (33000, "grid_three_passes", "f32", 1),
                            (16388, "grid_second_pass_of_4", "s32", 2)):
        c.append(case(f"{tag}_{fmt}_ch{ch}", [tag, "f0_positive", "last_rows_1"], fmt, ch, S=S, n_frames=3 * S + 1))
    c[0]["tags"] += ("grid_one_partial_block",)
    # stream ends x overlaps: k seg, k seg - 1, k seg + 1 (a trailing segment of one sample and seg - 1 zeros), a stream shorter than
    # one segment; overlap 0, seg / 4 and seg - 1 (a hop of one frame), and the short trailing segment an overlap leaves
    for ovl, kk in ((0, 7), (33, 7), (131, 2)):
        for end, tag in ((0, "end_exact"), (-1, "end_minus_1"), (1, "end_plus_1"), (None, "shorter_than_segment")):
            n = 57 if end is None else kk * 132 + end
            fmt, ch = (("s16", 1), ("s24", 1), ("s16", 2), ("f32", 1))[len(c) % 4]
            tags = [tag, f"overlap_{ovl}"] + (["short_trailing_segment"] if ovl and end is not None else [])
            c.append(case(f"ends_ovl{ovl}_{tag}_{fmt}", tags, fmt, ch, n_frames=n, overlap=ovl, n_frames2=n - 40))
    # routes: pinned caller memory, a file descriptor at an odd offset -- small and across segments of two kernel passes
    for route in ("pinned", "fd"):
        c.append(case(f"{route}_s16_ch2", [route, "f0_positive"], "s16", 2, n_frames=8 * 132 - 3, route=route))
        c.append(case(f"{route}_s24_ch1_16388", [route, "f0_positive", "grid_second_pass_of_4"], "s24", 1, S=16388, n_frames=4 * 16388 + 1, route=route))
    c.append(case("pinned_s32_ch3", ["pinned", "f0_positive"], "s32", 3, n_frames=7 * 132 + 1, route="pinned"))
    c.append(case("fd_f32_ch1_overlap", ["fd", "f0_positive", "overlap_33"], "f32", 1, n_frames=9 * 132 + 5, overlap=33, route="fd"))
    # the unstaged single copy, bytes > stage_cap, with the capacity equal to the segment count
    for fmt, ch in (("s32", 2), ("f32", 2), ("s24", 8), ("s16", 3)):
        c.append(case(f"unstaged_{fmt}_ch{ch}", ["unstaged", "one_slice", "f0_zero"], fmt, ch, cap=6, n_frames=6 * 132))
    # pieces, worker shares, sub-slices, lanes: 9-byte frames, 300 segments of 16 388 in one slice -- 44 MB, six 8-MiB pieces whose
    # boundaries and 4096-byte worker shares fall inside frames; the capacity is what stages that many bytes
    c.append(case("pieces_s24_ch3_300", ["pieces_6", "workers", "sub_slices", "torn_frames", "staged", "one_slice"], "s24", 3, S=16388, cap=700,
                  n_frames=300 * 16388 - 11, n_frames2=281 * 16388 + 5, sub_slices=(1, 2, 5, 0)))
    c.append(case("pieces_pinned_s24_ch3_300", ["pieces_6", "pinned", "sub_slices", "torn_frames", "one_slice"], "s24", 3, S=16388, cap=300,
                  n_frames=300 * 16388 - 11, n_frames2=281 * 16388 + 5, route="pinned"))
    # ... and many small segments for the sub-slice cuts alone (the slice's bytes equal the staging buffer's: the last staged size)
    c.append(case("sub_slices_s16_ch2_640", ["sub_slices", "staged", "stage_cap_exact", "one_slice"], "s16", 2, cap=640, n_frames=640 * 132,
                  n_frames2=600 * 132 + 17, sub_slices=(1, 2, 5, 0)))
    # the resampling route: an odd raw segment (12 000 samples at 44.1 -> 48 kHz: 11 025), decimation by two; a capacity below and
    # above the segment count; its sub-slices run in sequence on the context's stream (the resampler's scratch is one per context)
    for rate, seg in ((44100, 11025), (96000, 24000)):
        for cap, fmt, ch in ((3, "s16", 1), (6, "f32", 2)):
            c.append(case(f"resample_{rate}_cap{cap}_{fmt}_ch{ch}", ["resampling", f"raw_seg_{seg}", "f0_positive" if cap == 3 else "f0_zero"],
                          fmt, ch, S=12000, cap=cap, n_frames=4 * seg + 9, rate=rate))
    c.append(case("resample_44100_sequence_s24_ch2", ["resampling", "sub_slices", "raw_seg_122", "one_slice"], "s24", 2, cap=300, n_frames=300 * 122 - 5,
                  n_frames2=270 * 122 + 3, rate=44100, sub_slices=(2, 5, 0)))
    # bh_predict_pcm_at: repeated starts, a start at n_frames - 1, gaps longer than a segment (frames in the span nobody reads), more
    # starts than the capacity (a second slice whose f0 is an arbitrary start)
    c.append(case("at_repeated_s16_ch2", ["at", "at_repeated", "one_slice"], "s16", 2, cap=8, n_frames=1000, call="at", starts=[0, 0, 5, 5, 5, 700, 999, 999]))
    c.append(case("at_last_frame_s24_ch3", ["at", "at_last_frame", "f0_positive"], "s24", 3, cap=3, n_frames=1500, call="at", starts=[3, 140, 141, 1499]))
    c.append(case("at_gaps_f32_ch1", ["at", "at_gaps", "one_slice"], "f32", 1, cap=4, n_frames=2000, call="at", starts=[1, 500, 1500, 1990]))
    c.append(case("at_second_slice_s32_ch2", ["at", "at_gaps", "at_repeated", "f0_positive", "last_rows_2"], "s32", 2, cap=3, n_frames=2000, call="at",
                  starts=[0, 10, 10, 400, 977, 977, 1501, 1999]))
    # (a first slice with a wide span, then a short one far into the stream: the upload buffer is larger than the second slice needs)
    c.append(case("at_wide_then_narrow_s32_ch2", ["at", "at_gaps", "at_repeated", "f0_positive", "last_rows_3"], "s32", 2, cap=3, n_frames=4000, call="at",
                  starts=[0, 50, 3000, 3010, 3010, 3500]))
    # float32 streams that hold FLT_MAX, +-inf and NaNs (single slices; mono: as is, bit for bit; mixed: isnan on both sides)
    c.append(case("f32_nonfinite_ch1", ["nonfinite", "one_slice"], "f32", 1, cap=8, n_frames=5 * 132 + 3, nonfinite=True))
    c.append(case("f32_nonfinite_ch3", ["nonfinite", "one_slice"], "f32", 3, cap=12, n_frames=4 * 132 + 3, nonfinite=True))
    return c


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)
BY_ID = {c["id"]: c for c in CASES}


def case_model(S):
    return F.fe_model([(128, 4)], 40, S, n_frames=2)


def _places(c, run):
    """[(frame, direction)]: where the extremes are planted -- runs of consecutive frames going up from (+1) or down to (-1) the
    first and last frame of the stream, the first and last sample of the last slice's first segment, each side of every 8-MiB
    boundary of the last slice's span"""
    f = facts(c, run)
    n, last = f["n_frames"], f["last"]
    p = [(0, 1), (n - 1, -1), (last["starts"][0], 1), (min(n, last["starts"][0] + f["seg"]) - 1, -1)]
    for j in range(1, last["pieces"]):
        o = j * PIECE
        p += [(last["f0"] + (o - 1) // f["frame_bytes"], -1), (last["f0"] + o // f["frame_bytes"] + 1, 1)]
    return p


_STREAMS = {}


def case_stream(c, run=0):
    """-> the interleaved stream of run `run` as a uint8 array: seeded noise at three amplitudes (a third of the stream each) with
    the format's extreme values planted, one channel of one frame each, at _places"""
    key = (c["id"], run)
    if key in _STREAMS:
        return _STREAMS[key]
    fmt, ch, n = c["fmt"], c["channels"], c["n_frames"][run]
    rng = np.random.default_rng(sum(map(ord, c["id"])) * 2 + run)
    amp = np.repeat(np.array([1.0, 1.0 / 16, 1.0 / 512]), -(-n // 3))[:n, None]
    if fmt == "f32":
        raw = (rng.standard_normal((n, ch)) * 0.4 * amp).astype("<f4").view(np.uint8).reshape(n, ch, 4)
    elif fmt == "s16":
        raw = np.clip(np.rint(rng.standard_normal((n, ch)) * 9000 * amp), -32768, 32767).astype("<i2").view(np.uint8).reshape(n, ch, 2)
    else:
        v = np.clip(np.rint(rng.standard_normal((n, ch)) * 6e8 * amp), -2 ** 31, 2 ** 31 - 1).astype("<i4")
        raw = v.view(np.uint8).reshape(n, ch, 4)
        if fmt == "s24":
            raw = raw[:, :, 1:]                      # the upper three bytes: the 24-bit sample
    raw = np.ascontiguousarray(raw)
    ext = EXTREMES["f32_nonfinite" if c["nonfinite"] else fmt]
    for k, (frame, d) in enumerate(_places(c, run)):
        for i in range(len(ext)):
            fr = frame + i if d > 0 else frame - (len(ext) - 1 - i)
            if 0 <= fr < n:
                raw[fr, (k + i) % ch] = ext[i]
    raw = raw.reshape(-1)
    if len(_STREAMS) >= 4:
        _STREAMS.pop(next(iter(_STREAMS)))
    _STREAMS[key] = raw
    return raw


def case_reference(c, run=0, mut=None):
    """-> (the last slice's rows as segment_pcm_kernel must write them, [rows][seg] at the source rate; facts)"""
    f = facts(c, run)
    return segments_ref(case_stream(c, run), c["fmt"], f["n_frames"], c["channels"], f["last"]["starts"], f["seg"], mut), f


# ---------------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_mono(O, raw, fmt, n, ch):
    L = O.lib()
    out = np.zeros(n, np.float32)
    if fmt == "s16":
        L.bo_pcm16_to_mono(np.ascontiguousarray(raw[: n * ch * 2]).ctypes.data, n, ch, out)
    elif fmt == "f32":
        L.bo_f32_to_mono(np.ascontiguousarray(raw[: n * ch * 4]).view(np.float32), n, ch, out)
    else:
        if fmt == "s24":
            b = raw[: n * ch * 3].reshape(-1, 3).astype(np.uint32)
            wide = (b[:, 0] << 8 | b[:, 1] << 16 | b[:, 2] << 24).view(np.int32)      # symphonia widens 24-bit samples into its S32 buffer
        else:
            wide = np.ascontiguousarray(raw[: n * ch * 4]).view(np.int32)
        wide = np.ascontiguousarray(wide)
        L.bo_pcm32_to_mono(wide.ctypes.data, n, ch, out)
    return out


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_reference_equals_the_c_oracle_bit_for_bit(c, oracle_lib):
    for run in (0, 1):
        f = facts(c, run)
        raw, n, ch = case_stream(c, run), f["n_frames"], c["channels"]
        mono = _oracle_mono(oracle_lib, raw, c["fmt"], n, ch)
        mixed = ch > 1
        assert same_bits(mono_ref(raw, c["fmt"], n, ch), mono, mixed).all(), (c["id"], run)
        if c["call"] == "at":          # the oracle's segmenter on the stream from each start: its first window
            rows = [(oracle_lib.segment_stream(mono[s:], f["seg"], 0)[0][0], s) for s in f["starts"]]
        else:
            rows = oracle_lib.segment_stream(mono, f["seg"], src_len(c["overlap"], c["rate"]))
            # the library's restated segmenter (and the library's own, host code) against the oracle's starts
            assert [s for _, s in rows] == f["starts"], (c["id"], run)
            from birda_amd import _lib
            import ctypes as C
            buf = (C.c_uint64 * len(rows))()
            assert _lib.load().bh_segment_starts(n, f["seg"], src_len(c["overlap"], c["rate"]), buf, len(rows)) == len(rows)
            assert list(buf) == f["starts"]
        rows = rows[f["last"]["b0"]:]
        want = np.stack([r for r, _ in rows])
        got, _ = case_reference(c, run)
        assert got.shape == want.shape and same_bits(got, want, mixed).all(), (c["id"], run)


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_reference_within_the_derived_float64_bound(c):
    for run in (0, 1):
        n, ch, fmt = c["n_frames"][run], c["channels"], c["fmt"]
        raw = case_stream(c, run)
        b = np.ascontiguousarray(raw.reshape(n * ch, BYTES[fmt]))
        if fmt == "s16":
            s = b.view("<i2").astype(np.float64)
        elif fmt == "s32":
            s = b.view("<i4").astype(np.float64)
        elif fmt == "f32":
            s = b.view("<f4").astype(np.float64)
        else:                              # written apart from _samples: sign-extend the 24 bits, x 256
            u = b[:, 0].astype(np.int64) | b[:, 1].astype(np.int64) << 8 | b[:, 2].astype(np.int64) << 16
            s = (np.where(u >= 1 << 23, u - (1 << 24), u) * 256).astype(np.float64)
        s = (s / NORM[fmt]).reshape(n, ch)
        finite = np.isfinite(s).all(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            want = s.sum(axis=1) / ch
            bound = (ch + 1) * U * np.abs(s).sum(axis=1) / ch
        got = mono_ref(raw, fmt, n, ch).astype(np.float64)
        finite &= np.isfinite(got)
        err = np.abs(got[finite] - want[finite])
        assert finite.sum() >= n - 64 and (err <= bound[finite]).all(), (c["id"], run, float(err.max()))


def _torn(f):
    """the piece boundaries of the last slice, and the worker-share boundaries for 2 .. 8 gather threads (the default is 8) but 6 --
    whose share, 342 x 4096 bytes, is a whole number of 9-byte frames -- fall inside a frame"""
    last, fb = f["last"], f["frame_bytes"]
    piece = [j * PIECE % fb != 0 for j in range(1, last["pieces"])]
    shares = [(-(-PIECE // nt) + SHARE_ALIGN - 1 & ~(SHARE_ALIGN - 1)) % fb != 0 for nt in (2, 3, 4, 5, 7, 8)]
    return piece and all(piece) and all(shares)


TAG_CHECKS = {
    "staged": lambda c, f: all(s["route"] == "staged" and s["bytes"] <= c["cap"] * c["S"] * 4 for s in f["slices"]),
    "unstaged": lambda c, f: f["last"]["route"] == "unstaged" and f["last"]["bytes"] > c["cap"] * c["S"] * 4 and c["route"] == "staged",
    "pinned": lambda c, f: f["last"]["route"] == "pinned",
    "fd": lambda c, f: all(s["route"] == "fd" for s in f["slices"]),
    "stage_cap_exact": lambda c, f: f["last"]["bytes"] == c["cap"] * c["S"] * 4,
    "f0_positive": lambda c, f: len(f["slices"]) > 1 and f["last"]["f0"] > 0,
    "f0_zero": lambda c, f: len(f["slices"]) == 1 and f["last"]["f0"] == 0,
    "one_slice": lambda c, f: len(f["slices"]) == 1,
    "last_rows_1": lambda c, f: len(f["last"]["starts"]) == 1 and len(f["slices"]) > 1,
    "last_rows_2": lambda c, f: len(f["last"]["starts"]) == 2 and len(f["slices"]) > 1,
    "last_rows_3": lambda c, f: len(f["last"]["starts"]) == 3 == c["cap"] and len(f["slices"]) > 1,
    "end_exact": lambda c, f: f["n_frames"] % f["seg"] == 0 and (c["overlap"] or f["starts"][-1] + f["seg"] == f["n_frames"]),
    "end_minus_1": lambda c, f: f["n_frames"] % f["seg"] == f["seg"] - 1 and (c["overlap"] or f["starts"][-1] + f["seg"] == f["n_frames"] + 1),
    "end_plus_1": lambda c, f: f["n_frames"] % f["seg"] == 1 and (c["overlap"] or f["starts"][-1] == f["n_frames"] - 1),
    "shorter_than_segment": lambda c, f: f["n_frames"] < f["seg"] and f["starts"][0] == 0 and (c["overlap"] > 0 or f["starts"] == [0]),
    "overlap_0": lambda c, f: c["overlap"] == 0,
    "overlap_33": lambda c, f: c["overlap"] == c["S"] // 4 == 33,
    "overlap_131": lambda c, f: c["overlap"] == c["S"] - 1 and (len(f["starts"]) < 2 or f["starts"][1] == 1),
    "short_trailing_segment": lambda c, f: 0 < f["n_frames"] - f["starts"][-1] < f["seg"],
    "grid_one_partial_block": lambda c, f: f["blocks"] == 1 and f["seg"] < 256,
    "grid_one_full_pass": lambda c, f: f["blocks"] == 64 and f["seg"] == 64 * 256,
    "grid_second_pass_of_4": lambda c, f: f["blocks"] == 64 and f["seg"] - 64 * 256 == 4,
    "grid_three_passes": lambda c, f: f["blocks"] == 64 and f["passes"] == 3,
    "pieces_6": lambda c, f: f["last"]["pieces"] == 6,
    "workers": lambda c, f: f["last"]["workers"],
    "torn_frames": lambda c, f: _torn(f),
    "sub_slices": lambda c, f: len(f["last"]["starts"]) >= SUB_SLICES_FROM and any(n > 1 for n in c["sub_slices"] or (2,)),
    "resampling": lambda c, f: f["resampling"] and f["seg"] != c["S"],
    "raw_seg_11025": lambda c, f: f["seg"] == 11025 and f["seg"] % 2 == 1,
    "raw_seg_24000": lambda c, f: f["seg"] == 24000,
    "raw_seg_122": lambda c, f: f["seg"] == 122,
    "at": lambda c, f: c["call"] == "at" and all(a <= b for a, b in zip(f["starts"], f["starts"][1:])) and f["starts"][-1] < f["n_frames"],
    "at_repeated": lambda c, f: any(a == b for a, b in zip(f["starts"], f["starts"][1:])),
    "at_last_frame": lambda c, f: f["starts"][-1] == f["n_frames"] - 1,
    "at_gaps": lambda c, f: any(b - a > f["seg"] for s in f["slices"] for a, b in zip(s["starts"], s["starts"][1:])),
    "nonfinite": lambda c, f: c["nonfinite"] and c["fmt"] == "f32" and len(f["slices"]) == 1,
}
TAG_CHECKS.update({f"fmt_{k}": (lambda c, f, k=k: c["fmt"] == k) for k in BYTES})
TAG_CHECKS.update({f"ch{k}": (lambda c, f, k=k: c["channels"] == k) for k in (1, 2, 3, 8)})


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_every_case_is_the_edge_its_tags_claim(c):
    f = facts(c, 0)
    assert c["S"] % 4 == 0 and c["S"] >= 132 and c["tags"]
    for tag in c["tags"]:
        assert TAG_CHECKS[tag](c, f), (c["id"], tag)
    f1 = facts(c, 1)                                   # run 1: a shorter stream whose last row is padded
    assert f1["n_frames"] < f["n_frames"] and f1["starts"][-1] + f1["seg"] > f1["n_frames"], c["id"]
    if "sub_slices" in c["tags"]:
        assert len(f1["last"]["starts"]) >= SUB_SLICES_FROM
    # every start, length and offset is one the entry points accept: nothing here can be refused or read outside the stream
    for ff in (f, f1):
        assert all(0 <= s < ff["n_frames"] for s in ff["starts"]) and src_len(c["overlap"], c["rate"]) < ff["seg"]
        assert case_stream(c, 0 if ff is f else 1).size == ff["n_frames"] * ff["frame_bytes"]


def test_the_catalogue_covers_every_axis():
    tags = {t for c in CASES for t in c["tags"]}
    assert tags == set(TAG_CHECKS), sorted(set(TAG_CHECKS) ^ tags)
    assert {(c["fmt"], c["channels"]) for c in CASES} >= {(f, n) for f in BYTES for n in (1, 2, 3, 8)}
    routes = {(c["fmt"], facts(c)["last"]["route"]) for c in CASES}
    assert {r for _, r in routes} == {"staged", "pinned", "fd", "unstaged"}
    assert max(len(facts(c)["starts"]) for c in CASES) <= 700           # nothing larger than the 300-segment case's context is needed


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_every_mutant_of_the_reference_shows_in_every_case_of_its_family(c):
    """over the rows the GPU module compares: the last slice of both runs"""
    mixed = c["channels"] > 1
    truth = [case_reference(c, run)[0] for run in (0, 1)]
    for name, applies in MUTANTS.items():
        if not applies(c):
            continue
        seen = sum(int((~same_bits(case_reference(c, run, name)[0], truth[run], mixed)).sum()) for run in (0, 1))
        assert seen > 0, (c["id"], name)


def test_the_extremes_are_in_the_streams_and_decode_as_stated():
    """the listed values reach the compared rows of some case of their format, and decode to what the issue says"""
    x = _samples(EXTREMES["s16"].reshape(-1), "s16", 5, 1)[:, 0]
    assert list(x) == [0.0, 2.0 ** -15, -2.0 ** -15, 32767 / 32768, -1.0]
    x = _samples(EXTREMES["s24"].reshape(-1), "s24", 4, 1)[:, 0]
    assert list(x) == [2.0 ** -23, -2.0 ** -23, (2 ** 23 - 1) / 2 ** 23, -1.0]
    x = _samples(EXTREMES["s32"].reshape(-1), "s32", 5, 1)[:, 0]
    # -1 -> -2^-31; 2^24 + 1 ties to even 2^24, 2^24 + 3 ties to even 2^24 + 4; INT32_MAX rounds to 2^31: 1.0
    assert list(x) == [-2.0 ** -31, 2.0 ** -7, (2 ** 24 + 4) / 2 ** 31, 1.0, -1.0]
    for fmt in BYTES:
        ext = EXTREMES[fmt]
        c = BY_ID[f"{fmt}_ch1_slices"]
        rows, f = case_reference(c)
        want = _samples(ext.reshape(-1), fmt, len(ext), 1)[:, 0].view(np.uint32)
        assert (rows[0, :len(ext)].view(np.uint32) == want).all(), fmt       # the first samples of the last slice's first segment
    rows, _ = case_reference(BY_ID["f32_nonfinite_ch1"])
    bits = set(rows.view(np.uint32).reshape(-1).tolist())
    assert {0x7F7FFFFF, 0x7F800000, 0xFF800000, NAN_A, NAN_B, 0x00000001} <= bits
