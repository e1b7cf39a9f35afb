"""The spectrogram front end (kernels_frontend.hip minmax_kernel / mel_kernel / mel32_kernel, api_plan.hip build_gf): its float64
reference, the bound the device is held to, and the case table tests/test_frontend_gpu.py runs -- everything that needs no GPU.

The reference is oracle.frontend64, written from the definition: normalise, frame, periodic Hann, Re(rFFT),
mel matrix, square, power law, flip, affine.  It is checked here against the C oracle's bo_frontend (f32 arithmetic) and against
the committed float64 vectors.

The bound has no constant fitted to the kernels.  With u = 2^-24, v the value the power law is applied to, G the dense window x DFT
x mel operator, B = sum_j |x_j| |G[j][m]| over the frame's normalised samples, SG = sum_j |G[j][m]| and dc = sum_j G[j][m]:

    normalisation   the kernel's fl(fl(x - min) sc - 1), sc = fl(2 / fl(fl(max - min) + eps)), against the exact divide form:
                    sc carries three roundings (3u, the same factor on every x + 1 of the segment: 3u |v + dc| in v), x - min one
                    (u (x + 1)), the fma one (u |x|):                                      3u |v + dc| + u (2 B + SG)
    fold            y = x[a] + x[b], one f32 add:                                          u B
    operand         |Gf64 - f32(Gf)| entry by entry, and for the f16 kernels the exact |f32(Gf) 2^s - (hi + lo)| 2^-s of the two
                    planes (the lo halves of the small entries near the window's edge are subnormal or zero: an absolute term),
                    times |y|:                                                             |y| . E_G
    products        the per-GEMM tolerance of tests/test_layer_gemm_gpu.py for the f32 MFMA and for split f16 with both operands
                    split (tau = 4e-7 max(1, sqrt(K / 1024)), K = L / 2):                   tau B
    four waves      three f32 adds of partial sums:                                        3u B

delta is their sum.  With f(a) = a^(2 expo) the output is held to

    |out_scale| (f(|v| + delta) - f(max(|v| - delta, 0)))  +  |out_scale| f(|v| + delta) rel  +  u (|out_scale| f + |out|)

which stays valid through v = 0 where f has no derivative.  rel is the power law's own arithmetic, exp2(fma(expo, log2(p), bias)),
p = (v 2^s)^2: v_log_f32 and v_exp_f32 at 1 ulp (2^-23) each as the instruction set documents them, the rounding of v v (u), of
the fma (u |z|), of expo as create computes it in f32 (expf, an add, a divide: 4u, which costs |log2 p| expo as much in the exponent)
and of log2_bias (u |bias|); an error dz in the exponent is a relative ln 2 dz in f.  The last term is the affine's two roundings.

Near v = 0 that bound widens, so a test could pass by vacuity: for every case on ordinary audio the share of elements with
|v| < 8 delta is at most 1e-3, asserted here from the reference alone.  Those elements are still held to their own bound."""
import math
import os
import sys

import numpy as np
import pytest

from birda_amd import modelfile as mf, synth
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_layer_gemm_gpu import _tau                               # noqa: E402  (the per-GEMM tolerance, shared)

U = 2.0 ** -24
ULP = 2.0 ** -23
NEAR_ZERO_CAP = 1e-3        # share of elements with |v| < 8 delta, ordinary audio
LDS_BYTES = 160 * 1024
TOPS = (0.95, 0.8, 0.7, 0.6)          # each branch's fmax as a share of Nyquist (fe_model, live_band)
NARROW = (0.0, 3000.0)               # a band so narrow that most mel columns hold no weight (the zero_columns cases)
AFFINE = ((0.8, -0.4), (1.25, 0.1), (0.5, -1.0), (2.0, 0.3))


def K(mt, prec):
    return f"bh::mel_kernel<{mt}, {prec}, 1>"


def K32(mt):
    return f"bh::mel32_kernel<{mt}>"


REACHABLE = {K(mt, p) for mt in range(2, 9) for p in (0, 3)} | {K32(mt) for mt in range(1, 5)}     # what launch_mel can launch


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
def case(cid, kernel, branches, n_mels, S=12000, n_frames=None, flip=True, prec="f16x3", mel32=None, n_seg=2, signal="synth",
         alone=False, band=None):
    """branches: [(frame_length, hop)]; n_frames None: as many as the segment holds (the fewest over the branches); prec: the
    classifier's precision; mel32: BIRDA_HIP_MEL32 (None: unset); alone: every row must also equal the segment run alone; band:
    fe_model's"""
    if n_frames is None:
        n_frames = min((S - L) // H + 1 for L, H in branches)
    return dict(id=cid, kernel=kernel, branches=list(branches), n_mels=n_mels, S=S, n_frames=n_frames, flip=flip, prec=prec,
                mel32=mel32, n_seg=n_seg, signal=signal, alone=alone, band=band)


def _exact(nf, L, H, extra=0):
    return (nf - 1) * H + L + extra


def _cases():
    c = []
    # every instantiation, named: MT = 2 .. 8 in f32 and split f16, MT32 = 1 .. 4; with and without the flip; odd mel counts
    geo = {20: (512, 100), 40: (256, 103), 64: (512, 101), 72: (1024, 100), 96: (512, 278), 100: (256, 97), 128: (1024, 100)}
    for nm, (L, H) in geo.items():
        for prec, p in (("f32", 0), ("f16x3", 3)):
            for flip in (True, False):
                c.append(case(f"inst_mel{nm}_{prec}_{'flip' if flip else 'noflip'}", K((nm + 15) // 16, p), [(L, H)], nm, flip=flip,
                              prec=prec, mel32="0", signal="synth" if flip else "noise"))
    for nm, H, env in ((20, 96, None), (50, 320, None), (90, 100, "1"), (128, 80, None)):
        for flip in (True, False):
            c.append(case(f"inst_mel32_{nm}_{'flip' if flip else 'noflip'}", K32((nm + 31) // 32), [(512, H)], nm, flip=flip,
                          mel32=env, signal="noise" if flip else "synth"))
    # reduction depths, and which kernel create chooses for each: L % 256 != 0 -> the f32 kernel even in f16x3 (gpw = 1, 3),
    # L % 512 != 0 -> no mel32; spw = 1, 2, 3, 4, 8; nch = 1, 2, 4
    for L in (128, 256, 384, 512, 768, 1024, 2048):
        c.append(case(f"depth_L{L}_f32", K(3, 0), [(L, 100)], 40, prec="f32"))
        c.append(case(f"depth_L{L}_f16x3", K(3, 3 if L % 256 == 0 else 0), [(L, 100)], 40))
        c.append(case(f"depth_L{L}_mel32", K32(2) if L % 512 == 0 else K(4, 3 if L % 256 == 0 else 0), [(L, 96)], 50))
    # hops: one per frame pairing dd of mel32 (H mod 64 = 32: 1; 16: 2; 8: 4; 4: 8; 2: 16; odd and 0: the default 16) ...
    for H in (96, 80, 72, 100, 102, 101, 64):
        c.append(case(f"hop{H}_mel32", K32(2), [(512, H)], 50, mel32="1"))
    # ... odd and prime hops on mel_kernel, a hop longer than the frame
    for H, L in ((101, 512), (277, 1024), (7, 256), (300, 256)):
        for prec, p in (("f32", 0), ("f16x3", 3)):
            c.append(case(f"hop{H}_L{L}_{prec}", K(6, p), [(L, H)], 96, prec=prec, S=16000 if H == 277 else 12000))
    # frame counts around the 48- and 32-frame tiles, the last frame ending exactly at the segment's end (the staging fast path at
    # equality) and 4 / 12 samples before it
    # (enough segments that the table's conditioning cap, a share of 1e-3, can be resolved: >= 20 000 elements a case)
    segs_for = lambda nf, nm: max(3, -(-20000 // (nf * nm)))          # noqa: E731
    for nf in (1, 16, 47, 48, 49, 97):
        for extra in (0, 4, 12):
            c.append(case(f"frames{nf}_end{extra}", K(3, 3), [(512, 100)], 40, S=_exact(nf, 512, 100, extra), n_frames=nf,
                          n_seg=segs_for(nf, 40)))
        c.append(case(f"frames{nf}_f32_oddhop", K(3, 0), [(256, 101)], 40, S=(_exact(nf, 256, 101) + 3) & ~3, n_frames=nf, prec="f32",
                      n_seg=segs_for(nf, 40)))
    for nf in (1, 31, 32, 33, 65):
        for extra in (0, 8):
            c.append(case(f"frames{nf}_end{extra}_mel32", K32(2), [(512, 96)], 50, S=_exact(nf, 512, 96, extra), n_frames=nf,
                          n_seg=segs_for(nf, 50)))
    # spans beyond the prefetch capacity (15 or 16 x 4 KB in mel_kernel, 11 x 4 KB in mel32): the staging tail
    c.append(case("span_tail_f16x3", K(6, 3), [(2048, 400)], 96, S=24000, mel32="0"))
    c.append(case("span_tail_f32", K(7, 0), [(2048, 400)], 100, S=24000, prec="f32"))
    c.append(case("span_tail_mel32", K32(3), [(2048, 400)], 96, S=24000))
    # the largest span create accepts: 47 x 827 + 2048 samples = 163 680 bytes of LDS (mel32: 31 x 957 + 2048, + the staged rows)
    c.append(case("span_max_f16x3", K(3, 3), [(2048, 827)], 40, S=_exact(49, 2048, 827), n_frames=49))
    c.append(case("span_max_f32", K(8, 0), [(2048, 827)], 128, S=_exact(49, 2048, 827), n_frames=49, prec="f32"))
    c.append(case("span_max_mel32", K32(2), [(2048, 957)], 50, S=_exact(33, 2048, 957) + 3 & ~3, n_frames=33, mel32="1"))
    # branches and the work-item walk: 1 .. 4 branches of unequal L and H, launches of 1, 2 and 7 segments ...
    four = [(512, 100), (256, 103), (1024, 96), (768, 97)]
    for nb in (1, 2, 3, 4):
        for n_seg in (1, 2, 7):
            c.append(case(f"branches{nb}_seg{n_seg}", K(3, 3), four[:nb], 40, n_seg=n_seg, alone=n_seg == 7))
    c.append(case("branches4_f32_L128", K(5, 0), [(512, 100), (256, 103), (1024, 96), (128, 101)], 72, n_seg=7))
    c.append(case("branches2_mel32", K32(2), [(512, 96), (1024, 80)], 50, n_seg=7, alone=True))
    # ... and launches whose items exceed twice the resident workgroups: paired, several persistent steps, the grid trimmed to a
    # multiple of 8 n_branches (3 branches: 512 -> 504)
    c.append(case("walk_3branches_130seg", K(3, 3), four[:3], 40, n_seg=130, alone=True))
    c.append(case("walk_4branches_mt7_60seg", K(7, 3), four, 100, n_seg=60, alone=True))
    c.append(case("walk_2branches_f32_190seg", K(2, 0), four[:2], 20, n_seg=190, prec="f32", alone=True))
    c.append(case("walk_mel32_2branches_140seg", K32(1), [(512, 96), (1024, 80)], 20, n_seg=140, alone=True))
    # inputs
    for sig in ("square", "dc", "const", "minmax"):
        c.append(case(f"input_{sig}_f16x3", K(6, 3), [(512, 100), (1024, 96)], 96, signal=sig, n_seg=16 if sig == "minmax" else 3,
                      mel32="0"))
        c.append(case(f"input_{sig}_f32", K(3, 0), [(512, 100)], 40, prec="f32", signal=sig, n_seg=16 if sig == "minmax" else 3))
        c.append(case(f"input_{sig}_mel32", K32(4), [(512, 80)], 128, signal=sig, n_seg=16 if sig == "minmax" else 3))
    # a segment so short that minmax_kernel's last slices are empty (sample_count / 4 = 33 and 41: 7 of 8 slices hold samples)
    c.append(case("empty_slices_132", K(3, 0), [(128, 4)], 40, S=132, n_frames=2, n_seg=4, signal="noise"))
    c.append(case("empty_slices_164", K(2, 0), [(128, 12)], 20, S=164, n_frames=4, n_seg=4, signal="noise"))
    # mel columns without a single weight (0 .. 3000 Hz: 100 or 128 triangles on 8, 16, 32 bins): v = 0 exactly, the output exactly
    # out_shift.  (Every other case takes live_band: all columns live wherever the bins allow it.)
    c.append(case("zero_columns_f32", K(7, 0), [(128, 100)], 100, signal="noise", band=NARROW))
    c.append(case("zero_columns_f16x3", K(7, 3), [(256, 100)], 100, signal="noise", band=NARROW))
    c.append(case("zero_columns_mel32", K32(4), [(512, 96)], 128, signal="noise", band=NARROW))
    return c


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]
ORDINARY = ("synth", "noise")

# refused at create, each by its message: (id, message, keyword arguments of fe_model, BIRDA_HIP_MEL32 or None)
REFUSALS = [
    ("mels16", "n_mels 16 not built", dict(branches=[(512, 100)], n_mels=16, S=12000), None),
    ("mels129", "n_mels 129 not built", dict(branches=[(512, 100)], n_mels=129, S=12000), None),
    ("L192", "frame_length 192 must be a multiple of 128", dict(branches=[(192, 100)], n_mels=40, S=12000), None),
    ("S12002", "sample_count 12002 must be a multiple of 4", dict(branches=[(512, 100)], n_mels=40, S=12002), None),
    ("lds", "more than a CU's 160 KB of LDS", dict(branches=[(2048, 828)], n_mels=40, S=_exact(49, 2048, 828), n_frames=49), None),
    # mel32_kernel's own limit (the span of 32 frames + the staged rows): a hop of 957 is in the table, 958 is refused -- in f32, where
    # the same file lands on mel_kernel, by that kernel's limit
    ("lds_mel32", "more than a CU's 160 KB of LDS", dict(branches=[(2048, 958)], n_mels=50, S=_exact(33, 2048, 958), n_frames=33), "1"),
]


_BANDS = {}


def live_band(n_mels, n_bins, sr, top):
    """(fmin, fmax): up to `top` of Nyquist, from the lowest fmin at which every mel column holds a weight -- a triangle narrower
    than the bin spacing holds none, and such a column's output is out_shift whatever the kernel does.  Where no band leaves them
    all live (more mels than bins), the one that leaves the most."""
    key = (n_mels, n_bins, sr, top)
    if key not in _BANDS:
        fmax, best = top * sr / 2.0, None
        for fmin in (0.0, 200.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0, 12000.0):
            live = int(np.count_nonzero(synth.linear_to_mel_weight_matrix(n_mels, n_bins, sr, fmin, fmax).any(axis=0)))
            if best is None or live > best[0]:
                best = (live, fmin)
            if live == n_mels:
                break
        _BANDS[key] = (best[1], fmax)
    return _BANDS[key]


def fe_model(branches, n_mels, S, n_frames=None, flip=True, sr=48000, band=None):
    """A model file with the front end under test and a token network behind it (the pattern of tests/test_full_conv_gpu.py
    conv_model): a 3x3 stride-2 NCHW stem to 8 channels, the pool, a dense layer to 4 classes.  band: (fmin, fmax) of every
    branch; None: live_band, with a different top for each branch"""
    if n_frames is None:
        n_frames = min((S - L) // H + 1 for L, H in branches)
    b = synth._Builder(np.random.default_rng(11))
    brs = []
    for i, (L, H) in enumerate(branches):
        fmin, fmax = band if band is not None else live_band(n_mels, L // 2 + 1, sr, TOPS[i])
        br = mf.Branch(L, H, n_mels, n_frames, fmin, fmax, 1.23 - 0.2 * i)
        br.mel_w_off = b.put(synth.linear_to_mel_weight_matrix(n_mels, br.n_bins, sr, fmin, fmax))
        br.out_scale, br.out_shift = AFFINE[i]
        br.flags = 1 if flip else 0
        brs.append(br)
    t, h, w = b.conv(0, n_mels, n_frames, len(brs), 8, 3, 2, mf.ACT_GELU_ERF, in_layout=1)
    t = b.gap(t, h, w, 8)
    b.dense(t, 8, 4)
    return mf.Model(0, sr, S, S / sr, 4, 8, mf.OUT_SIGMOID, t, n_mels, n_frames, 1e-6, brs, b.layers, np.concatenate(b.chunks))


def case_model(c):
    return fe_model(c["branches"], c["n_mels"], c["S"], c["n_frames"], c["flip"], band=c["band"])


def case_segments(c):
    """[n_seg][S] float32, seeded by the case's name"""
    n, S, sig = c["n_seg"], c["S"], c["signal"]
    rng = np.random.default_rng(sum(map(ord, c["id"])))
    if sig == "synth":
        return synth.synth_segments(n, S, 48000, start=len(c["id"]))
    if sig == "noise":
        return (rng.standard_normal((n, S)) * rng.uniform(0.02, 0.5, (n, 1))).astype(np.float32)
    if sig == "square":             # full scale, a different period per segment
        t = np.arange(S)[None, :]
        return np.where((t // (17 + 31 * np.arange(n)[:, None])) % 2 == 0, 1.0, -1.0).astype(np.float32)
    if sig == "dc":                 # a 1e-4 signal riding on 0.3
        return (0.3 + 1e-4 * rng.standard_normal((n, S))).astype(np.float32)
    if sig == "const":
        return np.repeat(np.asarray([0.25, -1.0, 0.0][:n], np.float32)[:, None], S, axis=1)
    if sig == "minmax":             # the extremes at the first / last sample of each of minmax_kernel's 8 slices
        x = (rng.standard_normal((n, S)) * 0.1).astype(np.float32)
        per = -(-(S // 4) // 8) * 4
        for k in range(n):
            p, q, edge = (k // 2) % 8, (k // 2 + 3) % 8, k % 2
            first = lambda s: s * per                                   # noqa: E731
            last = lambda s: min(S, (s + 1) * per) - 1                  # noqa: E731
            x[k, first(p) if edge == 0 else last(p)] = 2.0
            x[k, last(q) if edge == 0 else first(q)] = -3.0
        return x
    raise ValueError(sig)


def plan_kernel(c):
    """bh_classifier_create's choice restated (api_create.hip build_front_end): the test module on the GPU holds it to what launch_mel reports"""
    nm_pad = (c["n_mels"] + 15) // 16 * 16
    prec = 0 if c["prec"] == "f32" else 3
    if any(L % 256 for L, _ in c["branches"]):
        prec = 0
    if prec == 3:
        want = any(H % 16 == 0 for _, H in c["branches"])
        can = nm_pad % 32 == 0 and all(L % 512 == 0 for L, _ in c["branches"])
        if c["mel32"] is not None:
            want = c["mel32"] == "1"
        if want and can:
            return K32(nm_pad // 32)
    return K(nm_pad // 16, prec)


def lds_bytes(c):
    """kernels_frontend.hip mel_lds_bytes restated"""
    nm_pad = (c["n_mels"] + 15) // 16 * 16
    if c["kernel"].startswith("bh::mel32"):
        span = max(31 * H + L for L, H in c["branches"])
        return max((((span + 3) & ~3) + 4 * 2 * 32 * 36) * 4, 4 * (nm_pad // 32) * 4 * 64 * 16)
    span = max(47 * H + L for L, H in c["branches"])
    return max(((span + 3) & ~3) * 4, 4 * 3 * (nm_pad // 16) * 64 * 16)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference and the bound
# ---------------------------------------------------------------------------------------------------------------------------
def _operand_error(G, L, f16):
    """E_G [K][n_mels]: |Gf64 - what the device holds| for the folded operator (row j <-> sample j + 1, the last row halved), and
    the f16 planes' scale exponent s (0 for the f32 operator)"""
    Kd = L // 2
    Gf = G[1:Kd + 1].copy()
    Gf[Kd - 1] *= 0.5
    g32 = Gf.astype(np.float32)
    err = np.abs(Gf - g32.astype(np.float64))
    s = 0
    if f16:
        mx = float(np.abs(g32).max())
        if mx > 0.0:
            s = min(max(14 - math.frexp(mx)[1], -60), 60)
        sc = np.ldexp(g32.astype(np.float64), s)
        with np.errstate(over="raise"):
            hi = sc.astype(np.float32).astype(np.float16)
            lo = (sc - hi.astype(np.float64)).astype(np.float32).astype(np.float16)
        err = err + np.ldexp(np.abs(sc - hi.astype(np.float64) - lo.astype(np.float64)), -s)
    return err, s


def reference(c, segs=None, chunk=16):
    """-> (spec [n][n_branches][n_mels][n_frames] float64, bound (same shape), near [n_branches]: share of |v| < 8 delta among the
    elements of LIVE mel columns (a column without a weight has v = 0 and delta = 0: exact, and no part of the denominator),
    zero_rows [n_branches]: output rows whose mel column has no weight at all)"""
    m = case_model(c)
    segs = case_segments(c) if segs is None else segs
    f16 = not c["kernel"].endswith(", 0, 1>")
    n = segs.shape[0]
    spec = np.empty((n, len(m.branches), m.spec_h, m.spec_w))
    bound = np.empty_like(spec)
    near = np.zeros(len(m.branches))
    live = np.zeros(len(m.branches))
    zero_rows = []
    ops = {}
    for i0 in range(0, n, chunk):
        sp, det = O.frontend64(m, segs[i0:i0 + chunk])
        spec[i0:i0 + chunk] = sp
        for b, (br, d) in enumerate(zip(m.branches, det)):
            L, H, nf, Kd = br.frame_length, br.frame_step, br.n_frames, br.frame_length // 2
            if b not in ops:
                ops[b] = _operand_error(d["G"], L, f16)
            EG, s = ops[b]
            v, B, G, expo = d["v"], d["B"], d["G"], d["expo"]
            fr = np.lib.stride_tricks.sliding_window_view(d["xn"], L, axis=1)[:, ::H][:, :nf]
            y = np.abs(fr[:, :, 1:Kd + 1] + fr[:, :, L - 1:Kd - 1:-1])
            SG, dc = np.abs(G).sum(axis=0), G.sum(axis=0)
            delta = (3 * U * np.abs(v + dc) + U * (2 * B + SG)) + U * B + y @ EG + _tau(3 if f16 else 0, Kd) * B + 3 * U * B
            a = np.abs(v)
            scale, shift = abs(float(np.float32(br.out_scale))), float(np.float32(br.out_shift))
            f_hi, f_lo, f_0 = np.power(a + delta, 2 * expo), np.power(np.maximum(a - delta, 0.0), 2 * expo), np.power(a, 2 * expo)
            lp = np.abs(2.0 * np.log2(np.maximum(np.maximum(a, delta), 1e-300)))      # |log2 p|, p = v^2 (unscaled)
            lps = np.abs(2.0 * np.log2(np.maximum(np.maximum(a, delta), 1e-300)) + 2.0 * s)
            dz = expo * lps * ULP + expo * 1.4427 * U + U * expo * lp + 4 * U * expo * lp + U * abs(2.0 * s * expo)
            rel = math.log(2.0) * dz + ULP
            e = scale * (f_hi - f_lo) + scale * f_hi * rel + U * (scale * f_0 + np.abs(scale * f_0 + shift))
            near[b] += np.count_nonzero((a < 8 * delta)[:, :, SG > 0.0])
            live[b] = np.count_nonzero(SG > 0.0)
            if br.flags & 1:
                e = e[:, :, ::-1]
            bound[i0:i0 + chunk, b] = np.transpose(e, (0, 2, 1))
            if i0 == 0:
                zc = np.flatnonzero(SG == 0.0)
                zero_rows.append(sorted((br.n_mels - 1 - zc) if br.flags & 1 else zc))
    return spec, bound, near / (n * np.maximum(live, 1) * m.spec_w), zero_rows


# ---------------------------------------------------------------------------------------------------------------------------
# the reference against the oracle and the committed vectors
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mini", "birdnet_v24_tiny", "birdnet_v24"])
def test_reference_matches_the_oracle_frontend(kind, oracle_lib, tmp_path):
    """bo_frontend works in f32 (normalisation, window, the FFT's input and output, the mel sums in sequence, powf) around a float64
    FFT.  It is held to the float64 reference at ITS accuracy, in the same form as the device bound: delta = (n_bins + 8) u Bt, with
    Bt = sum_j |x_j| w_j sum_k |cos(2 pi k j / L)| W[k][m] the magnitude sum of the un-folded route (n_bins u: an f32 sum of n_bins
    terms in sequence; 8 u: the single roundings in front of it), through the power law as above, plus 8 u (1 + |ln f|) f for powf
    and the f32 expo, plus the affine's ulp."""
    m = synth.build_model(kind)
    path = str(tmp_path / "m.bhm")
    mf.write_model(path, m)
    om = oracle_lib.OracleModel(path)
    segs = synth.synth_segments(2, m.sample_count, m.sample_rate, start=3)
    ref, det = O.frontend64(m, segs)
    bound = np.empty_like(ref)
    for b, (br, d) in enumerate(zip(m.branches, det)):
        L, H, nf = br.frame_length, br.frame_step, br.n_frames
        W = np.asarray(m.blob[br.mel_w_off:br.mel_w_off + br.n_bins * br.n_mels], np.float64).reshape(br.n_bins, br.n_mels)
        n = np.arange(L)
        At = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / L))[:, None] * (np.abs(np.cos(2.0 * np.pi * ((n[:, None] * np.arange(br.n_bins)) % L) / L)) @ W)
        fr = np.lib.stride_tricks.sliding_window_view(d["xn"], L, axis=1)[:, ::H][:, :nf]
        delta = (br.n_bins + 8) * U * (np.abs(fr) @ At)
        a, expo = np.abs(d["v"]), d["expo"]
        f_hi, f_lo = np.power(a + delta, 2 * expo), np.power(np.maximum(a - delta, 0.0), 2 * expo)
        e = br.out_scale * (f_hi - f_lo + 8 * U * (1.0 + np.abs(np.log(np.maximum(f_hi, 1e-300)))) * f_hi) + U * (br.out_scale * f_hi + 1.0)
        bound[:, b] = np.transpose(e[:, :, ::-1] if br.flags & 1 else e, (0, 2, 1))
    for i in range(2):
        got = om.frontend(segs[i]).reshape(ref.shape[1:]).astype(np.float64)
        err = np.abs(got - ref[i])
        print(f"{kind} segment {i}: oracle against float64 max {err.max():.3e} mean {err.mean():.3e}, worst err / bound "
              f"{(err / bound[i]).max():.3f}")
        assert (err <= bound[i]).all() and err.mean() < 2e-6


def test_reference_matches_the_committed_float64_vectors():
    m = synth.build_model("birdnet_v24_tiny")
    vec = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_vectors.npz"))
    ref, _ = O.frontend64(m, synth.synth_segment(3)[None])
    err = np.abs(ref[0][:, :, ::7] - vec["tiny_spec_seg3_frames_every7"].astype(np.float64))
    print(f"float64 vectors (stored as f32): max {err.max():.3e}")
    assert err.max() <= 2.0 ** -23 * max(1.0, float(np.abs(ref).max()))      # the vectors' own f32 rounding


def test_dense_operator_is_the_fft_route():
    rng = np.random.default_rng(0)
    for L, nm in ((128, 20), (768, 40)):
        W = synth.linear_to_mel_weight_matrix(nm, L // 2 + 1, 48000, 0.0, 8000.0)
        G = O.frontend_operator64(L, W)
        x = rng.standard_normal((5, L))
        hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / L)
        want = np.fft.rfft(x * hann, axis=1).real @ W.astype(np.float64)
        assert np.abs(x @ G - want).max() <= 1e-10 * np.abs(want).max()
        assert np.abs(G[0]).max() == 0.0 and np.abs(G[1:] - G[:0:-1]).max() <= 1e-12          # what the fold rests on


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_instantiation():
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    named = {c["kernel"] for c in CASES if c["id"].startswith("inst_")}
    assert named == REACHABLE and len(REACHABLE) == 18, sorted(REACHABLE - named)
    for k in REACHABLE:       # with and without the flip, and on a mel count that is not a multiple of 16 where the tile allows one
        flips = {c["flip"] for c in CASES if c["kernel"] == k and c["id"].startswith("inst_")}
        assert flips == {True, False}, k
    assert sum(1 for c in CASES if c["n_mels"] % 16 and c["flip"]) >= 10


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_case_is_accepted_and_lands_on_its_kernel(c, tmp_path):
    """The reader's rules ((n_frames - 1) H + L <= sample_count, equal mel and frame counts: validate_model, run here through the
    library's host-only bh_plan_fused_blocks), create's own conditions, the kernel the table names, and the conditioning cap."""
    from birda_amd import _lib
    m = case_model(c)
    for br in m.branches:
        assert (br.n_frames - 1) * br.frame_step + br.frame_length <= m.sample_count
        assert br.n_mels == m.spec_h and br.n_frames == m.spec_w and br.frame_length % 128 == 0
    assert m.sample_count % 4 == 0 and 17 <= c["n_mels"] <= 128 and len(m.branches) <= 4
    path = str(tmp_path / "case.bhm")
    mf.write_model(path, m)
    assert _lib.load().bh_plan_fused_blocks(path.encode(), 1, None, None, 0) >= 0, _lib.load().bh_last_error()
    assert plan_kernel(c) == c["kernel"] and c["kernel"] in REACHABLE
    assert lds_bytes(c) <= LDS_BYTES
    if c["alone"] and c["n_seg"] > 16:      # (the large launches: their first segments stand for the rest here; the GPU module
        c = dict(c, n_seg=16)               #  checks every row)
    spec, bound, near, zero_rows = reference(c)
    assert np.isfinite(spec).all() and np.isfinite(bound).all() and (bound >= 0).all()
    print(f"{c['id']}: share of |v| < 8 delta per branch {[f'{s:.1e}' for s in near]}, median bound {np.median(bound):.2e}")
    dead = [len(z) for z in zero_rows]
    print(f"{c['id']}: mel columns without a weight per branch {dead} of {m.spec_h}")
    if c["signal"] in ORDINARY:      # (over the live columns: an all-zero one has v = 0 and delta = 0, exact, and is not counted)
        assert near.max() <= NEAR_ZERO_CAP, near
    if c["band"] is None and all(br.n_bins >= 2 * m.spec_h for br in m.branches):
        assert not any(dead), dead       # the band leaves every column live where the bins allow it
    if c["id"].startswith("zero_columns"):
        assert all(len(z) > 0 for z in zero_rows)
        for b, z in enumerate(zero_rows):        # the reference itself gives exactly out_shift there, with a bound of one ulp of it
            shift = float(np.float32(m.branches[b].out_shift))
            assert (spec[:, b, z] == shift).all() and (bound[:, b, z] <= 2 * U * abs(shift)).all()
            assert len(z) < m.spec_h


def test_refusal_cases_break_exactly_one_rule():
    for rid, _msg, kw, _env in REFUSALS:
        m = fe_model(**kw)
        for br in m.branches:     # the reader accepts them all: the refusal is create's
            assert (br.n_frames - 1) * br.frame_step + br.frame_length <= m.sample_count, rid
    assert lds_bytes(dict(kernel=K(3, 3), n_mels=40, branches=[(2048, 827)])) == 163680
    assert lds_bytes(dict(kernel=K(3, 3), n_mels=40, branches=[(2048, 828)])) > LDS_BYTES
    assert lds_bytes(dict(kernel=K32(2), n_mels=50, branches=[(2048, 957)])) == 163728
    assert lds_bytes(dict(kernel=K32(2), n_mels=50, branches=[(2048, 958)])) > LDS_BYTES
    assert _exact(33, 2048, 958) % 4 == 0


def test_scale_exponent_is_the_library_s():
    """_operand_error restates kernels.hpp f16_scale_exponent (the exponent s with max |Gf| 2^s in [2^13, 2^14), clamped to +-60):
    it enters the bound only (E_G and the u |2 s expo| term; the reference is free of s).  The library has no entry point that
    returns s, so the source lines are held here: if the rule changes, this fails and the bound is revisited with it."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "birda_amd", "csrc", "kernels.hpp")).read()
    body = src[src.index("inline int f16_scale_exponent(float max_abs)"):]
    body = body[:body.index("\n}")]
    assert "const int s = 14 - e;" in body and "return s < -60 ? -60 : (s > 60 ? 60 : s);" in body and "std::frexp(max_abs, &e)" in body
    for mx, want in ((1.0, 13), (0.75, 14), (16383.0, 0), (16384.0, -1), (3e-5, 29)):
        assert min(max(14 - math.frexp(mx)[1], -60), 60) == want and 2 ** 13 <= mx * 2.0 ** want < 2 ** 14
