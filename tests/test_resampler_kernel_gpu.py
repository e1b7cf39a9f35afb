"""The resampler's operator as it lies on the device, tap by tap, and resample_kernel<FT> / resample16_kernel<FT>
(birda_amd/csrc/resample.hip) element by element, against float64 -- through include/birda_hip_resample_debug.h, no classifier.

tests/test_resampler_gpu.py holds the whole resampler to the oracle within 2e-5: the operator's own shift-variance, the dropped
taps, the table's f32 rounding and the kernels' arithmetic under one number, 300 times what an f32-grade sum of 1 200 taps needs.
Here each has its own bound.

(a) The table.  d_op, unpacked from the fragment-major layout of kernels.hpp (ResamplePlan), against tests/test_resampler.py
    plan64 (anchored to the oracle on the CPU):  |T - t64| <= 2^-24 |t64| + 1e-12 max |t64|  (the table's f32 rounding; the
    round-off of the library's double FFT), padding columns and taps past the plan's last exactly 0, dmin and K those of plan64;
    d_op16: hi == float16(T 2^s), lo == float16(T 2^s - hi) bit for bit, max |T| 2^s in [2^13, 2^14), padding +0.
(b) Both kernels against  ref[N m + p] = sum_k float64(T[p][k]) x[hop m + dmin + k]  with the DEVICE's T (so that (a)'s error is
    not counted twice), B the same sum over absolute values:
        f32:        |got - ref| <= 7 x 1.2 tau B,  tau = 4e-7 max(1, sqrt(K / 1024))  (tests/test_layer_gemm_gpu.py)
        split f16:  the same + F A sum_k |T[p][k]| + F max |T| sum_k |x| + 2^-150,  F = 2^-38
    Why 7 x and not 1.2 tau B alone ("The resampler, held to its own operator"): both kernels MISS 1.2 tau B,
    the f32 kernel by up to 2.71 x (8 000 -> 48 000; 8 to 91 of ~30 000 elements a launch), and the cause is not in the kernels.
    A float32 emulation on the CPU of resample_kernel's order -- one fused multiply-add per product, k ascending within a wave's
    quarter of K, the four partial sums added owner first -- gives the device's outputs: the same elements fail with the same
    errors to nine digits (44 100 -> 48 000: 8 elements, first 3348 / 3980 / 6261 / 7973; 8 000 -> 48 000: 91; 88 200 -> 32 000:
    17).  So the kernel is exactly the f32 chain, K + 3 roundings an output, each at most u |partial sum|, u = 2^-24.  tau was
    calibrated on GEMMs of operands with random signs, whose partial sums stay near B / sqrt(K); a resampling filter's sum is
    coherent -- for an output phase that falls on an input sample the taps are almost a delta and the partial sum IS B for half
    the chain.  With every partial sum at B the error's standard deviation is sigma_max = u B sqrt(K / 12) (K / 4 roundings of
    variance u^2 B_w^2 / 3 in each wave, sum B_w = B); 7 x 1.2 tau = 1.05e-7 sqrt(K) = 1.76 u sqrt(K) = 6.1 sigma_max, a factor
    sqrt(K) / 1.76 >= 18 inside the sequential-sum bound K u B it must never pass.  The split-f16 kernel rounds 3 K / 128 + 3
    times and errs by at most 3 x 2^-22 a product (two operand residues and the dropped lo x lo): less on these inputs, the same bound.
    The two floors are the operands that land among the f16 subnormals after the two block scalings.  A product's operand is
    v = hi + lo + e with hi, lo float16 (round to nearest even both times, lo = v - hi formed exactly); where lo is a normal f16,
    |e| <= 2^-11 |lo| <= 2^-22 |v|, which the tau term carries; where lo is subnormal (spacing 2^-24), |e| <= 2^-25 ABSOLUTE in the
    scaled domain.  The span is scaled so that its largest sample m 2^e (1 <= m < 2) becomes m 2^13: the absolute error of a sample
    is 2^-25 2^e / 2^13 = 2^-38 2^e <= 2^-38 A, A the largest |x| of the workgroup's span -- a sum over the K taps gives
    2^-38 A sum |T|.  The table is scaled to max |T| 2^s in [2^13, 2^14) alike: 2^-38 max |T| sum |x|.  (The mantissa m of the
    maximum only makes 2^e smaller than A: no doubling to 2^-37 is needed, the derived exponent is -38.)
    A span holding inf is not scaled (its A counts as 2^13: the floor is 2^-25 sum |T|); a NaN does not enter the maximum.
    2^-150 is half the spacing of the f32 subnormals: the one rounding of the store's multiply when the OUTPUT is subnormal (the
    spans of denormals of (d)); for any other output it is nothing.
    The span is [t0 hop + dmin, + (16 FT - 1) hop + K), t0 = 16 FT (m / (16 FT)), from the exported plan.
(c) Launches of three segments of different content (the third times 1e-3), in_stride = src_len + 13 with NaN behind each row,
    out_stride = out_len + 64: every element of [0, out_len) written, every element of [out_len, out_stride) still 0x7fc0beef;
    16 FT + 3 frames (the tile edge, truncating), an out_len that is no multiple of N nor of 4, a zero pad that starts inside a
    float4, src_len in {1, 7, K - 1, hop, hop + 1}.
(d) The f16 kernel's block floating point at the edges of its scale: span maxima of biased exponent 13, 14, 63, 64, 140, 141, 253,
    254, zeros, denormals only, 1e-4.
(e) One sample of 1.0: every output is one tap -- exact on the f32 kernel, |got - T| <= 2^-22 |T| + 2^-38 max |T| on f16, +0
    outside the window; the sample at the first and last k of every wave's quarter of K, seen from the frames on both sides of
    the tile edge.
(f) NaN, +inf, -inf: exactly the outputs whose K-window covers the sample are non-finite.
(g) A segment's row has the same bits at n_seg 1, 3 and 80 and anywhere in the batch.
(h) src_len, out_len above 2^31 - 1 and n_seg above 65 535 are refused before anything is touched.
(i) Both kernels ran at FT 1, 2 and 4.

Worst measured error / bound (MI355X; printed by the last test): DESIGN.md section 3.
"""
import ctypes as C

import numpy as np
import pytest

from birda_amd import _lib
from test_layer_gemm_gpu import _tau
from test_resampler import cached_plan64, frame_matrix, output_len

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
BH_ERR_INVALID, BH_ERR_UNSUPPORTED = -1, -6
TAU_FACTOR = 7.0                # of 1.2 tau: 6.1 sigma of a coherent f32 chain of K roundings, derived in the docstring, (b)
F16_FLOOR = 2.0 ** -38          # derived in the docstring, (b)
OUT_FLOOR = 2.0 ** -150
REACHED = set()
WORST = {}                      # (kernel name, pair) -> worst error / bound

# pair -> (form, FT, N, hop): chosen for the paths they reach
PAIRS = {
    (44100, 48000): (0, 4, 160, 147),      # one column block
    (22050, 48000): (0, 4, 320, 147),      # two column blocks
    (8000, 48000): (0, 4, 480, 80),        # three column blocks, the shortest hop
    (48000, 32000): (0, 4, 160, 240),      # decimating polyphase
    (96000, 48000): (1, 2, 512, 1024),     # block form: four column blocks, the last with 128 padding columns
    (96000, 32000): (1, 2, 342, 1026),     # N % 4 = 2: the element-wise stores, rows that start unaligned
    (240000, 48000): (1, 2, 205, 1025),    # N odd
    (500000, 48000): (1, 2, 108, 1125),    # N below one f16 column block and a half
    (88200, 32000): (1, 1, 480, 1323),     # hop 1 323: FT = 1
}
PAIR_IDS = [f"{a}-{b}" for a, b in PAIRS]
KERNELS = [pytest.param(0, id="f32"), pytest.param(1, id="f16")]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_DEV = {}


def device_plan(frm, to):
    """the plan as bh_debug_resample_plan exports it, the two layouts of kernels.hpp (ResamplePlan) undone:
    T [nblk 160][K] float32, hi / lo [nblk 160][K] float16"""
    if (frm, to) in _DEV:
        return _DEV[(frm, to)]
    lib = _lib.load()
    params = np.zeros(8, np.int32)
    rc = lib.bh_debug_resample_plan(0, frm, to, _p(params), None, 0, None, 0)
    assert rc == 0, (rc, lib.bh_last_error())
    hop, N, nblk, K, dmin, form, FT, s = (int(v) for v in params)
    assert nblk == -(-N // 160) and K % 128 == 0
    op, op16 = np.empty(nblk * K * 160, np.float32), np.empty(2 * nblk * K * 160, np.uint16)
    assert lib.bh_debug_resample_plan(0, frm, to, _p(params), _p(op), op.size - 1, None, 0) == BH_ERR_INVALID
    rc = lib.bh_debug_resample_plan(0, frm, to, _p(params), _p(op), op.size, _p(op16), op16.size)
    assert rc == 0, (rc, lib.bh_last_error())
    # d_op [nblk][K/16][10][64 lanes][4]: k = 16 g + 4 (lane >> 4) + c, p = 160 cb + 16 mt + (lane & 15)
    T = op.reshape(nblk, K // 16, 10, 4, 16, 4).transpose(0, 2, 4, 1, 3, 5).reshape(nblk * 160, K)
    # d_op16 [2 nblk][K/32][5]{hi, lo}[64 lanes][8]: k = 32 st + 8 (lane >> 4) + j, p = 80 cb + 16 mt + (lane & 15)
    planes = op16.view(np.float16).reshape(2 * nblk, K // 32, 5, 2, 4, 16, 8).transpose(3, 0, 2, 5, 1, 4, 6).reshape(2, nblk * 160, K)
    _DEV[(frm, to)] = dict(frm=frm, to=to, hop=hop, N=N, nblk=nblk, K=K, dmin=dmin, form=form, FT=FT, s=s,
                           T=np.ascontiguousarray(T), hi=np.ascontiguousarray(planes[0]), lo=np.ascontiguousarray(planes[1]))
    return _DEV[(frm, to)]


def run(dp, X, src_len, out_len, f16, out_stride=None):
    """one launch; X [n_seg][in_stride].  -> (out [n_seg][out_len], kernel name); every element of [0, out_len) was written,
    every element of [out_len, out_stride) still holds the fill"""
    lib = _lib.load()
    X = np.ascontiguousarray(X, np.float32)
    n_seg, in_stride = X.shape
    out_stride = out_len + 64 if out_stride is None else out_stride
    out = np.empty((n_seg, out_stride), np.float32)
    name = C.create_string_buffer(64)
    rc = lib.bh_debug_resample(0, _p(X), n_seg, in_stride, src_len, dp["frm"], dp["to"], _p(out), out_stride, out_len, f16, name, 64)
    assert rc == 0, (rc, lib.bh_last_error())
    name = name.value.decode()
    REACHED.add(name)
    assert name == f"resample{'16' if f16 else ''}_kernel<FT={dp['FT']}>", name
    bits = out.view(np.uint32)
    never = bits[:, :out_len] == UNWRITTEN
    assert not never.any(), (name, "elements never written", int(never.sum()), np.argwhere(never)[:4])
    past = bits[:, out_len:] != UNWRITTEN
    assert not past.any(), (name, "written past out_len", int(past.sum()), np.argwhere(past)[:4])
    return out[:, :out_len], name


def inputs(frm, n_seg, src_len, seed, pad=13):
    """segments of different content (noise + tone, noise, a chirp-like tone + noise), every third times 1e-3; NaN behind each row"""
    rng = np.random.default_rng(seed)
    X = np.full((n_seg, src_len + pad), np.nan, np.float32)
    t = np.arange(src_len)
    for s in range(n_seg):
        if s % 3 == 0:
            v = 0.3 * rng.standard_normal(src_len) + 0.5 * np.sin(2 * np.pi * 1234.5 * t / frm)
        elif s % 3 == 1:
            v = rng.uniform(-1.0, 1.0, src_len)
        else:
            v = 1e-3 * (0.6 * np.sin(2 * np.pi * (300.0 + 0.5 * t) * t / frm) + 0.2 * rng.standard_normal(src_len))
        X[s, :src_len] = np.clip(v, -1, 1)
    return X


def reference(dp, x, out_len, f16):
    """-> (ref, bound) [out_len] float64 for one segment's samples x (the valid ones); non-finite ref where the window holds a
    non-finite sample"""
    hop, N, K, dmin, FT = dp["hop"], dp["N"], dp["K"], dp["dmin"], dp["FT"]
    T = dp["T"][:N].astype(np.float64)
    aT = np.abs(T)
    frames = -(-out_len // N)
    n_valid = min(out_len, output_len(x.size, dp["frm"], dp["to"]))
    Xm = frame_matrix(x, hop, dmin, K, frames)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = (Xm @ T.T).reshape(-1)[:out_len]
        B = (np.abs(Xm) @ aT.T).reshape(-1)[:out_len]
        assert TAU_FACTOR * 1.2 * _tau(3, K) <= K * 2.0 ** -24 / 18             # never past the sequential-sum bound K 2^-24 B
        bound = TAU_FACTOR * 1.2 * _tau(3, K) * B
        if f16:
            xs = np.asarray(x, np.float64)
            A = np.zeros(frames)
            for t0 in range(0, frames, 16 * FT):
                lo, hi = t0 * hop + dmin, t0 * hop + dmin + (16 * FT - 1) * hop + K
                span = np.abs(xs[max(lo, 0):max(min(hi, xs.size), 0)])
                a = 0.0 if not np.isfinite(span).any() else float(span[np.isfinite(span)].max())
                A[t0:t0 + 16 * FT] = 2.0 ** 13 if np.isinf(span).any() else a          # (a span holding inf keeps scale 1)
            floor = F16_FLOOR * (A[:, None] * aT.sum(axis=1)[None, :] + aT.max() * np.abs(Xm).sum(axis=1)[:, None])
            bound = bound + floor.reshape(-1)[:out_len] + OUT_FLOOR
    ref[n_valid:] = 0.0
    bound[n_valid:] = 0.0
    return ref, bound


def check(dp, X, src_len, got, name, what, group=""):
    """every element of every segment; records and returns the worst error / bound"""
    f16 = name.startswith("resample16")
    worst = 0.0
    for s in range(X.shape[0]):
        ref, bound = reference(dp, X[s, :src_len], got.shape[1], f16)
        fin = np.isfinite(ref)
        g = got[s].astype(np.float64)
        assert (np.isfinite(g) == fin).all(), (what, name, s, "non-finite pattern", int((~np.isfinite(g)).sum()), int((~fin).sum()),
                                               np.argwhere(np.isfinite(g) != fin)[:4].ravel())
        err = np.abs(g[fin] - ref[fin])
        bd = bound[fin]
        bad = ~(err <= bd)
        assert not bad.any(), (what, name, s, int(bad.sum()), np.argwhere(bad)[:4].ravel(), err[bad][:4], bd[bad][:4])
        pos = bd > 0
        if pos.any():
            worst = max(worst, float((err[pos] / bd[pos]).max()))
    key = (name + group, (dp["frm"], dp["to"]))
    WORST[key] = max(WORST.get(key, 0.0), worst)
    return worst


# ---- (a) the operator, tap by tap ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frm,to", list(PAIRS), ids=PAIR_IDS)
def test_the_device_table_is_plan64_rounded_once(frm, to):
    dp, pl = device_plan(frm, to), cached_plan64(frm, to)
    form, FT, N, hop = PAIRS[(frm, to)]
    assert (dp["form"], dp["FT"], dp["N"], dp["hop"]) == (form, FT, N, hop)
    assert (dp["hop"], dp["N"], dp["form"]) == (pl["hop"], pl["N"], int(pl["block"]))
    assert (dp["dmin"], dp["K"]) == (pl["dmin"], pl["K"])                            # plan64's window, rounded up to 128
    K, T, t64 = dp["K"], dp["T"], pl["T"]
    tmax = np.abs(t64).max()
    err = np.abs(T[:N].astype(np.float64) - t64)
    tol = 2.0 ** -24 * np.abs(t64) + 1e-12 * tmax          # the table's f32 rounding + the round-off of the library's double FFT
    bad = err > tol
    print(f"{frm} -> {to}: hop {hop} N {N} K {K} dmin {dp['dmin']} FT {FT} s {dp['s']}: worst (|T - t64| - 2^-24 |t64|) / max |t64| = "
          f"{float((err - 2.0 ** -24 * np.abs(t64)).max() / tmax):.2e} (allowed 1e-12)")
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], err[bad][:4], tol[bad][:4])
    bits = T.view(np.uint32)
    assert not bits[N:].any()                                                         # padding columns: +0
    last = hop - 1 - dp["dmin"]                # the plan's last tap, impulse position hop - 1 (at or past K where the window ends before it)
    assert not bits[:, last + 1:].any() and T[:N, :last + 1].any()
    # the f16 planes
    s = dp["s"]
    scaled = np.ldexp(T, s)                                                           # float32, exact
    m = float(np.abs(scaled).max())
    assert 2.0 ** 13 <= m < 2.0 ** 14, (m, s)
    hi = scaled.astype(np.float16)
    lo = (scaled - hi.astype(np.float32)).astype(np.float16)
    assert np.isfinite(hi).all()
    assert (dp["hi"].view(np.uint16) == hi.view(np.uint16)).all()
    assert (dp["lo"].view(np.uint16) == lo.view(np.uint16)).all()
    assert not dp["hi"].view(np.uint16)[N:].any() and not dp["lo"].view(np.uint16)[N:].any()
    assert not dp["hi"].view(np.uint16)[:, last + 1:].any() and not dp["lo"].view(np.uint16)[:, last + 1:].any()


# ---- (b), (c) both kernels, element by element -----------------------------------------------------------------------------------
def _src_for(dp, out_len):
    """a source length whose resampled length is at least out_len"""
    n = -(-out_len // dp["N"]) * dp["hop"] + 5
    while output_len(n, dp["frm"], dp["to"]) < out_len:
        n += dp["hop"]
    return n


@pytest.mark.parametrize("f16", KERNELS)
@pytest.mark.parametrize("frm,to", list(PAIRS), ids=PAIR_IDS)
def test_every_element_against_float64(frm, to, f16):
    dp = device_plan(frm, to)
    N, hop, K, FT = dp["N"], dp["hop"], dp["K"], dp["FT"]
    launches = []
    # 16 FT + 3 frames: past the workgroup's frame tile into the next one's first rows, whose span starts at t0 hop + dmin > 0;
    # the source is longer than these outputs need -- out_len truncates
    full = (16 * FT + 3) * N
    src = _src_for(dp, full) + hop
    assert output_len(src, frm, to) > full and 16 * FT * hop + dp["dmin"] > 0
    launches.append(("tile edge, truncating", src, full))
    # an out_len that is a multiple neither of N nor of 4
    odd = full - N // 2 - 1
    while odd % 4 == 0 or odd % N == 0:
        odd -= 1
    launches.append(("odd out_len", src, odd))
    # out_len above the resampled length: zeros past n_valid, and the pad starts inside a float4
    short = (16 * FT + 1) * hop + 3
    while output_len(short, frm, to) % 4 == 0 or output_len(short, frm, to) % N == 0:
        short += 1
    n_valid = output_len(short, frm, to)
    launches.append(("zero pad", short, n_valid + N + 7))
    # spans that are mostly padding
    for n in (1, 7, K - 1, hop, hop + 1):
        launches.append((f"src_len {n}", n, 2 * N + 5))
    for i, (what, src_len, out_len) in enumerate(launches):
        X = inputs(frm, 3, src_len, 1000 * i + frm % 997)
        got, name = run(dp, X, src_len, out_len, f16)
        worst = check(dp, X, src_len, got, name, what)
        nv = min(out_len, output_len(src_len, frm, to))
        assert not got[:, nv:].view(np.uint32).any()                                  # the pad is +0
        print(f"{frm} -> {to} {name} {what}: src_len {src_len} out_len {out_len} n_valid {nv}: worst error / bound {worst:.3f}")


# ---- (d) amplitude: the f16 kernel's block floating point ------------------------------------------------------------------------
def _amplitude_input(src_len, ex):
    """|x| <= 0.4 2^(ex - 127) with a sample of 1.125 2^(ex - 127) every 97: every span's maximum has biased exponent ex (and
    at ex = 254 the outputs stay below the largest float)"""
    X = inputs(44100, 3, src_len, 4242)
    v = X[:, :src_len] * np.float32(0.4)
    v[:, ::97] = 1.125
    X[:, :src_len] = np.ldexp(v, ex - 127)
    return X


@pytest.mark.parametrize("case", ["ex13", "ex14", "ex63", "ex64", "ex140", "ex141", "ex253", "ex254", "zeros", "denormals", "1e-4"])
def test_f16_block_floating_point_at_the_edges_of_its_scale(case):
    """13 / 14: below and at the smallest span maximum one float factor can bring to 2^13; 63 / 64: the edge of the two-step
    scaling; 140: already in [2^13, 2^14), no scaling; 141: the smallest that is scaled down; 253 / 254: the largest finite
    exponents.  Before this test the kernel left spans below exponent 14 and at exponent 254 unscaled: silence for the first
    (every sample an f16 zero), inf for the second (every sample past 65 504)."""
    frm, to = 44100, 48000
    dp = device_plan(frm, to)
    out_len = (16 * dp["FT"] + 3) * dp["N"]
    src_len = _src_for(dp, out_len)
    if case.startswith("ex"):
        X = _amplitude_input(src_len, int(case[2:]))
        span_max = np.abs(X[:, :src_len]).max()
        assert (int(np.float32(span_max).view(np.uint32)) >> 23) & 255 == int(case[2:])
    else:
        X = inputs(frm, 3, src_len, 77)
        X[:, :src_len] *= {"zeros": np.float32(0.0), "denormals": np.float32(1e-40), "1e-4": np.float32(1e-4)}[case]
        if case == "denormals":
            v = np.abs(X[:, :src_len])
            assert v.max() < 2.0 ** -126 and (v > 0).sum() > v.size // 2
    got, name = run(dp, X, src_len, out_len, 1)
    assert np.isfinite(got).all(), (case, "non-finite outputs", int((~np.isfinite(got)).sum()))
    if case != "zeros":
        assert (got != 0).mean() > 0.9, (case, "silence")
    worst = check(dp, X, src_len, got, name, case, group=" amplitude edges")
    print(f"{name} {case}: worst error / bound {worst:.3f}")


# ---- (e) isolation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", KERNELS)
@pytest.mark.parametrize("frm,to", [(44100, 48000), (96000, 48000), (88200, 32000)], ids=["FT4", "FT2", "FT1"])
def test_one_sample_reads_the_table_back(frm, to, f16):
    """eight segments, each one sample of 1.0: for frame 16 FT - 1 (the last row of the first tile) it sits at the first or last k
    of a wave's quarter of K; frame 16 FT sees it `hop` columns earlier, every other frame that covers it somewhere else."""
    dp = device_plan(frm, to)
    N, hop, K, dmin, FT = dp["N"], dp["hop"], dp["K"], dp["dmin"], dp["FT"]
    frames = 16 * FT + 3
    out_len, src_len = frames * N, (16 * FT + 4) * hop
    ks = [0, K // 4 - 1, K // 4, K // 2 - 1, K // 2, 3 * K // 4 - 1, 3 * K // 4, K - 1]
    X = np.full((len(ks), src_len + 13), np.nan, np.float32)
    X[:, :src_len] = 0.0
    pos = [hop * (16 * FT - 1) + dmin + k for k in ks]
    assert min(pos) >= 0 and max(pos) < src_len and output_len(src_len, frm, to) >= out_len
    for s, j in enumerate(pos):
        X[s, j] = 1.0
    got, name = run(dp, X, src_len, out_len, f16)
    T = dp["T"][:N]
    tmax = float(np.abs(T).max())
    for s, j in enumerate(pos):
        k_of = j - hop * np.arange(frames) - dmin                                   # the tap each frame reads the sample with
        inside = (k_of >= 0) & (k_of < K)
        want = np.where(inside[:, None], T[:, np.clip(k_of, 0, K - 1)].T, np.float32(0.0)).astype(np.float32) + np.float32(0.0)
        assert inside[16 * FT - 1] and k_of[16 * FT - 1] == ks[s]
        g = got[s].reshape(frames, N)
        assert not g[~inside].view(np.uint32).any(), (name, s, "outputs whose window does not cover the sample are +0")
        if not f16:
            bad = g.view(np.uint32) != want.view(np.uint32)
            assert not bad.any(), (name, s, int(bad.sum()), np.argwhere(bad)[:4], g[bad][:4], want[bad][:4])
        else:       # hi + lo's residue, and the subnormal floor of the scaled planes; the sample itself is 2^13, exact
            err = np.abs(g.astype(np.float64) - want)
            tol = 2.0 ** -22 * np.abs(want) + 2.0 ** -38 * tmax
            bad = err > tol
            assert not bad.any(), (name, s, int(bad.sum()), np.argwhere(bad)[:4], err[bad][:4], tol[bad][:4])


# ---- (f) non-finite samples --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", KERNELS)
@pytest.mark.parametrize("frm,to", [(44100, 48000), (96000, 32000)], ids=PAIR_IDS[:1] + PAIR_IDS[5:6])
def test_a_non_finite_sample_reaches_exactly_the_outputs_that_cover_it(frm, to, f16):
    """The contract (stated beside the kernels): a NaN or an inf among the samples makes every output whose K-window covers it
    non-finite -- a zero padding tap times inf is NaN -- and no other; outputs at or past the resampled length stay 0.  Around
    it the f32 kernel gives the bits of the clean run; the f16 kernel, whose span scale an inf switches off, stays in its bound."""
    dp = device_plan(frm, to)
    N, hop, K, dmin, FT = dp["N"], dp["hop"], dp["K"], dp["dmin"], dp["FT"]
    out_len = (16 * FT + 3) * N - 3
    src_len = _src_for(dp, out_len)
    clean = inputs(frm, 3, src_len, 5)
    dirty = clean.copy()
    where = [hop * 7 + 11, hop * (16 * FT - 1) + 3, hop * (16 * FT + 1) + 5]         # mid-tile, across the tile edge, in the second tile
    for s, (j, v) in enumerate(zip(where, (np.nan, np.inf, -np.inf))):
        dirty[s, j] = v
    got0, name = run(dp, clean, src_len, out_len, f16)
    got1, _ = run(dp, dirty, src_len, out_len, f16)
    assert np.isfinite(got0).all()
    check(dp, clean, src_len, got0, name, "clean")
    check(dp, dirty, src_len, got1, name, "non-finite")                              # the pattern, and the bound around it
    for s, j in enumerate(where):
        m = np.arange(-(-out_len // N))
        covered = np.repeat((hop * m + dmin <= j) & (j < hop * m + dmin + K), N)[:out_len]
        assert 0 < covered.sum() < out_len
        assert (~np.isfinite(got1[s]) == covered).all(), (name, s)
        if not f16:
            assert (got1[s][~covered].view(np.uint32) == got0[s][~covered].view(np.uint32)).all(), (name, s)


# ---- (g) launch independence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", KERNELS)
@pytest.mark.parametrize("frm,to", [(44100, 48000), (96000, 32000)], ids=PAIR_IDS[:1] + PAIR_IDS[5:6])
def test_a_row_has_the_same_bits_in_any_launch(frm, to, f16):
    dp = device_plan(frm, to)
    out_len = (16 * dp["FT"] + 3) * dp["N"] - 1
    src_len = _src_for(dp, out_len)
    X = inputs(frm, 3, src_len, 31)
    three, name = run(dp, X, src_len, out_len, f16)
    check(dp, X, src_len, three, name, "n_seg 3")
    for s in range(3):
        one, _ = run(dp, X[s:s + 1], src_len, out_len, f16)
        assert (one.view(np.uint32) == three[s:s + 1].view(np.uint32)).all(), (name, s)
    order = np.random.default_rng(8).integers(0, 3, 80)
    order[:3] = (2, 0, 1)
    many, _ = run(dp, X[order], src_len, out_len, f16)
    assert (many.view(np.uint32) == three.view(np.uint32)[order]).all(), name


# ---- (h) argument ranges -----------------------------------------------------------------------------------------------------------
def test_lengths_past_int32_and_segment_counts_past_the_grid_are_refused(model_dir):
    """(written after the checks: api.hip resample_ranges looks at the numbers alone, and bh_debug_resample, bh_resample_device and
    bh_resample call it before a plan is built, a buffer allocated or copied, or a kernel launched -- the small buffers below are
    never indexed with the lengths they are passed with)"""
    import torch
    from birda_amd.classifier import BirdClassifier
    lib = _lib.load()
    small, out = np.zeros(64, np.float32), np.empty(128, np.float32)
    big = 2 ** 31

    def dbg(n_seg, in_stride, src_len, out_stride, out_len):
        return lib.bh_debug_resample(0, _p(small), n_seg, in_stride, src_len, 44100, 48000, _p(out), out_stride, out_len, 0, None, 0)

    assert dbg(1, 32, 32, 64, 40) == 0                                               # the buffers as they are
    assert dbg(1, big, big, 64, 40) == BH_ERR_INVALID and b"2^31 - 1" in lib.bh_last_error()
    assert dbg(1, 32, 32, big, big) == BH_ERR_INVALID and b"2^31 - 1" in lib.bh_last_error()
    assert dbg(65536, 32, 32, 64, 40) == BH_ERR_INVALID and b"65 535" in lib.bh_last_error()
    assert dbg(1, 32, 33, 64, 40) == BH_ERR_INVALID and dbg(1, 32, 32, 64, 65) == BH_ERR_INVALID and dbg(0, 32, 32, 64, 40) == BH_ERR_INVALID
    path, labels, _, _ = model_dir["mini"]
    clf = BirdClassifier(path, labels)
    ctx = clf.create_batch_context(4)
    d_in, d_out = torch.zeros(64, device="cuda"), torch.full((128,), 7.0, device="cuda")

    def dev(n_seg, in_stride, src_len, out_stride, out_len):
        return lib.bh_resample_device(clf._h, ctx._h, d_in.data_ptr(), in_stride, src_len, 44100, 48000, d_out.data_ptr(), out_stride, out_len, n_seg)

    assert dev(1, 32, 32, 64, 40) == 0
    ctx.synchronize()
    assert (d_out.cpu().numpy()[40:] == 7.0).all()
    assert dev(1, big, big, 64, 40) == BH_ERR_INVALID and b"2^31 - 1" in lib.bh_last_error()
    assert dev(1, 32, 32, big, big) == BH_ERR_INVALID and b"2^31 - 1" in lib.bh_last_error()
    assert dev(65536, 32, 32, 64, 40) == BH_ERR_INVALID and b"65 535" in lib.bh_last_error()
    assert dev(1, big - 1, 32, big - 1, 40) == 0                                     # strides are no lengths: one row, its stride unused
    ctx.synchronize()
    assert (d_out.cpu().numpy()[40:] == 7.0).all()
    n_out = C.c_size_t()
    assert lib.bh_resample(clf._h, _p(small), big, 44100, 48000, _p(out), 2 ** 40, C.byref(n_out)) == BH_ERR_INVALID
    assert b"2^31 - 1" in lib.bh_last_error()
    ctx.close(); clf.close()


def test_a_refused_pair_is_unsupported_with_the_plans_message():
    lib = _lib.load()
    params = np.zeros(8, np.int32)
    assert lib.bh_debug_resample_plan(0, 47999, 48000, _p(params), None, 0, None, 0) == BH_ERR_UNSUPPORTED
    assert b"resampler:" in lib.bh_last_error() and b"47999 -> 48000" in lib.bh_last_error()
    x, y = np.zeros(64, np.float32), np.empty(64, np.float32)
    assert lib.bh_debug_resample(0, _p(x), 1, 64, 64, 47999, 48000, _p(y), 64, 64, 0, None, 0) == BH_ERR_UNSUPPORTED
    assert lib.bh_debug_resample_plan(0, 48000, 48000, _p(params), None, 0, None, 0) == BH_ERR_INVALID


# ---- (i) every instantiation was reached (keep last: it reads what the tests above ran) --------------------------------------------
def test_every_resampler_instantiation_was_reached():
    if not REACHED:
        pytest.skip("reads the kernels the module's other tests ran: run the module whole")
    want = [f"resample{k}_kernel<FT={ft}>" for k in ("", "16") for ft in (1, 2, 4)]
    missing = [w for w in want if w not in REACHED]
    assert not missing, (missing, sorted(REACHED))
    print("\nworst error / bound by kernel and pair:")
    for (name, pair), v in sorted(WORST.items()):
        print(f"  {name:40s} {pair[0]:>6d} -> {pair[1]:<6d} {v:.3f}")
