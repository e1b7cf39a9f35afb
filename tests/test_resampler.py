"""The resampler's operator in float64, written from the definition (the header comment of birda_amd/csrc/resample.hip and
oracle/birda_oracle.c resampler_new / resampler_block), and anchored here -- on the CPU, before any kernel is involved -- to the
oracle's block-FFT restatement of the reference's resampler.  tests/test_resampler_kernel_gpu.py holds the device's table and
both kernels to plan64 / apply_taps.

plan64(from, to):  sizes as resample_sizes; cutoff powf(0.4f, 16.0f / ni) in float32 (x no / ni when decimating); the sinc windowed
by BlackmanHarris^2, unit sum, scaled 1 / (2 ni); R[i][n] (i < hop) the response of one block to a unit impulse -- irfft at 2 no,
un-normalised, of the first new_len bins of rfft(impulse, 2 ni) * Hf; y[N m0 + n] += x[hop m0 + i] R[i][n]; the taps
t_p[d] = R[hop m + d][N m + p], m = ceil(-d / hop); the window [dmin, dmin + K) is what holds a tap above 1e-9 max |t|, K rounded
up to 128.

What the oracle comparison shows (max |apply64 - oracle.resample| over the lengths below, |x| <= 1):
  * up-sampling and block-form pairs: <= 6e-8 = 2^-24, the oracle's own rounding of a block's output to f32 -- bound 2^-23;
  * 48 000 -> 32 000: 3.0e-6, 44 100 -> 32 000: 7.5e-7 -- the shift-variance of the reference's resampler when it decimates in
    polyphase form (resample.hip documents it): a property of that operator, no slack for a kernel, which is why the kernels are
    held to their own table and not to the oracle.
"""
import ctypes as C
import ctypes.util
import math

import numpy as np
import pytest

# up-sampling pairs, block-form pairs (every one tests/test_resampler_kernel_gpu.py uses), decimating polyphase pairs
UP_PAIRS = [(44100, 48000), (22050, 48000), (8000, 48000)]
BLOCK_PAIRS = [(96000, 48000), (96000, 32000), (240000, 48000), (384000, 48000), (500000, 48000), (88200, 32000)]
# pair -> bound = twice the measured difference from the oracle: the reference operator's own shift-variance, NOT slack for a kernel
SHIFT_VARIANT_PAIRS = {(48000, 32000): 2 * 3.0e-6, (44100, 32000): 2 * 7.5e-7}
ORACLE_ROUNDING = 2.0 ** -23        # twice 2^-24: the oracle rounds each block's output to f32, |y| <~ 1


def _powf(a, b):
    """libm's powf on float32 operands (the library and the oracle call it); numpy's float32 power where there is no libm to load"""
    name = ctypes.util.find_library("m")
    if name:
        f = C.CDLL(name).powf
        f.restype, f.argtypes = C.c_float, [C.c_float, C.c_float]
        return float(f(a, b))
    return float(np.power(np.float32(a), np.float32(b)))


def sizes(frm, to):
    g = math.gcd(frm, to)
    chunks = -(-1024 // (frm // g))
    return chunks * (frm // g), chunks * (to // g)


def output_len(n, frm, to):
    """bh_resample_output_len restated: whole blocks, then ceil(rem * to / from) of the zero-padded last one"""
    if frm == to:
        return n
    fi, fo = sizes(frm, to)
    full, rem = divmod(n, fi)
    return full * fo + (min(fo, math.ceil(rem * to / frm)) if rem else 0)


def plan64(frm, to):
    """-> dict(hop, N, K, dmin, block, ni, no, T [N][K] (0 for taps at d >= hop), full [N][d_hi - d_lo] with d_lo)"""
    ni, no = sizes(frm, to)
    g = math.gcd(frm, to)
    P, Q = frm // g, to // g
    block = 2 * frm > 3 * to
    N = no if block else Q * 160 // math.gcd(Q, 160)
    hop = ni if block else N // Q * P
    cut = np.float32(16.0) / np.float32(ni)
    cutoff = _powf(0.4, float(cut)) * ((no / ni) if ni > no else 1.0)
    i = np.arange(ni, dtype=np.float64)
    arg = np.pi * cutoff * (i - ni // 2)
    s = np.where(np.abs(arg) < 1e-12, 1.0, np.sin(arg) / np.where(arg == 0, 1.0, arg))
    xw = 2 * np.pi * i / ni
    w = 0.35875 - 0.48829 * np.cos(xw) + 0.14128 * np.cos(2 * xw) - 0.01168 * np.cos(3 * xw)
    h = s * w * w
    h = h / h.sum() / (2 * ni)
    new_len = ni + 1 if ni < no else no
    Hf = np.fft.rfft(h, 2 * ni)[:new_len]
    k = np.arange(new_len)
    ph = (np.arange(hop)[:, None] * k[None, :]) % (2 * ni)                          # rfft of a unit impulse at i, phase reduced exactly
    B = np.zeros((hop, no + 1), np.complex128)
    B[:, :new_len] = np.exp(-2j * np.pi * ph / (2 * ni)) * Hf[None, :]
    R = np.fft.irfft(B, 2 * no, axis=1) * (2 * no)                                  # [hop][2 no], un-normalised
    M = (2 * no + N - 1) // N + 1
    d_lo = -M * hop
    full = np.zeros((N, (M + 1) * hop), R.dtype)                                    # columns d = d_lo .. hop - 1
    for m in range(M + 1):                                                           # d = i - m hop, n = N m + p
        n0, n1 = N * m, min(N * m + N, 2 * no)
        if n1 > n0:
            full[:n1 - n0, (M - m) * hop:(M - m + 1) * hop] = R[:, n0:n1].T
    tmax = np.abs(full).max()
    live = np.nonzero(np.abs(full).max(axis=0) > 1e-9 * tmax)[0]
    dmin, dmax = int(live[0]) + d_lo, int(live[-1]) + d_lo
    K = (dmax - dmin + 1 + 127) // 128 * 128
    T = np.zeros((N, K), R.dtype)
    have = min(K, hop - dmin)
    T[:, :have] = full[:, dmin - d_lo:dmin - d_lo + have]
    return dict(frm=frm, to=to, hop=hop, N=N, K=K, dmin=dmin, dmax=dmax, block=block, ni=ni, no=no, T=T, full=full, d_lo=d_lo)


def frame_matrix(x, hop, dmin, K, frames):
    """X[m][k] = x[hop m + dmin + k] in float64, samples outside x counting as zero"""
    x = np.asarray(x, np.float64)
    idx = hop * np.arange(frames)[:, None] + dmin + np.arange(K)[None, :]
    ok = (idx >= 0) & (idx < x.size)
    return np.where(ok, x[np.clip(idx, 0, max(x.size - 1, 0))], 0.0) if x.size else np.zeros(idx.shape)


def apply_taps(T, hop, N, dmin, x, n_out, n_valid=None):
    """y[N m + p] = sum_k T[p][k] x[hop m + dmin + k] in float64, samples outside x counting as zero, outputs at or past n_valid
    zero.  -> (y [n_out], B [n_out] = the same sum over absolute values)"""
    T = np.asarray(T, np.float64)
    X = frame_matrix(x, hop, dmin, T.shape[1], -(-n_out // N))
    with np.errstate(invalid="ignore", over="ignore"):
        y = (X @ T.T).reshape(-1)[:n_out]
        B = (np.abs(X) @ np.abs(T).T).reshape(-1)[:n_out]
    if n_valid is not None:
        y[n_valid:] = 0.0
        B[n_valid:] = 0.0
    return y, B


def apply64(plan, x, n_out):
    return apply_taps(plan["T"], plan["hop"], plan["N"], plan["dmin"], x, n_out)


_PLANS = {}


def cached_plan64(frm, to):
    if (frm, to) not in _PLANS:
        _PLANS[(frm, to)] = plan64(frm, to)
    return _PLANS[(frm, to)]


def signal(n, frm, seed):
    """the suite's noise-plus-tone signal (tests/test_resampler_gpu.py)"""
    rng = np.random.default_rng(seed)
    return np.clip(0.3 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 1234.5 * np.arange(n) / frm), -1, 1).astype(np.float32)


def _lib_output_len(n, frm, to):
    from birda_amd import _lib
    out = C.c_size_t()
    assert _lib.load().bh_resample_output_len(n, frm, to, C.byref(out)) == 0
    return out.value


def _worst_against_oracle(oracle_lib, frm, to):
    pl = cached_plan64(frm, to)
    fi, fo = oracle_lib.resampler_sizes(frm, to)
    assert (fi, fo) == (pl["ni"], pl["no"]) == sizes(frm, to)
    worst = 0.0
    for n in (3 * fi + 17, fi, fi - 1, fi // 3, 1):
        x = signal(n, frm, 1)                               # (seed 1: the signal the bounds above were measured on)
        want = oracle_lib.resample(x, frm, to)
        n_out = _lib_output_len(n, frm, to)                  # a host function of the library: callable without a GPU
        assert n_out == output_len(n, frm, to) == want.size, (frm, to, n)
        got, B = apply64(pl, x, n_out)
        assert B.shape == got.shape == want.shape and (B >= np.abs(got) - 1e-15).all()
        worst = max(worst, float(np.abs(got - want).max()))
    return worst


@pytest.mark.parametrize("frm,to", UP_PAIRS + BLOCK_PAIRS)
def test_plan64_is_the_oracles_operator_to_its_last_bit(oracle_lib, frm, to):
    worst = _worst_against_oracle(oracle_lib, frm, to)
    print(f"{frm} -> {to}: max |apply64 - oracle| = {worst:.2e}")
    assert worst <= ORACLE_ROUNDING, (frm, to, worst)


@pytest.mark.parametrize("frm,to", sorted(SHIFT_VARIANT_PAIRS))
def test_plan64_on_decimating_polyphase_pairs_differs_by_the_operators_shift_variance(oracle_lib, frm, to):
    worst = _worst_against_oracle(oracle_lib, frm, to)
    print(f"{frm} -> {to}: max |apply64 - oracle| = {worst:.2e}")
    # twice the measured 3.0e-6 (48 000 -> 32 000) / 7.5e-7 (44 100 -> 32 000): the reference resampler's own shift-variance when
    # it decimates -- the oracle applies the block operator at every block offset, plan64 reads it at the first `hop` -- and not slack
    # for a kernel: the kernels are held to their own table (tests/test_resampler_kernel_gpu.py)
    assert worst <= SHIFT_VARIANT_PAIRS[(frm, to)], (frm, to, worst)
    assert worst > ORACLE_ROUNDING                            # ... and it is there: were it gone, these pairs belong in the list above


@pytest.mark.parametrize("frm,to", UP_PAIRS + BLOCK_PAIRS + sorted(SHIFT_VARIANT_PAIRS))
def test_tap_support(frm, to):
    """outside the densest window of K columns every tap is below 1e-9 max |t|; the window ends before an impulse position of
    the next frame; K is a multiple of 128 (four waves x an even number of 16-deep groups) that wastes less than 128 columns"""
    pl = cached_plan64(frm, to)
    full, K = np.abs(pl["full"]), pl["K"]
    tmax = full.max()
    col = full.max(axis=0)
    mass = np.convolve(col, np.ones(K), "valid")              # the window of K columns that holds the most
    best = int(mass.argmax())
    outside = np.concatenate([col[:best], col[best + K:]])
    assert outside.size == 0 or outside.max() < 1e-9 * tmax
    lo = pl["dmin"] - pl["d_lo"]
    outside = np.concatenate([col[:lo], col[lo + K:]])
    assert outside.size == 0 or outside.max() < 1e-9 * tmax
    assert K % 128 == 0 and 0 <= K - (pl["dmax"] - pl["dmin"] + 1) < 128 and pl["dmax"] < pl["hop"]
    assert col[lo] > 1e-9 * tmax and col[pl["dmax"] - pl["d_lo"]] > 1e-9 * tmax
    assert 0.5 * min(1.0, to / frm) < tmax < 1.5              # a resampling filter of unit gain: its peak is about the cutoff


def test_shapes_the_kernel_tests_count_on():
    """hop, N and the form of every pair tests/test_resampler_kernel_gpu.py picks for the path it reaches"""
    want = {(44100, 48000): (147, 160, False), (22050, 48000): (147, 320, False), (8000, 48000): (80, 480, False),
            (48000, 32000): (240, 160, False), (96000, 48000): (1024, 512, True), (96000, 32000): (1026, 342, True),
            (240000, 48000): (1025, 205, True), (500000, 48000): (1125, 108, True), (88200, 32000): (1323, 480, True)}
    for (frm, to), (hop, N, block) in want.items():
        ni, no = sizes(frm, to)
        g = math.gcd(frm, to)
        is_block = 2 * frm > 3 * to
        n = no if is_block else (to // g) * 160 // math.gcd(to // g, 160)
        assert ((ni if is_block else n // (to // g) * (frm // g)), n, is_block) == (hop, N, block), (frm, to)
