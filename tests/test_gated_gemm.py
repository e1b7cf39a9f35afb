"""What tests/test_gated_gemm_f32_gpu.py holds the f32 gated project GEMM (kernels_conv.hip pw_gemm_kernel<BM, NT, GATE>) to, held
in turn on the CPU before the kernel is trusted to it:

* the float64 reference (oracle/oracle.py gated64, gated_bound64) against torch.addmm in float64;
* a mirror of the launcher's choice of instantiation (pick_nt and the `small` rule), from which the GPU module takes the names it
  expects, and the case table's reach: all sixteen names;
* a numpy float32 emulation of the GATE kernel's arithmetic as the source states it -- a x g rounded to f32 once on the way into
  LDS, the sum in f32 over k in the kernel's order (32-deep chunks, two 16-deep groups, MFMA step cc of lane quad q taking
  k = 32 c + 16 g + 4 q + cc), the gate row min(m, M - 1) // rows_per_seg, zero for k >= K -- which must meet the GPU module's own
  inequality on every case, and six mutants of it (the gate-row, K-tail and gate-column mistakes the GATE code could make) which
  must each miss it on at least one case: the inputs discriminate.

The inequality, every element (act = none here):  |got - ref| <= tau (1.2 bound + |R|) + eps_act,  bound = |A g| |W| + |b|,
tau = 4e-7 max(1, sqrt(K / 1024)) + 2^-24: the project's bound for this kernel family (tests/test_layer_gemm_gpu.py) and the one
extra rounding of a x g per product."""
import functools
import math
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_layer_gemm_gpu as TL  # noqa: E402  (_check, _tau: the inequality is imported, not restated)

TAU_GATE = 2.0 ** -24          # the rounding of a x g

# (n_seg, rows per segment, K, N, residual); M = n_seg * rows per segment
SMALL = [  # fewer than 512 blocks of 128 rows: BM = 64
    (9, 7, 4, 4, False),          # M = 63 < 64: one partial tile; K = 4: a tail of 4 and nothing else; N < 16
    (70, 1, 8, 12, True),         # a gate row per row; the last tile holds 6 rows
    (5, 7, 12, 10, False),        # N % 4 != 0: W's rows padded, ld = 12 != N; a tail of 12
    (5, 50, 36, 20, True),        # tiles straddling two segments; one chunk + 4; N % 16 != 0
    (3, 64, 44, 32, False),       # a segment exactly one tile; one chunk + 12
    (3, 50, 44, 48, False),
    (30, 7, 100, 44, True),       # up to ten segments a tile; three chunks + 4
    (2, 1000, 8, 64, True),       # a segment larger than the tile: the gate row changes inside tile 15
    (4, 50, 320, 68, False),      # whole chunks
    (1, 50, 36, 80, True),        # one segment, M < 64
    (130, 1, 44, 96, True),
    (19, 7, 1392, 100, True),     # 43 chunks + 16: one whole 16-deep group in the last chunk
    (6, 7, 100, 112, False),
    (2, 64, 36, 128, False),
    (3, 64, 320, 16, True),
    (3, 50, 100, 136, True),      # NT 3 in three column blocks, the last of 40 columns
    (11, 7, 8, 232, False),       # NT 5 in three column blocks
    (2, 64, 4, 384, True),        # NT 8 in three column blocks
    (4, 50, 52, 64, False),       # a tail of 20: two groups, the second of 4
]
BIG = [  # 512 blocks of 128 rows and more: BM = 128.  One column block at K = 8 (4, 44), and N = 136 in three
    (65536, 1, 8, 4, True),
    (9345, 7, 4, 20, False),      # M = 65 415: the last tile holds 7 rows
    (1309, 50, 8, 44, True),
    (1024, 64, 8, 64, False),     # two whole segments a tile
    (66, 1000, 8, 68, True),
    (9345, 7, 44, 96, False),
    (1309, 50, 8, 100, True),
    (1024, 64, 8, 128, False),
    (22, 1000, 36, 136, True),
]
CASES = SMALL + BIG
ALL_NAMES = {f"pw_gemm_kernel<BM={bm},NT={nt},GATE>" for bm in (64, 128) for nt in range(1, 9)}


def case_id(c):
    return "n%d_P%d_K%d_N%d_r%d" % c


# ---------------------------------------------------------------------------------------------------------------------------
# the launcher's choice (kernels_conv.hip pick_nt, launch_pw_gemm_gated)
# ---------------------------------------------------------------------------------------------------------------------------
def pick_nt(N):
    """the widest column tile that wastes the fewest padded columns"""
    best, best_pad = 1, -1
    for nt in range(8, 0, -1):
        bn = nt * 16
        padded = -(-N // bn) * bn
        if best_pad < 0 or padded < best_pad:
            best_pad, best = padded, nt
    return best


def kernel_name(M, N, gated=True):
    nt = pick_nt(N)
    blocks128 = -(-M // 128) * -(-N // (16 * nt))
    return f"pw_gemm_kernel<BM={64 if blocks128 < 512 else 128},NT={nt}{',GATE' if gated else ''}>"


def test_the_mirror_of_pick_nt():
    want = {4: 1, 12: 1, 16: 1, 20: 2, 32: 2, 44: 3, 48: 3, 64: 4, 68: 5, 80: 5, 96: 6, 100: 7, 112: 7, 128: 8, 136: 3, 232: 5, 384: 8}
    assert {n: pick_nt(n) for n in want} == want
    assert kernel_name(65408, 128) == "pw_gemm_kernel<BM=64,NT=8,GATE>" and kernel_name(65409, 128) == "pw_gemm_kernel<BM=128,NT=8,GATE>"
    assert kernel_name(21760, 136) == "pw_gemm_kernel<BM=64,NT=3,GATE>" and kernel_name(21761, 136) == "pw_gemm_kernel<BM=128,NT=3,GATE>"
    assert kernel_name(64, 20, gated=False) == "pw_gemm_kernel<BM=64,NT=2>"


def test_the_cases_reach_all_sixteen_instantiations_and_every_edge():
    assert {kernel_name(n * P, N) for n, P, K, N, _ in CASES} == ALL_NAMES
    assert {kernel_name(n * P, N) for n, P, K, N, _ in SMALL} == {n for n in ALL_NAMES if "BM=64" in n}
    assert {kernel_name(n * P, N) for n, P, K, N, _ in BIG} == {n for n in ALL_NAMES if "BM=128" in n}
    assert {P for _, P, _, _, _ in SMALL} == {P for _, P, _, _, _ in BIG} == {1, 7, 50, 64, 1000}
    assert {4, 8, 36, 44, 100, 320, 1392} <= {K for _, _, K, _, _ in CASES}
    assert {4, 12, 20, 44, 100, 16, 32, 48, 64, 80, 96, 112, 128} <= {N for _, _, _, N, _ in CASES}
    assert any(N % 4 for _, _, _, N, _ in CASES)                                     # ld != N
    assert any(n * P < 64 for n, P, _, _, _ in CASES) and any((n * P) % 64 for n, P, _, _, _ in CASES)
    assert {r for *_, r in SMALL} == {r for *_, r in BIG} == {False, True}


# ---------------------------------------------------------------------------------------------------------------------------
# operands and the reference
# ---------------------------------------------------------------------------------------------------------------------------
def make_operands(seed, n_seg, P, K, N, residual):
    """D with channels of different scale (tests/test_gated_gemm_gpu._operands), gates uniform in (0, 1) times a scale of their
    segment's (neighbours 0.3 .. 1 apart by 0.35 at least), W of order 1 / sqrt(K), a bias of order 1, R on request."""
    rng = np.random.default_rng(seed)
    M = n_seg * P
    A = (rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (1, K))).astype(np.float32)
    scale = np.array([1.0, 0.3, 0.65])[np.arange(n_seg) % 3][:, None]
    gate = (rng.uniform(0.0, 1.0, (n_seg, K)) * scale).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    R = rng.standard_normal((M, N)).astype(np.float32) if residual else None
    return A, gate, W, bias, R


@functools.lru_cache(maxsize=3)
def reference(case):
    """(A, gate, W, bias, R, pre, bound) of a case: computed once, shared by the tests that need it, never written to."""
    n_seg, P, K, N, residual = case
    A, gate, W, bias, R = make_operands(K * 131 + N + 7 * P + n_seg, n_seg, P, K, N, residual)
    out = (A, gate, W, bias, R, O.gated64(A, gate, W, bias, None, P), O.gated_bound64(A, gate, W, bias, P))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def tau(K):
    return TL._tau(0, K) + TAU_GATE


def check(got, name, pre, bound, R, act, K, what):
    """tests/test_layer_gemm_gpu.py's _check at terms 0 with the gate's rounding added to tau; returns the worst share of the GEMM
    part of the tolerance, max (err - eps_act) / (tau (1.2 bound + |R|))."""
    worst = dict(TL.WORST)
    try:
        TL._check(got, name, pre, bound, R, act, 0, K, what, tau_extra=TAU_GATE)
    finally:
        TL.WORST.clear(); TL.WORST.update(worst)       # (that module's table of its own kernels' shares stays its own)
    r = 0.0 if R is None else np.abs(R.astype(np.float64))
    ref = O.act64(pre, act) + (0.0 if R is None else R.astype(np.float64))
    err = np.maximum(np.abs(got.astype(np.float64) - ref) - TL._eps_act(pre, act), 0.0)
    return float(np.max(err / (tau(K) * (1.2 * bound + r))))


def test_the_reference_matches_torch():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(4)
    for n_seg, P, K, N in ((3, 5, 12, 7), (1, 9, 4, 3), (6, 1, 20, 5)):
        A, W, b = rng.standard_normal((n_seg * P, K)), rng.standard_normal((K, N)), rng.standard_normal(N)
        g, R = rng.uniform(0, 1, (n_seg, K)), rng.standard_normal((n_seg * P, N))
        t = torch.from_numpy
        Ag = t(A) * t(g).repeat_interleave(P, dim=0)
        want = torch.addmm(t(b), Ag, t(W))
        np.testing.assert_allclose(O.gated64(A, g, W, b, None, P), want.numpy(), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(O.gated64(A, g, W, b, R, P), (want + t(R)).numpy(), rtol=1e-13, atol=1e-13)
        wantb = torch.addmm(t(np.abs(b)), Ag.abs(), t(W).abs())
        np.testing.assert_allclose(O.gated_bound64(A, g, W, b, P), wantb.numpy(), rtol=1e-13, atol=1e-13)
    # float32 operands are widened, not rounded again; by hand: one row, two channels
    assert O.gated64(np.float32([[3, 5]]), np.float32([[0.5, 0.25]]), np.float32([[2], [4]]), np.float32([1]), None, 1)[0, 0] == 3 + 5 + 1
    assert O.gated_bound64(np.float32([[-3, 5]]), np.float32([[0.5, 0.25]]), np.float32([[2], [-4]]), np.float32([-1]), 1)[0, 0] == 3 + 5 + 1


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_inputs_can_tell_gate_rows_and_columns_apart(case):
    n_seg, P, K, N, _ = case
    A, gate, W, bias, R, pre, bound = reference(case)
    assert (gate > 0).all() and (gate < 1).all()
    assert (np.ptp(gate, axis=1) > 0).all()                                    # no gate row is constant ...
    assert (np.abs(np.diff(gate, axis=1)) > 0).all()                           # ... and neighbours along k differ
    if K > 4:
        assert (gate[:, 4:] != gate[:, :-4]).all()
    if n_seg > 1:
        assert (gate[1:] != gate[:-1]).all()                                   # neighbouring segments differ, every k
    tail = K - (K - 1) // 32 * 32
    assert (A[:, K - tail:] != 0).all() and (W[K - tail:] != 0).all()          # D (and W) non-zero in the K tail


# ---------------------------------------------------------------------------------------------------------------------------
# the emulation and its mutants
# ---------------------------------------------------------------------------------------------------------------------------
def k_order(K):
    """the order in which pw_gemm_kernel adds an element's products: chunk c, group g, MFMA step cc, lane quad q"""
    order = [32 * c + 16 * g + 4 * q + cc for c in range(-(-K // 32)) for g in range(2) for cc in range(4) for q in range(4)]
    order = [k for k in order if k < K]           # (past K both operands are zero in LDS: the sum does not move)
    assert sorted(order) == list(range(K))
    return order


MUTANTS = {
    "a": "the gate row of the tile's first row for the whole 64-row tile",
    "b": "(m + 1) // rows_per_seg",
    "c": "no gate in the last, partial K chunk",
    "d": "the gate column shifted by 4",
    "e": "the gate row clamped to segment 0 past the first tile",
    "f": "the gate applied twice",
}


def emulate(A, gate, W, bias, R, P, mutant=None):
    f = np.float32
    M, K = A.shape
    m = np.arange(M)
    seg = np.minimum(m, M - 1) // P
    if mutant == "a":
        seg = np.minimum(m // 64 * 64, M - 1) // P
    elif mutant == "b":
        seg = np.minimum((m + 1) // P, gate.shape[0] - 1)
    elif mutant == "e":
        seg = np.where(m >= 64, 0, seg)
    g = gate[seg]
    if mutant == "d":
        g = np.roll(g, -4, axis=1)
    ag = A * g                                    # float32 x float32: rounded once
    assert ag.dtype == f
    if mutant == "c" and K % 32:
        ag[:, K // 32 * 32:] = A[:, K // 32 * 32:]
    if mutant == "f":
        ag = ag * g
    acc = np.zeros((M, W.shape[1]), f)
    for k in k_order(K):
        acc += ag[:, k:k + 1] * W[k]              # the product and the sum each rounded to f32
    out = acc + bias
    if R is not None:
        out = out + R
    assert out.dtype == f
    return out


SHARES = {}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_emulation_meets_the_inequality(case):
    n_seg, P, K, N, _ = case
    A, gate, W, bias, R, pre, bound = reference(case)
    name = kernel_name(n_seg * P, N)
    SHARES[case] = share = check(emulate(A, gate, W, bias, R, P), name, pre, bound, R, O.ACT_NONE, K, "emulation " + case_id(case))
    print(f"emulation {case_id(case)} {name}: worst share of tau {share:.3f}")
    assert share <= 1.0


def _fails(case, mutant):
    n_seg, P, K, N, _ = case
    A, gate, W, bias, R, pre, bound = reference(case)
    try:
        check(emulate(A, gate, W, bias, R, P, mutant), kernel_name(n_seg * P, N), pre, bound, R, O.ACT_NONE, K, f"mutant {mutant}")
    except pytest.fail.Exception:
        return True
    return False


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_misses_the_inequality_somewhere(mutant):
    caught = [case_id(c) for c in SMALL if _fails(c, mutant)]
    print(f"mutant ({mutant}) {MUTANTS[mutant]}: caught on {len(caught)} of {len(SMALL)} BM = 64 cases: {', '.join(caught)}")
    assert caught, MUTANTS[mutant]
    big = {"a": BIG[1], "b": BIG[0], "c": BIG[5], "d": BIG[2], "e": BIG[4], "f": BIG[3]}[mutant]     # and on a BM = 128 case
    assert _fails(big, mutant), (mutant, case_id(big))


def test_a_mutant_is_a_mistake_of_order_one():
    """The mutants are caught by a wide margin, not by the last bit: on a straddling case (a) is off by more than a thousand tau."""
    case = SMALL[3]
    n_seg, P, K, N, _ = case
    A, gate, W, bias, R, pre, bound = reference(case)
    r = np.abs(R.astype(np.float64))
    err = np.abs(emulate(A, gate, W, bias, R, P, "a").astype(np.float64) - (pre + R))
    assert np.max(err / (tau(K) * (1.2 * bound + r))) > 1e3
    assert math.isclose(tau(1024), 4e-7 + 2.0 ** -24) and math.isclose(tau(4096), 8e-7 + 2.0 ** -24)
