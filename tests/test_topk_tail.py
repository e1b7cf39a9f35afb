"""The tail of `topk_kernel` restated in float64: BSG calibration (+ SDM prior), the range filter, the species list.

After the selection passes (tests/test_topk.py) thread 0 of `topk_kernel` (birda_amd/csrc/kernels_conv.hip) works on the kept
predictions: `tail64` states that stage once more, in float64, from the FLOAT32 confidences the stage receives (what the same
classifier returns with no table set).  The order of the stage:

  1. BSG: p0 = clamp(conf), lg = log(p0 / (1 - p0)), q = sigmoid(intercept[c] + slope[c] * lg), then q * prior[c] when a prior is
     set, then a STABLE descending re-sort.  The clamp bounds are the float32 numbers float32(1e-7) and float32(1) -
     float32(1e-7) = 1 - 2^-23; everything else is float64.  [EXT] The crate that owns BsgPostProcessor is not among the
     reference's sources: this form is the project's restatement (kernels.hpp says so beside TopkFilter).
  2. a range table, when one is set (geomodel_filter.rs:39-43):

         |                  | score >= threshold | score < threshold | no entry (NaN)             |
         | rerank off, keep | keep               | drop              | keep, confidence untouched |
         | rerank off, drop | keep               | drop              | drop                       |
         | rerank on        | keep, conf * score | drop              | drop                       |

     then, when reranking, a stable descending re-sort.  The reference sorts with `sort_unstable_by(total_cmp)`: any order of
     equal confidences is a permitted outcome of it, the stable one among them (for +0.0 / -0.0, which total_cmp tells apart and
     a comparison does not, only where all zeros carry one sign: true of every sigmoid / softmax row here).
  3. ELSE the species list (classifier.rs:591-642 is an `else if`: with a range table set the list is ignored).

Saturation.  A calibrated value within 2^-26 of 1 is returned as exactly 1.0 and one below 2^-160 as exactly 0.0: for those the
f32 arithmetic gives exactly 1.0f / 0.0f (1 + e rounds to 1 for e < 2^-24; expf overflows to inf beyond 88.8), so they are TIES
on the device and must be ties in the restatement for the order to be the restatement's.

The confidence bound, derived (u = 2^-24, the f32 unit roundoff; every f32 operation rounds once, relative u):

  * p0 is exact (a clamp).  1 - p0 is exact for p0 >= 0.5 (Sterbenz) and rounds once below; the division rounds once: the
    argument of logf is off by <= 2u relative, which is 2u ABSOLUTE in lg.
  * logf and expf are held to 2 ulp, the figure tests/test_topk.py derives its sigmoid and softmax tolerances from; an ulp is at
    most 2^-23 relative, so 4u each.  |d lg| <= 2u + 4u |lg|.
  * t = a + b * lg, one multiply-add: as an fma one rounding, as two operations two; u |b lg| + u |t| <= u (|a| + 2 |b lg|),
    plus |b| |d lg|.  Together  darg = u (|a| + 6 |b lg| + 2 |b|) <= u (|a| + 8 |b| max(|lg|, 1))  -- the issue's
    u (|a| + c' |b lg|) with c' = 8 and |lg| held to at least 1 (the 2u |b| of the division does not shrink with lg).
  * e = expf(-t): relative darg (carried) + 4u.  q = 1 / (1 + e) has dq = q (1 - q) de / e; the add and the reciprocal round
    once each, the prior multiply once more: |dq| <= q (1 - q) darg exp(darg) + (4 (1 - q) + 3) u q <= q (1 - q) darg' + 7 u q
    (exp(darg): q (1 - q) is taken at the reference argument, the device's lies within darg of it).
  * with a prior: prior * (that) + u |ref|.  A rerank product is one f32 multiply: score * (bound so far) + u |ref|.
  * 2^-126 is added wherever a bound is not zero: below the normal range an f32 result is only good to its subnormal spacing
    (or flushed).
  * exact, bound 0: a saturated q (above), a prior or a score of 0, a score of +inf, an exact confidence times a score that is
    a power of two (1.0 among them; the product a normal number), and every confidence that neither BSG nor
    rerank touched (bit-equal to the unfiltered run's).

Order is decided by the restatement alone: `undecided` lists every pair of adjacent re-sorted values that is neither exactly
equal (a prior of 0, saturated values, equal tables on equal inputs, equal products of powers of two: equal by construction, on
the device too) nor further apart than four times the larger of their two bounds.  This module asserts over the whole table that
there is none (with the confidences as float32 of float64, and shifted four ulps either way); tests/test_topk_tail_gpu.py asserts
it again on the confidences the device produced.  No row is left out.

0 * inf: a zero confidence under a +inf score would be NaN, whose place the reference's total_cmp and a comparison sort disagree
on.  A geomodel ends in a sigmoid and cannot produce +inf; the table keeps its +inf scores (classes 5 mod 23) off prior zeros and
off the softmax rows' -inf classes, and `tail64` refuses a NaN.
"""
import functools
import json
import math
import os
from collections import namedtuple

import numpy as np
import pytest

import test_topk as T
from conftest import GOLDEN

U = 2.0 ** -24
FLOOR = 2.0 ** -126
LO32, HI32 = np.float32(1e-7), np.float32(1.0) - np.float32(1e-7)
LO, HI = float(LO32), float(HI32)
ULPS = 2                      # logf / expf, as tests/test_topk.py takes expf
C_FN = 2 * ULPS               # ... in units of u (an ulp is at most 2^-23 relative)
C_ARG = 2 + C_FN + 2          # the multiply-add, logf, the division carried through the log
C_OUT = C_FN + 3              # expf, the add, the reciprocal, the prior multiply
SAT_ONE, SAT_ZERO = 1.0 - 2.0 ** -26, 2.0 ** -160

Bsg = namedtuple("Bsg", "a b prior", defaults=(None,))
Range = namedtuple("Range", "scores threshold keep rerank")
Tail = namedtuple("Tail", "idx conf bound sorts")      # sorts: [(values, bounds)] of every re-sort, in sorted order


def calibrate64(c32, a, b):
    """-> (q, bound) of one confidence (prior not applied)"""
    p0 = min(max(float(c32), LO), HI)
    lg = math.log(p0 / (1.0 - p0))
    t = a + b * lg
    if -t > 700.0:
        return 0.0, 0.0
    e = math.exp(-t)
    q = 1.0 / (1.0 + e)
    if q >= SAT_ONE:
        return 1.0, 0.0
    if q <= SAT_ZERO:
        return 0.0, 0.0
    darg = U * (abs(a) + C_ARG * abs(b) * max(abs(lg), 1.0))
    return q, e / ((1.0 + e) * (1.0 + e)) * darg * math.exp(darg) + C_OUT * U * q + FLOOR


def _resort(idx, v, bd, sorts):
    order = sorted(range(len(v)), key=lambda i: -v[i])          # sorted() is stable; -0.0 and 0.0 are one key
    idx, v, bd = [idx[i] for i in order], [v[i] for i in order], [bd[i] for i in order]
    sorts.append((list(v), list(bd)))
    return idx, v, bd


def tail_trace(idx, conf32, n_classes, bsg=None, rng=None, species=None):
    idx = [int(i) for i in idx]
    c32 = np.asarray(conf32, np.float32)
    assert len(idx) == c32.size and all(0 <= i < n_classes for i in idx) and not np.isnan(c32).any()
    v, bd, sorts = [float(x) for x in c32], [0.0] * len(idx), []
    if bsg is not None:
        assert len(bsg.a) == len(bsg.b) == n_classes and (bsg.prior is None or len(bsg.prior) == n_classes)
        for k, c in enumerate(idx):
            q, bq = calibrate64(c32[k], float(np.float32(bsg.a[c])), float(np.float32(bsg.b[c])))
            if bsg.prior is not None:
                pr = float(np.float32(bsg.prior[c]))
                ref = q * pr
                bq = pr * bq + U * abs(ref) + FLOOR if bq > 0.0 and pr != 0.0 else 0.0
                q = ref
            v[k], bd[k] = q, bq
        idx, v, bd = _resort(idx, v, bd, sorts)
    if rng is not None:
        sc_all, thr = np.asarray(rng.scores, np.float32), np.float32(rng.threshold)
        assert sc_all.size == n_classes
        keeps = bool(rng.keep) and not rng.rerank
        oi, ov, ob = [], [], []
        for c, x, b in zip(idx, v, bd):
            sc = sc_all[c]
            if np.isnan(sc):
                if keeps:
                    oi.append(c); ov.append(x); ob.append(b)
            elif sc >= thr:
                if rng.rerank:
                    s = float(sc)
                    assert not (math.isinf(s) and x == 0.0) and not (s == 0.0 and math.isinf(x)), "0 * inf"
                    ref = x * s
                    exact = math.isinf(s) or s == 0.0 or x == 0.0 or (b == 0.0 and math.frexp(s)[0] == 0.5 and abs(ref) >= FLOOR)
                    oi.append(c); ov.append(ref); ob.append(0.0 if exact else s * b + U * abs(ref) + FLOOR)
                else:
                    oi.append(c); ov.append(x); ob.append(b)
        idx, v, bd = oi, ov, ob
        if rng.rerank:
            idx, v, bd = _resort(idx, v, bd, sorts)
    elif species is not None:
        keep = np.asarray(species)
        assert keep.size == n_classes
        sel = [k for k, c in enumerate(idx) if keep[c]]
        idx, v, bd = [idx[k] for k in sel], [v[k] for k in sel], [bd[k] for k in sel]
    assert not any(math.isnan(x) for x in v)
    return Tail(idx, np.asarray(v, np.float64), np.asarray(bd, np.float64), sorts)


def tail64(idx, conf32, n_classes, bsg=None, rng=None, species=None):
    """-> (indices, float64 confidences) of one row's kept predictions after the tail"""
    t = tail_trace(idx, conf32, n_classes, bsg, rng, species)
    return t.idx, t.conf


def undecided(trace):
    """Adjacent re-sorted values that neither are equal nor lie four bounds apart"""
    bad = []
    for vals, bds in trace.sorts:
        for i in range(len(vals) - 1):
            x, y = vals[i], vals[i + 1]
            if x != y and not (x - y > 4.0 * max(bds[i], bds[i + 1])):
                bad.append((i, x, y, bds[i], bds[i + 1]))
    return bad


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------
CLASS_COUNTS = (257, 2049)
TOP_KS = (1, 5, 32)
ACTS = (T.SIGMOID, T.SOFTMAX, T.NONE)
CASES = [(n, a) for n in CLASS_COUNTS for a in ACTS]
POS = (14.0, 15.0, 15.9, 16.0, 17.0, 20.0)               # below, at and past both clamps
NEG = tuple(-x for x in POS)
MIN_CONF = {T.SIGMOID: 0.0, T.SOFTMAX: 0.0, T.NONE: -1e30}   # nothing is cut (NONE: the confidence is the logit, negative ones too)
SOFTMAX_FLOOR = -30.0                                     # a softmax row's +inf-score classes where the rest is -inf

Row = namedtuple("Row", "name logits")
Stage = namedtuple("Stage", "name bsg rng species", defaults=(None, None, None))


def inf_classes(n):
    return np.arange(5, n, 23)


def _makers(n, act):
    """name -> make(rng): the rows, each a function of its draw (where the planted values sit, what fills the rest)"""
    def rest_row(values):
        """values planted, the rest out of the running: NaN (never chosen), under softmax -inf (confidence 0; one NaN would
        make every confidence NaN) with the +inf-score classes at a finite floor"""
        def make(rng):
            x = T._planted(n, rng, list(values), lambda m: np.full(m, -np.inf if act == T.SOFTMAX else np.nan, np.float32))
            if act == T.SOFTMAX:
                at = inf_classes(n)
                x[at[np.isneginf(x[at])]] = SOFTMAX_FLOOR
            return x
        return make

    def low(rng, m):                       # distinct logits around -6: under every table far below the planted ones
        return T._distinct(rng, m, 0.3) - np.float32(6.0)

    def unit(rng):                         # forty mid-range values (NONE: confidences inside (0, 1)), the rest far below
        x = np.full(n, -12.0, np.float32)
        x[rng.permutation(n)[:40]] = (0.6 + 0.25 * rng.random(40)).astype(np.float32)
        return x

    def plateau(rng):
        x = np.full(n, -2.0, np.float32)
        pos = rng.permutation(n)
        x[pos[:3]] = (3.0, 2.5, 2.0)
        x[pos[3:43]] = 1.5                 # a tied plateau wider than top_k
        return x

    def pow2(rng):
        x = np.full(n, -1.0, np.float32)
        x[[7, 100, 2]] = (0.5, 0.25, 0.25)  # NONE: products of powers of two
        return x

    def dominant(rng):
        x = low(rng, n)
        x[n // 2] = 40.0                   # confidence exactly 1.0 under sigmoid AND softmax
        return x

    return [("planted_pos", lambda rng: T._planted(n, rng, list(POS), lambda m: low(rng, m))),
            ("planted_all", rest_row(POS + NEG)), ("planted_neg", rest_row(NEG)),
            ("distinct", lambda rng: T._distinct(rng, n, 3.0)),              # a full top-32 of distinct logits
            ("unit", unit), ("plateau", plateau),
            ("few", rest_row((0.0, 2.0, 1.0))),                              # fewer finite classes than top_k
            ("pow2", pow2), ("dominant", dominant)]


def shifted(c32, act):
    """The confidences, and (sigmoid / softmax) the same four ulps up and four down"""
    if act == T.NONE:
        return [c32]
    up = down = c32
    for _ in range(4):
        up, down = np.nextafter(up, np.float32(2.0)), np.nextafter(down, np.float32(-1.0))
    zero = c32 == 0                       # (expf(-inf): exactly 0 on the device too)
    return [c32, np.where(zero, c32, np.minimum(up, np.float32(1.0))), np.where(zero, c32, np.maximum(down, np.float32(0.0)))]


def row_problems(n, act, logits):
    """(top_k, stage, shift, pairs) wherever the order of one row is not the restatement's alone"""
    bad = []
    for top_k in TOP_KS:
        idx, c32 = kept32(logits, act, top_k)
        for k, c in enumerate(shifted(c32, act)):
            for st in stages(n):
                try:
                    und = undecided(tail_trace(idx, c, n, st.bsg, st.rng, st.species))
                except AssertionError as e:
                    und = [str(e)]
                if und:
                    bad.append((top_k, st.name, k, und))
    return bad


@functools.lru_cache(maxsize=None)
def rows(n, act):
    """The logit rows of one (class count, activation): one batch for the kernel, whatever the top_k and the tables.  Each row
    is drawn (seed, seed + 1, ...) until its order under every table is decided (test_order_is_decided_over_the_whole_table
    holds the result to that, none left out)."""
    R = []
    for j, (name, make) in enumerate(_makers(n, act)):
        for s in range(40):
            x = make(np.random.default_rng(7000 + 10 * n + act + 100000 * j + 1000000 * s))
            if not row_problems(n, act, x):
                break
        R.append(Row(name, x))               # (a row that never settled is still a row: the test below fails on it)
    return R


def _prior01(n, rng):
    pr = rng.random(n).astype(np.float32)
    cat = rng.integers(0, 10, n)
    pr[cat < 3] = 0.0
    pr[cat == 3] = 1.0
    at = inf_classes(n)
    pr[at] = np.float32(0.25) + np.float32(0.5) * rng.random(at.size).astype(np.float32)     # never 0 under a +inf score
    return pr


def score_table(n, thr, rng):
    """NaN (no entry), 0, exactly the threshold, just below it, 1, +inf, and ordinary scores"""
    s = (np.float32(0.02) + np.float32(0.96) * rng.random(n)).astype(np.float32)
    cat = rng.integers(0, 20, n)
    t = np.float32(thr)
    s[cat < 3] = np.nan
    s[(cat == 3) | (cat == 4)] = 0.0
    s[(cat >= 5) & (cat <= 7)] = t
    s[(cat == 8) | (cat == 9)] = np.nextafter(t, np.float32(-1.0))
    s[(cat == 10) | (cat == 11)] = 1.0
    s[inf_classes(n)] = np.inf
    return s


@functools.lru_cache(maxsize=None)
def stages(n):
    """Every table setting of one class count"""
    rng = np.random.default_rng(9000 + n)
    f32 = lambda a: np.asarray(a, np.float32)
    a_rand, b_rand = f32(rng.normal(0.0, 1.0, n)), f32(rng.uniform(0.1, 0.4, n))        # (a logit of 16 stays mid-range)
    a_conf = f32(-16.0 + rng.normal(0.0, 0.5, n))                             # a confident detection lands mid-range
    pr_rand = f32(0.05 + 0.9 * rng.random(n))
    pr_01 = _prior01(n, rng)
    two = f32(np.where(np.arange(n) % 3 == 0, 1.0, -0.5))
    zeros, ones = np.zeros(n, np.float32), np.ones(n, np.float32)
    S = [Stage("bsg_slope0", Bsg(two, zeros)),                                 # everything collapses to sigmoid(a): ties keep the order
         Stage("bsg_negative_slope", Bsg(f32(np.full(n, -16.0)), -ones)),       # the order reverses (a logit of -16 mid-range)
         Stage("bsg_slope50", Bsg(zeros, f32(np.full(n, 50.0)))),              # saturates to exact 0 / 1
         Stage("bsg_random", Bsg(a_rand, b_rand)),
         Stage("bsg_random_prior", Bsg(a_rand, b_rand, pr_rand)),
         Stage("bsg_random_prior01", Bsg(a_rand, b_rand, pr_01)),
         Stage("bsg_confident", Bsg(a_conf, ones)),
         Stage("bsg_slope0_prior01", Bsg(two, zeros, pr_01))]
    tables = {thr: score_table(n, thr, rng) for thr in (0.0, 0.01, 1.0)}
    for thr, sc in tables.items():
        for keep in (True, False):
            for rerank in (False, True):
                S.append(Stage(f"range_{thr}_{'keep' if keep else 'drop'}{'_rerank' if rerank else ''}", rng=Range(sc, thr, keep, rerank)))
    S.append(Stage("range_all_out", rng=Range(np.full(n, 0.001, np.float32), 0.01, False, False)))      # everything is dropped
    S.append(Stage("range_rerank_all_zero", rng=Range(zeros, 0.0, True, True)))                        # every product 0: the order stays
    alt = (np.arange(n) % 2).astype(np.uint8)
    S += [Stage("species_all", species=np.ones(n, np.uint8)), Stage("species_none", species=np.zeros(n, np.uint8)),
          Stage("species_alternating", species=alt),
          Stage("species_and_range", rng=Range(tables[0.01], 0.01, True, False), species=alt),          # the list is ignored
          Stage("bsg_then_species", Bsg(a_rand, b_rand, pr_01), species=alt),
          Stage("bsg_then_range_keep", Bsg(a_rand, b_rand, pr_01), Range(tables[0.01], 0.01, True, False)),
          Stage("bsg_then_range_rerank", Bsg(a_rand, b_rand, pr_rand), Range(tables[0.01], 0.01, True, True)),
          Stage("bsg_confident_then_rerank", Bsg(a_conf, ones, pr_01), Range(tables[0.0], 0.0, False, True))]
    return S


def stage_kind(st):
    return "+".join(k for k, on in (("bsg", st.bsg is not None), ("prior", st.bsg is not None and st.bsg.prior is not None),
                                    ("rerank", st.rng is not None and st.rng.rerank), ("range", st.rng is not None and not st.rng.rerank),
                                    ("species", st.rng is None and st.species is not None)) if on)


def kept32(logits, act, top_k):
    """What the selection hands the tail at MIN_CONF: indices, and the confidences as float32 of float64"""
    idx, p = T.topk64(logits, act, top_k, MIN_CONF[act])
    return idx.tolist(), p.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------
def test_the_restatement_reproduces_the_references_own_cases():
    """Every geomodel_filter.rs case of tests/golden/reference_unit_cases.json (threshold 0.01 as there): species and order as
    the reference asserts, confidences to its own 1e-6 and, where rerank is off, bit for bit.  (The reference sorts unstably
    with total_cmp; a stable sort is one of its permitted outcomes, and its cases hold no ties.)"""
    from test_oracle_golden import filter_case_tables
    with open(os.path.join(GOLDEN, "reference_unit_cases.json")) as f:
        cases = json.load(f)["filter_predictions"]
    assert len(cases) == 11
    for c in cases:
        species, index, scores, idx, conf = filter_case_tables(c)
        oi, oc = tail64(idx, conf, scores.size, rng=Range(scores, 0.01, c["policy"] == "keep", c["rerank"]))
        assert [species[i] for i in oi] == [s for s, _ in c["out"]], c["src"]
        assert np.allclose(oc, [p for _, p in c["out"]], atol=1e-6), c["src"]
        if not c["rerank"]:
            assert np.array_equal(oc.astype(np.float32), [np.float32(p) for _, p in c["out"]]), c["src"]


def test_the_clamp_is_the_float32_one_in_the_restatement_and_in_the_oracle(oracle_lib):
    """1.0f - 1e-7f is 1 - 2^-23: logit 15.942.  Intercept -16, slope 1 on a saturated confidence gives 0.486 (a float64 clamp
    at 1 - 1e-7: 0.529), in `tail64` and in oracle.bsg_postprocess alike; on unsaturated inputs the two agree to 1e-12."""
    assert HI == 1.0 - 2.0 ** -23 and abs(math.log(HI / (1.0 - HI)) - 15.942) < 1e-3
    a, b = np.full(4, -16.0, np.float32), np.ones(4, np.float32)
    for c in (1.0, float(HI32), 20.0):
        _, q = tail64([2], [c], 4, bsg=Bsg(a, b))
        _, qo = oracle_lib.bsg_postprocess(np.array([2]), [np.float32(c)], a, b)
        assert abs(q[0] - 0.4856) < 1e-4 and abs(qo[0] - q[0]) < 1e-12, (c, q, qo)
    _, q = tail64([1], [0.0], 4, bsg=Bsg(-a, b))
    _, qo = oracle_lib.bsg_postprocess(np.array([1]), [np.float32(0.0)], -a, b)
    assert abs(q[0] - 1.0 / (1.0 + math.exp(-(16.0 + math.log(LO / (1.0 - LO)))))) < 1e-15 and abs(qo[0] - q[0]) < 1e-12
    rng = np.random.default_rng(3)
    n = 500
    A, B, P = rng.normal(0, 1, n).astype(np.float32), rng.uniform(0.5, 2, n).astype(np.float32), rng.random(n).astype(np.float32)
    for prior in (None, P):
        for _ in range(20):
            idx = rng.permutation(n)[:32]
            conf = np.sort(rng.uniform(1e-4, 1.0 - 1e-4, 32).astype(np.float32))[::-1]
            wi, wc = oracle_lib.bsg_postprocess(idx, conf, A, B, prior)
            gi, gc = tail64(idx, conf, n, bsg=Bsg(A, B, prior))
            assert gi == wi and np.abs(gc - np.asarray(wc)).max() <= 1e-12


def test_saturated_values_are_exact_ties():
    a, b = np.zeros(8, np.float32), np.full(8, 50.0, np.float32)
    t = tail_trace([3, 1, 6, 2], np.asarray([0.9, 0.8, 0.01, 0.001], np.float32), 8, bsg=Bsg(a, b))
    assert t.idx == [3, 1, 6, 2] and t.conf.tolist() == [1.0, 1.0, 0.0, 0.0] and not t.bound.any() and not undecided(t)
    # one value just short of the saturation beside a saturated one: not decided, and `undecided` says so
    b[1] = 17.0 / math.log(0.8 / 0.2)
    t = tail_trace([3, 1], np.asarray([0.9, 0.8], np.float32), 8, bsg=Bsg(a, b))
    assert t.conf[0] == 1.0 and 0.0 < 1.0 - t.conf[1] < 1e-7 and len(undecided(t)) == 1


def test_hand_made_rows():
    nan, inf = np.nan, np.inf
    sc = np.asarray([0.5, nan, 0.01, np.nextafter(np.float32(0.01), np.float32(0)), 1.0, inf, 0.0], np.float32)
    idx, conf = [0, 1, 2, 3, 4, 5, 6], np.asarray([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3], np.float32)
    f = lambda keep, rerank: tail64(idx, conf, 7, rng=Range(sc, 0.01, keep, rerank))
    assert f(True, False)[0] == [0, 1, 2, 4, 5] and f(False, False)[0] == [0, 2, 4, 5]
    assert f(True, True)[0] == f(False, True)[0] == [5, 4, 0, 2]                 # inf, 0.5, 0.45, 0.007: NaN dropped whatever the policy
    assert f(True, False)[1].astype(np.float32).tolist() == conf[[0, 1, 2, 4, 5]].tolist()
    # a range table AND a list: the list is ignored
    assert tail64(idx, conf, 7, rng=Range(sc, 0.01, True, False), species=np.zeros(7))[0] == [0, 1, 2, 4, 5]
    assert tail64(idx, conf, 7, species=[1, 0, 1, 0, 1, 0, 1])[0] == [0, 2, 4, 6]
    # BSG comes first: a negative slope reverses the order, the prior's zero then sinks to the end, the filter sees THAT order
    b = Bsg(np.zeros(7, np.float32), -np.ones(7, np.float32), np.asarray([1, 1, 1, 1, 1, 1, 0], np.float32))
    assert tail64(idx, conf, 7, bsg=b)[0] == [5, 4, 3, 2, 1, 0, 6]
    assert tail64(idx, conf, 7, bsg=b, rng=Range(sc, 0.01, True, False))[0] == [5, 4, 2, 1, 0]
    with pytest.raises(AssertionError):
        tail64([5], [0.0], 7, rng=Range(sc, 0.01, True, True))                   # 0 * inf


@pytest.mark.parametrize("n,act", CASES)
def test_order_is_decided_over_the_whole_table(n, act):
    """Every row x every table setting x every top_k: no adjacent pair of re-sorted reference values is undecided -- with the
    confidences as float32 of float64 and shifted four ulps up and down (the device's sigmoid / softmax is within that of
    them; the GPU test repeats the check on what the device really produced).  The rows named in the issue are all there."""
    R, S = rows(n, act), stages(n)
    assert [r.name for r in R] == ["planted_pos", "planted_all", "planted_neg", "distinct", "unit", "plateau", "few", "pow2", "dominant"]
    assert len(S) == 30 and len({s.name for s in S}) == 30
    checked = reordered = dropped_all = zero_ties = 0
    for top_k in TOP_KS:
        for r in R:
            idx, c32 = kept32(r.logits, act, top_k)
            assert len(idx) == min(top_k, int((~np.isnan(r.logits)).sum())), r.name
            for st in S:
                for k, c in enumerate(shifted(c32, act)):
                    t = tail_trace(idx, c, n, st.bsg, st.rng, st.species)
                    assert not undecided(t), (r.name, st.name, top_k, k, undecided(t))
                    checked += 1
                    if k == 0:
                        reordered += st.rng is not None and st.rng.rerank and st.bsg is None and t.idx != [i for i in idx if i in t.idx]
                        dropped_all += st.rng is not None and len(idx) > 0 and not t.idx
                        zero_ties += st.name == "range_rerank_all_zero" and t.idx == idx and not t.conf.any()
    assert checked >= 3 * 9 * 30 and reordered >= 10 and dropped_all >= 27 and zero_ties >= 20, (checked, reordered, dropped_all, zero_ties)


def test_the_planted_rows_reach_both_clamps():
    for act in (T.SIGMOID, T.NONE):
        r = {x.name: x for x in rows(257, act)}
        idx, c32 = kept32(r["planted_all"].logits, act, 32)
        assert len(idx) == 12
        assert (c32 >= HI32).sum() >= 3 and (c32 <= LO32).sum() >= 2 and ((c32 > LO32) & (c32 < HI32)).sum() >= (4 if act == T.SIGMOID else 0)
    idx, c32 = kept32({x.name: x for x in rows(257, T.SOFTMAX)}["dominant"].logits, T.SOFTMAX, 5)
    assert c32[0] == 1.0 and (c32[1:] < LO32).all()


def test_constants_are_the_derived_ones():
    assert (C_ARG, C_OUT) == (8, 7) and ULPS == 2
    assert "2 ulp for expf" in open(T.__file__).read()            # (where the figure comes from)
