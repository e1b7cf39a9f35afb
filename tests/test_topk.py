"""The activation / top-k stage restated in float64, and the table of inputs the GPU test feeds the kernel.

`topk_kernel` (birda_amd/csrc/kernels_conv.hip) serves every prediction the library returns: output activation, ranking on
the logit with ties to the lower class index, the `min_confidence` cut, at most `top_k` predictions.  `topk64` below states
that stage once more in plain NumPy, in float64, by the rules of the oracle's `bo_topk`:

  * the f32 logits are cast to f64 and the activation is computed in f64;
  * a class whose logit or confidence is NaN is skipped (for softmax a single NaN or +inf logit makes EVERY confidence NaN);
  * the order is (logit descending, index ascending) -- +0.0 and -0.0 are equal;
  * the first confidence that is not >= min_confidence -- both as f32 -- ends the row;
  * at most min(top_k, n_classes) predictions.

This module (CPU) holds the restatement to `oracle.topk` on INDICES: over a grid of class counts / activations / top_k /
input families, and over every row of the table the GPU test uses (tests/test_topk_gpu.py imports `topk64`, the table and
the tolerances from here).  The C oracle is not the confidence reference: its softmax sums 32 768 f32 terms in sequence
(1.5e-4 relative from float64), which is why the restatement exists.

Expected rows never depend on rounding: `margin_ok` keeps every confidence the cut looks at 1e-3 relative away from
min_confidence, except in the rows built to sit exactly ON it (`Row.exact`: the test is `>=`, the class is kept).

The module also holds the class-count ceiling (BH_MAX_CLASSES, include/birda_hip.h): a model above it is refused at create,
before any device is touched, so that test runs here too.
"""
import math
import os
import re
from collections import namedtuple

import numpy as np
import pytest

from conftest import ROOT

NONE, SIGMOID, SOFTMAX = 0, 1, 2           # bh_model_info.output_activation (modelfile.OUT_*)
ACTS = (NONE, SIGMOID, SOFTMAX)
BH_MAX_TOP_K = 32

# around BH_MAX_TOP_K, a wave, a block, the 8 x 256 staging chunk, the Perch width, 64 KB of LDS, and the ceiling
CLASS_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 14795, 16384, 16385, 32768)
ALL_ACT_COUNTS = (1, 33, 257, 2049, 16385, 32768)      # all three activations here, sigmoid alone at the rest
TOP_KS = (1, 5, 32)
# per activation a cut that some but not all classes of the rows below pass (and 0, which every non-NaN confidence of a
# sigmoid / softmax passes)
MIN_CONF = {NONE: 0.25, SIGMOID: 0.6, SOFTMAX: 0.02}
GPU_TABLE = [(n, a) for n in CLASS_COUNTS for a in ((SIGMOID, NONE, SOFTMAX) if n in ALL_ACT_COUNTS else (SIGMOID,))]
MARGIN = 1e-3

# Confidence tolerances against float64 (relative), derived:
#   NONE     no arithmetic: the confidence is the logit, bit for bit
#   sigmoid  1 / (1 + expf(-x)): 2 ulp for expf, one rounding each for the add and the divide = 4 * 2^-24, x 2 margin.
#            Logits >= -80 so that p stays a normal f32.
#   softmax  expf(x - mx) / sum over the row: the per-thread sequential sum of ceil(n / 256) terms, the 8-step tree (6 lane
#            shuffles + 2 over the waves), expf on the numerator and on the terms (2 ulp each, plus d = mx - x ulps of the
#            argument's own rounding carried through expf), the f32 subtractions and the divide: 8 + 16 in all beside the n- and
#            d-dependent terms.  d <= 30.
SIGMOID_RTOL = 2.0 ** -21
SIGMOID_MIN_LOGIT = -80.0
SOFTMAX_MAX_D = 30.0


def softmax_rtol(n, d):
    return (math.ceil(n / 256) + d + 24) * 2.0 ** -24


def conf64(logits, act):
    """Every class's confidence in float64 (NaN where the stage would skip it for its confidence)."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if act == SIGMOID:
            return 1.0 / (1.0 + np.exp(-x))
        if act == SOFTMAX:
            e = np.exp(x - np.max(x))          # (np.max hands a NaN on; inf - inf is NaN: one NaN / +inf logit and every p is NaN)
            return e / e.sum()
    return x.copy()


def ranked(logits, act):
    """The live classes (neither logit nor confidence NaN) by (logit descending, index ascending), and all confidences."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    p = conf64(logits, act)
    live = np.flatnonzero(~(np.isnan(x) | np.isnan(p)))
    return live[np.argsort(-x[live], kind="stable")], p      # stable: equal logits (+0.0 / -0.0 among them) keep index order


def topk64(logits, act, top_k, min_conf):
    """-> (indices int64 [k], confidences float64 [k]) of one row."""
    order, p = ranked(logits, act)
    mc = np.float32(min_conf)
    idx = []
    with np.errstate(all="ignore"):
        for i in order[:min(top_k, np.asarray(logits).size)]:
            if not (np.float32(p[i]) >= mc):
                break
            idx.append(int(i))
    return np.asarray(idx, np.int64), p[idx] if idx else np.zeros(0)


def margin_ok(logits, act, top_k, min_conf):
    """No confidence the cut looks at lies within MARGIN (relative) of min_conf.  (NONE: the confidence IS the f32 logit and
    the comparison is exact, nothing can round across the cut.)"""
    if act == NONE or min_conf <= 0:
        return True
    order, p = ranked(logits, act)
    seen = p[order[:top_k]]
    return bool(np.all(np.abs(seen - min_conf) >= MARGIN * min_conf))


# ---------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------
# conf: hold the confidences to float64 (False: saturating rows, order and count only); exact: a confidence equals min_conf on
# purpose; passes: how many classes pass the cut by construction (None: whatever the restatement says)
Row = namedtuple("Row", "name logits conf exact passes", defaults=(True, False, None))


def _distinct(rng, n, scale):
    x = (rng.standard_normal(n) * scale).astype(np.float32)
    while True:
        _, first = np.unique(x, return_index=True)
        if first.size == n:
            return x
        dup = np.setdiff1d(np.arange(n), first)
        x[dup] = (rng.standard_normal(dup.size) * scale).astype(np.float32)


def _settled(make, act, top_k, min_conf, seed):
    """make(rng) redrawn (seed, seed + 1, ...) until no confidence sits within the margin of the cut."""
    for s in range(seed, seed + 50):
        x = make(np.random.default_rng(s))
        if margin_ok(x, act, top_k, min_conf):
            return x
    raise AssertionError("no draw clear of the cut")


def _planted(n, rng, values, fill):
    """fill (a function of the count) everywhere, values[i] at scattered positions: rank order is not index order"""
    pos = rng.permutation(n)
    x = np.empty(n, np.float32)
    k = min(len(values), n)
    x[pos[:k]] = np.asarray(values[:k], np.float32)
    x[pos[k:]] = fill(n - k)
    return x


def ramp(n, act, min_conf, j, rng):
    """A strictly descending ramp (at scattered positions) in which exactly min(j, n) classes pass the cut; None when no such
    row exists (a sigmoid / softmax confidence is never below 0; a softmax row of <= 50 classes has one >= 0.02)."""
    i = np.arange(max(n, 1), dtype=np.float64)
    if act == NONE:
        hi, lo = min_conf + 1.0 + 0.5 * (j - i[:j]), lambda m: (min_conf - 1.0 - 0.001 * i[:m]).astype(np.float32)
    elif min_conf <= 0:
        return None
    elif act == SIGMOID:
        t = math.log(min_conf / (1.0 - min_conf))
        hi, lo = t + 1.0 + 0.25 * (j - i[:j]), lambda m: (t - 1.0 - 0.001 * i[:m]).astype(np.float32)
    else:
        if j == 0:          # a flat row: every confidence ~ 1 / n
            if n * min_conf * (1.0 - 2 * MARGIN) <= math.exp(0.0001 * n):
                return None
            return _planted(n, rng, [], lambda m: (-0.0001 * i[:m]).astype(np.float32))
        # j classes near 0 share the mass (each >= e^-0.31 / 32 = 0.023 > 0.02), the rest 25 below: 1e-11 each
        assert min_conf * (1.0 + 2 * MARGIN) < math.exp(-0.01 * j) / (j + 1e-6)
        hi, lo = -0.01 * i[:j], lambda m: (-25.0 - 0.0001 * i[:m]).astype(np.float32)
    return _planted(n, rng, list(hi), lo)


def family_rows(n, act, top_k, min_conf):
    """The rows of one (class count, activation, top_k, min_confidence) case: one batch for the kernel."""
    seed = 1000 * n + 10 * act
    R = []
    # a confidence exactly ON the cut is kept (the test is >=): NONE 0.25 at min_conf 0.25, sigmoid(+-0) = 0.5 at min_conf 0.5
    if (act, min_conf) in ((NONE, 0.25), (SIGMOID, 0.5)):
        on = 0.25 if act == NONE else 0.0
        x = (on - 3.0 - 0.001 * np.arange(n)).astype(np.float32)
        x[0] = on + 2.0
        x[n - 1] = on
        R.append(Row("on_the_cut", x, True, True, min(n, 2)))
        tied = np.full(n, on, np.float32)
        if act == SIGMOID:
            tied[1::2] = -0.0                  # sigmoid(-0.0) = sigmoid(+0.0) = 0.5: all on the cut, all equal, the index decides
        R.append(Row("on_the_cut_tied", tied, True, True, n))
    if (act, min_conf) == (SIGMOID, 0.5):      # (the classifier built for these rows alone: the families below hold more zeros)
        return R

    def settled(name, make, salt, conf=True):
        R.append(Row(name, _settled(make, act, top_k, min_conf, seed * 100 + salt * 50), conf))

    def with_values(base_scale, put):
        def make(rng):
            x = _distinct(rng, n, base_scale)
            put(x, rng)
            return x
        return make

    settled("distinct", lambda rng: _distinct(rng, n, 3.0), 0)
    settled("integers", lambda rng: np.round(rng.standard_normal(n) * 3.0).astype(np.float32), 1)       # many ties, some -0.0
    R.append(Row("one_value", np.full(n, 1.5, np.float32)))
    R.append(Row("zeros", np.where(np.random.default_rng(seed + 2).random(n) < 0.5, 0.0, -0.0).astype(np.float32)))

    def top_at(*where):
        def put(x, rng):
            x[[w for w in where if 0 <= w < n]] = x.max() + 2.0
        return put
    settled("max_first", with_values(1.0, top_at(0)), 3)
    settled("max_last", with_values(1.0, top_at(n - 1)), 4)              # a clamped duplicate of the tail must not count twice
    settled("max_last_two", with_values(1.0, top_at(n - 1, n - 2)), 5)

    def nan_some(x, rng):
        x[rng.random(n) < 0.3] = np.nan
    settled("nan_30", with_values(3.0, nan_some), 6)
    R.append(Row("nan_all", np.full(n, np.nan, np.float32)))
    settled("nan_first_32", with_values(3.0, lambda x, rng: x.__setitem__(slice(0, 32), np.nan)), 7)
    settled("nan_last_32", with_values(3.0, lambda x, rng: x.__setitem__(slice(max(n - 32, 0), n), np.nan)), 8)
    settled("pos_inf", with_values(3.0, lambda x, rng: x.__setitem__([n - 1, n // 2], np.inf)), 9)
    settled("neg_inf", with_values(3.0, lambda x, rng: x.__setitem__([0, n // 3, n - 1], -np.inf)), 10)
    three = {n - 1: 1.0, n // 2: 2.0, 0: 0.5}           # (fewer than three where positions coincide)
    for name, rest in (("three_finite_rest_nan", np.nan), ("three_finite_rest_neg_inf", -np.inf)):
        x = np.full(n, rest, np.float32)
        for pos, v in three.items():
            x[pos] = v
        assert margin_ok(x, act, top_k, min_conf)
        R.append(Row(name, x))
    settled("very_negative", lambda rng: (-70.0 - 9.0 * rng.random(n)).astype(np.float32), 11)
    settled("saturating", lambda rng: _distinct(rng, n, 30.0), 12, conf=False)
    for j in sorted({0, 1, top_k - 1, top_k}):
        x = ramp(n, act, min_conf, j, np.random.default_rng(seed + 20 + j))
        if x is not None:
            R.append(Row(f"ramp_{j}_pass", x, True, False, min(j, n)))
    return R


def configs(act):
    return [(k, mc) for k in TOP_KS for mc in (0.0, MIN_CONF[act])]


ON_THE_CUT_COUNTS = (33, 2049)


def exact_configs(n, act):
    """(top_k, min_confidence) of the classifier that exists for the sigmoid's on-the-cut rows (NONE has them at its own cut)"""
    return [(5, 0.5)] if act == SIGMOID and n in ON_THE_CUT_COUNTS else []


# ---------------------------------------------------------------------------------------------------------------
# the restatement against the C oracle
# ---------------------------------------------------------------------------------------------------------------
def _grid_rows(n, rng):
    x = (rng.standard_normal(n) * 3.0).astype(np.float32)
    nan30 = x.copy()
    nan30[rng.random(n) < 0.3] = np.nan
    return {"random": x, "integers": np.round(x), "all_equal": np.full(n, x[0], np.float32), "nan_30": nan30,
            "saturating": x * 30.0, "very_negative": (-60.0 - 20.0 * rng.random(n)).astype(np.float32)}


def test_restatement_gives_the_oracles_indices(oracle_lib):
    """Class counts 1 ... 32 768 x the three activations x top_k 1 / 5 / 32 x six input families, at min_confidence 0 and at
    the activation's cut (where the row keeps clear of it): the float64 restatement and bo_topk choose the same classes in the
    same order."""
    cases = mismatches = 0
    for n in CLASS_COUNTS + (3, 50, 1000, 6522):
        rows = _grid_rows(n, np.random.default_rng(n))
        for act in ACTS:
            for top_k in TOP_KS:
                for name, x in rows.items():
                    for mc in (0.0, MIN_CONF[act]):
                        if not margin_ok(x, act, top_k, mc) or (mc and n > 2049 and top_k != 5):   # (keeps the oracle's n x k scan short)
                            continue
                        want, _ = oracle_lib.topk(x, act, top_k, mc)
                        got, _ = topk64(x, act, top_k, mc)
                        cases += 1
                        if got.tolist() != want.tolist():
                            mismatches += 1
                            print(f"n {n} act {act} top_k {top_k} min_conf {mc} {name}: restatement {got.tolist()} oracle {want.tolist()}")
    assert cases >= 1500 and mismatches == 0, (cases, mismatches)


def test_restatement_on_hand_made_rows():
    nan, inf = np.nan, np.inf
    x = np.asarray([1.0, 3.0, 3.0, nan, 2.0, -0.0, 0.0], np.float32)
    assert topk64(x, SIGMOID, 5, 0.0)[0].tolist() == [1, 2, 4, 0, 5]                   # ties and +-0 by index, the NaN skipped
    assert topk64(x, NONE, 32, 0.0)[0].tolist() == [1, 2, 4, 0, 5, 6]                  # -0.0 >= 0
    assert topk64(x, NONE, 32, 2.0)[0].tolist() == [1, 2, 4] and topk64(x, NONE, 32, 2.5)[0].tolist() == [1, 2]
    assert topk64(x, SOFTMAX, 5, 0.0)[0].size == 0                                     # one NaN: no softmax confidence is a number
    assert topk64(np.asarray([0.0, inf, 1.0], np.float32), SOFTMAX, 3, 0.0)[0].size == 0
    i, p = topk64(np.asarray([0.0, inf, -inf, inf], np.float32), SIGMOID, 5, 0.0)
    assert i.tolist() == [1, 3, 0, 2] and p.tolist() == [1.0, 1.0, 0.5, 0.0]             # -inf is a class like any other: confidence 0
    assert topk64(np.asarray([0.0, -inf], np.float32), SIGMOID, 5, 0.5)[0].tolist() == [0]   # kept ON the cut
    i, p = topk64(np.asarray([-inf, 0.0, 0.0], np.float32), SOFTMAX, 5, 0.0)
    assert i.tolist() == [1, 2, 0] and p.tolist() == [0.5, 0.5, 0.0]
    assert topk64(np.full(4, nan, np.float32), NONE, 5, 0.0)[0].size == 0
    assert topk64(np.asarray([7.0], np.float32), SOFTMAX, 32, 0.5)[1].tolist() == [1.0]


@pytest.mark.parametrize("n,act", GPU_TABLE)
def test_gpu_rows_are_settled_and_the_oracle_agrees(oracle_lib, n, act):
    """Every row the GPU test submits: clear of the cut (or exactly on it, where that is the point), inside the range its
    confidence tolerance was derived for, passing the cut as often as it was built to -- and ranked by bo_topk as by the
    restatement."""
    names = set()
    for top_k, mc in configs(act) + exact_configs(n, act):
        for r in family_rows(n, act, top_k, mc):
            names.add(re.sub(r"\d+", "#", r.name))
            assert r.logits.dtype == np.float32 and r.logits.shape == (n,)
            assert r.exact or margin_ok(r.logits, act, top_k, mc), r.name
            idx, p = topk64(r.logits, act, top_k, mc)
            assert idx.size <= min(top_k, n)
            assert idx.tolist() == oracle_lib.topk(r.logits, act, top_k, mc)[0].tolist(), (r.name, top_k, mc)
            if r.passes is not None:
                assert idx.size == min(r.passes, top_k), (r.name, top_k, mc, idx.size)
            kept = r.logits[idx].astype(np.float64)
            kept = kept[np.isfinite(kept)]
            if r.conf and act == SIGMOID:
                assert (kept >= SIGMOID_MIN_LOGIT).all(), r.name
            if r.conf and act == SOFTMAX and kept.size:
                assert kept.max() - kept.min() <= SOFTMAX_MAX_D, r.name
            if r.name == "one_value":
                assert idx.tolist() == list(range(idx.size))
    want = {"distinct", "integers", "one_value", "zeros", "max_first", "max_last", "max_last_two", "nan_#", "nan_all", "nan_first_#",
            "nan_last_#", "pos_inf", "neg_inf", "three_finite_rest_nan", "three_finite_rest_neg_inf", "very_negative", "saturating"}
    want |= {"ramp_#_pass"} | ({"on_the_cut", "on_the_cut_tied"} if act == NONE or (act == SIGMOID and n in ON_THE_CUT_COUNTS) else set())
    assert names == want, names ^ want


def test_tolerances_are_the_derived_ones():
    assert SIGMOID_RTOL == 8 * 2.0 ** -24
    assert softmax_rtol(32768, 30.0) == (128 + 30 + 24) * 2.0 ** -24 and softmax_rtol(1, 0.0) == 25 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------
# the class-count ceiling: refused at create, before any device is asked for
# ---------------------------------------------------------------------------------------------------------------
def test_class_count_ceiling_is_one_number_everywhere():
    from birda_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "birda_hip.h")).read()
    assert int(re.search(r"#define\s+BH_MAX_CLASSES\s+(\d+)", hdr).group(1)) == _lib.BH_MAX_CLASSES == CLASS_COUNTS[-1] == 32768
    kh = open(os.path.join(ROOT, "birda_amd", "csrc", "kernels.hpp")).read()
    assert int(re.search(r"TOPK_MAX_CLASSES\s*=\s*(\d+)", kh).group(1)) * 4 == 128 * 1024
    assert "BH_MAX_CLASSES" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_a_model_above_the_ceiling_is_refused_at_create(tmp_path):
    """32 769 classes: one more than a workgroup's LDS row holds.  BHM1 container, .onnx file and custom classifier alike are
    refused with BH_ERR_UNSUPPORTED and a message that states the limit and the model's class count; nothing is launched (the
    refusal comes before the device is looked for, so it is the same with and without one)."""
    from birda_amd import convert, modelfile as mf, onnx_io as ox, synth
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier, CustomClassifier
    m = synth.build_model("mini", n_classes=32769)
    bhm, onnx, bhc = str(tmp_path / "wide.bhm"), str(tmp_path / "wide.onnx"), str(tmp_path / "wide.bhc")
    mf.write_model(bhm, m)
    with open(onnx, "wb") as f:
        f.write(ox.dump(convert.graph_from_model(m)))
    mf.write_custom_classifier(bhc, synth.build_custom_classifier(4, 32769))
    for make in (lambda: BirdClassifier(bhm), lambda: BirdClassifier(onnx), lambda: CustomClassifier(bhc)):
        with pytest.raises(BirdaHipError) as e:
            make()
        assert e.value.code == -6, str(e.value)
        assert "32769 classes" in str(e.value) and "at most 32768" in str(e.value), str(e.value)
    # the accepted side of the boundary gets past this check (no device here: BH_ERR_NO_DEVICE, not UNSUPPORTED; with one the
    # GPU test runs this width through the kernel)
    ok = str(tmp_path / "widest.bhm")
    mf.write_model(ok, synth.build_model("mini", n_classes=32768))
    try:
        BirdClassifier(ok).close()
    except BirdaHipError as err:
        assert err.code == -3, str(err)
