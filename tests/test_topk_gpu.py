"""`topk_kernel` alone, held to the float64 restatement of tests/test_topk.py.

Hand-made logits go through `BirdClassifier.topk_from_logits` (the model file only supplies the class count and the output
activation; no labels) and through `CustomClassifier.predict_batch` (identity weights plant the logits).  The rows, the class
counts, the cuts and the tolerances are the table of tests/test_topk.py, which holds them to the C oracle on the CPU:

  * indices and prediction counts equal the restatement's, no tolerance (ranking is on the logit: the order is determined);
  * confidences: NONE bit-equal to the logit, sigmoid 2^-21, softmax (ceil(n / 256) + d + 24) 2^-24 relative to float64
    (derived in test_topk.py); saturating rows are held to order and count only;
  * a row's result does not depend on the batch it was submitted in, nor on the run.

What these tests notice in a scratch copy of the kernel: `oi > bi` for `oi < bi` in topk_better, `> min_conf` for `>=`, a softmax
sum without `- mx`.  What no test can: dropping `i >= n_classes` from the selection scan.  A clamped read past the row has class
n - 1's value under a higher index, so it loses every tie to the class itself (which is always among the candidates), and it reads
NaN from the pass that chose that class on; the guard saves comparisons, the result is the same with and without it.
"""

import numpy as np
import pytest

import test_topk as T                                              # noqa: E402  (the restatement, the table, the tolerances)

pytestmark = pytest.mark.gpu

MINI_PLAN = {"sr": 48000, "n": 12000, "branches": [(512, 100, 32, 0.0, 3000.0), (256, 103, 32, 500.0, 15000.0)], "stem": 8,
             "stages": [(1, 3, 1, 8, 1), (4, 5, 2, 16, 2), (4, 3, 2, 24, 1)], "head": 64}    # synth's "mini": only its last layer matters here


class Shop:
    """Model files by (class count, activation) and classifiers by (class count, activation, top_k, min_confidence): each
    built once per module."""

    def __init__(self, d):
        self.d, self.models, self.clfs, self.built = d, {}, {}, []

    def model(self, n, act):
        from birda_amd import modelfile as mf, synth
        if (n, act) not in self.models:
            path = str(self.d / f"topk_{n}_{act}.bhm")
            mf.write_model(path, synth.build_model("custom", plan=dict(MINI_PLAN, classes=n, out_act=act)))
            self.models[(n, act)] = path
        return self.models[(n, act)]

    def clf(self, n, act, top_k, min_conf):
        from birda_amd.classifier import BirdClassifier
        key = (n, act, top_k, min_conf)
        if key not in self.clfs:
            assert key not in self.built, f"classifier {key} built a second time"
            self.built.append(key)
            c = BirdClassifier(self.model(n, act), None, top_k=top_k, min_confidence=min_conf)
            assert c.n_classes() == n and int(c.info.output_activation) == act
            self.clfs[key] = c
        return self.clfs[key]

    def close(self, keep=()):
        for key in [k for k in self.clfs if k not in keep]:
            self.clfs.pop(key).close()


# classifiers the later tests share with the table (left open by it)
SHARED = {(2049, T.SIGMOID, 5, T.MIN_CONF[T.SIGMOID]), (2049, T.SOFTMAX, 5, T.MIN_CONF[T.SOFTMAX]), (257, T.SIGMOID, 5, 0.0),
          (257, T.NONE, 5, 0.0)}


@pytest.fixture(scope="module")
def shop(tmp_path_factory):
    s = Shop(tmp_path_factory.mktemp("topk"))
    yield s
    s.close()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _got(res):
    return [q.index for q in res.predictions], np.asarray([q.confidence for q in res.predictions], np.float32)


def check_row(row, res, n, act, top_k, min_conf, worst):
    """One row of the kernel's output against the restatement.  worst: {activation: largest error / tolerance seen}."""
    want_i, want_p = T.topk64(row.logits, act, top_k, min_conf)
    got_i, got_c = _got(res)
    where = f"{row.name}: n {n} act {act} top_k {top_k} min_conf {min_conf}"
    assert got_i == want_i.tolist(), where
    if not row.conf or not got_i:
        return
    kept = row.logits[want_i]
    if act == T.NONE:
        assert np.array_equal(_bits(got_c), _bits(kept)), where
        return
    if act == T.SIGMOID:
        rtol = T.SIGMOID_RTOL
    else:
        fin = kept[np.isfinite(kept)].astype(np.float64)
        rtol = T.softmax_rtol(n, float(fin.max() - fin.min()) if fin.size else 0.0)     # (the first kept class is the row's maximum)
    err = np.abs(got_c.astype(np.float64) - want_p)
    with np.errstate(all="ignore"):
        ratio = np.where(want_p > 0, err / (rtol * want_p), np.where(err == 0, 0.0, np.inf))
    worst[act] = max(worst.get(act, 0.0), float(ratio.max()))
    assert (err <= rtol * want_p).all(), (where, got_c.tolist(), want_p.tolist(), rtol)


@pytest.mark.parametrize("n,act", T.GPU_TABLE)
def test_topk_kernel_matches_float64(shop, n, act):
    """Every family of the table as one batch, at top_k 1 / 5 / 32, at min_confidence 0 and at the activation's cut (and, for the
    sigmoid at two class counts, the classifier whose cut the rows sit exactly on)."""
    worst, rows_run = {}, 0
    try:
        for top_k, mc in T.configs(act) + T.exact_configs(n, act):
            rows = T.family_rows(n, act, top_k, mc)
            res = shop.clf(n, act, top_k, mc).topk_from_logits(np.stack([r.logits for r in rows]))
            assert len(res) == len(rows)
            for row, r in zip(rows, res):
                check_row(row, r, n, act, top_k, mc, worst)
            rows_run += len(rows)
    finally:
        print(f"topk n {n} act {act}: {rows_run} rows, worst confidence error / tolerance {worst}")
        shop.close(keep=SHARED)


@pytest.mark.parametrize("act", [T.SIGMOID, T.SOFTMAX])
def test_rows_do_not_depend_on_the_batch_or_the_run(shop, act):
    """257 rows cycling through the families (each cycle rotated by one more class): every row
    bit-equal to the same row submitted alone, the batch bit-equal to itself submitted again -- one block per row, the static
    LDS arrays reused across the selection passes and nothing carried from row to row."""
    n, top_k, mc = 2049, 5, T.MIN_CONF[act]
    fam = T.family_rows(n, act, top_k, mc)
    rows = [np.roll(fam[i % len(fam)].logits, i // len(fam)) for i in range(257)]
    clf = shop.clf(n, act, top_k, mc)
    batch = np.stack(rows)
    a, b = clf.topk_from_logits(batch), clf.topk_from_logits(batch)
    kept = 0
    for i, x in enumerate(rows):
        (ai, ac), (bi, bc) = _got(a[i]), _got(b[i])
        assert ai == T.topk64(x, act, top_k, mc)[0].tolist(), (i, fam[i % len(fam)].name)
        assert ai == bi and np.array_equal(_bits(ac), _bits(bc)), (i, "second run differs")
        oi, oc = _got(clf.topk_from_logits(x[None, :])[0])
        assert ai == oi and np.array_equal(_bits(ac), _bits(oc)), (i, fam[i % len(fam)].name, "alone differs")
        kept += len(ai)
    assert kept > 400      # (932 / 407 by the restatement: the batch is not one of empty rows)


@pytest.mark.parametrize("n", [1, 3, 32, 33])
def test_custom_classifier_keeps_every_class_up_to_32_in_order(tmp_path, n):
    """top_k = 0: all classes up to BH_MAX_TOP_K, min_confidence 0.  Identity weights and a zero bias plant the logits (x * 1 and
    sums with exact zeros: the f32 GEMM hands them on unchanged)."""
    from birda_amd import modelfile as mf
    from birda_amd.classifier import CustomClassifier
    path = str(tmp_path / "identity.bhc")
    mf.write_custom_classifier(path, mf.CustomClassifierModel(n, mf.OUT_SIGMOID, [mf.CustomLayer(np.eye(n, dtype=np.float32), np.zeros(n, np.float32), mf.ACT_NONE)]))
    cc = CustomClassifier(path, None, top_k=0)
    try:
        assert cc.num_classes() == n
        rng = np.random.default_rng(n)
        rows = [T._distinct(rng, n, 3.0), np.round(rng.standard_normal(n) * 3.0).astype(np.float32) + 0.0, np.full(n, 1.5, np.float32),
                np.arange(n, dtype=np.float32) - 2.0]
        worst = {}
        for x, r in zip(rows, cc.predict_batch(np.stack(rows))):
            assert len(r.predictions) == min(n, T.BH_MAX_TOP_K)
            check_row(T.Row("custom", x), r, n, T.SIGMOID, min(n, T.BH_MAX_TOP_K), 0.0, worst)
        print(f"custom classifier n {n}: worst confidence error / tolerance {worst}")
    finally:
        cc.close()


def test_species_list_keeps_index_order_inside_a_tied_group(shop):
    n, top_k = 257, 5
    clf = shop.clf(n, T.SIGMOID, top_k, 0.0)
    tied = np.full(n, 1.5, np.float32)                       # kept: 0 1 2 3 4
    groups = np.full(n, -2.0, np.float32)
    groups[[200, 9, 120]] = 3.0                              # kept: 9 120 200, then 4 33 of the next group
    groups[[33, 4, 256]] = 1.0
    batch = np.stack([tied, groups])
    plain = [_got(r) for r in clf.topk_from_logits(batch)]
    assert [p[0] for p in plain] == [[0, 1, 2, 3, 4], [9, 120, 200, 4, 33]]
    keep = np.ones(n, np.uint8)
    keep[[1, 3, 120, 4]] = 0
    try:
        clf.set_species_list(keep)
        got = [_got(r) for r in clf.topk_from_logits(batch)]
    finally:
        clf.clear_filters()
    for (pi, pc), (gi, gc), want in zip(plain, got, ([0, 2], [9, 200, 33])):
        assert gi == want
        assert np.array_equal(_bits(gc), _bits([c for i, c in zip(pi, pc) if keep[i]]))


def test_rerank_keeps_the_order_of_equal_products(shop):
    """Products that come out equal keep the order the ranking gave them (a stable sort): by logit, not by index."""
    n, top_k = 257, 5
    clf = shop.clf(n, T.NONE, top_k, 0.0)
    x = np.full(n, -1.0, np.float32)
    x[[7, 100, 2]] = (0.5, 0.25, 0.25)                       # ranked 7, 2, 100
    tied = np.full(n, 0.75, np.float32)                      # ranked 0 1 2 3 4
    scores = np.ones(n, np.float32)
    scores[7] = 0.5                                          # 0.5 * 0.5 = 0.25 * 1 = 0.25 * 1
    scores[:5] = (0.5, 0.5, 1.0, 0.5, 0.5)                   # row 2: 0.375 0.375 0.75 0.375 0.375 -> 2 0 1 3 4
    try:
        clf.set_range_filter(scores, 0.01, "keep", rerank=True)
        a, b = [_got(r) for r in clf.topk_from_logits(np.stack([x, tied]))]
    finally:
        clf.clear_filters()
    assert a[0] == [7, 2, 100] and a[1].tolist() == [0.25, 0.25, 0.25]
    assert b[0] == [2, 0, 1, 3, 4] and b[1].tolist() == [0.75, 0.375, 0.375, 0.375, 0.375]
