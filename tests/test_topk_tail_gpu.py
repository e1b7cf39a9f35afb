"""The tail of `topk_kernel` on the device, held to `tail64` (tests/test_topk_tail.py): BSG calibration with and without the
SDM prior, the range filter under its four policy / rerank pairs, the species list, and their combinations.

The rows and the table settings are those of tests/test_topk_tail.py, which shows on the CPU that their order is decided by the
restatement alone.  Each (class count, activation, top_k) has one classifier (`Shop` of tests/test_topk_gpu.py); a batch first
runs with no table set -- that run's float32 confidences are what the tail receives -- and then under every setting:

  * indices and counts equal `tail64`'s, no tolerance (and the order is decided on THESE confidences too: `undecided` is empty);
  * confidences within the derived bound; where neither BSG nor rerank touched them, or the result is exact (saturated, a prior or
    score of 0, +inf), bit-equal;
  * the tables' lifecycle, batch independence, and every entry point that launches the kernel.

Worst confidence error / bound on the MI355X (sigmoid / softmax / none, the larger of the two class counts):
    bsg 0.597 / 0.503 / 0.547      bsg+prior 0.254 / 0.285 / 0.279      bsg+prior+range 0.254 / 0.277 / 0.260
    bsg+prior+rerank 0.519 / 0.425 / 0.406      bsg+prior+species 0.247 / 0.284 / 0.266      rerank 0.928 / 0.982 / 0.918
(rerank alone is one f32 rounding against u |ref|: it comes close to 1 and cannot pass it); lifecycle 0.247.

Mutants (a scratch copy of the library; DESIGN.md section 3 lists what each trips): `<=` in either insertion sort, the upper
clamp removed, the upper clamp as a double constant, `sc > threshold`, `keeps` without `!rerank`, the species list applied
although a range table is set, BSG moved behind the filter, the `for (i = w; i < n; ...)` clean-up dropped.
"""
import numpy as np
import pytest

import test_topk as T
import test_topk_tail as TT
from test_topk_gpu import Shop, _bits, _got

pytestmark = pytest.mark.gpu


class TailShop(Shop):
    """(a test closes what it opened: a later test may build the same classifier again)"""

    def close(self, keep=()):
        super().close(keep)
        self.built = [k for k in self.built if k in self.clfs]


@pytest.fixture(scope="module")
def shop(tmp_path_factory):
    s = TailShop(tmp_path_factory.mktemp("topk_tail"))
    yield s
    s.close()


def apply(clf, st):
    if st.bsg is not None:
        clf.set_bsg(st.bsg.a, st.bsg.b, st.bsg.prior)
    if st.rng is not None:
        clf.set_range_filter(st.rng.scores, st.rng.threshold, "keep" if st.rng.keep else "drop", st.rng.rerank)
    if st.species is not None:
        clf.set_species_list(st.species)


def clear(clf):
    clf.clear_filters()
    clf.clear_bsg()


def check(where, plain, got, n, st, worst, key):
    """One row: the device's (indices, confidences) under the setting `st` against tail64 of the unfiltered run's"""
    want = TT.tail_trace(plain[0], plain[1], n, st.bsg, st.rng, st.species)
    assert not TT.undecided(want), (where, TT.undecided(want))
    gi, gc = got
    assert gi == want.idx, (where, gi, want.idx)
    if not gi:
        return
    exact = want.bound == 0
    assert np.array_equal(_bits(gc[exact]), _bits(want.conf[exact].astype(np.float32))), (where, gc.tolist(), want.conf.tolist())
    if (~exact).any():
        err = np.abs(gc[~exact].astype(np.float64) - want.conf[~exact])
        worst[key] = max(worst.get(key, 0.0), float((err / want.bound[~exact]).max()))
        assert (err <= want.bound[~exact]).all(), (where, gc.tolist(), want.conf.tolist(), want.bound.tolist())


@pytest.mark.parametrize("n,act", TT.CASES)
def test_tail_matches_float64(shop, n, act):
    """Every row under every table setting, at top_k 1 / 5 / 32."""
    rows, worst, run = TT.rows(n, act), {}, 0
    batch = np.stack([r.logits for r in rows])
    try:
        for top_k in TT.TOP_KS:
            clf = shop.clf(n, act, top_k, TT.MIN_CONF[act])
            plain = [_got(r) for r in clf.topk_from_logits(batch)]
            for r, (pi, pc) in zip(rows, plain):
                assert pi == T.topk64(r.logits, act, top_k, TT.MIN_CONF[act])[0].tolist(), (r.name, top_k)
            for st in TT.stages(n):
                try:
                    apply(clf, st)
                    got = [_got(r) for r in clf.topk_from_logits(batch)]
                finally:
                    clear(clf)
                for r, p, g in zip(rows, plain, got):
                    check((r.name, st.name, n, act, top_k), p, g, n, st, worst, TT.stage_kind(st))
                    run += 1
            after = [_got(r) for r in clf.topk_from_logits(batch)]
            for (pi, pc), (ai, ac) in zip(plain, after):
                assert pi == ai and np.array_equal(_bits(pc), _bits(ac))
    finally:
        for k in sorted(worst):
            print(f"tail n {n} act {act} {k}: worst confidence error / bound {worst[k]:.3f}")
        print(f"tail n {n} act {act}: {run} rows")
        shop.close()


def test_table_lifecycle(shop):
    """Set BSG with a prior, then without: the prior is off.  clear_filters leaves BSG on, clear_bsg leaves the range table on.  A
    table of the wrong length is refused and the previous one stays in force.  After everything is cleared the results are
    bit-equal to those of a classifier that never had a table."""
    from birda_amd._lib import BirdaHipError
    n, act, top_k = 257, T.SIGMOID, 5
    rows = TT.rows(n, act)
    batch = np.stack([r.logits for r in rows])
    S = {s.name: s for s in TT.stages(n)}
    clf = shop.clf(n, act, top_k, 0.0)
    plain = [_got(r) for r in clf.topk_from_logits(batch)]
    worst = {}

    def expect(tag, bsg=None, rng=None, species=None):
        st = TT.Stage(tag, bsg, rng, species)
        for r, p, g in zip(rows, plain, [_got(x) for x in clf.topk_from_logits(batch)]):
            check((r.name, tag), p, g, n, st, worst, tag)

    with_prior, rng, alt = S["bsg_random_prior01"].bsg, S["range_0.01_drop"].rng, S["species_alternating"].species
    no_prior = TT.Bsg(with_prior.a, with_prior.b)
    try:
        clf.set_bsg(with_prior.a, with_prior.b, with_prior.prior)
        expect("prior on", with_prior)
        clf.set_bsg(no_prior.a, no_prior.b)
        expect("prior off again", no_prior)
        apply(clf, TT.Stage("", None, rng))
        expect("bsg + range", no_prior, rng)
        clf.clear_filters()
        expect("clear_filters leaves BSG on", no_prior)
        apply(clf, TT.Stage("", None, rng))
        clf.clear_bsg()
        expect("clear_bsg leaves the range table on", None, rng)
        # wrong lengths: refused, the previous tables stay
        clf.set_bsg(with_prior.a, with_prior.b, with_prior.prior)
        for bad in (lambda: clf.set_bsg(with_prior.a[:-1], with_prior.b[:-1], with_prior.prior[:-1]),
                    lambda: clf.set_range_filter(np.zeros(n + 1, np.float32), 0.5, "keep", True),
                    lambda: clf.set_species_list(np.zeros(n - 1, np.uint8))):
            with pytest.raises(BirdaHipError):
                bad()
            expect("after a refused table", with_prior, rng)
        clf.clear_filters()
        clf.set_species_list(alt)
        with pytest.raises(BirdaHipError):
            clf.set_species_list(np.ones(2 * n, np.uint8))
        expect("after a refused list", with_prior, None, alt)
    finally:
        clear(clf)
    cleared = [_got(r) for r in clf.topk_from_logits(batch)]
    shop.close()
    fresh = shop.clf(n, act, top_k, 0.0)                         # (the shop forgot the first one: this classifier never had a table)
    never = [_got(r) for r in fresh.topk_from_logits(batch)]
    shop.close()
    for other in (cleared, plain):
        assert all(oi == ni and np.array_equal(_bits(oc), _bits(nc)) for (oi, oc), (ni, nc) in zip(other, never))
    print(f"lifecycle: worst confidence error / bound {max(worst.values()):.3f}")


@pytest.mark.parametrize("act", [T.SIGMOID, T.SOFTMAX])
def test_rows_do_not_depend_on_the_batch_or_the_run(shop, act):
    """257 rows cycling through the table with BSG + prior + rerank on: every row bit-equal to the same row alone and to a second
    run (thread 0's tail works in the static LDS arrays of its own block; nothing is carried from row to row)."""
    n, top_k = 257, 32
    fam = TT.rows(n, act)
    rows = [fam[i % len(fam)].logits for i in range(257)]
    st = {s.name: s for s in TT.stages(n)}["bsg_then_range_rerank"]
    clf = shop.clf(n, act, top_k, 0.0)
    batch = np.stack(rows)
    try:
        apply(clf, st)
        a, b = clf.topk_from_logits(batch), clf.topk_from_logits(batch)
        kept = 0
        for i, x in enumerate(rows):
            (ai, ac), (bi, bc) = _got(a[i]), _got(b[i])
            assert ai == bi and np.array_equal(_bits(ac), _bits(bc)), (i, "second run differs")
            oi, oc = _got(clf.topk_from_logits(x[None, :])[0])
            assert ai == oi and np.array_equal(_bits(ac), _bits(oc)), (i, fam[i % len(fam)].name, "alone differs")
            j = i % len(fam)
            if i >= len(fam):
                ci, cc = _got(a[j])
                assert ai == ci and np.array_equal(_bits(ac), _bits(cc)), (i, "differs from its first copy in the batch")
            kept += len(ai)
        assert kept > 1000
    finally:
        clear(clf)
        shop.close()


# ---------------------------------------------------------------------------------------------------------------
# every entry point that launches the kernel hands it the same tables
# ---------------------------------------------------------------------------------------------------------------
def _tables(n, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 1.0, n).astype(np.float32)
    b = rng.uniform(0.5, 2.0, n).astype(np.float32)
    prior = rng.random(n).astype(np.float32)
    sc = (0.02 + 0.9 * rng.random(n)).astype(np.float32)
    sc[rng.random(n) < 0.2] = np.nan
    sc[rng.random(n) < 0.2] = 0.001
    return TT.Stage("bsg+rerank", TT.Bsg(a, b, prior), TT.Range(sc, 0.01, True, True))


def _same(tag, got, want):
    assert len(got) == len(want)
    kept = 0
    for i, (g, w) in enumerate(zip(got, want)):
        (gi, gc), (wi, wc) = _got(g), _got(w)
        assert gi == wi and np.array_equal(_bits(gc), _bits(wc)), (tag, i, gi, wi, gc.tolist(), wc.tolist())
        kept += len(gi)
    return kept


def _device_rows(di, dc):
    from birda_amd.classifier import Prediction, PredictionResult
    return [PredictionResult([Prediction(str(int(i)), float(c), int(i)) for i, c in zip(ri, rc) if i >= 0]) for ri, rc in zip(di, dc)]


def test_every_entry_point_applies_the_tables(shop):
    """predict_batch_with_context, the device-resident forward_device with top-k outputs and MultiClassifier with two logical
    shards, on the mini model with 257 classes under BSG + prior + rerank: row for row and bit for bit what topk_from_logits
    returns for the logits of the same segments (forward_device reports them itself; for the others predict_logits does, and a
    row's logits do not depend on the batch it ran in)."""
    import torch
    from birda_amd import synth
    from birda_amd.classifier import BirdClassifier
    from birda_amd.multi import MultiClassifier
    n, top_k, nseg = 257, 5, 12
    path = shop.model(n, T.SIGMOID)
    st = _tables(n)
    clf = BirdClassifier(path, None, top_k=top_k, min_confidence=0.0, precision="f16x3")
    segs = synth.synth_segments(nseg, clf.sample_count(), clf.sample_rate(), start=30)
    ctx = clf.create_batch_context(nseg)
    mc = None
    try:
        plain = clf.predict_batch_with_context(ctx, list(segs))
        apply(clf, st)
        logits = clf.predict_logits(ctx, segs)
        want = clf.topk_from_logits(logits)
        assert [_got(r)[0] for r in want] != [_got(r)[0] for r in plain]              # the tables change what comes out
        assert _same("predict_batch_with_context", clf.predict_batch_with_context(ctx, list(segs)), want) >= nseg
        _same("predict", [clf.predict(segs[3])], want[3:4])
        x = torch.from_numpy(segs).cuda()
        lg = torch.empty((nseg, n), device="cuda")
        di = torch.empty((nseg, top_k), dtype=torch.int32, device="cuda")
        dc = torch.empty((nseg, top_k), device="cuda")
        clf.forward_device(ctx, x.data_ptr(), nseg, lg.data_ptr(), di.data_ptr(), dc.data_ptr())
        ctx.synchronize()
        dev_logits = lg.cpu().numpy()
        assert np.array_equal(_bits(dev_logits), _bits(logits))
        _same("forward_device", _device_rows(di.cpu().numpy(), dc.cpu().numpy()), clf.topk_from_logits(dev_logits))
        mc = MultiClassifier(path, None, devices=[0, 0], top_k=top_k, min_confidence=0.0, precision="f16x3", max_batch=4)
        for g in range(2):
            apply(mc.shard_classifier(g), st)
        _same("MultiClassifier.predict_batch_contig", mc.predict_batch_contig(segs), want)
        _same("MultiClassifier.forward_device", mc.forward_device([x.data_ptr(), x.data_ptr() + 7 * segs.shape[1] * 4], [7, 5]), want)
    finally:
        if mc is not None:
            mc.close()
        clear(clf)
        ctx.close(); clf.close()


def test_the_f32_rerun_of_auto_rows_applies_the_tables(tmp_path):
    """BH_FLAG_AUTO on a model whose rows leave the f16 range (as tests/test_multi_gpu.py builds it): the rows re-run on the f32
    kernels come back under the same tables."""
    from birda_amd import modelfile as mf, synth
    from birda_amd.classifier import BirdClassifier
    from test_parity_gpu import _rescale_trunk
    m = synth.build_model("mini_b0")
    m2, _ = _rescale_trunk(m, [2.0 ** 14])
    path = str(tmp_path / "overflow.bhm")
    mf.write_model(path, m2)
    nseg = 12
    segs = synth.synth_segments(nseg, m.sample_count, m.sample_rate, start=40)
    st = _tables(m.n_classes, seed=6)
    clf = BirdClassifier(path, None, top_k=5, min_confidence=0.0, precision="auto")
    ctx = clf.create_batch_context(nseg)
    try:
        apply(clf, st)
        got = clf.predict_batch_with_context(ctx, list(segs))
        assert clf.fallback_segments() > 0
        logits = clf.predict_logits(ctx, segs)
        assert np.isfinite(logits).all()
        assert _same("auto", got, clf.topk_from_logits(logits)) >= nseg
        plain_idx = [np.argsort(-row.astype(np.float64), kind="stable")[:5].tolist() for row in logits]
        assert [_got(r)[0] for r in got] != plain_idx
    finally:
        clear(clf)
        ctx.close(); clf.close()
