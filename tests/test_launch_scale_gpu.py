"""A segment's logits do not depend on how large its launch is -- also past what the chip holds at once.

Every other parity test runs launches of 1-300 segments (the full model's batch test 1 000), small enough that every workgroup of
most launches is resident at once.  A race between workgroups of one launch -- or between two kernels of one launch pair that
share arena bytes (tests/test_arena_plan_gpu.py) -- stays hidden there: all of them are still in their read phase when the first
ones write.  Here each model forces one path of forward_slice (birda_amd/csrc/api.hip) and 8 192 distinct segments go through it
in ONE launch; every row must be bit-identical to the same segment run in launches of 16, and a spread of rows (the last ones
included) must match the C oracle at the fp32 logit tolerance -- for the two families the oracle has no layers for, a multi-branch
plan (OP_CONCAT, the one-launch chain) and a DenseNet / pre-activation plan (OP_BNACT), the float64 forwards of tests/test_concat.py
and tests/test_bnact.py, at the same tolerance.

Residency: 256 CUs x at most 8 workgroups of 256 threads (32 waves a CU) = 2 048 workgroups at once, an upper bound.  At 8 192
segments the front end's min/max launch alone has at least one such workgroup per segment (4x that bound) and
  * the gate launches of a 3 840-channel chain: ceil(8 192 / 16) x ceil(3 840 / 256) = 512 x 15 = 7 680 workgroups (3.75x);
  * of a 672-channel chain: 512 x 3 = 1 536 -- not past the bound on their own, but behind the fused passes of 8 192 segments;
so every forward below runs launches of at least 3x what the chip can hold.

branchy_plan0 and dense_plan0 (synth.random_branchy_plan(0), synth.random_dense_plan(0): 44 layers each on 16 x 58-pixel images) run
at N_BIG = 8 192 as well.  Their concat, pool and norm + activation launches are grid-stride loops capped at 256 x 8 = 2 048
workgroups -- the bound itself, every one of them resident, each walking rows of many segments --, and the 1x1 convolutions between
them are GEMMs of 8 192 x 928 rows at no more than 128 rows a workgroup: at least 59 392 workgroups a launch, 29x the bound.
Time allowance of a new case: twice the slowest case the file had before, measured in the same run on one MI355X (the library and
those cases are the parent commit's, unchanged): mini_b0 [f32] 1.15 s, so 2.30 s.  Measured: branchy_plan0 0.84 s (f32) and 0.56 s
(f16x3), dense_plan0 0.52 s and 0.32 s, the float64 forward of 15 rows included -- no segment count had to be halved.
"""
import os
import time

import numpy as np
import pytest

from birda_amd import modelfile as mf
from test_arena_plan_gpu import (FUSED_WIDE_SE_PLAN, PATH_CONCAT, PATH_FUSED, PATH_FUSED_SE, PATH_HEAD_GAP, PATH_LAYER, PATH_SE_GATE,
                                 WIDE_GATE_PLAN, arena_plan, tail_gate_model)

pytestmark = pytest.mark.gpu

LOGIT_RTOL = 2e-5
N_BIG = 8192
N_SMALL = 16
N_ORACLE = 16


def _build(kind, d):
    from birda_amd import modelfile as mf, synth
    m = {"wide_gate": lambda: synth.build_model("custom", plan=WIDE_GATE_PLAN),
         "fused_wide_se": lambda: synth.build_model("custom", plan=FUSED_WIDE_SE_PLAN),
         "branchy_plan0": lambda: synth.build_model("branchy_plan", plan=synth.random_branchy_plan(0)),
         "dense_plan0": lambda: synth.build_model("dense_plan", plan=synth.random_dense_plan(0)),
         "tail_gate": tail_gate_model}.get(kind, lambda: synth.build_model(kind))()
    path = os.path.join(str(d), f"{kind}.bhm")
    mf.write_model(path, m)
    return path, m


@pytest.fixture(scope="module")
def segs_big():
    """8 192 distinct segments of the mini front-end's length (12 000 samples at 48 kHz), on the device"""
    import torch
    from birda_amd import synth
    rng = np.random.default_rng(0x5CA1E)
    t = np.arange(12000, dtype=np.float32) / 48000.0
    f = rng.uniform(300.0, 15000.0, size=(N_BIG, 2)).astype(np.float32)
    x = 0.1 * rng.standard_normal((N_BIG, 12000), dtype=np.float32)
    x += 0.3 * np.sin(2 * np.pi * f[:, :1] * t) + 0.3 * np.sin(2 * np.pi * f[:, 1:] * t)
    x[:4] = synth.synth_segments(4, 12000, 48000)
    x = np.clip(x, -1.0, 1.0).astype(np.float32)
    return x, torch.from_numpy(x).cuda()


def _forward(clf, ctx, d_x, n, n_classes):
    import torch
    out = torch.empty((n, n_classes), device="cuda")
    t0 = time.perf_counter()
    clf.forward_device(ctx, d_x.data_ptr(), n, out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy(), time.perf_counter() - t0


# (model, the path it exists for, a predicate on (model, path tags) that says the path is taken)
def _takes(tag, cond=lambda m, i: True):
    return lambda m, tags: any(t == tag and cond(m, i) for i, t in enumerate(tags))


CASES = {
    "wide_gate": _takes(PATH_SE_GATE, lambda m, i: m.layers[i].cout == 3840),                   # (a) the gate fast path
    "fused_wide_se": _takes(PATH_FUSED_SE, lambda m, i: m.layers[i + 1].cout > 576),            # (b) se_gate16 on the fused path
    "mini_se": _takes(PATH_FUSED_SE),                                                           # (c) se_gate_kernel
    "mini_hg": _takes(PATH_HEAD_GAP),                                                           # (d) head conv + pool
    "mini_b0": _takes(PATH_FUSED),                                                              # (e) plain fused blocks
    "branchy_plan0": _takes(PATH_CONCAT),                                                       # (f) the one-launch concat chain
    "dense_plan0": _takes(PATH_LAYER, lambda m, i: m.layers[i].op == mf.OP_BNACT),              # (g) norm + activation layers
}


def _reference(kind, path, m, x, oracle_lib):
    """The yardstick's logits for the rows x: the C oracle, and for the two families it has no layers for (OP_CONCAT, OP_BNACT) the
    float64 forwards of tests/test_concat.py and tests/test_bnact.py"""
    if kind == "branchy_plan0":
        from test_concat import forward64
        return forward64(m, x)
    if kind == "dense_plan0":
        from test_bnact import forward64
        return forward64(m, x)
    return oracle_lib.OracleModel(path).forward(x)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("kind", list(CASES))
def test_launch_past_residency_matches_small_launches_and_oracle(kind, precision, segs_big, tmp_path, oracle_lib):
    from birda_amd.classifier import BirdClassifier
    path, m = _build(kind, tmp_path)
    x, d_x = segs_big
    clf = BirdClassifier(path, None, precision=precision)
    big, small = clf.create_batch_context(N_BIG), clf.create_batch_context(N_SMALL)
    try:
        _, _, tags = arena_plan(clf, big, 0)
        # (the head conv + pool launch takes the f16 weight planes: in f32 the head runs as conv and pool -- still a launch of 8 192)
        if not (kind == "mini_hg" and precision == "f32"):
            assert CASES[kind](m, tags), (kind, precision, tags)
        got, t_big = _forward(clf, big, d_x, N_BIG, m.n_classes)
        want, t_small = _forward(clf, small, d_x, N_BIG, m.n_classes)
    finally:
        big.close(); small.close(); clf.close()
    bad = np.flatnonzero((got != want).any(axis=1))
    rows = np.unique(np.concatenate([np.linspace(0, N_BIG - 1, N_ORACLE - 2).astype(int), [N_BIG - 2, N_BIG - 1]]))
    ref = _reference(kind, path, m, x[rows], oracle_lib)
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got[rows] - ref).max())
    print(f"{kind} [{precision}]: {N_BIG} segments in one launch {t_big * 1e3:.1f} ms, in launches of {N_SMALL} {t_small * 1e3:.1f} ms; "
          f"{len(bad)} rows differ; reference max|dlogit| {err:.3e} on {len(rows)} rows (max|logit| {scale:.3f})")
    assert np.isfinite(got).all()
    assert len(bad) == 0, f"{len(bad)} of {N_BIG} rows differ from launches of {N_SMALL}, first {bad[:8].tolist()}"
    assert err <= LOGIT_RTOL * scale, (err, LOGIT_RTOL * scale)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_model_that_ends_in_a_gate_chain_writes_its_logits(precision, segs_big, tmp_path, oracle_lib):
    """Pool -> 1x1 (640 -> 160) -> 1x1 (160 -> 640) as the model's last three layers (640 classes, 16 pixels): the gate fast path
    writes the gate -- the logits -- to the caller's logits buffer, not to an arena slot past the last layer."""
    import torch
    from birda_amd.classifier import BirdClassifier
    path, m = _build("tail_gate", tmp_path)
    x, d_x = segs_big
    n = 40
    clf = BirdClassifier(path, None, precision=precision)
    ctx = clf.create_batch_context(n)
    try:
        _, _, tags = arena_plan(clf, ctx, 0)
        assert tags[len(m.layers) - 3] == PATH_SE_GATE, tags[-3:]
        out = torch.full((n, m.n_classes), float("nan"), device="cuda")
        clf.forward_device(ctx, d_x.data_ptr(), n, out.data_ptr())
        ctx.synchronize()
        got = out.cpu().numpy()
        host = clf.predict_logits(ctx, x[:n])
    finally:
        ctx.close(); clf.close()
    ref = oracle_lib.OracleModel(path).forward(x[:n])
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print(f"tail gate [{precision}]: oracle max|dlogit| {err:.3e} (max|logit| {scale:.3f})")
    assert np.isfinite(got).all() and err <= LOGIT_RTOL * scale, err
    assert (host == got).all()


def test_se_group_mb_keeps_a_segments_bits(segs_big, tmp_path, monkeypatch):
    """BIRDA_HIP_SE_GROUP_MB cuts a squeeze-excite block's three launches into groups of segments; the gate of a block beyond 576
    channels must be the same kernel in the groups as in whole launches (se_gate16), so the bits do not change."""
    from birda_amd.classifier import BirdClassifier
    path, m = _build("fused_wide_se", tmp_path)
    _, d_x = segs_big
    n = 1000
    out = {}
    for mb in (None, "2"):       # (2 MB: groups of ~13 segments of the 672-channel block's 161 KB depthwise output)
        if mb is None:
            monkeypatch.delenv("BIRDA_HIP_SE_GROUP_MB", raising=False)
        else:
            monkeypatch.setenv("BIRDA_HIP_SE_GROUP_MB", mb)
        clf = BirdClassifier(path, None, precision="f16x3")
        ctx = clf.create_batch_context(n)
        try:
            _, _, tags = arena_plan(clf, ctx, 0)
            assert CASES["fused_wide_se"](m, tags), tags
            out[mb], _ = _forward(clf, ctx, d_x, n, m.n_classes)
        finally:
            ctx.close(); clf.close()
    bad = np.flatnonzero((out[None] != out["2"]).any(axis=1))
    assert np.isfinite(out[None]).all()
    assert len(bad) == 0, f"{len(bad)} of {n} rows change with BIRDA_HIP_SE_GROUP_MB=2, first {bad[:8].tolist()}"
