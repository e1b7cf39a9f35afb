"""The spectrogram front end on the device (kernels_frontend.hip minmax_kernel, mel_kernel<MT, PREC>, mel32_kernel<MT32>, and the
operator api_plan.hip build_gf hands them), every output element held to the float64 reference oracle.frontend64 under the bound
derived in tests/test_frontend.py -- which also holds the case table, checked there without a GPU.

Each case goes through the product path: a model file with the branches under test and a token network, bh_classifier_create (its
validation, build_gf, the kernel choice), a forward pass with BIRDA_HIP_KEEP_TENSORS=1, read_tensor(ctx, 0, n).  The kernel that
ran is what launch_mel itself reported (bh_classifier_frontend_kernel after a forward), asserted against the table for every case;
the last test requires instantiations run == instantiations launch_mel can reach (14 mel_kernel + 4 mel32_kernel), no exemptions.

Worst err / bound measured on the MI355X over the whole table: mel_kernel f32 0.31 and split f16 0.32 (both on a constant
segment, where every v is the rounding residue of sum Gf; 0.14 and 0.29 on every other input), mel32_kernel 0.25.  The mutants
the module was shown to fail on are listed in DESIGN.md section 3."""
import os
import sys
import time

import numpy as np
import pytest

from birda_amd import modelfile as mf

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frontend as F                                          # noqa: E402  (the table, the reference and the bound)

pytestmark = pytest.mark.gpu

RAN = {}                 # instantiation -> cases it ran
WORST = {}               # (kernel family, front-end precision) -> worst err / bound
T0 = time.time()


def _family(kernel):
    if kernel.startswith("bh::mel32"):
        return ("mel32_kernel", "split f16")
    return ("mel_kernel", "f32" if kernel.endswith(", 0, 1>") else "split f16")


def _env(monkeypatch, c):
    monkeypatch.setenv("BIRDA_HIP_KEEP_TENSORS", "1")
    for name in ("BIRDA_HIP_MEL32", "BIRDA_HIP_MEL_F32", "BIRDA_HIP_PRECISION"):
        monkeypatch.delenv(name, raising=False)
    if c["mel32"] is not None:
        monkeypatch.setenv("BIRDA_HIP_MEL32", c["mel32"])


def _forward(clf, segs):
    """-> the spectrogram tensor [n][n_branches x n_mels x n_frames] of one launch of all of segs"""
    n = segs.shape[0]
    ctx = clf.create_batch_context(n)
    ctx.set_sub_slices(1)
    logits = clf.predict_logits(ctx, segs)
    spec = clf.read_tensor(ctx, 0, n)
    ctx.close()
    assert np.isfinite(logits).all()
    return spec


def run_case(c, tmp_path, monkeypatch):
    from birda_amd.classifier import BirdClassifier
    _env(monkeypatch, c)
    m = F.case_model(c)
    path = str(tmp_path / "fe.bhm")
    mf.write_model(path, m)
    segs = F.case_segments(c)
    clf = BirdClassifier(path, None, precision=c["prec"])
    planned = clf.mel_kernel_name()
    got = _forward(clf, segs)
    ran = clf.mel_kernel_name()
    assert ran == c["kernel"] and planned == ran, (c["id"], planned, ran, c["kernel"])
    RAN.setdefault(ran, []).append(c["id"])
    ref, bound, _near, zero_rows = F.reference(c, segs)
    got = got.reshape(ref.shape)
    assert np.isfinite(got).all(), (c["id"], "non-finite spectrogram")
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    fam = _family(ran)
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)
    print(f"{c['id']} {ran}: worst err / bound {ratio:.3f}, max err {err.max():.3e}, median bound {np.median(bound):.2e}")
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)
        pytest.fail(f"{c['id']} {ran}: {int(bad.sum())} of {bad.size} elements off, worst at [segment, branch, mel, frame] {i}: got "
                    f"{got[i]!r} want {ref[i]!r}, err {err[i]:.3e} > bound {bound[i]:.3e}")
    for b, rows in enumerate(zero_rows):     # a mel column without a weight: v = 0 exactly, the output exactly out_shift
        if len(rows):
            assert (got[:, b, rows] == np.float32(m.branches[b].out_shift)).all(), (c["id"], b)
    if c["alone"]:                           # every row of the launch equals the same segment run alone, bit for bit
        ctx = clf.create_batch_context(1)
        flat = got.reshape(got.shape[0], -1).view(np.uint32)
        differ = []
        for i in range(segs.shape[0]):
            clf.predict_logits(ctx, segs[i:i + 1])
            if not (clf.read_tensor(ctx, 0, 1).view(np.uint32)[0] == flat[i]).all():
                differ.append(i)
        ctx.close()
        assert not differ, (c["id"], differ[:8], len(differ))
    clf.close()


@pytest.mark.parametrize("c", F.CASES, ids=F.CASE_IDS)
def test_frontend_matches_float64(c, tmp_path, monkeypatch):
    run_case(c, tmp_path, monkeypatch)


@pytest.mark.parametrize("rid,message,kw,mel32", F.REFUSALS, ids=[r[0] for r in F.REFUSALS])
def test_create_refuses_by_message(rid, message, kw, mel32, tmp_path, monkeypatch):
    """Refused by bh_classifier_create -- no context exists yet, nothing has been launched -- each with its own message, in
    every precision"""
    from birda_amd._lib import BirdaHipError
    from birda_amd.classifier import BirdClassifier
    _env(monkeypatch, dict(mel32=mel32))
    path = str(tmp_path / "refused.bhm")
    mf.write_model(path, F.fe_model(**kw))
    for prec in ("f32", "f16x3", "auto"):
        with pytest.raises(BirdaHipError) as e:
            BirdClassifier(path, None, precision=prec)
        assert message in str(e.value), (rid, prec, str(e.value))


def test_every_reachable_instantiation_ran(tmp_path, monkeypatch):
    """Instantiations run == instantiations launch_mel can reach in the product build.  (Run on its own, this test first runs the
    named case of whatever the tests above have not.)"""
    for c in F.CASES:
        if c["id"].startswith("inst_") and c["kernel"] not in RAN:
            run_case(c, tmp_path, monkeypatch)
    assert set(RAN) == F.REACHABLE and len(RAN) == 18, (sorted(F.REACHABLE - set(RAN)), sorted(set(RAN) - F.REACHABLE))
    print(f"\n{len(RAN)} of {len(F.REACHABLE)} front-end instantiations ran:")
    for k in sorted(RAN):
        print(f"  {k:28s} {len(RAN[k]):3d} cases")
    print("worst err / bound by kernel family and precision:")
    for (fam, prec), v in sorted(WORST.items()):
        print(f"  {fam:14s} {prec:10s} {v:.3f}")
    print(f"module wall time {time.time() - T0:.0f} s")
