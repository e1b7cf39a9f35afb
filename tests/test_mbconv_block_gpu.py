"""Every shipped instantiation of the fused MBConv kernel (mbconv_kernel.hpp x mbconv_cfgs.inc x three activations, and pass A of
the squeeze-excite blocks) alone on host operands through bh_debug_mbconv_block, every output element held to the float64
reference O.mbconv64 -- at the shapes of tests/test_mbconv_block.py's catalogue: the row's natural shape, last tiles partly
outside the image, stride 2 on odd images, partial last chunks and project tiles, relaxed k steps, column tasks at and below
their height, odd segment counts on two-segment tiles, launches past the resident grid, the stem, no-expand and gated forms, the
channel split, and D in both layouts.  A logit test averages a wrong halo pixel or a wrong last channel away; here nothing is.

The tolerance has no constants of its own.  It is the forward propagation, stage by stage in float64, of the per-GEMM tolerances
of tests/test_layer_gemm_gpu.py (tau = 4e-7 max(1, sqrt(K / 1024)) for f32 and split f16, 1.5e-3 for plain f16; slope 1.2;
eps_act), with (*) the depthwise taps:

    e_E = tau_e 1.2 (|X| |We| + |be|) + eps_act(preE)                                     (0 for a no-expand block: E is X)
    e_D = 1.2 (|Wd| (*) e_E + tau_d (|Wd| (*) |E| + |bd|)) + eps_act(preD)                (x |gate| where there is one)
    e_Y = |Wp|^T e_D + tau_p (|D| |Wp| + |bp| + |R|)

and |got - ref| <= e_Y element by element (pass A: |D_got - D| <= e_D, the sum of pool_part over tiles against the float64 channel
sum within e_D summed over the image).  tau describes operands rounded to their format's nominal precision (2^-11 of the value
for the f16 hi plane, 2^-22 for hi + lo).  Where the weights are so small against the plane's exponent that a lo half goes
subnormal (the |se| <= 21 clamp of the GELU blocks: test_weight_scales_far_from_the_usual), the representation error
|w - (hi + lo)| is computed per weight in float64 from the same exponents plan_fusion uses, and what exceeds the nominal precision
is propagated into e_E (|X| dWe) and e_Y (|D| dWp).

Every device buffer sits in NaN guard bands; outputs start as the payload 0x7fc0beef.  The last test compares the set of
instantiations that ran with the set the library ships: no list exempts an entry."""
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_mbconv_block as CAT                                   # noqa: E402  (the catalogue, checked on the CPU there)
from test_layer_gemm_gpu import _eps_act, _tau                     # noqa: E402  (the per-GEMM tolerances, shared)

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
REACHED = set()          # instantiation names that ran
WORST = {}               # (family, precision) -> worst err / e
T0 = time.time()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _family(r_or_shape, se):
    s = r_or_shape
    f = "stem" if s[16] else "noexp" if s[13] else "expand"
    return f + ("_passA" if se else "")


# -----------------------------------------------------------------------------------------------------------------------------
# operands
# -----------------------------------------------------------------------------------------------------------------------------
def operands(shape, n, residual, gate, seed, we_scale=1.0, wd_scale=1.0, wp_scale=1.0):
    """Channels of different scale (0.2-3x), He-scaled weights, biases of order 1 with entries that push ReLU6 into both clamps."""
    H, W, Cin, Cexp, Cout, Ho, Wo = shape[:7]
    KS, noexp = shape[9], shape[13]
    stem_c, stem_h, stem_w = shape[16:19]
    rng = np.random.default_rng(seed)
    f = np.float32
    if stem_c:
        X = (rng.standard_normal((n, stem_c, stem_h, stem_w)) * rng.uniform(0.2, 3.0, stem_c)[:, None, None]).astype(f)
    else:
        X = (rng.standard_normal((n, H, W, Cin)) * rng.uniform(0.2, 3.0, Cin)).astype(f)
    We = (rng.standard_normal((Cin, Cexp)) * math.sqrt(2.0 / Cin) * we_scale).astype(f)
    be = (rng.standard_normal(Cexp) * we_scale).astype(f)
    be[:2] = (7.5 * we_scale, -7.5 * we_scale)
    be[-1] = 7.5 * we_scale                      # (the last channel of a partial last chunk, too)
    Wd = (rng.standard_normal((KS * KS, Cexp)) * math.sqrt(2.0 / (KS * KS)) * wd_scale).astype(f)
    bd = rng.standard_normal(Cexp).astype(f)
    bd[1:4] = (7.5, -7.5, 7.0)
    bd[-1] = 7.5
    Wp = (rng.standard_normal((Cexp, Cout)) * math.sqrt(2.0 / Cexp) * wp_scale).astype(f)
    bp = (rng.standard_normal(Cout) * wp_scale).astype(f)
    R = (rng.standard_normal((n, Ho, Wo, Cout)) * wp_scale).astype(f) if residual else None
    g = rng.uniform(0.0, 1.0, (n, Cexp)).astype(f) if gate else None
    if noexp:
        We, be = None, None
    return dict(X=X, We=We, be=be, Wd=Wd, bd=bd, Wp=Wp, bp=bp, R=R, gate=g)


def run_block(shape, n, ops, force=-1, variant=0, ksplit=0, dnull=False):
    """bh_debug_mbconv_block -> (dict of outputs, record, name)."""
    lib = CAT._lib()
    Cexp, Cout, Ho, Wo = shape[3], shape[4], shape[5], shape[6]
    se = shape[14]
    rc0, rec0, _ = CAT.plan(shape, force, variant)
    assert rc0 == 0, (rc0, lib.bh_last_error(), shape)
    tiles = int(rec0[2] * rec0[3])
    Y = None if se else np.empty((n, Ho, Wo, Cout), np.float32)
    D = np.empty((n * Ho * Wo * Cexp,), np.float32) if (se and not dnull) else None
    PP = np.empty((n, tiles, Cexp), np.float32) if se else None
    rec = np.zeros(24, np.int32)
    name = C.create_string_buffer(160)
    rc = lib.bh_debug_mbconv_block(0, _p(np.asarray(shape, np.int32)), n, _p(ops["X"]), _p(ops["We"]), _p(ops["be"]), _p(ops["Wd"]),
                                   _p(ops["bd"]), _p(ops["Wp"]), _p(ops["bp"]), _p(ops["R"]), _p(ops["gate"]), force, variant, ksplit,
                                   _p(Y), _p(D), _p(PP), _p(rec), name, 160)
    assert rc == 0, (rc, lib.bh_last_error(), shape)
    nm = name.value.decode()
    REACHED.add(nm)
    for what, a in (("Y", Y), ("D", D), ("pool_part", PP)):
        if a is not None:
            assert not (a.view(np.uint32) == UNWRITTEN).any(), (nm, what, "elements never written", shape)
    if D is not None:
        if shape[15]:     # blocked: [row tile of 16 pixels][Cexp / 16][16 rows][16 channels] -> NHWC
            D = D.reshape(n * Ho * Wo // 16, Cexp // 16, 16, 16).transpose(0, 2, 1, 3)
        D = np.ascontiguousarray(D).reshape(n, Ho, Wo, Cexp)
    return dict(Y=Y, D=D, PP=PP), rec, nm


# -----------------------------------------------------------------------------------------------------------------------------
# the reference and its tolerance
# -----------------------------------------------------------------------------------------------------------------------------
def _scale_exponent(max_abs):
    """kernels.hpp f16_scale_exponent"""
    if not (max_abs > 0.0) or not math.isfinite(max_abs):
        return 0
    s = 14 - math.frexp(float(max_abs))[1]
    return max(-60, min(60, s))


def plane_excess(Wt, prec, clamp21):
    """|w - what the f16 plane(s) hold| beyond the format's nominal precision, per weight, in float64: the planes hold w 2^s as
    hi = f16(v), lo = f16(v - hi) (api_plan.hip mb_prepare_weights); plain f16 reads hi alone."""
    if prec == 0 or Wt is None:
        return None
    s = _scale_exponent(float(np.abs(Wt).max()))
    if clamp21:
        s = max(-21, min(21, s))
    v = np.ldexp(Wt.astype(np.float32), s).astype(np.float32)
    with np.errstate(over="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    rep = hi.astype(np.float64) + (lo.astype(np.float64) if prec == 3 else 0.0)
    err = np.abs(np.ldexp(rep, -s) - Wt.astype(np.float64))
    nominal = (2.0 ** -11 if prec == 1 else 2.0 ** -22) * np.abs(Wt.astype(np.float64))
    return np.maximum(err - nominal, 0.0)


def reference(shape, ops):
    """O.mbconv64 and the propagated bounds e_E, e_D (gated where there is a gate), e_Y."""
    H, W, Cin, Cexp, Cout, Ho, Wo, pad_t, pad_l, KS, ST, act, prec, noexp = shape[:14]
    stem_c, stem_h, stem_w, stem_k, stem_s, stem_pt, stem_pl = shape[16:23]
    stem = (stem_k, stem_s, stem_pt, stem_pl, H, W) if stem_c else None
    ref = O.mbconv64(ops["X"], ops["We"], ops["be"], ops["Wd"], ops["bd"], ops["Wp"], ops["bp"], ops["R"], KS, ST, pad_t, pad_l, Ho, Wo,
                     act, noexp=bool(noexp), gate=ops["gate"], stem=stem)
    f = np.float64
    aWd, aWp = np.abs(ops["Wd"].astype(f)), np.abs(ops["Wp"].astype(f))
    if noexp:
        e_E = np.zeros_like(ref["E"])
    else:
        aA, aWe = np.abs(ref["A"]), np.abs(ops["We"].astype(f))
        e_E = _tau(prec, Cin) * 1.2 * (aA @ aWe + np.abs(ops["be"].astype(f))) + _eps_act(ref["preE"], act)
        dWe = plane_excess(ops["We"], prec, clamp21=(act == O.ACT_GELU_ERF))
        if dWe is not None and dWe.any():
            e_E = e_E + 1.2 * (aA @ dWe)
    dw = lambda t: O.depthwise64(t, aWd, KS, ST, pad_t, pad_l, Ho, Wo)
    e_D = 1.2 * (dw(e_E) + _tau(prec, KS * KS) * (dw(np.abs(ref["E"])) + np.abs(ops["bd"].astype(f)))) + _eps_act(ref["preD"], act)
    e_Dg = e_D if ops["gate"] is None else e_D * np.abs(ops["gate"].astype(f))[:, None, None, :]
    aR = 0.0 if ops["R"] is None else np.abs(ops["R"].astype(f))
    e_Y = e_Dg @ aWp + _tau(prec, Cexp) * (np.abs(ref["Dg"]) @ aWp + np.abs(ops["bp"].astype(f)) + aR)
    dWp = plane_excess(ops["Wp"], prec, clamp21=False)
    if dWp is not None and dWp.any():
        e_Y = e_Y + np.abs(ref["Dg"]) @ dWp
    ref.update(e_E=e_E, e_D=e_D, e_Y=e_Y)
    return ref


def _hold(got, want, tol, key, what):
    assert np.isfinite(got).all(), (what, "non-finite output")
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / np.maximum(tol, 1e-300)
    worst = float(ratio.max())
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if worst > 1.0:
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        pytest.fail(f"{what}: {int((ratio > 1).sum())} of {ratio.size} elements off, worst at {i}: got {got[i]!r} want {want[i]!r}, "
                    f"err {err[i]:.3e} > tol {tol[i]:.3e}")


def check(shape, n, ops, out, name, what):
    ref = reference(shape, ops)
    prec, se = shape[12], shape[14]
    key = (_family(shape, se), prec)
    what = f"{what} {name} shape {list(shape)} n {n}"
    if not se:
        _hold(out["Y"], ref["Y"], ref["e_Y"], key, what + " Y")
        return ref
    if out["D"] is not None:
        _hold(out["D"], ref["D"], ref["e_D"], key, what + " D")
    _hold(out["PP"].astype(np.float64).sum(axis=1), ref["Dsum"], ref["e_D"].sum(axis=(1, 2)), (key[0] + "_sums", prec), what + " pool sums")
    return ref


# -----------------------------------------------------------------------------------------------------------------------------
# the catalogue
# -----------------------------------------------------------------------------------------------------------------------------
def _run_case(r, c, seed):
    shape, n = c["shape"], c["n"]
    ops = operands(shape, n, c["residual"], c["gate"], seed)
    what = "entry %d %s %s" % (r["base"], CAT.ACT_NAMES[r["ACT"]], "+".join(sorted(c["tags"])))
    out, rec, name = run_block(shape, n, ops, r["base"], ksplit=c["ksplit"], dnull=c["dnull"])
    assert rec[0] == r["ci"] and name == "mbconv<%s,%d>" % (r["name"], c["se"]), (what, rec, name)
    check(shape, n, ops, out, name, what)
    if c["ksplit"]:
        assert rec[12] >= 2, (what, rec)
        # bit-stable across n: the first two segments alone
        ops2 = {k: (v[:2] if k in ("X", "R", "gate") and v is not None else v) for k, v in ops.items()}
        out2, rec2, _ = run_block(shape, 2, ops2, r["base"], ksplit=1)
        assert rec2[12] == rec[12] and (out2["Y"] == out["Y"][:2]).all(), (what, "the channel split's bits depend on n")
    if c["oversub"]:
        # the same three segments over and over, past the resident grid: every segment must come out as in the small launch
        n_big = CAT.oversub_segments(r, rec)
        reps = -(-n_big // n)
        big = {k: (np.concatenate([v] * reps)[:n_big] if k in ("X", "R", "gate") and v is not None else v) for k, v in ops.items()}
        outb, recb, _ = run_block(shape, n_big, big, r["base"])
        assert -(-n_big // rec[8]) * rec[2] * rec[3] > r["OCC"] * CAT.N_CU
        yb = outb["Y"]
        assert (yb[:n] == out["Y"]).all(), (what, "the first rows of the large launch differ from the small launch")
        for k in range(n):
            assert (yb[k::n] == out["Y"][k]).all(), (what, "segment %d of the large launch depends on its place" % k)
    return out, rec, name, ops




@pytest.mark.parametrize("act", CAT.ACTS, ids=lambda a: CAT.ACT_NAMES[a])
def test_every_instantiation_at_its_edges(act):
    """Each live row of the table in this activation's copy, forced, on every case of the catalogue (test_mbconv_block.py)."""
    rows = [r for r in CAT.table() if r["ACT"] == act]
    assert rows
    for i, r in enumerate(rows):
        if i % 25 == 0:
            print("  %s: row %d of %d, %.0f s" % (CAT.ACT_NAMES[act], i, len(rows), time.time() - T0), flush=True)
        cs = CAT.cases_for(r)
        assert cs, r["base"]
        for k, c in enumerate(cs):
            _run_case(r, c, seed=1000 * r["base"] + 10 * k + act)


@pytest.mark.parametrize("act", CAT.ACTS, ids=lambda a: CAT.ACT_NAMES[a])
def test_twins_give_the_same_bits(act):
    """The one-segment twin (mb_plan_twin) and the narrow-tile twin (mb_plan_narrow) of a planned entry give the block's bits
    (mb_plan_narrow's comment: a pixel's sums do not depend on the tile it is computed in); pass A's sums where
    mb_twin_sums_match says so."""
    seen_twin = seen_narrow = seen_sums = 0
    for r in (q for q in CAT.table() if q["ACT"] == act):
        for c in CAT.cases_for(r):
            if not ({"natural", "se_nhwc", "colth_low", "k_relaxed"} & c["tags"]):
                continue
            rc, rec, _ = CAT.plan(c["shape"], r["base"])
            if not (rec[13] or rec[14]):
                continue
            n = 3
            ops = operands(c["shape"], n, c["residual"], c["gate"], seed=77 + r["base"])
            base, _, _ = run_block(c["shape"], n, ops, r["base"])
            if rec[13] and (not c["se"] or rec[15]):
                tw, rect, nm = run_block(c["shape"], n, ops, r["base"], variant=1)
                assert rect[8] == 1 and rect[0] != rec[0]
                if c["se"]:
                    assert (tw["PP"] == base["PP"]).all() and (tw["D"] == base["D"]).all(), (r["base"], nm)
                    seen_sums += 1
                else:
                    assert (tw["Y"] == base["Y"]).all(), (r["base"], nm, "the one-segment twin's bits differ")
                seen_twin += 1
            if rec[14] and not c["se"]:
                nw, recn, nm = run_block(c["shape"], n, ops, r["base"], variant=2)
                assert recn[3] >= 2 and recn[0] != rec[0]
                assert (nw["Y"] == base["Y"]).all(), (r["base"], nm, "the narrow twin's bits differ")
                seen_narrow += 1
    assert seen_twin and seen_narrow and seen_sums, (seen_twin, seen_narrow, seen_sums)


# -----------------------------------------------------------------------------------------------------------------------------
# weight scales far from the usual: se, sp away from zero, the |se| <= 21 clamp
# -----------------------------------------------------------------------------------------------------------------------------
def _planned_rows(prec, act):
    """a plain expand row, a column-task row and a stride-2 row of this precision"""
    t = [r for r in CAT.table() if r["ACT"] == act and r["PREC"] == prec and r["KG"] and not r["STEM"]]
    picks = [next(r for r in t if not r["COLTH"] and r["ST"] == 1), next(r for r in t if r["COLTH"]), next(r for r in t if r["ST"] == 2)]
    return picks


@pytest.mark.parametrize("scales", [(2.0 ** 10, 2.0 ** -10, 2.0 ** -9), (2.0 ** -12, 2.0 ** 12, 2.0 ** 8), (2.0 ** -20, 2.0 ** 20, 2.0 ** -6)],
                         ids=["We*2^10_Wp*2^-9", "We*2^-12_Wp*2^8_past_the_clamp", "We*2^-20_Wp*2^-6_lo_subnormal"])
@pytest.mark.parametrize("prec", [0, 1, 3])
@pytest.mark.parametrize("act", CAT.ACTS, ids=lambda a: CAT.ACT_NAMES[a])
def test_weight_scales_far_from_the_usual(act, prec, scales):
    """We, Wp (and Wd the other way, so that D keeps its size) scaled by large powers of two: the plane exponents se and sp move far
    from their usual 13-15, for the GELU blocks past the |se| <= 21 clamp, where the hi + lo pair of the small weights loses bits
    (lo subnormal) -- the representation error, computed per weight, enters the bound (plane_excess); nothing else changes."""
    we, wd, wp = scales
    for r in _planned_rows(prec, act):
        c = next(q for q in CAT.cases_for(r) if "natural" in q["tags"])
        ops = operands(c["shape"], 2, True, False, seed=5 + r["base"], we_scale=we, wd_scale=wd, wp_scale=wp)
        if prec and act == O.ACT_GELU_ERF and we < 2.0 ** -11:
            assert _scale_exponent(float(np.abs(ops["We"]).max())) > 21          # the clamp is in force
        out, rec, name = run_block(c["shape"], 2, ops, r["base"])
        check(c["shape"], 2, ops, out, name, "scales %g %g %g entry %d" % (we, wd, wp, r["base"]))


# -----------------------------------------------------------------------------------------------------------------------------
# the planner's own choice on blocks nobody shaped by hand
# -----------------------------------------------------------------------------------------------------------------------------
def _model_blocks(m):
    """(shape without precision, se) of every inverted-residual block of a synth model, taken out of its network."""
    from birda_amd import modelfile as mf
    out = []
    L = m.layers
    for i, d in enumerate(L):
        if d.op != mf.OP_DWCONV or d.kh != d.kw or d.sh != d.sw:
            continue
        e = L[i - 1] if i > 0 and L[i - 1].op == mf.OP_PWCONV and d.in_tensor == i else None
        stem = L[i - 1] if i > 0 and L[i - 1].op == mf.OP_CONV and L[i - 1].in_layout == 1 and d.in_tensor == i else None
        se = i + 5 < len(L) and L[i + 1].op == mf.OP_GAP
        p = L[i + 5] if se else (L[i + 1] if i + 1 < len(L) else None)
        if p is None or p.op != mf.OP_PWCONV or p.act != mf.ACT_NONE or d.act not in CAT.ACTS:
            continue
        if e is not None and e.act != d.act:
            continue
        st = None
        if stem is not None:
            if stem.kh != 3 or stem.act != d.act:
                continue
            st = (stem.cin, stem.in_h, stem.in_w, 3, stem.sh, stem.pad_t, stem.pad_l)
            cin = 9 * stem.cin
        else:
            cin = e.cin if e is not None else d.cout
        out.append((d.in_h, d.in_w, cin, d.cout, p.cout, d.out_h, d.out_w, d.pad_t, d.pad_l, d.kh, d.sh, d.act, int(e is None and stem is None), int(se),
                    st, p.res_tensor != mf.NO_TENSOR))
    return out


def test_planner_chosen_blocks_of_plans_nobody_wrote():
    """The blocks of synth.random_plan seeds and of the probe plans, taken out of their networks and run alone with the planner's
    own choice (force_cfg = -1) in f32 and split f16: the relaxed pass on shapes nobody wrote by hand."""
    from birda_amd import synth
    seen, ran, relaxed = set(), 0, 0
    plans = [synth.random_plan(s) for s in range(12)] + [synth.random_plan(1000, big=True)]
    for name in ("mobilenet_v2", "b0_plus8"):
        P = synth.probe_plan(name, se=(name == "b0_plus8"))
        P.update(classes=16, head=64)          # (the blocks are what is wanted; a 6 522-class head only costs time)
        plans.append(P)
    for P in plans:
        m = synth.build_model("custom", plan=P)
        for blk in _model_blocks(m):
            if blk in seen:
                continue
            seen.add(blk)
            H, W, cin, cexp, cout, Ho, Wo, pt, pl, ks, st, act, noexp, se, stem, res = blk
            for prec in (3, 0):
                shape = CAT.make_shape(H, W, cin, cexp, cout, Ho, Wo, pt, pl, ks, st, act, prec, noexp, se, 0, stem)
                rc, rec, _ = CAT.plan(shape, -1)
                if rc != 0:
                    continue            # (left to the layer kernels by the planner: not this module's subject)
                n = 2
                ops = operands(shape, n, res and not se, False, seed=len(seen) * 7 + prec)
                out, rec, nm = run_block(shape, n, ops, -1)
                check(shape, n, ops, out, nm, "planner's choice")
                ran += 1
                relaxed += int(not noexp and not stem and rec[5] > -(-cin // (32 if prec else 16)))
    assert ran >= 40 and relaxed >= 5, (ran, relaxed)


def test_refused_shapes_launch_nothing():
    """A shape the planner refuses comes back BH_ERR_UNSUPPORTED from the launching entry too, with no output touched."""
    r = next(q for q in CAT.table() if q["ACT"] == 4 and q["PREC"] == 3 and q["KG"] == 1 and not q["STEM"] and not q["COLTH"])
    c = CAT.cases_for(r)[0]
    shape = list(c["shape"])
    shape[4] = 16 * r["WN"] * r["NT"] + 16
    ops = operands(shape, 1, False, False, seed=1)
    Y = np.full((1, shape[5], shape[6], shape[4]), 123.0, np.float32)
    lib = CAT._lib()
    rc = lib.bh_debug_mbconv_block(0, _p(np.asarray(shape, np.int32)), 1, _p(ops["X"]), _p(ops["We"]), _p(ops["be"]), _p(ops["Wd"]), _p(ops["bd"]),
                                   _p(ops["Wp"]), _p(ops["bp"]), None, None, r["base"], 0, 0, _p(Y), None, None, None, None, 0)
    assert rc == CAT.BH_ERR_UNSUPPORTED and b"project tiles" in lib.bh_last_error()
    assert (Y == 123.0).all()


# -----------------------------------------------------------------------------------------------------------------------------
# completeness (runs last: pytest keeps the file's order)
# -----------------------------------------------------------------------------------------------------------------------------
def test_every_shipped_instantiation_ran():
    """REACHED == shipped: every live row x activation, and pass A wherever it is instantiated -- no exemptions."""
    shipped = CAT.shipped_names()
    ran = {n for n in REACHED}
    print("\nworst err / tolerance per (family, precision):")
    for k in sorted(WORST):
        print("  %-22s prec %d  %.3f" % (k[0], k[1], WORST[k]))
    print("instantiations shipped %d, ran %d; module wall time %.0f s" % (len(shipped), len(ran & shipped), time.time() - T0))
    assert not (shipped - ran), ("never launched", sorted(shipped - ran)[:20], len(shipped - ran))
    assert not (ran - shipped), ("ran but not in the table", sorted(ran - shipped)[:20])
