"""The shape catalogue tests/test_mbconv_block_gpu.py runs every shipped instantiation of the fused MBConv kernel on, and its
completeness, checked here without a GPU through the host-only planning entry bh_debug_mbconv_plan
(include/birda_hip_block_debug.h): for every live row of mbconv_cfgs.inc x every activation copy the generator below derives,
from the row's own template arguments, at least one shape per applicable edge that mb_plan accepts ON THAT ROW --

    natural        the row's own k steps, tile height and width, Cout at the row's maximum 16 WN NT_W, a residual, n = 3
    partial_tiles  Ho, Wo not multiples of TH, 2^TWL; with it cexp_partial (Cexp % CE != 0), cout_partial (Cout % 16 != 0), n = 1
    s2_even / s2_odd / s2_odd_asym   stride-2 rows: an even image with TF's SAME padding (pad_b = pad_t + 1), an odd image with
                   symmetric padding, an odd image with one row / column less padding on top / left than below / right
    k_relaxed      Cin giving fewer k steps than the row's KG (rows of KG >= 2; the relaxed match), k_partial for KG = 1
    colth_exact / colth_low   column-task rows: the image at COLTH rows and one lower
    s2seg_odd_n    S = 2 rows: n odd, the last workgroup has one live segment
    oversub        n large enough that the launch exceeds the resident grid (OCC workgroups on each of 256 CUs)
    stem           stem rows: the planar spectrogram with the row's channel count, stem stride 2 and 1
    noexp / gate   no-expand rows, plain and with the squeeze-excite gate of the one-launch form
    ksplit         the channel split BH_FLAG_LOW_LATENCY gives a block of six chunks or more
    se_nhwc / se_sums_only / se_blocked   pass A (rows that have the instantiation): D in NHWC, no D at all, D blocked where
                   pw_gemm16_gated_wants_blocked chooses it (f16 modes, 6-15 project tiles)

-- and the diagnostic refuses, before any launch, what mb_try_th refuses."""
import ctypes as C
import functools

import numpy as np
import pytest

FIELDS = "KS ST CE KG RT NCS WM WN MT NT TWL XBL S OCC STEM PREC PERSIST ACT COLTH".split()
ACTS = (4, 3, 2)                  # GELU, swish, ReLU6 (the model file's codes): the three copies of the table
ACT_NAMES = {4: "gelu", 3: "swish", 2: "relu6"}
N_CU = 256
BH_ERR_INVALID, BH_ERR_UNSUPPORTED = -1, -6


def _lib():
    from birda_amd import _lib
    return _lib.load()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_shape(H, W, Cin, Cexp, Cout, Ho, Wo, pad_t, pad_l, KS, ST, act, prec, noexp=0, se=0, dblk=0, stem=None):
    """The 23 int32 of include/birda_hip_block_debug.h; stem = (c, h, w, k, s, pad_t, pad_l)."""
    return [H, W, Cin, Cexp, Cout, Ho, Wo, pad_t, pad_l, KS, ST, act, prec, int(noexp), int(se), int(dblk)] + list(stem or (0,) * 7)


def plan(shape, force_cfg=-1, variant=0):
    """bh_debug_mbconv_plan: (return code, the 24-int record, the instantiation's name)."""
    rec = np.zeros(24, np.int32)
    name = C.create_string_buffer(160)
    rc = _lib().bh_debug_mbconv_plan(_p(np.asarray(shape, np.int32)), force_cfg, variant, _p(rec), name, 160)
    return rc, rec, name.value.decode()


@functools.lru_cache(maxsize=None)
def table():
    """Every live instantiation the library ships: a list of dicts (the row's template arguments, TH, base index, full index,
    has_se), enumerated through bh_mb_config_name; rows that are not part of the build (KS == 0) skipped."""
    lib = _lib()
    names = []
    while True:
        buf = C.create_string_buffer(128)
        if lib.bh_mb_config_name(len(names), buf, 128) <= 0:
            break
        names.append(buf.value.decode())
    assert names and len(names) % 3 == 0
    nbase = len(names) // 3
    out = []
    for ci, nm in enumerate(names):
        r = dict(zip(FIELDS, (int(v) for v in nm.split(","))))
        if r["KS"] == 0:
            continue
        _, rec, _ = plan(make_shape(*([0] * 11), r["ACT"], r["PREC"]), ci % nbase)      # (refused; the row's facts come back)
        r.update(TH=int(rec[7]), has_se=bool(rec[6]), base=ci % nbase, ci=ci, name=nm, nbase=nbase)
        assert r["TH"] > 0, nm
        out.append(r)
    return out


def shipped_names():
    """The instantiations as the diagnostic names them: every live row, and pass A where it is instantiated."""
    s = set()
    for r in table():
        s.add("mbconv<%s,0>" % r["name"])
        if r["has_se"]:
            s.add("mbconv<%s,1>" % r["name"])
    return s


# -----------------------------------------------------------------------------------------------------------------------------
# the generator
# -----------------------------------------------------------------------------------------------------------------------------
def _geom(r, Ho, Wo, mode="same"):
    """(H, W, pad_t, pad_l) of an image the row's depthwise convolution turns into Ho x Wo."""
    KS, ST = r["KS"], r["ST"]
    if ST == 1:
        return Ho, Wo, (KS - 1) // 2, (KS - 1) // 2
    if mode == "odd":                 # 2 Ho - 1 rows: SAME padding is symmetric
        return ST * Ho - 1, ST * Wo - 1, (KS - 1) // 2, (KS - 1) // 2
    if mode == "odd_asym":            # ... one row / column less above / left, one more below / right (an exporter's explicit pads)
        return ST * Ho - 1, ST * Wo - 1, (KS - 1) // 2 - 1, (KS - 1) // 2 - 1
    return ST * Ho, ST * Wo, (KS - ST) // 2, (KS - ST) // 2     # an even image, TF's SAME: pad_b = pad_t + 1


def _case(r, tags, Ho, Wo, Cin=None, Cexp=None, Cout=None, n=3, residual=True, mode="same", H=None, gate=False, se=0, dblk=0,
          dnull=False, ksplit=0, stem_s=2, oversub=False, th=None):
    step = 32 if r["PREC"] else 16
    CE, KG = r["CE"], r["KG"]
    Hh, W, pad_t, pad_l = _geom(r, Ho, Wo, mode)
    if H is not None:
        Hh = H
    Cexp = 2 * CE if Cexp is None else Cexp
    Cout = 16 * r["WN"] * r["NT"] if Cout is None else Cout
    stem = None
    noexp = KG == 0
    if r["STEM"]:
        c = r["STEM"]
        Cin = 9 * c
        if stem_s == 2:               # an odd spectrogram, symmetric SAME padding
            stem = (c, 2 * Hh - 1, 2 * W - 1, 3, 2, 1, 1)
        else:
            stem = (c, Hh, W, 3, 1, 1, 1)
    elif noexp:
        Cin = Cexp
    elif Cin is None:
        Cin = step * KG
    shape = make_shape(Hh, W, Cin, Cexp, Cout, Ho, Wo, pad_t, pad_l, r["KS"], r["ST"], r["ACT"], r["PREC"], noexp, se, dblk, stem)
    return dict(tags=set(tags), shape=shape, n=n, residual=bool(residual and not se), gate=gate, se=se, dblk=dblk, dnull=dnull,
                ksplit=ksplit, oversub=oversub, th=th)


def _accepted(r, case):
    rc, rec, _ = plan(case["shape"], r["base"])
    return rc == 0 and rec[0] == r["ci"] and (case["th"] is None or rec[1] == case["th"])


def _first(r, cands):
    for c in cands:
        if c is not None and _accepted(r, c):
            return c
    return None


def applicable_tags(r):
    t = {"natural", "partial_tiles", "cexp_partial", "cout_partial", "cout_max", "residual", "no_residual", "n1", "n3", "oversub", "ksplit"}
    if r["ST"] == 2:
        t |= {"s2_even", "s2_odd", "s2_odd_asym"}
    if r["KG"] >= 2 and not r["STEM"]:
        t.add("k_relaxed")
    if r["KG"] == 1 and not r["STEM"]:
        t.add("k_partial")
    if r["COLTH"]:
        t |= {"colth_exact", "colth_low"}
    if r["S"] == 2:
        t.add("s2seg_odd_n")
    if r["STEM"]:
        t |= {"stem", "stem_s1"}
    if r["KG"] == 0:
        t |= {"noexp", "gate"}
    if r["STEM"]:
        t.add("gate")
    if r["has_se"]:
        t |= {"se_nhwc", "se_sums_only"}
        if r["PREC"] != 0 and r["WN"] * r["NT"] >= 6:
            t.add("se_blocked")
    return t


@functools.lru_cache(maxsize=None)
def _cases_cached(ci):
    r = next(q for q in table() if q["ci"] == ci)
    TH, TW, CE, KG = r["TH"], 1 << r["TWL"], r["CE"], r["KG"]
    step = 32 if r["PREC"] else 16
    cout_max = 16 * r["WN"] * r["NT"]
    col = r["COLTH"]
    full_h = col if col else 2 * TH
    part_h = col if col else (2 * TH - 1 if TH > 1 else 3)
    base_tags = ["natural", "cout_max", "residual", "n3"] + (["colth_exact"] if col else []) + (["s2seg_odd_n"] if r["S"] == 2 else []) + \
                (["s2_even"] if r["ST"] == 2 else []) + (["stem"] if r["STEM"] else []) + (["noexp"] if KG == 0 else [])
    out = []

    def add(*cands):
        c = _first(r, cands)
        if c is not None:
            out.append(c)
        return c

    # the row's natural shape: two tile rows and columns where the row tiles, else one
    nat_th = col or TH
    add(_case(r, base_tags, full_h, 2 * TW, th=nat_th), _case(r, base_tags, nat_th, 2 * TW, th=nat_th), _case(r, base_tags, nat_th, TW, th=nat_th))
    def sized(tags, w_pref, **kw):
        """the case at the preferred size, else (rows whose tile is the whole image) at one tile with a partial last column"""
        sizes = [(part_h, w_pref), (part_h, TW - 3), (col or TH, TW - 3), (col or max(TH - 1, 1), TW - 3)]
        hfix = kw.pop("hfix", None)
        return add(*[_case(r, tags, (hfix or h), w, H=hfix, **kw) for (h, w) in sizes])

    # last tiles partly outside the image, a partial last chunk, a partial last project tile; one segment, no residual
    ptags = ["partial_tiles", "cexp_partial", "cout_partial", "no_residual", "n1"] + (["colth_exact"] if col else [])
    sized(ptags, 2 * TW - 3, Cexp=2 * CE - 4, Cout=cout_max - 4, n=1, residual=False)
    if r["ST"] == 2:
        sized(["s2_odd", "partial_tiles"], TW + 3, Cexp=CE + 8, n=2, mode="odd")
        sized(["s2_odd_asym", "partial_tiles", "cout_partial"], TW + 1, Cexp=CE + 4, Cout=max(cout_max - 12, 4), n=2, residual=False, mode="odd_asym")
    if KG >= 2 and not r["STEM"]:
        sized(["k_relaxed", "partial_tiles"], TW + 5, Cin=step * (KG - 1) - 4, Cexp=CE + 12, n=2)
    if KG == 1 and not r["STEM"]:
        sized(["k_partial", "partial_tiles"], TW + 5, Cin=step - 4, Cexp=CE + 12, n=2)
    if col:
        sized(["colth_low", "partial_tiles"], TW + 5, Cexp=CE + 4, n=3, hfix=col - 1)
    if r["STEM"]:
        sized(["stem", "stem_s1", "partial_tiles"], 2 * TW - 5, n=2, stem_s=1, residual=False)
        sized(["stem", "gate", "partial_tiles"], TW + 2, n=2, gate=True)
    if KG == 0:
        sized(["noexp", "gate", "partial_tiles"], TW + 7, Cexp=2 * CE - 8, n=3, gate=True)
    # six chunks: the depth BH_FLAG_LOW_LATENCY splits (api.hip mb_ksplit_of); one tile, n = 2 and n = 5 must agree bit for bit
    add(_case(r, ["ksplit"], col or TH, TW, Cexp=6 * CE, Cout=min(cout_max, 32), n=5, ksplit=1))
    # a launch past the resident grid: few channels, many segments; its n = 3 twin is the same case with oversub unset
    tiles_small = _case(r, ["oversub"], full_h, 2 * TW, Cin=None if (KG <= 1 or r["STEM"]) else 4, Cexp=CE + 4, Cout=8, n=3, oversub=True)
    one_tile = _case(r, ["oversub"], col or TH, TW, Cin=None if (KG <= 1 or r["STEM"]) else 4, Cexp=CE + 4, Cout=8, n=3, oversub=True)
    if KG == 1 and not r["STEM"]:
        tiles_small["shape"][2] = one_tile["shape"][2] = 4
    add(tiles_small, one_tile)
    if r["has_se"]:
        add(_case(r, ["se_nhwc"] + (["s2seg_odd_n"] if r["S"] == 2 else []), full_h, 2 * TW, n=3, se=1),
            _case(r, ["se_nhwc"] + (["s2seg_odd_n"] if r["S"] == 2 else []), col or TH, TW, n=3, se=1))
        sized(["se_sums_only", "partial_tiles", "cexp_partial"], 2 * TW - 3, Cexp=2 * CE - 4, n=2, se=1, dnull=True)
        if r["PREC"] != 0 and r["WN"] * r["NT"] >= 6:
            cout = min(cout_max, 16 * 15)
            add(*[_case(r, ["se_blocked"], h, w, Cexp=3 * CE if (3 * CE) % 16 == 0 else 2 * CE, Cout=cout, n=2, se=1, dblk=1)
                  for (h, w) in ((full_h, 2 * TW), (col or TH, TW), (col or TH, 2 * TW), (2, 8), (1, 16), (4, 4))])
    return out


def cases_for(r):
    """The catalogue's cases of one instantiation (a row of table()), every one accepted by mb_plan on that row."""
    return _cases_cached(r["ci"])


def oversub_segments(r, rec):
    """Segments that make the launch exceed the resident grid: more workgroups than OCC on each of 256 CUs."""
    tiles = int(rec[2]) * int(rec[3])
    wgs = r["OCC"] * N_CU + 1
    return -(-wgs // tiles) * r["S"] + 1


# -----------------------------------------------------------------------------------------------------------------------------
# the tests
# -----------------------------------------------------------------------------------------------------------------------------
def test_table_is_the_documented_size():
    t = table()
    assert len(t) % 3 == 0
    per_act = {a: [r for r in t if r["ACT"] == a] for a in ACTS}
    assert len({len(v) for v in per_act.values()}) == 1 and len(per_act[4]) >= 150
    # (the three copies are one list)
    for a in ACTS[1:]:
        assert [{k: v for k, v in r.items() if k not in ("ACT", "ci", "name")} for r in per_act[a]] == \
               [{k: v for k, v in r.items() if k not in ("ACT", "ci", "name")} for r in per_act[4]]
    assert len(shipped_names()) == len(t) + sum(r["has_se"] for r in t)


def test_catalogue_covers_every_instantiation_at_every_applicable_edge():
    missing = []
    n_cases = 0
    for r in table():
        cs = cases_for(r)
        n_cases += len(cs)
        have = set().union(*[c["tags"] for c in cs]) if cs else set()
        for c in cs:
            rc, rec, name = plan(c["shape"], r["base"])
            assert rc == 0 and rec[0] == r["ci"] and name == "mbconv<%s,%d>" % (r["name"], c["se"]), (r["base"], c)
            if "natural" in c["tags"]:
                assert rec[5] == r["KG"] and rec[1] == (r["COLTH"] or r["TH"]), (r["base"], rec)
            if "partial_tiles" in c["tags"]:
                assert c["shape"][5] % rec[1] or c["shape"][6] % (1 << r["TWL"]), (r["base"], c)
            if "k_relaxed" in c["tags"]:
                assert -(-c["shape"][2] // (32 if r["PREC"] else 16)) < r["KG"]
            if "ksplit" in c["tags"]:
                assert rec[12] >= 2, (r["base"], rec)
            if "oversub" in c["tags"]:
                n_big = oversub_segments(r, rec)
                assert -(-n_big // r["S"]) * rec[2] * rec[3] > r["OCC"] * N_CU
            assert 0 < rec[11] <= 160 * 1024, (r["base"], rec[11])       # LDS
            if c["se"]:
                assert rec[6] == 1
            if c["dblk"]:
                assert rec[19] == 1, (r["base"], c)
        lack = applicable_tags(r) - have
        if lack:
            missing.append((r["base"], ACT_NAMES[r["ACT"]], sorted(lack)))
    assert not missing, "%d instantiations lack a shape: %s" % (len(missing), missing[:40])
    print("catalogue: %d instantiations, %d cases" % (len(table()), n_cases))


def _row(**want):
    for r in table():
        if all(r[k] == v for k, v in want.items()):
            return r
    raise AssertionError(want)


def test_diagnostic_refuses_what_the_planner_refuses():
    """On the host-only entry, before any launch: the wrong KS / ST for the forced row, Cin % 4, Cexp % 4, more project tiles than
    the row has, a wrong activation copy, the 2^24 offset limit just above (and acceptance just below); and arguments no block
    can have are BH_ERR_INVALID."""
    lib = _lib()
    r = _row(KS=3, ST=1, PREC=3, STEM=0, COLTH=0, S=1, KG=1, ACT=4)
    good = cases_for(r)[0]
    assert plan(good["shape"], r["base"])[0] == 0

    def refused(shape, force, why=None):
        rc, rec, _ = plan(shape, force)
        assert rc == BH_ERR_UNSUPPORTED, (rc, shape)
        assert rec[0] == -1
        msg = lib.bh_last_error().decode()
        assert "refused by" in msg, msg
        if why:
            assert why in msg, msg

    def edit(shape, **kv):
        names = "H W Cin Cexp Cout Ho Wo pad_t pad_l KS ST act prec noexp se dblk".split()
        s = list(shape)
        for k, v in kv.items():
            s[names.index(k)] = v
        return s

    s = good["shape"]
    refused(edit(s, KS=5, pad_t=2, pad_l=2), r["base"])
    refused(edit(s, ST=2, Ho=s[5] // 2, Wo=s[6] // 2), r["base"])
    refused(edit(s, Cin=s[2] - 2), r["base"])
    refused(edit(s, Cexp=s[3] - 2), r["base"])
    refused(edit(s, prec=0), r["base"])
    refused(edit(s, Cout=16 * r["WN"] * r["NT"] + 4), r["base"], "project tiles")
    refused(edit(s, Cin=64), r["base"], "k steps")
    # the 2^24 offset limit: S H W Cin (and S Ho Wo Cout) must stay below it -- just below is planned, at it is not
    W24 = (1 << 24) // (64 * 32)
    below = edit(s, H=64, Ho=64, W=W24 - 1, Wo=W24 - 1, Cin=32, Cout=16)
    assert (below[0] * below[1] * below[2]) < (1 << 24) <= 64 * W24 * 32
    assert plan(below, r["base"])[0] == 0, lib.bh_last_error()
    refused(edit(s, H=64, Ho=64, W=W24, Wo=W24, Cin=32, Cout=16), r["base"])
    out24 = edit(s, H=64, Ho=64, W=W24, Wo=W24, Cin=16, Cout=32)        # ... and S Ho Wo Cout
    refused(out24, r["base"])
    assert plan(edit(out24, Cout=28), r["base"])[0] == 0, lib.bh_last_error()
    # (LDS over 160 KB: a tile's LDS is a function of the row and the tile height alone, and mb_try lowers the height until the tile
    #  fits, so no shape makes a shipped row refuse for it; what holds instead is that every plan the catalogue makes stays within
    #  160 KB -- test_catalogue_covers_every_instantiation_at_every_applicable_edge)
    # (the planner's own choice refuses a block nothing fits: a 7x7 depthwise)
    refused(edit(s, KS=7, pad_t=3, pad_l=3), -1)
    # arguments no block can have
    for bad in (edit(s, H=0), edit(s, prec=2), edit(s, noexp=1, Cexp=s[3] + 16), edit(s, dblk=1), edit(s, Ho=s[0] + s[7] + 1)):
        assert plan(bad, r["base"])[0] == BH_ERR_INVALID, bad
    assert plan(s, r["base"], 3)[0] == BH_ERR_INVALID
    # a twin the entry does not have
    rc, rec, _ = plan(s, r["base"], 1)
    assert rc == (0 if plan(s, r["base"])[1][13] else BH_ERR_UNSUPPORTED)


def test_forced_plan_reports_the_row_it_ran():
    """The record names the full index (activation copy included) and the planner's own choice agrees with a forward pass's for a
    block of the BirdNET stack: 16 -> 96 -> 24 stride 2 at 48x256 in split f16 is entry 48."""
    rc, rec, name = plan(make_shape(48, 256, 16, 96, 24, 24, 128, 0, 0, 3, 2, 4, 3))
    assert rc == 0, _lib().bh_last_error()
    nbase = table()[0]["nbase"]
    assert rec[0] % nbase == 48 and name.startswith("mbconv<3,2,16,1,") and name.endswith(",0>")
    assert rec[2] == 24 // rec[1] and rec[3] == 128 // 16 and rec[4] == 6
