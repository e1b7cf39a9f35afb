"""The catalogue tests/test_gate_layers_gpu.py runs the squeeze-excite gate (three forms: se_gate_kernel; se_hidden_kernel +
se_gate16_kernel; se_pool_kernel + two launch_pw_gemm) and the plain f32 layer kernels (dwconv_kernel<KS,ST>, conv_direct_kernel<NC>,
gap_kernel, scale_kernel) on, checked here without a device:

* every case is what it claims.  The small host formulas of kernels_conv.hip / api.hip are restated in Python (se_hidden_shape, crp,
  lanes, nparts, the grid caps, se_gate_form), as tests/test_mbconv_block.py restates the planner, and each case's claim ("lanes 10,
  240 of 256 threads pool", "18 slices: a second 16-deep batch", "total > cap * 256") is asserted from them;
* the float64 references (oracle.se_gate64, direct_conv64, depthwise64) fit the tolerance.  The tolerance has no constants of its
  own: tau = _tau(0, K), the slope 1.2 and eps_act of tests/test_layer_gemm_gpu.py, propagated stage by stage in float64,

      dwconv / conv_direct   tau(K) 1.2 (|W| (*) |X| + |b|) + eps_act(pre),   K = KS KS / kh kw cin
      gap                    tau(P) mean|x|
      scale                  2^-23 |x g|                                        (one rounding)
      gate   e_pool = tau(tiles) sum_t |part| / P
             e_H    = 1.2 (|W1|^T e_pool + tau(C) (|pooled| |W1| + |b1|)) + eps_act(preH)
             e_G    = s2  (|W2|^T e_H    + tau(Cr) (|H| |W2| + |b2|))     + eps_act(preG),   s2 = 0.25 (sigmoid) or 1 (none)

  tau was set for MFMA GEMMs and these kernels are serial f32 FMA chains in a documented order, so each kernel's summation order
  is emulated here in numpy float32 (sequential; the same lanes, slices, parts and batches as the comments in kernels_conv.hip
  state; an FMA is one rounding of the float64 product-sum; activations exact) and must stay within HALF of the tolerance at every
  element of every case.  (The two GEMMs of the three-launch form run on the MFMA, whose order inside an instruction is not
  documented: they are emulated as one sequential chain over K, the longest chain the product could be.)
  The tap stage of three cases did not fit: dw5s1_7x9_c20_none (0.73 of the tolerance), dw5s2_7x9_c20_none (0.55) and
  cd_3x3s2_3to32 (0.54) -- 25 and 27 roundings of partial sums that sit near a bias of 7.5, each up to 2^-24 of the bound.  The
  tap stage of these three cases, and of no other, takes the rigorous bound K 2^-24 (|W| (*) |X| + |b|) of its chain in place of
  tau(K): RIGOROUS below.  Every other case, the other 5x5 depthwise and K >= 25 stem cases included, is held to tau(K); no stage
  of any gate case needed the rigorous bound.
* the tolerance still tells right from wrong: for every case each applicable mutation of the float64 reference (last tile dropped,
  last channel of a slice dropped, b1 omitted, two segments exchanged, 1/P taken with tiles where the two differ, last tap of the
  window dropped, the neighbouring segment's gate row) moves at least one element by more than 4x its tolerance."""
import functools
import math
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_layer_gemm_gpu import _eps_act, _tau                     # noqa: E402  (the per-GEMM tolerances, shared)

f32, f64 = np.float32, np.float64
OP_CONV, OP_DWCONV, OP_GAP, OP_SCALE = 1, 2, 4, 6                   # model.hpp Op
BH_ERR_INVALID, BH_ERR_UNSUPPORTED = -1, -6
# (case name, stage) that take K 2^-24 sum|terms| instead of tau(K) x sum|terms|: the emulation of these alone passed half of tau
RIGOROUS = {("dw5s1_7x9_c20_none", "taps"), ("dw5s2_7x9_c20_none", "taps"), ("cd_3x3s2_3to32", "taps")}

# ---------------------------------------------------------------------------------------------------------------------------------
# the host formulas, restated
# ---------------------------------------------------------------------------------------------------------------------------------
SE_SG, SE_RB, BH_SE_GATE16_MIN = 16, 32, 577
DW_CAP_BLOCKS = SCALE_CAP_BLOCKS = 256 * 64
CONV_CAP_BLOCKS = 256 * 32


def se_hidden_shape(C, Cr):
    """kernels_conv.hip se_hidden_shape -> (slice, slices)"""
    sl = 256
    while sl > 64 and sl * Cr > SE_RB * 256:
        sl >>= 1
    while sl < 256 and -(-C // sl) * Cr > C:
        sl <<= 1
    return sl, -(-C // sl)


def se_gate16_supports(C, Cr):
    return C >= 1 and 1 <= Cr <= 256 and se_hidden_shape(C, Cr)[1] * Cr <= C


def se_gate_supports(C, Cr):
    return C >= 1 and 1 <= Cr <= 256 and (C + 256 + Cr) * 4 <= 64 * 1024


def se_gate_form(C, Cr):
    """api.hip se_gate_form"""
    if C >= BH_SE_GATE16_MIN and se_gate16_supports(C, Cr):
        return 1
    if C > 576:
        return 2
    return 0 if se_gate_supports(C, Cr) else -1


def crp_of(Cr):
    """launch_se_gate: the power of two >= Cr, at least 4"""
    crp = 4
    while crp < Cr:
        crp <<= 1
    return crp


def lanes_of(C, tiles):
    """se_gate_kernel: threads sharing the tiles of one channel"""
    return 256 // C if C <= 128 and tiles >= 8 else 1


def dw_supports(kh, kw, sh, sw, c):
    return c % 4 == 0 and kh == kw and sh == sw and kh in (3, 5) and sh in (1, 2)


def conv_direct_supports(kh, kw, cin, cout):
    return cout % 4 == 0 and kh * kw * cin * cout * 4 <= 64 * 1024


FORM_KERNELS = {0: "se_gate_kernel", 1: "se_hidden_kernel+se_gate16_kernel", 2: "se_pool_kernel+pw_gemm_kernel"}
EVERY_KERNEL = {"dwconv_kernel<3,1>", "dwconv_kernel<3,2>", "dwconv_kernel<5,1>", "dwconv_kernel<5,2>", "conv_direct_kernel<NC=8>",
                "conv_direct_kernel<NC=4>", "gap_kernel", "scale_kernel", "se_gate_kernel", "se_hidden_kernel", "se_gate16_kernel",
                "se_pool_kernel", "pw_gemm_kernel"}

# ---------------------------------------------------------------------------------------------------------------------------------
# the gate cases
# ---------------------------------------------------------------------------------------------------------------------------------
ACT1S = (O.ACT_RELU, O.ACT_SWISH, O.ACT_GELU_ERF)
ACT2S = (O.ACT_SIGMOID, O.ACT_NONE)


def _g(name, form, C, Cr, tiles, n=3, P=None, claim=None):
    return dict(name=name, form=form, C=C, Cr=Cr, tiles=tiles, n=n, P=7 * tiles + 3 if P is None else P, claim=claim or {})


GATE_CASES = [
    # se_gate_kernel: the pool's lane split
    _g("g0_c24_t13_lanes10", 0, 24, 8, 13, claim=dict(lanes=10, pooling_threads=240, tiles_mod_lanes=3)),
    _g("g0_c96_t8_lanes2", 0, 96, 24, 8, claim=dict(lanes=2, pooling_threads=192)),
    _g("g0_c128_t8_exact", 0, 128, 32, 8, claim=dict(lanes=2, pooling_threads=256)),
    _g("g0_c96_t7_serial", 0, 96, 24, 7, claim=dict(lanes=1)),
    _g("g0_c144_t9_nolanes", 0, 144, 36, 9, claim=dict(lanes=1)),
    _g("g0_c260_wraps", 0, 260, 12, 4, claim=dict(channel_rounds=2)),
    _g("g0_c576_wraps", 0, 576, 24, 4, claim=dict(channel_rounds=3)),
    # ... its hidden split
    _g("g0_cr1", 0, 32, 1, 8, claim=dict(crp=4, nparts=64)),
    _g("g0_cr4_c24_empty_slices", 0, 24, 4, 13, claim=dict(crp=4, nparts=64, empty_parts=40)),
    _g("g0_cr6", 0, 48, 6, 4, claim=dict(crp=8, nparts=32)),
    _g("g0_cr48", 0, 192, 48, 4, claim=dict(crp=64, nparts=4)),
    _g("g0_cr129_one_slice", 0, 260, 129, 4, claim=dict(crp=256, nparts=1)),
    _g("g0_cr256", 0, 512, 256, 4, claim=dict(crp=256, nparts=1)),
    _g("g0_c24_n1", 0, 24, 8, 13, n=1),
    _g("g0_c260_n1", 0, 260, 12, 4, n=1),
    # the two sixteen-segment launches
    _g("g1_c580_cr24", 1, 580, 24, 4, claim=dict(slice=256, slices=3, last_slice=68, column_blocks=3, last_block=68)),
    _g("g1_c816_cr34", 1, 816, 34, 4, claim=dict(slice=128, slices=7, nparts=7, idle_threads=18)),
    _g("g1_c1024_cr256_full", 1, 1024, 256, 4, n=17, claim=dict(slice=256, slices=4, scratch_slack=0, nparts=1, weight_batches=8)),
    _g("g1_c2304_cr96", 1, 2304, 96, 4, claim=dict(slice=128, slices=18, slice_batches=2)),
    _g("g1_c640_cr8", 1, 640, 8, 4, claim=dict(run=128, slices=3)),
    _g("g1_c580_n1", 1, 580, 24, 4, n=1),
    _g("g1_c580_n15", 1, 580, 24, 4, n=15),
    _g("g1_c580_n16", 1, 580, 24, 4, n=16),
    _g("g1_c580_n17", 1, 580, 24, 4, n=17),
    _g("g1_c580_n33", 1, 580, 24, 4, n=33),
    _g("g1_c580_gap_chain_p64", 1, 580, 24, 64, P=64, claim=dict(tiles_is_p=True)),
    _g("g1_c580_gap_chain_p49", 1, 580, 24, 49, P=49, claim=dict(tiles_is_p=True)),
    # the pool and two GEMMs: widths the two-launch form refuses
    _g("g2_c640_cr256_n1", 2, 640, 256, 4, n=1, claim=dict(gate16=False)),
    _g("g2_c640_cr256_n37", 2, 640, 256, 4, n=37, claim=dict(gate16=False)),
    _g("g2_c580_cr200_n1", 2, 580, 200, 4, n=1, claim=dict(gate16=False)),
    _g("g2_c580_cr200_n37", 2, 580, 200, 4, n=37, claim=dict(gate16=False)),
]
for _i, _c in enumerate(GATE_CASES):
    _c["act1"] = ACT1S[_i % 3]
GATE_BY_NAME = {c["name"]: c for c in GATE_CASES}
# form = -1: one width per branch of the selection -> the form a fused block of that width takes
SELECTION = [("g0_c576_wraps", 0), ("g1_c580_cr24", 1), ("g2_c640_cr256_n1", 2)]
# bit stability: n = 33 made of three distinct segments repeated against n = 3, one width per form
STABILITY = ["g0_c96_t8_lanes2", "g1_c580_cr24", "g2_c580_cr200_n1"]


@functools.lru_cache(maxsize=None)
def gate_operands(name, n=None):
    """part with channels of different scale (0.2-3x) and a mean, sized so that pooled is of order 1; He-scaled W1 / W2; biases of
    order 1.  n: another segment count on the same weights (the first segments are the case's own)."""
    c = GATE_BY_NAME[name]
    n = c["n"] if n is None else n
    C, Cr, tiles, P = c["C"], c["Cr"], c["tiles"], c["P"]
    rng = np.random.default_rng(GATE_CASES.index(c) + 1000)
    W1 = (rng.standard_normal((C, Cr)) * math.sqrt(2.0 / C)).astype(f32)
    b1 = rng.standard_normal(Cr).astype(f32)
    W2 = (rng.standard_normal((Cr, C)) * math.sqrt(2.0 / Cr)).astype(f32)
    b2 = rng.standard_normal(C).astype(f32)
    scale = rng.uniform(0.2, 3.0, C) * (P / tiles)
    part = ((rng.standard_normal((max(n, 3), tiles, C)) + 0.5) * scale).astype(f32)[:n]
    return dict(part=np.ascontiguousarray(part), W1=W1, b1=b1, W2=W2, b2=b2)


def _tau_stage(name, stage, K, terms):
    """tau(K) x the stage's bound; the rigorous K 2^-24 x the same bound for a (case, stage) listed in RIGOROUS"""
    return (K * 2.0 ** -24 if (name, stage) in RIGOROUS else _tau(0, K)) * terms


def gate_reference(name, act2, ops=None, **mut):
    """O.se_gate64 and the propagated tolerance e_G.  mut: the mutations of the float64 reference (drop_tile, drop_channel = index,
    no_b1, tiles_for_p)."""
    c = GATE_BY_NAME[name]
    ops = ops or gate_operands(name)
    part, W1, b1, W2, b2 = (ops[k].astype(f64) for k in ("part", "W1", "b1", "W2", "b2"))
    C, Cr, tiles = c["C"], c["Cr"], c["tiles"]
    P = tiles if mut.get("tiles_for_p") else c["P"]
    if mut.get("drop_tile"):
        part = part[:, :-1]
    if mut.get("no_b1"):
        b1 = np.zeros_like(b1)
    if mut.get("drop_channel") is not None:
        W1 = W1.copy()
        W1[mut["drop_channel"]] = 0.0
    gate, pooled, preH, H, preG = O.se_gate64(part, P, W1, b1, c["act1"], W2, b2, act2)
    aW1, aW2 = np.abs(W1), np.abs(W2)
    e_pool = _tau_stage(name, "pool", tiles, np.abs(part).sum(axis=1) / P)
    e_H = 1.2 * (e_pool @ aW1 + _tau_stage(name, "hidden", C, np.abs(pooled) @ aW1 + np.abs(b1))) + _eps_act(preH, c["act1"])
    s2 = 0.25 if act2 == O.ACT_SIGMOID else 1.0
    e_G = s2 * (e_H @ aW2 + _tau_stage(name, "gate", Cr, np.abs(H) @ aW2 + np.abs(b2))) + _eps_act(preG, act2)
    return dict(gate=gate, pooled=pooled, preH=preH, H=H, preG=preG, tol=e_G)


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 emulations of the kernels' summation orders
# ---------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """one rounding of a b + c (the product of two floats is exact in float64)"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _act32(v, act):
    return O.act64(np.asarray(v, f64), act).astype(f32)


def _pool_serial32(part, inv_p):
    acc = np.zeros(part[:, 0].shape, f32)
    for t in range(part.shape[1]):
        acc = acc + part[:, t]
    return acc * inv_p


def emulate_gate(name, act2, ops=None):
    """The gate as the case's form computes it, in float32, in the kernel's order."""
    c = GATE_BY_NAME[name]
    ops = ops or gate_operands(name)
    part, W1, b1, W2, b2 = (ops[k] for k in ("part", "W1", "b1", "W2", "b2"))
    n, tiles, C = part.shape
    Cr, form = c["Cr"], c["form"]
    inv_p = f32(1.0) / f32(c["P"])
    if form == 0:
        lanes = lanes_of(C, tiles)
        if lanes > 1:        # lane l sums the tiles l, l + lanes, ...; the lanes' sums add in lane order
            sums = []
            for l in range(lanes):
                s = np.zeros((n, C), f32)
                for t in range(l, tiles, lanes):
                    s = s + part[:, t]
                sums.append(s)
            tot = sums[0]
            for s in sums[1:]:
                tot = tot + s
            pooled = tot * inv_p
        else:
            pooled = _pool_serial32(part, inv_p)
        crp = crp_of(Cr)
        nparts = 256 // crp
        sl = -(-C // nparts)
        hsum = np.broadcast_to(b1, (n, Cr)).astype(f32)
        for pt in range(nparts):       # thread (r, pt): an FMA chain over its slice of the channels; the parts add onto b1 in order
            s = np.zeros((n, Cr), f32)
            for ch in range(pt * sl, min(C, pt * sl + sl)):
                s = _fma(pooled[:, ch:ch + 1], W1[ch][None, :], s)
            hsum = hsum + s
        hid = _act32(hsum, c["act1"])
    elif form == 1:
        sl, slices = se_hidden_shape(C, Cr)
        nparts = 256 // Cr
        hsum = np.broadcast_to(b1, (n, Cr)).astype(f32)
        for ks in range(slices):       # se_hidden_kernel: slice ks, parts of `sub` rows, each an FMA chain from zero (batches of 32 in order)
            c0 = ks * sl
            ln = min(sl, C - c0)
            pooled = _pool_serial32(part[:, :, c0:c0 + ln], inv_p)
            sub = -(-ln // nparts)
            acc = np.zeros((n, Cr), f32)
            for pt in range(nparts):
                s0 = min(pt * sub, ln)
                s = np.zeros((n, Cr), f32)
                for r in range(s0, min(ln, s0 + sub)):
                    s = _fma(pooled[:, r:r + 1], W1[c0 + r][None, :], s)
                acc = acc + s
            hsum = hsum + acc          # se_gate16_kernel: b1 + the slices' partial sums in ascending order
        hid = _act32(hsum, c["act1"])
    else:
        pooled = _pool_serial32(part, inv_p)
        s = np.zeros((n, Cr), f32)
        for ch in range(C):
            s = _fma(pooled[:, ch:ch + 1], W1[ch][None, :], s)
        hid = _act32(s + b1, c["act1"])
    if form == 2:
        s = np.zeros((n, C), f32)
        for q in range(Cr):
            s = _fma(hid[:, q:q + 1], W2[q][None, :], s)
        s = s + b2
    else:
        s = np.broadcast_to(b2, (n, C)).astype(f32)
        for q in range(Cr):
            s = _fma(hid[:, q:q + 1], W2[q][None, :], s)
    return _act32(s, act2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plain layers: shape = (in_h, in_w, out_h, out_w, c, kh, kw, sh, sw, pad_t, pad_l, cin) as bh_debug_plain_layer takes it
# ---------------------------------------------------------------------------------------------------------------------------------
def _pl(name, op, n, shape, act=O.ACT_NONE, claim=None):
    return dict(name=name, op=op, n=n, shape=tuple(shape), act=act, claim=claim or {})


def _dw_cases():
    out = []
    for ks in (3, 5):
        for st in (1, 2):
            p = (ks - 1) // 2
            sym = lambda h: (h + 2 * p - ks) // st + 1
            tag = f"dw{ks}s{st}"
            for act in (O.ACT_NONE, O.ACT_RELU6, O.ACT_SWISH):
                out.append(_pl(f"{tag}_7x9_c20_{O.ACT_NAMES[act]}", OP_DWCONV, 3, (7, 9, sym(7), sym(9), 20, ks, ks, st, st, p, p, 20), act))
            # no padding on top / left, the last windows reach past the bottom / right edge (odd image; stride 2: TF's SAME)
            out.append(_pl(f"{tag}_7x9_pad0_past_edge", OP_DWCONV, 3, (7, 9, -(-7 // st), -(-9 // st), 20, ks, ks, st, st, 0, 0, 20), O.ACT_SWISH,
                           claim=dict(past_edge=True)))
            out.append(_pl(f"{tag}_2x2_to_1x1", OP_DWCONV, 3, (2, 2, 1, 1, 8, ks, ks, st, st, 0, 0, 8), O.ACT_RELU6))
            out.append(_pl(f"{tag}_5x6_c4", OP_DWCONV, 2, (5, 6, sym(5), sym(6), 4, ks, ks, st, st, p, p, 4), O.ACT_NONE))
    return out


def _conv_cases():
    out = []
    acts = (O.ACT_SWISH, O.ACT_RELU6, O.ACT_NONE, O.ACT_GELU_ERF, O.ACT_RELU)
    for i, (cin, cout) in enumerate(((1, 8), (2, 20), (3, 32), (2, 32), (1, 20), (3, 8))):
        out.append(_pl(f"cd_3x3s2_{cin}to{cout}", OP_CONV, 3, (9, 11, 5, 6, cout, 3, 3, 2, 2, 1, 1, cin), acts[i % 5], claim=dict(nc=4 if cout % 8 else 8)))
    out.append(_pl("cd_3x5_s1x2_2to20", OP_CONV, 2, (8, 11, 8, 6, 20, 3, 5, 1, 2, 1, 2, 2), O.ACT_SWISH, claim=dict(nc=4)))
    out.append(_pl("cd_4x4_2to512_lds_64k", OP_CONV, 2, (5, 5, 4, 4, 512, 4, 4, 1, 1, 1, 1, 2), O.ACT_RELU6, claim=dict(nc=8, lds_bytes=65536)))
    return out


DW_CASES, CONV_CASES = _dw_cases(), _conv_cases()
CONV_PAST_LDS = _pl("cd_4x4_2to516_past_lds", OP_CONV, 2, (5, 5, 4, 4, 516, 4, 4, 1, 1, 1, 1, 2))          # refused, nothing launched
GAP_CASES = [_pl(f"gap_p{P}_c{C}", OP_GAP, 3, (ih, iw, 1, 1, C, ih, iw, 1, 1, 0, 0, C))
             for (P, ih, iw) in ((1, 1, 1), (49, 7, 7), (1000, 40, 25)) for C in (4, 1280)]
SCALE_CASES = [_pl(f"scale_p{P}_c{C}", OP_SCALE, 3, (ih, iw, ih, iw, C, 1, 1, 1, 1, 0, 0, C)) for (P, ih, iw) in ((1, 1, 1), (35, 5, 7)) for C in (4, 20)]
# past the grid caps: three distinct segments repeated, compared bit for bit with the three-segment launch, segment by segment
OVERSUB = [
    _pl("dw3s1_past_cap", OP_DWCONV, 33, (357, 357, 357, 357, 4, 3, 3, 1, 1, 1, 1, 4), O.ACT_SWISH, claim=dict(cap_blocks=DW_CAP_BLOCKS, per_pixel=1)),
    _pl("cd_past_cap", OP_CONV, 33, (253, 253, 253, 253, 4, 3, 3, 1, 1, 1, 1, 1), O.ACT_SWISH, claim=dict(cap_blocks=CONV_CAP_BLOCKS, per_pixel=1)),
    _pl("scale_past_cap", OP_SCALE, 33, (357, 357, 357, 357, 4, 1, 1, 1, 1, 0, 0, 4), claim=dict(cap_blocks=SCALE_CAP_BLOCKS, per_pixel=1)),
]
PLAIN_CASES = DW_CASES + CONV_CASES + GAP_CASES + SCALE_CASES
PLAIN_BY_NAME = {c["name"]: c for c in PLAIN_CASES + OVERSUB + [CONV_PAST_LDS]}


@functools.lru_cache(maxsize=None)
def plain_operands(name, n=None):
    """Channels of different scale (0.2-3x), He-scaled weights, biases of order 1 with entries that push ReLU6 into both clamps (as
    operands() of tests/test_mbconv_block_gpu.py); n: another segment count (the first segments are the case's own)."""
    c = PLAIN_BY_NAME[name]
    n = c["n"] if n is None else n
    ih, iw, oh, ow, C, kh, kw, sh, sw, pt, pl, cin = c["shape"]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))          # (a seed of the name's, the same in every process)
    op = c["op"]
    W = b = g = None
    if op == OP_CONV:
        X = (rng.standard_normal((max(n, 3), cin, ih, iw)) * rng.uniform(0.2, 3.0, cin)[:, None, None]).astype(f32)[:n]
        W = (rng.standard_normal((kh, kw, cin, C)) * math.sqrt(2.0 / (kh * kw * cin))).astype(f32)
    else:
        X = (rng.standard_normal((max(n, 3), ih, iw, C)) * rng.uniform(0.2, 3.0, C)).astype(f32)[:n]
    if op == OP_DWCONV:
        W = (rng.standard_normal((kh * kw, C)) * math.sqrt(2.0 / (kh * kw))).astype(f32)
    if op in (OP_CONV, OP_DWCONV):
        b = rng.standard_normal(C).astype(f32)
        b[1:4] = (7.5, -7.5, 7.0)
        b[-1] = 7.5
    if op == OP_SCALE:
        g = rng.uniform(0.0, 1.0, (max(n, 3), C)).astype(f32)[:n]
    return dict(X=np.ascontiguousarray(X), W=W, b=b, gate=g)


def _last_live_tap(c):
    """the last tap (dy, dx) of the window that lies inside the image for at least one output pixel"""
    ih, iw, oh, ow, C, kh, kw, sh, sw, pt, pl, cin = c["shape"]
    live_y = [dy for dy in range(kh) if any(0 <= oy * sh - pt + dy < ih for oy in range(oh))]
    live_x = [dx for dx in range(kw) if any(0 <= ox * sw - pl + dx < iw for ox in range(ow))]
    return live_y[-1], live_x[-1]


def plain_reference(name, ops=None, **mut):
    """(ref [n][out_h][out_w][c] float64, tol).  mut: drop_tap, drop_pixel, neighbour_gate."""
    c = PLAIN_BY_NAME[name]
    ops = ops or plain_operands(name)
    ih, iw, oh, ow, C, kh, kw, sh, sw, pt, pl, cin = c["shape"]
    X = ops["X"].astype(f64)
    n = X.shape[0]
    op, act = c["op"], c["act"]
    if op == OP_DWCONV:
        W = ops["W"].astype(f64).copy()
        if mut.get("drop_tap"):
            dy, dx = _last_live_tap(c)
            W[dy * kw + dx] = 0.0
        b = ops["b"].astype(f64)
        pre = O.depthwise64(X, W, kh, sh, pt, pl, oh, ow) + b
        bound = O.depthwise64(np.abs(X), np.abs(W), kh, sh, pt, pl, oh, ow) + np.abs(b)
        return O.act64(pre, act), _tau_stage(name, "taps", kh * kw, 1.2 * bound) + _eps_act(pre, act)
    if op == OP_CONV:
        W = ops["W"].astype(f64).copy()
        if mut.get("drop_tap"):
            dy, dx = _last_live_tap(c)
            W[dy, dx] = 0.0
        b = ops["b"].astype(f64)
        pre, A = O.direct_conv64(X, W, b, sh, sw, pt, pl, oh, ow)
        bound = np.abs(A) @ np.abs(W.reshape(-1, C)) + np.abs(b)
        tol = _tau_stage(name, "taps", kh * kw * cin, 1.2 * bound) + _eps_act(pre, act)
        return O.act64(pre, act).reshape(n, oh, ow, C), tol.reshape(n, oh, ow, C)
    if op == OP_GAP:
        P = ih * iw
        x = X.reshape(n, P, C)
        ref = (x[:, :-1] if mut.get("drop_pixel") else x).sum(axis=1) / P
        return ref.reshape(n, 1, 1, C), (_tau(0, P) * np.abs(x).mean(axis=1)).reshape(n, 1, 1, C)
    g = ops["gate"].astype(f64)
    if mut.get("neighbour_gate"):
        g = np.roll(g, 1, axis=0)
    ref = X * g[:, None, None, :]
    return ref, 2.0 ** -23 * np.abs(X * ops["gate"].astype(f64)[:, None, None, :])


def emulate_plain(name):
    """The layer in float32 in its kernel's order: bias first, then one FMA a tap in (dy, dx[, channel]) order (a tap outside the
    image is skipped, which leaves the sum as an FMA with a zero does); the pool sums in pixel order, then x (1 / P)."""
    c = PLAIN_BY_NAME[name]
    ops = plain_operands(name)
    ih, iw, oh, ow, C, kh, kw, sh, sw, pt, pl, cin = c["shape"]
    X = ops["X"]
    n = X.shape[0]
    op, act = c["op"], c["act"]
    if op == OP_DWCONV:
        need_h, need_w = (oh - 1) * sh + kh, (ow - 1) * sw + kw
        Xp = np.zeros((n, max(need_h, pt + ih), max(need_w, pl + iw), C), f32)
        Xp[:, pt:pt + ih, pl:pl + iw] = X
        acc = np.broadcast_to(ops["b"], (n, oh, ow, C)).astype(f32)
        for dy in range(kh):
            for dx in range(kw):
                acc = _fma(Xp[:, dy:dy + (oh - 1) * sh + 1:sh, dx:dx + (ow - 1) * sw + 1:sw], ops["W"][dy * kw + dx], acc)
        return _act32(acc, act)
    if op == OP_CONV:
        A = O.im2col_nhwc(np.transpose(X, (0, 2, 3, 1)), kh, kw, sh, sw, pt, pl, oh, ow).astype(f32)      # (exact: float32 values)
        Wm = ops["W"].reshape(-1, C)
        acc = np.broadcast_to(ops["b"], (A.shape[0], C)).astype(f32)
        for k in range(A.shape[1]):
            acc = _fma(A[:, k:k + 1], Wm[k][None, :], acc)
        return _act32(acc, act).reshape(n, oh, ow, C)
    if op == OP_GAP:
        P = ih * iw
        return (_pool_serial32(X.reshape(n, P, C), f32(1.0) / f32(P))).reshape(n, 1, 1, C)
    return X * ops["gate"][:, None, None, :]


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------------
def test_gate_cases_are_what_they_claim():
    names = [c["name"] for c in GATE_CASES]
    assert len(set(names)) == len(names)
    for c in GATE_CASES:
        C, Cr, tiles, n, P, form, k = c["C"], c["Cr"], c["tiles"], c["n"], c["P"], c["form"], c["claim"]
        what = c["name"]
        assert C % 4 == 0 and (tiles <= 16 or k.get("tiles_is_p")), what
        assert k.get("tiles_is_p", False) == (tiles == P), what               # 1 / P and 1 / tiles differ wherever that is not the point
        if form == 0:
            assert se_gate_supports(C, Cr), what
            lanes, crp = lanes_of(C, tiles), crp_of(Cr)
            nparts = 256 // crp
            sl = -(-C // nparts)
            facts = dict(lanes=lanes, pooling_threads=lanes * C if lanes > 1 else None, tiles_mod_lanes=tiles % lanes, channel_rounds=-(-C // 256),
                         crp=crp, nparts=nparts, empty_parts=sum(1 for pt in range(nparts) if pt * sl >= C))
            if "lanes" in k and k["lanes"] > 1:
                assert lanes * C <= 256 and tiles >= 8, what
        elif form == 1:
            assert se_gate16_supports(C, Cr), what
            sl, slices = se_hidden_shape(C, Cr)
            nparts = 256 // Cr
            assert sl * Cr <= SE_RB * 256 or sl == 64 or slices * Cr <= C, what
            facts = dict(slice=sl, slices=slices, last_slice=C - (slices - 1) * sl, column_blocks=-(-C // 256), last_block=C - (-(-C // 256) - 1) * 256,
                         nparts=nparts, idle_threads=256 - nparts * Cr, scratch_slack=C - slices * Cr, weight_batches=-(-(-(-sl // nparts)) // SE_RB),
                         slice_batches=-(-slices // 16), run=SE_SG * Cr, tiles_is_p=tiles == P)
            if "run" in k:
                assert SE_SG * Cr < 256, what                                  # i0 + 256 lies beyond the run for every thread
        else:
            assert C % 4 == 0 and Cr % 4 == 0 and C > 576, what
            facts = dict(gate16=se_gate16_supports(C, Cr))
        for key, want in k.items():
            assert facts[key] == want, (what, key, facts[key], want)
    # the claims the table asks for, by name
    claimed = lambda key: [c for c in GATE_CASES if key in c["claim"]]
    assert any(c["claim"]["slice_batches"] == 2 and se_hidden_shape(c["C"], c["Cr"])[1] > 16 for c in claimed("slice_batches"))
    assert any(c["claim"]["scratch_slack"] == 0 for c in claimed("scratch_slack"))
    assert {c["n"] for c in GATE_CASES if c["form"] == 1} >= {1, 15, 16, 17, 33}
    assert {c["n"] for c in GATE_CASES if c["form"] == 0} >= {1, 3}
    assert {c["n"] for c in GATE_CASES if c["form"] == 2} == {1, 37}
    assert {c["P"] for c in claimed("tiles_is_p")} == {64, 49}
    assert {c["act1"] for c in GATE_CASES} == set(ACT1S)
    for form in (0, 1, 2):
        assert {c["act1"] for c in GATE_CASES if c["form"] == form} == set(ACT1S), form


def test_the_selection_cases_cover_every_branch():
    got = []
    for name, form in SELECTION:
        c = GATE_BY_NAME[name]
        assert se_gate_form(c["C"], c["Cr"]) == form == c["form"], name
        got.append((c["C"] <= 576, c["C"] >= BH_SE_GATE16_MIN and se_gate16_supports(c["C"], c["Cr"])))
    assert got == [(True, False), (False, True), (False, False)]
    assert [GATE_BY_NAME[nm]["form"] for nm in STABILITY] == [0, 1, 2]
    # every case runs in the form its own widths take in a forward
    for c in GATE_CASES:
        assert c["form"] == se_gate_form(c["C"], c["Cr"]), c["name"]


def test_plain_cases_are_what_they_claim():
    names = [c["name"] for c in PLAIN_CASES + OVERSUB]
    assert len(set(names)) == len(names)
    assert {(c["shape"][5], c["shape"][7]) for c in DW_CASES} == {(3, 1), (3, 2), (5, 1), (5, 2)}
    for c in DW_CASES:
        ih, iw, oh, ow, C, kh, kw, sh, sw, pt, pl, cin = c["shape"]
        assert dw_supports(kh, kw, sh, sw, C) and cin == C, c["name"]
        assert (oh - 1) * sh - pt < ih and (ow - 1) * sw - pl < iw, c["name"]          # every window holds a pixel
        if c["claim"].get("past_edge"):
            assert pt == pl == 0 and (oh - 1) * sh + kh > ih and (ow - 1) * sw + kw > iw and ih % 2 and iw % 2, c["name"]
    for ks in (3, 5):
        for st in (1, 2):
            mine = [c for c in DW_CASES if c["shape"][5] == ks and c["shape"][7] == st]
            assert {c["act"] for c in mine} >= {O.ACT_NONE, O.ACT_RELU6, O.ACT_SWISH}
            assert any(c["shape"][:4] == (2, 2, 1, 1) for c in mine) and any(c["shape"][4] == 4 for c in mine) and any(c["claim"].get("past_edge") for c in mine)
    for c in CONV_CASES:
        ih, iw, oh, ow, C, kh, kw, sh, sw, pt, pl, cin = c["shape"]
        assert conv_direct_supports(kh, kw, cin, C), c["name"]
        assert c["claim"]["nc"] == (4 if C % 8 else 8), c["name"]
        if "lds_bytes" in c["claim"]:
            assert kh * kw * cin * C * 4 == c["claim"]["lds_bytes"] == 64 * 1024
    assert {c["shape"][11] for c in CONV_CASES} >= {1, 2, 3} and {c["shape"][4] for c in CONV_CASES} >= {8, 20, 32}
    assert any(c["shape"][5:9] == (3, 5, 1, 2) for c in CONV_CASES)
    sh = CONV_PAST_LDS["shape"]
    assert not conv_direct_supports(sh[5], sh[6], sh[11], sh[4]) and sh[4] % 4 == 0 and sh[5] * sh[6] * sh[11] * (sh[4] - 4) * 4 == 64 * 1024
    assert {(c["shape"][0] * c["shape"][1], c["shape"][4]) for c in GAP_CASES} == {(P, C) for P in (1, 49, 1000) for C in (4, 1280)}
    assert all((c["n"] * c["shape"][4] // 4) % 256 for c in GAP_CASES)
    assert {(c["shape"][2] * c["shape"][3], c["shape"][4], c["n"]) for c in SCALE_CASES} == {(P, C, 3) for P in (1, 35) for C in (4, 20)}
    # the rigorous bound goes to tap stages of catalogue cases only, and never to a gate stage
    assert all(stage == "taps" and PLAIN_BY_NAME[nm]["op"] in (OP_CONV, OP_DWCONV) for nm, stage in RIGOROUS) and len(RIGOROUS) == 3
    for c in OVERSUB:
        ih, iw, oh, ow, C, kh, kw, sh, sw, pt, pl, cin = c["shape"]
        nc = 4 if c["op"] != OP_CONV or C % 8 else 8
        assert C // nc == c["claim"]["per_pixel"]
        total, cap = c["n"] * oh * ow * (C // nc), c["claim"]["cap_blocks"]
        assert cap * 256 < total < 2 * cap * 256 and (total - cap * 256) % (cap * 256) != 0, (c["name"], total)    # past the cap by a partial stride
        assert c["n"] % 3 == 0
        # the smallest square image past the cap at this segment count
        assert c["n"] * (oh - 1) * (ow - 1) * (C // nc) <= cap * 256, c["name"]


@pytest.mark.parametrize("case", [c["name"] for c in GATE_CASES])
def test_gate_emulation_fits_half_the_tolerance_and_mutations_show(case):
    c = GATE_BY_NAME[case]
    ops = gate_operands(case)
    sl = {0: -(-c["C"] // (256 // crp_of(c["Cr"]))), 1: se_hidden_shape(c["C"], c["Cr"])[0], 2: c["C"]}[c["form"]]
    for act2 in ACT2S:
        ref = gate_reference(case, act2)
        assert np.isfinite(ref["gate"]).all() and (ref["tol"] > 0).all()
        emu = emulate_gate(case, act2).astype(f64)
        share = float((np.abs(emu - ref["gate"]) / ref["tol"]).max())
        assert share <= 0.5, (case, O.ACT_NAMES[act2], share)
        muts = dict(drop_tile=dict(drop_tile=True), drop_channel=dict(drop_channel=min(sl, c["C"]) - 1), no_b1=dict(no_b1=True))
        if c["tiles"] != c["P"]:
            muts["tiles_for_p"] = dict(tiles_for_p=True)
        for what, m in muts.items():
            moved = np.abs(gate_reference(case, act2, **m)["gate"] - ref["gate"]) / ref["tol"]
            assert moved.max() > 4.0, (case, O.ACT_NAMES[act2], what, float(moved.max()))
        if c["n"] >= 2:     # two segments of a group exchanged = each takes the neighbouring segment's gate row
            moved = np.abs(ref["gate"][[1, 0]] - ref["gate"][:2]) / ref["tol"][:2]
            assert moved.max() > 4.0, (case, "segments exchanged", float(moved.max()))


@pytest.mark.parametrize("case", [c["name"] for c in PLAIN_CASES])
def test_plain_emulation_fits_half_the_tolerance_and_mutations_show(case):
    c = PLAIN_BY_NAME[case]
    ref, tol = plain_reference(case)
    assert np.isfinite(ref).all()
    emu = emulate_plain(case).astype(f64)
    err = np.abs(emu - ref)
    assert (err <= 0.5 * tol).all(), (case, float((err / np.maximum(tol, 1e-300)).max()))
    mut = {OP_DWCONV: "drop_tap", OP_CONV: "drop_tap", OP_GAP: "drop_pixel", OP_SCALE: "neighbour_gate"}[c["op"]]
    moved = np.abs(plain_reference(case, **{mut: True})[0] - ref)
    assert (moved > 4.0 * tol).any(), (case, mut)
    moved = np.abs(ref[[1, 0]] - ref[:2])                # two segments exchanged
    assert (moved > 4.0 * tol[:2]).any(), (case, "segments exchanged")
    if c["act"] == O.ACT_RELU6:                          # both clamps are reached
        assert (ref == 6.0).any() and (ref == 0.0).any(), case


def test_only_cases_that_do_not_fit_tau_take_the_rigorous_bound(monkeypatch):
    """with RIGOROUS emptied, exactly its cases exceed half of the tau tolerance"""
    listed = {nm for nm, _ in RIGOROUS}
    monkeypatch.setattr(sys.modules[__name__], "RIGOROUS", set())
    over = set()
    for c in DW_CASES + CONV_CASES:
        ref, tol = plain_reference(c["name"])
        if (np.abs(emulate_plain(c["name"]).astype(f64) - ref) > 0.5 * tol).any():
            over.add(c["name"])
    assert over == listed


def test_oversub_cases_repeat_three_distinct_segments():
    for c in OVERSUB:
        ops = plain_operands(c["name"], 3)
        assert ops["X"].shape[0] == 3
        assert not np.array_equal(ops["X"][0], ops["X"][1]) and not np.array_equal(ops["X"][1], ops["X"][2])
