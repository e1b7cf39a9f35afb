"""The squeeze-excite gate in its three forms (se_gate_kernel; se_hidden_kernel + se_gate16_kernel; se_pool_kernel + two
launch_pw_gemm) through bh_debug_se_gate, and the plain f32 layer kernels (dwconv_kernel<KS,ST>, conv_direct_kernel<NC>, gap_kernel,
scale_kernel) through bh_debug_plain_layer (include/birda_hip_gate_debug.h), one launch each on host operands through the launcher
a forward pass takes, every output element held to float64 (oracle.se_gate64, direct_conv64, depthwise64) at the cases of
tests/test_gate_layers.py -- which checks on the CPU that each case is the edge it claims, that the float64 reference fits the
tolerance (a float32 emulation of each kernel's summation order within half of it) and that the tolerance still sees a dropped
tile, channel, tap or bias and a neighbour's gate row.  Whole-model logits average a wrong channel or segment away; here nothing is.

The tolerance is the one stated there: the constants of tests/test_layer_gemm_gpu.py (tau = _tau(0, K), slope 1.2, eps_act),
propagated stage by stage for the gate; every gate case runs with act2 = sigmoid and with act2 = none, which holds preG itself.
Every device buffer sits in NaN guard bands; outputs and the scratch buffers (of exactly the forward's sizes) start as the payload
0x7fc0beef: an element never written, a read past an operand and a write past an output or a scratch buffer all fail the call.
A segment's gate must not depend on its launch: n = 33 made of three segments repeated gives the bits of n = 3, in every form; and
the three grid-stride kernels past their grid caps give, segment by segment, the bits of the three-segment launch.

Measured on the MI355X, worst err / tolerance (the last test prints the table): se_gate_kernel 0.044 (sigmoid) / 0.097 (none);
se_hidden_kernel + se_gate16_kernel 0.012 / 0.015; se_pool_kernel + pw_gemm_kernel 0.008 / 0.010; dwconv_kernel<3,1> 0.36, <3,2>
0.36, <5,1> 0.37, <5,2> 0.42; conv_direct_kernel<NC=4> 0.38, <NC=8> 0.46 (all on tau(K) but the tap stage of the three cases
test_gate_layers.RIGOROUS names: dw5s1_7x9_c20_none, dw5s2_7x9_c20_none, cd_3x3s2_3to32); gap_kernel 0.34; scale_kernel 0.49 (of one rounding: 2^-23 |x g|).  The gate's shares are small because tau allows 6.7 roundings of the whole bound
per stage and three stages add up, where the kernels make a few roundings of partial sums; the CPU module's mutation checks show
that the same tolerance still rejects every wrong sum by more than 4x."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gate_layers as CAT                                    # noqa: E402  (the catalogue, checked on the CPU there)

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x7fc0beef
REACHED = set()          # kernel names the entry points reported
WORST = {}               # (kernels, act2 / op) -> worst err / tol


def _lib():
    from birda_amd import _lib
    return _lib.load()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _reached(name):
    for k in name.split("+"):
        REACHED.add(k)
    return name


def run_gate(case, act2, form, ops=None):
    """bh_debug_se_gate -> (gate [n][C], the kernels' names)"""
    lib = _lib()
    c = CAT.GATE_BY_NAME[case]
    ops = ops or CAT.gate_operands(case)
    n = ops["part"].shape[0]
    gate = np.empty((n, c["C"]), np.float32)
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_se_gate(0, _p(ops["part"]), n, c["tiles"], c["P"], c["C"], c["Cr"], _p(ops["W1"]), _p(ops["b1"]), c["act1"], _p(ops["W2"]),
                              _p(ops["b2"]), act2, form, _p(gate), name, 128)
    assert rc == 0, (case, rc, lib.bh_last_error())
    assert not (gate.view(np.uint32) == UNWRITTEN).any(), (case, "elements never written")
    return gate, _reached(name.value.decode())


def run_plain(case, ops=None):
    """bh_debug_plain_layer -> (Y [n][out_h][out_w][c], the instantiation's name)"""
    lib = _lib()
    c = CAT.PLAIN_BY_NAME[case]
    ops = ops or CAT.plain_operands(case)
    n = ops["X"].shape[0]
    sh = c["shape"]
    Y = np.empty((n, sh[2], sh[3], sh[4]), np.float32)
    name = C.create_string_buffer(128)
    rc = lib.bh_debug_plain_layer(0, c["op"], _p(ops["X"]), _p(ops["W"]), _p(ops["b"]), _p(ops["gate"]), _p(Y), n, _p(np.asarray(sh, np.int32)),
                                  c["act"], name, 128)
    assert rc == 0, (case, rc, lib.bh_last_error())
    assert not (Y.view(np.uint32) == UNWRITTEN).any(), (case, "elements never written")
    return Y, _reached(name.value.decode())


def _hold(got, want, tol, key, what):
    assert np.isfinite(got).all(), (what, "non-finite output")
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / np.maximum(tol, 1e-300)
    worst = float(ratio.max())
    print(f"{what}: worst err / tol {worst:.3f}")
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if worst > 1.0:
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        pytest.fail(f"{what}: {int((ratio > 1).sum())} of {ratio.size} elements off, worst at {i}: got {got[i]!r} want {want[i]!r}, "
                    f"err {err[i]:.3e} > tol {tol[i]:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c["name"] for c in CAT.GATE_CASES])
def test_gate_against_float64(case):
    c = CAT.GATE_BY_NAME[case]
    for act2 in CAT.ACT2S:
        gate, name = run_gate(case, act2, c["form"])
        assert name == CAT.FORM_KERNELS[c["form"]], (case, name)
        ref = CAT.gate_reference(case, act2)
        _hold(gate, ref["gate"], ref["tol"], (name, O.ACT_NAMES[act2]), f"{case} {name} act2 {O.ACT_NAMES[act2]}")


@pytest.mark.parametrize("case,form", CAT.SELECTION)
def test_form_minus_one_is_the_forward_s_choice(case, form):
    """form = -1 reports the kernels of the form a fused block of this width takes, and computes the same bits as that form forced"""
    got, name = run_gate(case, O.ACT_SIGMOID, -1)
    assert name == CAT.FORM_KERNELS[form], (case, name)
    forced, _ = run_gate(case, O.ACT_SIGMOID, form)
    assert np.array_equal(got.view(np.uint32), forced.view(np.uint32))


def test_a_forced_form_that_does_not_support_the_widths_is_refused():
    lib = _lib()
    for case, form in (("g2_c640_cr256_n1", 1), ("g2_c580_cr200_n1", 1)):          # the two-launch form refuses these widths
        c = CAT.GATE_BY_NAME[case]
        ops = CAT.gate_operands(case)
        gate = np.zeros((c["n"], c["C"]), np.float32)
        name = C.create_string_buffer(b"untouched", 128)
        rc = lib.bh_debug_se_gate(0, _p(ops["part"]), c["n"], c["tiles"], c["P"], c["C"], c["Cr"], _p(ops["W1"]), _p(ops["b1"]), c["act1"],
                                  _p(ops["W2"]), _p(ops["b2"]), O.ACT_SIGMOID, form, _p(gate), name, 128)
        assert rc == CAT.BH_ERR_UNSUPPORTED, (case, rc)
        assert not gate.any() and name.value == b"untouched"                       # nothing launched, nothing written
    # 260 hidden channels: the one-launch kernel has 256 threads for them at most, and at 520 channels no other form is selected
    rng = np.random.default_rng(5)
    Cw, Crw = 520, 260
    assert not CAT.se_gate_supports(Cw, Crw) and CAT.se_gate_form(Cw, Crw) == -1
    part, W1, b1 = (rng.standard_normal(s).astype(np.float32) for s in ((2, 4, Cw), (Cw, Crw), (Crw,)))
    W2, b2 = (rng.standard_normal(s).astype(np.float32) for s in ((Crw, Cw), (Cw,)))
    for form in (0, -1):
        gate = np.zeros((2, Cw), np.float32)
        name = C.create_string_buffer(b"untouched", 128)
        rc = lib.bh_debug_se_gate(0, _p(part), 2, 4, 31, Cw, Crw, _p(W1), _p(b1), O.ACT_RELU, _p(W2), _p(b2), O.ACT_SIGMOID, form, _p(gate), name, 128)
        assert rc == CAT.BH_ERR_UNSUPPORTED, (form, rc)
        assert not gate.any() and name.value == b"untouched"
    # Cr not a multiple of 4 has no GEMM form
    c = CAT.GATE_BY_NAME["g0_cr6"]
    ops = CAT.gate_operands("g0_cr6")
    gate = np.zeros((c["n"], c["C"]), np.float32)
    rc = lib.bh_debug_se_gate(0, _p(ops["part"]), c["n"], c["tiles"], c["P"], c["C"], c["Cr"], _p(ops["W1"]), _p(ops["b1"]), c["act1"], _p(ops["W2"]),
                              _p(ops["b2"]), O.ACT_SIGMOID, 2, _p(gate), None, 0)
    assert rc == CAT.BH_ERR_UNSUPPORTED and not gate.any()


@pytest.mark.parametrize("case", CAT.STABILITY)
def test_a_segment_s_gate_does_not_depend_on_its_launch(case):
    """n = 33 made of three distinct segments repeated against n = 3: each segment's row, bit for bit"""
    c = CAT.GATE_BY_NAME[case]
    ops3 = dict(CAT.gate_operands(case, 3))
    ops33 = dict(ops3, part=np.ascontiguousarray(np.tile(ops3["part"], (11, 1, 1))))
    for act2 in CAT.ACT2S:
        g3, _ = run_gate(case, act2, c["form"], ops3)
        g33, _ = run_gate(case, act2, c["form"], ops33)
        for s in range(33):
            assert np.array_equal(g33[s].view(np.uint32), g3[s % 3].view(np.uint32)), (case, O.ACT_NAMES[act2], s)
        assert not np.array_equal(g3[0], g3[1]) and not np.array_equal(g3[1], g3[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# the plain layers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c["name"] for c in CAT.PLAIN_CASES])
def test_plain_layer_against_float64(case):
    c = CAT.PLAIN_BY_NAME[case]
    Y, name = run_plain(case)
    sh = c["shape"]
    if c["op"] == CAT.OP_DWCONV:
        assert name == f"dwconv_kernel<{sh[5]},{sh[7]}>", name
    elif c["op"] == CAT.OP_CONV:
        assert name == f"conv_direct_kernel<NC={c['claim']['nc']}>", name
    else:
        assert name == {CAT.OP_GAP: "gap_kernel", CAT.OP_SCALE: "scale_kernel"}[c["op"]], name
    ref, tol = CAT.plain_reference(case)
    _hold(Y, ref, tol, (name, O.ACT_NAMES[c["act"]]), f"{case} {name}")


def test_what_create_refuses_the_entry_refuses():
    lib = _lib()

    def refused(case, shape=None, op=None):
        c = CAT.PLAIN_BY_NAME[case]
        sh = np.asarray(c["shape"] if shape is None else shape, np.int32)
        X = np.zeros(1 << 16, np.float32)
        W = np.zeros(1 << 16, np.float32)
        Y = np.zeros(1 << 16, np.float32)
        name = C.create_string_buffer(b"untouched", 128)
        rc = lib.bh_debug_plain_layer(0, c["op"] if op is None else op, _p(X), _p(W), _p(W), _p(W), _p(Y), 1, _p(sh), c["act"], name, 128)
        assert rc == CAT.BH_ERR_UNSUPPORTED, (case, shape, rc, lib.bh_last_error())
        assert not Y.any() and name.value == b"untouched"
        return lib.bh_last_error().decode()

    assert "64 KiB" in refused(CAT.CONV_PAST_LDS["name"])                           # one size past the LDS boundary
    base = list(CAT.PLAIN_BY_NAME["dw3s1_5x6_c4"]["shape"])
    for change in (dict(c=6), dict(kh=4, kw=4), dict(kh=3, kw=5), dict(sh=3, sw=3), dict(sh=1, sw=2), dict(kh=7, kw=7)):
        sh = list(base)
        for k, v in change.items():
            sh[{"c": 4, "kh": 5, "kw": 6, "sh": 7, "sw": 8}[k]] = v
        if "c" in change:
            sh[11] = change["c"]
        assert "depthwise" in refused("dw3s1_5x6_c4", sh), change
    for case in ("gap_p49_c4", "scale_p35_c4"):
        sh = list(CAT.PLAIN_BY_NAME[case]["shape"])
        sh[4] = sh[11] = 6
        assert "multiple of 4" in refused(case, sh)
    sh = list(CAT.PLAIN_BY_NAME["cd_3x3s2_1to8"]["shape"])
    sh[4] = 10
    assert "direct conv" in refused("cd_3x3s2_1to8", sh)


@pytest.mark.parametrize("case", [c["name"] for c in CAT.OVERSUB])
def test_past_the_grid_cap_every_segment_keeps_its_bits(case):
    """three distinct segments repeated past the launcher's grid cap (the grid-stride loop's second, partial round) against the
    three-segment launch, segment by segment, bit for bit"""
    c = CAT.PLAIN_BY_NAME[case]
    ops3 = dict(CAT.plain_operands(case, 3))
    reps = c["n"] // 3
    opsN = dict(ops3, X=np.ascontiguousarray(np.tile(ops3["X"], (reps, 1, 1, 1))))
    if ops3["gate"] is not None:
        opsN["gate"] = np.ascontiguousarray(np.tile(ops3["gate"], (reps, 1)))
    Y3, name3 = run_plain(case, ops3)
    YN, nameN = run_plain(case, opsN)
    assert name3 == nameN
    assert np.isfinite(Y3).all()
    assert not np.array_equal(Y3[0], Y3[1]) and not np.array_equal(Y3[1], Y3[2])
    for s in range(c["n"]):
        assert np.array_equal(YN[s].view(np.uint32), Y3[s % 3].view(np.uint32)), (case, nameN, s)


def test_every_kernel_was_reached():
    """the names the entry points reported against the full set: the four dwconv instantiations, both NC values, gap, scale and the
    five gate kernels (the GEMM of the three-launch form by its family name, as launch_se_gate_gemm reports it: its instantiations
    are held one by one in tests/test_layer_gemm_gpu.py)"""
    print("\nworst err / tolerance per (kernels, act2 or activation):")
    for k in sorted(WORST):
        print("  %-36s %-8s %.3f" % (k[0], k[1], WORST[k]))
    assert REACHED == CAT.EVERY_KERNEL, (sorted(CAT.EVERY_KERNEL - REACHED), sorted(REACHED - CAT.EVERY_KERNEL))
    assert len(REACHED) == 13
