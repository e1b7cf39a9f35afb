"""include/birda_hip_lnorm_debug.h (one channel LayerNorm launch alone, for tests/test_convnext_gpu.py) against its ctypes table
_lib.LNORM_DEBUG_SYMBOLS, type for type, and the library's exports; no other header, no other table, and not the generated Rust
binding, names it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_parse as A  # noqa: E402

INCLUDE = os.path.join(ROOT, "include")


def _eq_ctypes(a: str, b: str) -> bool:
    """ctypes has one type for size_t and uint64_t on this platform"""
    norm = lambda s: s.replace("usize", "u64")
    return norm(a) == norm(b)


def test_lnorm_debug_table_matches_its_header():
    from birda_amd import _lib
    _, functions, _ = A.parse_c_header(os.path.join(INCLUDE, "birda_hip_lnorm_debug.h"))
    assert {n for n, _, _ in _lib.LNORM_DEBUG_SYMBOLS} == set(functions) == {"bh_debug_lnorm"}
    for name, res, args in _lib.LNORM_DEBUG_SYMBOLS:
        want_ret, want_args = functions[name]
        assert _eq_ctypes(A.ctypes_class(res), want_ret), name
        assert len(args) == len(want_args) == 10, name
        for i, (a, b) in enumerate(zip(args, want_args)):
            assert _eq_ctypes(A.ctypes_class(a), b), (name, i, a, b)
        assert A.ctypes_class(args[4]) == "f32"                                # eps travels by value, as a float
        assert hasattr(_lib.load(), name), f"{name} declared in include/birda_hip_lnorm_debug.h but not exported"
        fn = getattr(_lib.load(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args)          # load() binds the table


def test_no_other_header_and_no_other_table_names_the_lnorm_entry():
    others = sorted(f for f in os.listdir(INCLUDE) if f != "birda_hip_lnorm_debug.h")
    assert {"birda_hip.h", "birda_hip_debug.h", "birda_hip_audit.h", "birda_hip_layer_debug.h", "birda_hip_gate_debug.h",
            "birda_hip_dilated_debug.h", "birda_hip_sys.rs"} <= set(others)
    for f in others:
        assert "bh_debug_lnorm" not in open(os.path.join(INCLUDE, f)).read(), f
    from birda_amd import _lib
    for table in (_lib.SYMBOLS, _lib.HOST_SYMBOLS, _lib.AUDIT_SYMBOLS, _lib.LAYER_DEBUG_SYMBOLS, _lib.BLOCK_DEBUG_SYMBOLS, _lib.TERMS_DEBUG_SYMBOLS,
                  _lib.POOL_DEBUG_SYMBOLS, _lib.GCONV_DEBUG_SYMBOLS, _lib.GATE_DEBUG_SYMBOLS, _lib.RESACT_DEBUG_SYMBOLS, _lib.CONCAT_DEBUG_SYMBOLS,
                  _lib.PCM_DEBUG_SYMBOLS, _lib.RESAMPLE_DEBUG_SYMBOLS, _lib.CUSTOM_DEBUG_SYMBOLS, _lib.GATED_DEBUG_SYMBOLS, _lib.DILATED_DEBUG_SYMBOLS):
        assert "bh_debug_lnorm" not in {n for n, _, _ in table}


def test_the_depthwise_entries_are_declared_as_they_were():
    """the 7x7 depthwise is reached through bh_debug_dilated_layer (dilation 1 included); that declaration and bh_debug_plain_layer's,
    which keeps its 3x3 / 5x5 windows, did not change"""
    _, gate, _ = A.parse_c_header(os.path.join(INCLUDE, "birda_hip_gate_debug.h"))
    _, dil, _ = A.parse_c_header(os.path.join(INCLUDE, "birda_hip_dilated_debug.h"))
    assert len(gate["bh_debug_plain_layer"][1]) == 12 and len(dil["bh_debug_dilated_layer"][1]) == 14
    assert "7x7" not in open(os.path.join(INCLUDE, "birda_hip_gate_debug.h")).read()
    assert "7x7" in open(os.path.join(INCLUDE, "birda_hip_dilated_debug.h")).read()
