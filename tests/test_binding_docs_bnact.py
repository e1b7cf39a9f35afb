"""include/birda_hip_bnact_debug.h (one norm + activation launch alone, for tests/test_bnact_gpu.py) against its ctypes table
_lib.BNACT_DEBUG_SYMBOLS, type for type, and the library's exports; no other header, no other table, and not the generated Rust
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


def test_bnact_debug_table_matches_its_header():
    from birda_amd import _lib
    _, functions, _ = A.parse_c_header(os.path.join(INCLUDE, "birda_hip_bnact_debug.h"))
    assert {n for n, _, _ in _lib.BNACT_DEBUG_SYMBOLS} == set(functions) == {"bh_debug_bnact", "bh_debug_bnact_on_device", "bh_debug_scale_on_device"}
    for name, res, args in _lib.BNACT_DEBUG_SYMBOLS:
        want_ret, want_args = functions[name]
        assert _eq_ctypes(A.ctypes_class(res), want_ret), name
        assert len(args) == len(want_args) == {"bh_debug_bnact": 10, "bh_debug_bnact_on_device": 11, "bh_debug_scale_on_device": 9}[name], name
        for i, (a, b) in enumerate(zip(args, want_args)):
            assert _eq_ctypes(A.ctypes_class(a), b), (name, i, a, b)
        if name != "bh_debug_scale_on_device":
            assert A.ctypes_class(args[4]) == "i32"                            # the activation travels by value
        assert hasattr(_lib.load(), name), f"{name} declared in include/birda_hip_bnact_debug.h but not exported"
        fn = getattr(_lib.load(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args)          # load() binds the table


def test_no_other_header_and_no_other_table_names_the_bnact_entry():
    others = sorted(f for f in os.listdir(INCLUDE) if f != "birda_hip_bnact_debug.h")
    assert {"birda_hip.h", "birda_hip_debug.h", "birda_hip_audit.h", "birda_hip_layer_debug.h", "birda_hip_pool_debug.h",
            "birda_hip_lnorm_debug.h", "birda_hip_reduce_debug.h", "birda_hip_sys.rs"} <= set(others)
    for f in others:
        assert "bh_debug_bnact" not in open(os.path.join(INCLUDE, f)).read() and "bh_debug_scale_on_device" not in open(os.path.join(INCLUDE, f)).read(), f
    from birda_amd import _lib
    for table in (_lib.SYMBOLS, _lib.HOST_SYMBOLS, _lib.AUDIT_SYMBOLS, _lib.LAYER_DEBUG_SYMBOLS, _lib.BLOCK_DEBUG_SYMBOLS, _lib.TERMS_DEBUG_SYMBOLS,
                  _lib.POOL_DEBUG_SYMBOLS, _lib.GCONV_DEBUG_SYMBOLS, _lib.GATE_DEBUG_SYMBOLS, _lib.RESACT_DEBUG_SYMBOLS, _lib.CONCAT_DEBUG_SYMBOLS,
                  _lib.PCM_DEBUG_SYMBOLS, _lib.RESAMPLE_DEBUG_SYMBOLS, _lib.CUSTOM_DEBUG_SYMBOLS, _lib.GATED_DEBUG_SYMBOLS, _lib.DILATED_DEBUG_SYMBOLS,
                  _lib.LNORM_DEBUG_SYMBOLS, _lib.REDUCE_DEBUG_SYMBOLS):
        assert not any(n.startswith("bh_debug_bnact") or n == "bh_debug_scale_on_device" for n, _, _ in table)


def test_the_norm_and_reduce_entries_are_declared_as_they_were():
    _, ln, _ = A.parse_c_header(os.path.join(INCLUDE, "birda_hip_lnorm_debug.h"))
    _, red, _ = A.parse_c_header(os.path.join(INCLUDE, "birda_hip_reduce_debug.h"))
    assert len(ln["bh_debug_lnorm"][1]) == 10 and len(red["bh_debug_reduce"][1]) == 9
