"""include/birda_hip_gated_debug.h (the f32 gated project GEMM of a squeeze-excite block alone, for
tests/test_gated_gemm_f32_gpu.py) against its ctypes table _lib.GATED_DEBUG_SYMBOLS, type for type, and the library's exports; no
other header, and not the generated Rust binding, names the entry."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_parse as A  # noqa: E402

INCLUDE = os.path.join(ROOT, "include")
NAMES = {"bh_debug_gated_gemm_f32": 14}


def _eq_ctypes(a: str, b: str) -> bool:
    """ctypes has one type for size_t and uint64_t on this platform"""
    norm = lambda s: s.replace("usize", "u64")
    return norm(a) == norm(b)


def test_gated_debug_table_matches_its_header():
    from birda_amd import _lib
    _, functions, _ = A.parse_c_header(os.path.join(INCLUDE, "birda_hip_gated_debug.h"))
    assert {n for n, _, _ in _lib.GATED_DEBUG_SYMBOLS} == set(functions) == set(NAMES)
    for name, res, args in _lib.GATED_DEBUG_SYMBOLS:
        want_ret, want_args = functions[name]
        assert _eq_ctypes(A.ctypes_class(res), want_ret), name
        assert len(args) == len(want_args) == NAMES[name], name
        for i, (a, b) in enumerate(zip(args, want_args)):
            assert _eq_ctypes(A.ctypes_class(a), b), (name, i, a, b)
        assert hasattr(_lib.load(), name), f"{name} declared in include/birda_hip_gated_debug.h but not exported"
        fn = getattr(_lib.load(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args)          # load() binds the table


def test_no_other_header_names_the_gated_entry():
    others = sorted(f for f in os.listdir(INCLUDE) if f != "birda_hip_gated_debug.h")
    assert {"birda_hip.h", "birda_hip_debug.h", "birda_hip_audit.h", "birda_hip_layer_debug.h", "birda_hip_block_debug.h",
            "birda_hip_terms_debug.h", "birda_hip_pool_debug.h", "birda_hip_resact_debug.h", "birda_hip_gconv_debug.h",
            "birda_hip_gate_debug.h", "birda_hip_pcm_debug.h", "birda_hip_resample_debug.h", "birda_hip_concat_debug.h",
            "birda_hip_custom_debug.h", "birda_hip_sys.rs"} <= set(others)
    for f in others:
        text = open(os.path.join(INCLUDE, f)).read()
        for name in NAMES:
            assert name not in text, (f, name)
    from birda_amd import _lib
    for table in (_lib.SYMBOLS, _lib.HOST_SYMBOLS, _lib.AUDIT_SYMBOLS, _lib.LAYER_DEBUG_SYMBOLS, _lib.BLOCK_DEBUG_SYMBOLS, _lib.TERMS_DEBUG_SYMBOLS,
                  _lib.POOL_DEBUG_SYMBOLS, _lib.RESACT_DEBUG_SYMBOLS, _lib.GCONV_DEBUG_SYMBOLS, _lib.GATE_DEBUG_SYMBOLS, _lib.PCM_DEBUG_SYMBOLS,
                  _lib.RESAMPLE_DEBUG_SYMBOLS, _lib.CONCAT_DEBUG_SYMBOLS, _lib.CUSTOM_DEBUG_SYMBOLS):
        assert not set(NAMES) & {n for n, _, _ in table}
