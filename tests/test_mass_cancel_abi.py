"""The mass cancel's boundary: me_mass_cancel and me_service_mass_cancel are declared in the headers, exported by
the library and prototyped for ctypes with the headers' argument lists; the entry dtype the call fills is
me_book_entry as the C compiler lays it out; a null engine or service is refused. No GPU."""
import ctypes as C
import os
import re
import subprocess

from tests.abi_layout import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_FIELDS = ("seq", "price_q4", "qty", "side", "pad")


def test_declared_exported_and_prototyped(built):
    from matching_engine_amd import _abi

    eh = open(os.path.join(ROOT, "include", "me_engine.h")).read()
    sh = open(os.path.join(ROOT, "include", "me_service.h")).read()
    assert re.search(r"\bint\s+me_mass_cancel\s*\(\s*me_engine\s*\*\s*e\s*,\s*const\s+uint32_t\s*\*\s*symbols\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*sides\s*,\s*size_t\s+n\s*,\s*me_book_entry\s*\*\s*out\s*,\s*size_t\s+cap\s*,"
                     r"\s*size_t\s*\*\s*n_out\s*,\s*uint64_t\s*\*\s*counts\b", eh)
    assert re.search(r"\bint\s+me_service_mass_cancel\s*\(\s*me_service\s*\*\s*s\s*,\s*const\s+char\s*\*\s*const\s*\*\s*symbols\s*,"
                     r"\s*size_t\s+n\s*,\s*int32_t\s+sides\s*,\s*uint64_t\s*\*\s*n_cancelled\s*\)\s*;", sh)
    syms = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], check=True, capture_output=True,
                          text=True).stdout
    lib = C.CDLL(_abi.LIB_PATH)
    for name in ("me_mass_cancel", "me_service_mass_cancel"):
        assert re.search(rf"\bT {name}\b", syms), name
        assert hasattr(lib, name), name
        assert name in _abi.PROTOTYPES, name
    assert len(_abi.PROTOTYPES["me_mass_cancel"][1]) == 8
    assert len(_abi.PROTOTYPES["me_service_mass_cancel"][1]) == 5


def test_a_null_engine_or_service_is_refused(built):
    from matching_engine_amd import _abi

    lib = _abi.load()
    n = C.c_size_t(77)
    assert lib.me_mass_cancel(None, None, None, 0, None, 0, C.byref(n), None) == _abi.ME_E_INVALID
    assert n.value == 0  # *n_out is written before anything is looked at
    assert lib.me_mass_cancel(None, None, None, 3, None, 0, None, None) == _abi.ME_E_INVALID
    k = C.c_uint64(77)
    assert lib.me_service_mass_cancel(None, None, 0, 3, C.byref(k)) == _abi.ME_E_INVALID
    assert k.value == 0


def test_the_entry_dtype_matches_the_header(built, tmp_path):
    from matching_engine_amd import _abi

    c = c_layout(tmp_path, "me_engine.h", "me_book_entry", ENTRY_FIELDS)
    dt = _abi.BOOK_ENTRY_DTYPE
    assert dt.itemsize == 24 == c["sizeof"]
    assert dt.names == ENTRY_FIELDS
    for f in ENTRY_FIELDS:
        assert dt.fields[f][1] == c[f], (f, dt.fields[f][1], c[f])


def test_the_python_methods_exist(built):
    import matching_engine_amd as me

    assert callable(me.Engine.mass_cancel) and callable(me.MatchingEngineService.mass_cancel)
