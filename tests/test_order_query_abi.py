"""The order query's boundary: me_order_query and me_service_order_status are declared in the headers, exported
by the library and prototyped for ctypes; ORDER_INFO_DTYPE and MeOrderStatus lay their fields out as the C
compiler lays out the headers' structs. No GPU."""
import ctypes as C
import os
import re
import subprocess

from tests import order_query_model as oq
from tests.abi_layout import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_FIELDS = ("seq", "price_q4", "qty_ahead", "level_qty", "qty_better", "qty", "orders_ahead", "levels_better",
               "symbol", "side", "found", "pad")
STATUS_FIELDS = ("order_id", "state", "side", "scale", "quantity", "price", "qty_ahead", "level_qty", "qty_better",
                 "orders_ahead", "levels_better")


def test_declared_exported_and_prototyped(built):
    from matching_engine_amd import _abi

    eh = open(os.path.join(ROOT, "include", "me_engine.h")).read()
    sh = open(os.path.join(ROOT, "include", "me_service.h")).read()
    assert re.search(r"\bint\s+me_order_query\s*\(\s*me_engine\s*\*\s*e\s*,\s*const\s+uint64_t\s*\*\s*seqs\s*,\s*size_t\s+n\s*,"
                     r"\s*me_order_info\s*\*\s*out\s*\)\s*;", eh)
    assert re.search(r"\bint\s+me_service_order_status\s*\(", sh)
    assert re.search(r"typedef\s+struct\s+me_order_info\b", eh) and re.search(r"typedef\s+struct\s+me_order_status\b", sh)
    for name in ("ME_OS_NOT_RESTING", "ME_OS_PENDING", "ME_OS_RESTING"):
        assert name in sh, name
    syms = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], check=True, capture_output=True,
                          text=True).stdout
    lib = C.CDLL(_abi.LIB_PATH)
    for name in ("me_order_query", "me_service_order_status"):
        assert re.search(rf"\bT {name}\b", syms), name
        assert hasattr(lib, name), name
        assert name in _abi.PROTOTYPES, name
    assert (_abi.OS_NOT_RESTING, _abi.OS_PENDING, _abi.OS_RESTING) == (0, 1, 2)
    # a null engine or service is refused, not dereferenced
    lib = _abi.load()
    assert lib.me_order_query(None, None, 0, None) == _abi.ME_E_INVALID
    assert lib.me_service_order_status(None, None, None, 0, None) == _abi.ME_E_INVALID


def test_order_info_dtype_matches_the_header(built, tmp_path):
    from matching_engine_amd import _abi

    c = c_layout(tmp_path, "me_engine.h", "me_order_info", INFO_FIELDS)
    dt = _abi.ORDER_INFO_DTYPE
    assert dt.itemsize == 64 == c["sizeof"]
    assert dt.names == INFO_FIELDS
    for f in INFO_FIELDS:
        assert dt.fields[f][1] == c[f], (f, dt.fields[f][1], c[f])
    assert dt == oq.ORDER_INFO_DTYPE  # the model restates it
    import matching_engine_amd as me

    assert me.ORDER_INFO_DTYPE is dt


def test_order_status_struct_matches_the_header(built, tmp_path):
    from matching_engine_amd import _abi

    c = c_layout(tmp_path, "me_service.h", "me_order_status", STATUS_FIELDS)
    assert C.sizeof(_abi.MeOrderStatus) == c["sizeof"] == 88
    assert tuple(n for n, _ in _abi.MeOrderStatus._fields_) == STATUS_FIELDS
    for f in STATUS_FIELDS:
        assert getattr(_abi.MeOrderStatus, f).offset == c[f], f
