"""The trigger book's C-ABI surface (include/me_engine.h me_stop, me_stop_event, me_stops_*): struct sizes, field
order and offsets against the header, the exports, null-engine refusals and stop_records. Runs on CPU."""
import ctypes as C
import os
import re

import numpy as np

from tests import stops_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("me_stops_enable", "me_stops_add", "me_stops_cancel", "me_stops_read", "me_stops_stats", "me_stops_dump")
CTYPES = {"uint64_t": C.c_uint64, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
          "uint8_t": C.c_uint8}


def _header_struct(name):
    """The struct as a ctypes.Structure built from the header's own declarations: the C layout rules applied to
    the header's text, independent of the dtypes under test."""
    src = open(os.path.join(ROOT, "include", "me_engine.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(\w+)\s+(\w+)(?:\[(\d+)\])?\s*$", decl)
        if m:
            t = CTYPES[m.group(1)]
            fields.append((m.group(2), t * int(m.group(3)) if m.group(3) else t))
    return type(name, (C.Structure,), {"_fields_": fields})


def _check_layout(name, dtype, size):
    st = _header_struct(name)
    assert C.sizeof(st) == size == dtype.itemsize
    assert [f[0] for f in st._fields_] == list(dtype.names)
    for fname, _ in st._fields_:
        assert getattr(st, fname).offset == dtype.fields[fname][1], fname
        assert getattr(st, fname).size == dtype.fields[fname][0].itemsize, fname


def test_me_stop_is_40_bytes_and_matches_the_header(built):
    from matching_engine_amd import _abi

    assert _abi.STOP_DTYPE == sm.STOP_DTYPE
    _check_layout("me_stop", _abi.STOP_DTYPE, 40)
    assert [_abi.STOP_DTYPE.fields[n][1] for n in ("id", "stop_px_q4", "limit_px_q4", "qty", "symbol", "kind", "pad")] == \
        [0, 8, 16, 24, 28, 32, 33]


def test_me_stop_event_is_64_bytes_and_matches_the_header(built):
    from matching_engine_amd import _abi

    assert _abi.STOP_EVENT_DTYPE == sm.STOP_EVENT_DTYPE
    _check_layout("me_stop_event", _abi.STOP_EVENT_DTYPE, 64)
    assert [_abi.STOP_EVENT_DTYPE.fields[n][1] for n in
            ("id", "stop_px_q4", "limit_px_q4", "trigger_px_q4", "batches", "qty", "symbol", "kind", "pad")] == \
        [0, 8, 16, 24, 32, 40, 44, 48, 49]


def test_library_exports_exactly_the_six_calls(built):
    from matching_engine_amd import _abi
    from tests.abi_layout import declared_functions

    lib = C.CDLL(_abi.LIB_PATH)
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in _abi.PROTOTYPES
    assert sorted(f for f in declared_functions() if f.startswith("me_stops_")) == sorted(EXPORTS)
    assert sorted(f for f in _abi.PROTOTYPES if f.startswith("me_stops_")) == sorted(EXPORTS)
    lib = _abi.load()  # a null engine is refused, not dereferenced
    n, left = C.c_size_t(7), C.c_size_t(7)
    assert lib.me_stops_enable(None, 16) == _abi.ME_E_INVALID
    assert lib.me_stops_add(None, None, 0) == _abi.ME_E_INVALID
    assert lib.me_stops_cancel(None, None, 0, None) == _abi.ME_E_INVALID
    assert lib.me_stops_read(None, None, 0, C.byref(n), C.byref(left)) == _abi.ME_E_INVALID
    assert (n.value, left.value) == (0, 0)  # written on every return
    assert lib.me_stops_stats(None, None, None, None) == _abi.ME_E_INVALID
    n = C.c_size_t(7)
    assert lib.me_stops_dump(None, None, 0, C.byref(n)) == _abi.ME_E_INVALID and n.value == 0


def test_stop_records_turns_events_into_new_records(built):
    import matching_engine_amd as me

    ev = np.zeros(3, dtype=me.STOP_EVENT_DTYPE)
    ev["id"] = [7, 9, 11]
    ev["limit_px_q4"] = [-5, 0, 2 ** 63 - 1]
    ev["stop_px_q4"] = [1, 2, 3]
    ev["trigger_px_q4"] = [4, 5, 6]
    ev["qty"] = [1, 2 ** 31 - 1, 3]
    ev["symbol"] = [2, 0, 2 ** 32 - 1]
    ev["kind"] = [me.kind(2, 1), me.kind(1, 0, 0, me.TIF_IOC), me.kind(2)]
    b = me.stop_records(ev, 2 ** 40)
    assert b.seq.tolist() == [2 ** 40, 2 ** 40 + 1, 2 ** 40 + 2] and b.seq.dtype == np.uint64
    assert b.price_q4.tolist() == [-5, 0, 2 ** 63 - 1]
    assert b.qty.tolist() == [1, 2 ** 31 - 1, 3] and b.symbol.tolist() == [2, 0, 2 ** 32 - 1]
    assert b.kind.tolist() == ev["kind"].tolist()
    assert len(me.stop_records(ev[:0], 5)) == 0
