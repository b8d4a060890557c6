"""The C-ABI surface of stop orders through the service (include/me_service.h me_stop_request,
me_stop_cancel_request, me_stop_update, me_matcher's four stop hooks, me_service_stops_enable / _submit_stop /
_cancel_stop / _stop_updates / _stops / _stop_stats): struct sizes, field order and offsets against the header, the
exports and the NULL refusals. Runs on CPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("me_service_stops_enable", "me_service_submit_stop", "me_service_cancel_stop", "me_service_stop_updates",
           "me_service_stops", "me_service_stop_stats")
CTYPES = {"uint64_t": C.c_uint64, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
          "uint8_t": C.c_uint8, "char": C.c_char, "const char*": C.c_char_p}


def _header():
    return open(os.path.join(ROOT, "include", "me_service.h")).read()


def _header_struct(name):
    """The struct as a ctypes.Structure built from the header's own declarations (comma lists and arrays
    included): the C layout rules applied to the header's text, independent of the classes under test."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(const char\*|\w+)\s+(.+?)\s*$", decl, flags=re.S)
        if not m:
            continue
        t = CTYPES[m.group(1)]
        for item in m.group(2).split(","):
            f = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            fields.append((f.group(1), t * int(f.group(2)) if f.group(2) else t))
    return type(name, (C.Structure,), {"_fields_": fields})


def _same_layout(name, cls, size):
    st = _header_struct(name)
    assert C.sizeof(st) == size == C.sizeof(cls), (C.sizeof(st), C.sizeof(cls))
    assert [f[0] for f in st._fields_] == [f[0] for f in cls._fields_]
    for fname, _ in st._fields_:
        assert getattr(st, fname).offset == getattr(cls, fname).offset, fname
        assert getattr(st, fname).size == getattr(cls, fname).size, fname


def test_structs_match_the_header(built):
    from matching_engine_amd import _abi

    _same_layout("me_stop_request", _abi.MeStopRequest, 56)
    _same_layout("me_stop_cancel_request", _abi.MeStopCancelRequest, 16)
    _same_layout("me_stop_update", _abi.MeStopUpdate, 200)
    u = _abi.MeStopUpdate
    assert [getattr(u, f).offset for f in ("stop_id", "order_id", "client_id", "symbol", "state", "scale", "stop_price",
                                           "limit_price", "trigger_price", "quantity", "kind", "pad")] == \
        [0, 32, 64, 128, 160, 164, 168, 176, 184, 192, 196, 197]
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    enum = re.search(r"enum \{ (ME_SS_ARMED.*?) \};", src).group(1)
    got = {k.strip(): int(v) for k, v in (kv.split("=") for kv in enum.split(","))}
    assert got == {"ME_SS_ARMED": _abi.SS_ARMED, "ME_SS_TRIGGERED": _abi.SS_TRIGGERED, "ME_SS_CANCELED": _abi.SS_CANCELED,
                   "ME_SS_CANCEL_REJECTED": _abi.SS_CANCEL_REJECTED, "ME_SS_QUEUED": _abi.SS_QUEUED}
    assert list(got.values()) == [0, 1, 2, 3, 4]


def test_the_matcher_ends_with_the_four_stop_hooks(built):
    from matching_engine_amd import _abi

    body = re.search(r"typedef struct me_matcher \{(.*?)\} me_matcher;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"\(\*(\w+)\)\(|^\s*(?:void\*|uint32_t|uint64_t)\s+(\w+);", body, flags=re.M)
    names = [a or b for a, b in members]
    # MeMatcherStops is the whole struct: MeMatcher (the members up to order_preview) and then the four hooks
    whole = _abi.MeMatcherStops
    assert issubclass(whole, _abi.MeMatcher)
    assert names == [f[0] for f in _abi.MeMatcher._fields_] + [f[0] for f in whole._fields_]
    assert names[-4:] == ["stops_enable", "stops_add", "stops_cancel", "stops_read"]
    assert C.sizeof(whole) == 24 + 8 * (len(names) - 4)  # ctx, two uint32, one uint64, then pointers
    assert whole.stops_enable.offset == C.sizeof(_abi.MeMatcher) and whole.stops_read.offset == C.sizeof(whole) - 8
    assert not any(n.startswith("stops_") for n, _ in _abi.MeShardOps._fields_)  # the cluster carries none
    m = whole()  # zero-initialised: no stop orders
    assert not m.stops_enable and not m.stops_add and not m.stops_cancel and not m.stops_read


def test_every_matcher_the_package_builds_is_the_whole_struct(built):
    """me_cluster_matcher clears sizeof(me_matcher) bytes and me_service_create_matcher reads as many: what
    python_matcher hands out must be that long, with the stop hooks NULL unless the object has all four."""
    from matching_engine_amd import _abi
    from matching_engine_amd.cluster import python_matcher
    from tests.stops_service_common import PlainMatcher, StopMatcher

    plain = python_matcher(PlainMatcher(1))
    assert isinstance(plain, _abi.MeMatcherStops)
    assert not plain.stops_enable and not plain.stops_add and not plain.stops_cancel and not plain.stops_read
    full = python_matcher(StopMatcher(1))
    assert full.stops_enable and full.stops_add and full.stops_cancel and full.stops_read

    class Three(PlainMatcher):  # three of the four: none is wired
        stops_enable = stops_add = stops_cancel = lambda self, *a: None

    some = python_matcher(Three(1))
    assert not some.stops_enable and not some.stops_add and not some.stops_cancel and not some.stops_read


def test_exports_and_null_refusals(built):
    from matching_engine_amd import _abi
    from tests.abi_layout import declared_functions

    lib = C.CDLL(_abi.LIB_PATH)
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in _abi.PROTOTYPES and name in declared_functions()
    assert sorted(f for f in declared_functions() if "stop" in f and f.startswith("me_service_") and
                  f != "me_service_stop") == sorted(EXPORTS)  # (me_service_stop ends the background flusher)
    lib = _abi.load()  # a null service is refused, not dereferenced
    assert lib.me_service_stops_enable(None, 8) == _abi.ME_E_INVALID
    n = C.c_size_t(7)
    assert lib.me_service_stop_updates(None, None, None, 0, C.byref(n)) == _abi.ME_E_INVALID and n.value == 0
    n = C.c_size_t(7)
    assert lib.me_service_stops(None, None, None, 0, C.byref(n)) == _abi.ME_E_INVALID and n.value == 0
    assert lib.me_service_stop_stats(None, None, None, None) == _abi.ME_E_INVALID
    resp = _abi.MeOrderResponse()
    req = _abi.MeStopRequest(b"a", b"A", 1, 1, 0, 5, 4, 1, 0)
    assert lib.me_service_submit_stop(None, C.byref(req), C.byref(resp)) == 0
    assert (resp.success, resp.order_id, resp.error_message) == (0, b"", b"stop orders are not enabled")
    creq = _abi.MeStopCancelRequest(b"a", b"SID-1")
    assert lib.me_service_cancel_stop(None, C.byref(creq), C.byref(resp)) == 0
    assert (resp.success, resp.error_message) == (0, b"stop orders are not enabled")


def test_a_service_without_a_backend_refuses_the_enable(built):
    import matching_engine_amd as me

    svc = me.MatchingEngineService(None, ["A"])
    try:
        rc = svc.lib.me_service_stops_enable(svc.h, 4)
        assert rc == me.ME_E_STATE
        out = (me._abi.MeStopUpdate * 1)()
        n = C.c_size_t(7)
        assert svc.lib.me_service_stops(svc.h, None, None, 1, C.byref(n)) == me.ME_E_INVALID  # cap without out
        assert svc.lib.me_service_stops(svc.h, None, out, 1, C.byref(n)) == 0 and n.value == 0
        assert svc.stop_stats() == {"live": 0, "triggered": 0, "recovered": 0}
    finally:
        svc.close()


def test_the_prototypes_take_only_the_whole_matcher(built):
    """MeMatcher is the struct's head, 32 bytes short of me_matcher: the two calls that read or clear the whole
    struct refuse it before anything is dereferenced."""
    import pytest

    from matching_engine_amd import _abi

    lib = _abi.load()
    assert C.sizeof(_abi.MeMatcherStops) - C.sizeof(_abi.MeMatcher) == 32
    head = _abi.MeMatcher()
    with pytest.raises(C.ArgumentError):
        lib.me_service_create_matcher(C.byref(head), None, 0, None)
    with pytest.raises(C.ArgumentError):
        lib.me_cluster_matcher(None, C.byref(head))
    assert lib.me_cluster_matcher(None, C.byref(_abi.MeMatcherStops())) == _abi.ME_E_INVALID
