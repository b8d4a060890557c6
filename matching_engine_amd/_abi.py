"""ctypes view of include/me_engine.h (the C-ABI of libme_engine.so).

The library is built in-tree (``make -C matching_engine_amd``); loading fails loudly when it is
missing — there is no Python or CPU fallback for the matching path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ME_ENGINE_LIB selects a diagnostic variant (e.g. build/libme_engine_stamps.so) for profiling runs.
LIB_PATH = os.environ.get("ME_ENGINE_LIB") or os.path.join(_HERE, "libme_engine.so")

# ---- enums (include/me_engine.h) -------------------------------------------------------------
SIDE_UNSPECIFIED, SIDE_BUY, SIDE_SELL = 0, 1, 2
TYPE_LIMIT, TYPE_MARKET = 0, 1
OP_NEW, OP_CANCEL = 0, 1
# A REDUCE has no ME_OP_* value of its own: it is a CANCEL record with the type bit set (ME_KIND_REDUCE).
# OP_REDUCE is kind()'s spelling of that: its bit 1 becomes the type bit, so kind(side, op=OP_REDUCE) & 0x0C == 0x0C.
OP_REDUCE = 3
KIND_REDUCE = 0x0D
ST_NEW, ST_PARTIALLY_FILLED, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
RJ_NONE, RJ_BAD_QTY, RJ_BAD_SIDE, RJ_OUT_OF_WINDOW, RJ_BAD_SYMBOL, RJ_UNKNOWN_ORDER, RJ_BAD_SEQ, RJ_CAPACITY = range(8)
RJ_WOULD_CROSS, RJ_BAD_TIF = 8, 9
TIF_GTC, TIF_IOC, TIF_FOK, TIF_POST_ONLY = 0, 1, 2, 3
ME_OK, ME_E_INVALID, ME_E_HIP, ME_E_CAPACITY, ME_E_STATE, ME_E_SQLITE = 0, -1, -2, -3, -4, -5
CHUNK_SLOTS = 16


def kind(side: int, otype: int = TYPE_LIMIT, op: int = OP_NEW, tif: int = TIF_GTC) -> int:
    """ME_KIND_TIF(side, type, op, tif) (ME_KIND with tif = 0); op = OP_REDUCE sets bits 3 and 2."""
    return (side & 3) | (((otype | (op >> 1)) & 1) << 2) | ((op & 1) << 3) | ((tif & 3) << 4)


# ---- structs ---------------------------------------------------------------------------------
class MeConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("num_symbols", C.c_uint32),
        ("levels", C.c_uint32),
        ("max_batch", C.c_uint32),
        ("max_resting", C.c_uint64),
        ("max_chunks", C.c_uint64),
        ("seq_ring", C.c_uint64),
        ("base_price", C.POINTER(C.c_int64)),
        ("symbol_ids", C.POINTER(C.c_uint32)),
        ("batches_per_launch", C.c_uint32),
        ("far_levels", C.c_uint32),
        ("host_slots", C.c_uint32),
        ("host_tape_cap", C.c_uint64),
    ]


class MeOrderSoa(C.Structure):
    _fields_ = [
        ("seq", C.c_void_p),
        ("price_q4", C.c_void_p),
        ("qty", C.c_void_p),
        ("symbol", C.c_void_p),
        ("kind", C.c_void_p),
    ]


class MeOrderSoaW(C.Structure):
    _fields_ = [
        ("seq", C.c_void_p),
        ("price_q4", C.c_void_p),
        ("qty", C.c_void_p),
        ("symbol", C.c_void_p),
        ("kind", C.c_void_p),
    ]


class MeGenParams(C.Structure):
    _fields_ = [
        ("config", C.c_uint32),
        ("seed", C.c_uint64),
        ("num_symbols", C.c_uint32),
        ("levels", C.c_uint32),
        ("spread_ticks", C.c_int32),
        ("max_qty", C.c_int32),
        ("market_pct", C.c_uint32),
        ("cancel_pct", C.c_uint32),
        ("zipf_s", C.c_double),
        ("market_qty_mult", C.c_int32),
        ("seq_start", C.c_uint64),
        ("drift_step", C.c_int32),
        ("drift_every", C.c_uint32),
        ("far_pct", C.c_uint32),
    ]


FILL_DTYPE = np.dtype(
    [("taker_seq", "<u8"), ("maker_seq", "<u8"), ("price_q4", "<i8"), ("qty", "<i4"), ("symbol", "<u4")]
)
RESULT_DTYPE = np.dtype(
    [
        ("filled_qty", "<i4"),
        ("remaining_qty", "<i4"),
        ("fill_count", "<u4"),
        ("tape_offset", "<u4"),
        ("status", "u1"),
        ("reason", "u1"),
        ("pad", "u1", (2,)),
    ]
)
LEVEL_DTYPE = np.dtype([("price_q4", "<i8"), ("total_qty", "<i8"), ("order_count", "<u4"), ("pad", "<u4")])
BOOK_ENTRY_DTYPE = np.dtype(
    [("seq", "<u8"), ("price_q4", "<i8"), ("qty", "<i4"), ("side", "u1"), ("pad", "u1", (3,))]
)
assert FILL_DTYPE.itemsize == 32 and RESULT_DTYPE.itemsize == 20
assert LEVEL_DTYPE.itemsize == 24 and BOOK_ENTRY_DTYPE.itemsize == 24
# me_quote: one top-of-book change (flags bit 0 has_bid, bit 1 has_ask)
QUOTE_DTYPE = np.dtype(
    [("bid_price_q4", "<i8"), ("ask_price_q4", "<i8"), ("bid_qty", "<i8"), ("ask_qty", "<i8"), ("batches", "<u8"),
     ("symbol", "<u4"), ("flags", "<u4")]
)
QUOTE_HAS_BID, QUOTE_HAS_ASK = 1, 2
assert QUOTE_DTYPE.itemsize == 48
# me_depth_event: one price-level change of a top-D view (qty 0 = the level left the view)
DEPTH_DTYPE = np.dtype(
    [("price_q4", "<i8"), ("qty", "<i8"), ("batches", "<u8"), ("symbol", "<u4"), ("side", "u1"), ("pad", "u1", (3,))]
)
DEPTH_MAX = 32
assert DEPTH_DTYPE.itemsize == 32
# me_trade: one symbol's trade summary (the fills since its previous event; the five last-fill fields are a me_fill)
TRADE_DTYPE = np.dtype(
    [("taker_seq", "<u8"), ("maker_seq", "<u8"), ("last_price_q4", "<i8"), ("open_price_q4", "<i8"),
     ("high_price_q4", "<i8"), ("low_price_q4", "<i8"), ("volume", "<i8"), ("trades", "<u8"), ("cum_volume", "<i8"),
     ("cum_trades", "<u8"), ("batches", "<u8"), ("last_qty", "<i4"), ("symbol", "<u4")]
)
assert TRADE_DTYPE.itemsize == 96
# me_stop: one stop / stop-limit order of the trigger book; me_stop_event: a triggered one, the NEW record it becomes
STOP_DTYPE = np.dtype(
    [("id", "<u8"), ("stop_px_q4", "<i8"), ("limit_px_q4", "<i8"), ("qty", "<i4"), ("symbol", "<u4"), ("kind", "u1"),
     ("pad", "u1", (7,))]
)
STOP_EVENT_DTYPE = np.dtype(
    [("id", "<u8"), ("stop_px_q4", "<i8"), ("limit_px_q4", "<i8"), ("trigger_px_q4", "<i8"), ("batches", "<u8"),
     ("qty", "<i4"), ("symbol", "<u4"), ("kind", "u1"), ("pad", "u1", (15,))]
)
STOPS_CAP_MAX = 1 << 22
assert STOP_DTYPE.itemsize == 40 and STOP_EVENT_DTYPE.itemsize == 64
# me_order_info: one answer of me_order_query (found 0: every field but seq is 0)
ORDER_INFO_DTYPE = np.dtype(
    [("seq", "<u8"), ("price_q4", "<i8"), ("qty_ahead", "<i8"), ("level_qty", "<i8"), ("qty_better", "<i8"),
     ("qty", "<i4"), ("orders_ahead", "<u4"), ("levels_better", "<u4"), ("symbol", "<u4"), ("side", "u1"),
     ("found", "u1"), ("pad", "u1", (6,))]
)
assert ORDER_INFO_DTYPE.itemsize == 64
# me_preview: one answer of me_order_preview (the notional is a signed 128-bit integer in two halves: preview_notional)
PREVIEW_DTYPE = np.dtype(
    [("first_price_q4", "<i8"), ("last_price_q4", "<i8"), ("opp_price_q4", "<i8"), ("notional_hi", "<i8"),
     ("notional_lo", "<u8"), ("filled_qty", "<i4"), ("remaining_qty", "<i4"), ("fill_count", "<u4"), ("levels", "<u4"),
     ("status", "u1"), ("reason", "u1"), ("flags", "u1"), ("pad", "u1", (5,))]
)
PV_HAS_OPP, PV_CROSSES, PV_RESTS = 1, 2, 4
assert PREVIEW_DTYPE.itemsize == 64


def preview_notional(row) -> int:
    """The signed 128-bit notional (sum of price_q4 * qty over the fills) of one PREVIEW_DTYPE row as a Python int."""
    return (int(row["notional_hi"]) << 64) | int(row["notional_lo"])


# ---- raw export of the resident book (me_debug_layout / me_debug_export: diagnostic) -------------------
class MeDebugInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "num_symbols", "levels", "level_words", "nchunks", "ring_mask", "old_mask", "far_levels", "far_half",
        "far_inline", "far_entries", "sq_idx", "chunk_slots", "fcache_row", "n_far_ctl", "n_cpool", "n_stats",
        "sizeof_level", "sizeof_symstate", "sizeof_chunk", "sizeof_farlevel", "sizeof_fardir", "sizeof_oldent",
        "sizeof_seqstate")]


# me_layout.hpp's structs restated (Engine.debug_export checks every itemsize against me_debug_info)
DBG_LEVEL_DTYPE = np.dtype([("total", "<i8"), ("head", "<u4"), ("tail", "<u4")])
DBG_SYM_DTYPE = np.dtype([("base", "<i8"), ("best_bid", "<i4"), ("best_ask", "<i4"), ("free_head", "<u4"),
                          ("resting", "<u4"), ("nfree", "<u4"), ("nfar", "<u4", (2,)), ("pad", "<u4", (7,))])  # alignas(64): 64 B
assert (DBG_LEVEL_DTYPE.itemsize, DBG_SYM_DTYPE.itemsize) == (16, 64)
DBG_CHUNK_DTYPE = np.dtype([("next", "<u4"), ("prev", "<u4"), ("price", "<i8"), ("owner", "<u4"),
                            ("pad", "<u4", (11,)), ("qty", "<i4", (CHUNK_SLOTS,)), ("seq", "<u8", (CHUNK_SLOTS,))])
DBG_FAR_DTYPE = np.dtype([("price", "<i8"), ("total", "<i8"), ("head", "<u4"), ("tail", "<u4"), ("tend", "<u4"),
                          ("pad", "<u4")])
DBG_FDIR_DTYPE = np.dtype([("off", "<u8"), ("cap", "<u4"), ("pad", "<u4")])
DBG_OLD_DTYPE = np.dtype([("epoch", "<u4"), ("slot", "<u4"), ("seq", "<u8")])
DBG_SQ_DTYPE = np.dtype([("horizon", "<u8"), ("last", "<u8"), ("epoch", "<u4"), ("pad", "<u4", (3,))])
assert (DBG_CHUNK_DTYPE.itemsize, DBG_FAR_DTYPE.itemsize, DBG_FDIR_DTYPE.itemsize, DBG_OLD_DTYPE.itemsize,
        DBG_SQ_DTYPE.itemsize) == (256, 32, 16, 16, 32)
# name -> (ME_DBG_* index, dtype, me_debug_info field holding sizeof of the struct or None)
DBG_ARRAYS = {
    "levels": (0, DBG_LEVEL_DTYPE, "sizeof_level"),
    "occ": (1, np.dtype("<u8"), None),
    "tend": (2, np.dtype("u1"), None),
    "sym": (3, DBG_SYM_DTYPE, "sizeof_symstate"),
    "chunks": (4, DBG_CHUNK_DTYPE, "sizeof_chunk"),
    "fcache": (5, np.dtype("<u4"), None),
    "loc": (6, np.dtype("<u4"), None),
    "old": (7, DBG_OLD_DTYPE, "sizeof_oldent"),
    "sq": (8, DBG_SQ_DTYPE, "sizeof_seqstate"),
    "far": (9, DBG_FAR_DTYPE, "sizeof_farlevel"),
    "fdir": (10, DBG_FDIR_DTYPE, "sizeof_fardir"),
    "far_ctl": (11, np.dtype("<u8"), None),
    "chunk_top": (12, np.dtype("<u4"), None),
    "recl": (13, np.dtype("<u4"), None),
    "cpool": (14, np.dtype("<u4"), None),
    "stats": (15, np.dtype("<u8"), None),
    "err": (16, np.dtype("<u4"), None),
}
# indices into the exported counter arrays (me_layout.hpp ST_*, FC_*, CP_*)
DBG_ST_RESTING = 1
DBG_FC_TOP0, DBG_FC_TOP1, DBG_FC_HALF = 0, 1, 2
DBG_CP_NRECL, DBG_CP_FRESH = 0, 1

# every symbol include/me_engine.h declares -> (restype, argtypes)
_P = C.c_void_p
_SZ = C.c_size_t
PROTOTYPES = {
    "me_normalize_to_q4": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "me_build_info": (C.c_char_p, []),
    "me_create": (_P, [C.POINTER(MeConfig)]),
    "me_destroy": (None, [_P]),
    "me_submit_batch": (C.c_int, [_P, C.POINTER(MeOrderSoa), _SZ, _P, _SZ, C.POINTER(_SZ), _P]),
    "me_fill_bound": (C.c_uint64, [_P, _SZ]),
    "me_submit_host": (C.c_int, [_P, C.POINTER(MeOrderSoa), _SZ, C.POINTER(C.c_uint64)]),
    "me_collect": (C.c_int, [_P, C.c_uint64, C.POINTER(_P), C.POINTER(_SZ), C.POINTER(_P), C.POINTER(_SZ)]),
    "me_host_inputs": (C.c_int, [_P, _SZ, C.POINTER(MeOrderSoaW)]),
    "me_get_config": (C.c_int, [_P, C.POINTER(MeConfig)]),
    "me_host_reserve": (C.c_int, [_P, C.c_uint32]),
    "me_submit_batch_device": (C.c_int, [_P, C.POINTER(MeOrderSoa), _SZ]),
    "me_submit_device_limits": (C.c_int, [_P, C.POINTER(MeOrderSoa), _SZ, C.c_uint64]),
    "me_sync": (C.c_int, [_P]),
    "me_fetch_outputs": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ), _P, _SZ]),
    "me_last_group_size": (C.c_uint32, [_P]),
    "me_fetch_group_outputs": (C.c_int, [_P, C.c_uint32, _P, _SZ, C.POINTER(_SZ), _P, _SZ]),
    "me_copy_tape_device": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ)]),
    "me_copy_results_device": (C.c_int, [_P, _P, _SZ]),
    "me_device_alloc": (C.c_int, [_P, _SZ, C.POINTER(_P)]),
    "me_device_free": (C.c_int, [_P, _P]),
    "me_memcpy_h2d": (C.c_int, [_P, _P, _P, _SZ]),
    "me_set_stream": (C.c_int, [_P, _P]),
    "me_book_snapshot": (C.c_int, [_P, C.c_uint32, _P, _P, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_book_dump": (C.c_int, [_P, C.c_uint32, _P, _SZ, C.POINTER(_SZ)]),
    "me_book_orders": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _SZ, C.POINTER(_SZ), _P, _SZ, C.POINTER(_SZ),
                                 _P, _P, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_book_levels_all": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "me_resting_count": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "me_order_query": (C.c_int, [_P, _P, _SZ, _P]),
    "me_order_preview": (C.c_int, [_P, C.POINTER(MeOrderSoa), _SZ, _P]),
    "me_mass_cancel": (C.c_int, [_P, _P, _P, _SZ, _P, _SZ, C.POINTER(_SZ), _P]),
    "me_timing_enable": (C.c_int, [_P, C.c_int]),
    "me_timing_read": (
        C.c_int,
        [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
         C.POINTER(C.c_uint64)],
    ),
    "me_last_error": (C.c_int, [_P, C.c_char_p, _SZ]),
    "me_stats_read": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "me_hot_stats_read": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "me_far_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "me_chunk_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "me_paths_read": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "me_debug_layout": (C.c_int, [_P, C.POINTER(MeDebugInfo)]),
    "me_debug_export": (C.c_int, [_P, C.c_uint32, _P, _SZ, C.POINTER(_SZ)]),
    "me_admission_read": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "me_admission_check": (C.c_int, [_P, C.c_uint64, C.POINTER(C.c_int)]),
    "me_quotes_enable": (C.c_int, [_P, C.c_uint64]),
    "me_quotes_read": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_quotes_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "me_depth_enable": (C.c_int, [_P, C.c_uint32, C.c_uint64]),
    "me_depth_read": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_depth_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "me_trades_enable": (C.c_int, [_P, C.c_uint64]),
    "me_trades_read": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_trades_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "me_stops_enable": (C.c_int, [_P, C.c_uint64]),
    "me_stops_add": (C.c_int, [_P, _P, _SZ]),
    "me_stops_cancel": (C.c_int, [_P, _P, _SZ, _P]),
    "me_stops_read": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_stops_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "me_stops_dump": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ)]),
    "me_gen_create": (_P, [C.POINTER(MeGenParams)]),
    "me_gen_destroy": (None, [_P]),
    "me_gen_base_prices": (C.c_int, [_P, _P]),
    "me_gen_next": (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P]),
    "me_gen_seed_book": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, _P, _P]),
    "me_shard_of": (C.c_uint32, [C.c_uint32, C.c_uint32]),
}

_lib = None


def load() -> C.CDLL:
    """Load libme_engine.so (built in-tree). Raises if it is missing: no fallback exists."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `make -C matching_engine_amd` "
            "(the matching path has no CPU/Python fallback)"
        )
    # libme_engine.so and torch's ROCm wheel both need libamdhip64.so.7; torch resolves it by a
    # different file name, so if our library were loaded first the process would end up with two
    # HIP runtimes. Letting torch (when installed) load first keeps one runtime per process.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    variant = bool(os.environ.get("ME_ENGINE_LIB"))  # an older build in an A/B run may lack newer entries
    for name, (res, args) in PROTOTYPES.items():
        if variant and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def ptr(a: np.ndarray) -> int:
    return a.ctypes.data


# ---- include/me_service.h ---------------------------------------------------------------------
class MeOrderRequest(C.Structure):
    _fields_ = [
        ("client_id", C.c_char_p),
        ("symbol", C.c_char_p),
        ("order_type", C.c_int32),
        ("side", C.c_int32),
        ("price", C.c_int64),
        ("scale", C.c_int32),
        ("quantity", C.c_int32),
    ]


class MeOrderResponse(C.Structure):
    _fields_ = [
        ("order_id", C.c_char * 32),
        ("success", C.c_int32),
        ("grpc_status", C.c_int32),
        ("error_message", C.c_char * 64),
    ]


class MeCancelRequest(C.Structure):
    _fields_ = [
        ("client_id", C.c_char_p),
        ("symbol", C.c_char_p),
        ("order_id", C.c_char_p),
    ]


class MeReduceRequest(C.Structure):
    _fields_ = [
        ("client_id", C.c_char_p),
        ("symbol", C.c_char_p),
        ("order_id", C.c_char_p),
        ("quantity", C.c_int32),
    ]


class MeOrderUpdate(C.Structure):
    _fields_ = [
        ("order_id", C.c_char * 32),
        ("client_id", C.c_char * 64),
        ("symbol", C.c_char * 32),
        ("status", C.c_int32),
        ("scale", C.c_int32),
        ("fill_price", C.c_int64),
        ("fill_quantity", C.c_int32),
        ("remaining_quantity", C.c_int32),
    ]


assert C.sizeof(MeOrderUpdate) == 152, "me_order_update layout"


# stop orders through the service (me_service_stops_enable / _submit_stop / _cancel_stop / _stop_updates / _stops)
SS_ARMED, SS_TRIGGERED, SS_CANCELED, SS_CANCEL_REJECTED, SS_QUEUED = 0, 1, 2, 3, 4


class MeStopRequest(C.Structure):
    _fields_ = [
        ("client_id", C.c_char_p),
        ("symbol", C.c_char_p),
        ("order_type", C.c_int32),
        ("side", C.c_int32),
        ("price", C.c_int64),
        ("stop_price", C.c_int64),
        ("scale", C.c_int32),
        ("quantity", C.c_int32),
        ("tif", C.c_int32),
    ]


class MeStopCancelRequest(C.Structure):
    _fields_ = [
        ("client_id", C.c_char_p),
        ("stop_id", C.c_char_p),
    ]


class MeStopUpdate(C.Structure):
    _fields_ = [
        ("stop_id", C.c_char * 32),
        ("order_id", C.c_char * 32),
        ("client_id", C.c_char * 64),
        ("symbol", C.c_char * 32),
        ("state", C.c_int32),
        ("scale", C.c_int32),
        ("stop_price", C.c_int64),
        ("limit_price", C.c_int64),
        ("trigger_price", C.c_int64),
        ("quantity", C.c_int32),
        ("kind", C.c_uint8),
        ("pad", C.c_uint8 * 3),
    ]


assert C.sizeof(MeStopRequest) == 56 and C.sizeof(MeStopCancelRequest) == 16, "me_stop_request layout"
assert C.sizeof(MeStopUpdate) == 200, "me_stop_update layout"


class MeMarketData(C.Structure):
    _fields_ = [
        ("best_bid", C.c_int64),
        ("best_ask", C.c_int64),
        ("scale", C.c_int32),
        ("bid_size", C.c_int32),
        ("ask_size", C.c_int32),
        ("has_bid", C.c_int32),
        ("has_ask", C.c_int32),
        ("pad", C.c_int32),
    ]

class MeMarketUpdate(C.Structure):
    _fields_ = [("symbol", C.c_char * 32), ("md", MeMarketData)]


assert C.sizeof(MeMarketUpdate) == 72, "me_market_update layout"


class MeDepthLevel(C.Structure):
    _fields_ = [("price", C.c_int64), ("size", C.c_int32), ("pad", C.c_int32)]


class MeDepthBook(C.Structure):
    _fields_ = [
        ("symbol", C.c_char * 32),
        ("scale", C.c_int32),
        ("n_bids", C.c_uint32),
        ("n_asks", C.c_uint32),
        ("pad", C.c_uint32),
        ("bids", MeDepthLevel * DEPTH_MAX),
        ("asks", MeDepthLevel * DEPTH_MAX),
    ]


assert C.sizeof(MeDepthLevel) == 16 and C.sizeof(MeDepthBook) == 48 + 2 * 16 * DEPTH_MAX, "me_depth_book layout"


class MeTradeUpdate(C.Structure):
    _fields_ = [
        ("symbol", C.c_char * 32),
        ("scale", C.c_int32),
        ("last_size", C.c_int32),
        ("last_price", C.c_int64),
        ("open_price", C.c_int64),
        ("high_price", C.c_int64),
        ("low_price", C.c_int64),
        ("volume", C.c_int64),
        ("trades", C.c_uint64),
        ("cum_volume", C.c_int64),
        ("cum_trades", C.c_uint64),
    ]


assert C.sizeof(MeTradeUpdate) == 104, "me_trade_update layout"


class MeBookOrder(C.Structure):
    _fields_ = [
        ("order_id", C.c_char * 32),
        ("client_id", C.c_char * 64),
        ("price", C.c_int64),
        ("scale", C.c_int32),
        ("quantity", C.c_int32),
        ("side", C.c_int32),
        ("pad", C.c_int32),
    ]


assert C.sizeof(MeBookOrder) == 120, "me_book_order layout"

OS_NOT_RESTING, OS_PENDING, OS_RESTING = 0, 1, 2


class MeOrderStatus(C.Structure):
    _fields_ = [
        ("order_id", C.c_char * 32),
        ("state", C.c_int32),
        ("side", C.c_int32),
        ("scale", C.c_int32),
        ("quantity", C.c_int32),
        ("price", C.c_int64),
        ("qty_ahead", C.c_int64),
        ("level_qty", C.c_int64),
        ("qty_better", C.c_int64),
        ("orders_ahead", C.c_uint32),
        ("levels_better", C.c_uint32),
    ]


assert C.sizeof(MeOrderStatus) == 88, "me_order_status layout"

MATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(MeOrderSoa), C.c_size_t, C.POINTER(C.c_void_p),
                       C.POINTER(C.c_size_t), C.POINTER(C.c_void_p))
BOOK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                      C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t),
                      C.POINTER(C.c_size_t))
SUBMIT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(MeOrderSoa), C.c_size_t, C.POINTER(C.c_uint64))
COLLECT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                         C.POINTER(C.c_void_p))
QUOTES_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t))
# the depth and trade feeds' readers have QUOTES_FN's shape (events out, cap, n, left)
DEPTH_ENABLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint64)
TRADES_ENABLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64)
ORDER_QUERY_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.c_void_p)
ORDER_PREVIEW_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(MeOrderSoa), C.c_size_t, C.c_void_p)
# the optional hooks me_matcher and me_shard_ops share after `quotes`, in declaration order
PARITY_HOOKS = [
    ("depth_enable", DEPTH_ENABLE_FN),
    ("depth", QUOTES_FN),
    ("trades_enable", TRADES_ENABLE_FN),
    ("trades", QUOTES_FN),
    ("order_query", ORDER_QUERY_FN),
    ("order_preview", ORDER_PREVIEW_FN),
]


# me_matcher's stop hooks (all four or none; me_shard_ops has none: the cluster carries no stop orders)
STOPS_ENABLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64)
STOPS_ADD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
STOPS_CANCEL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint8))
STOP_HOOKS = [
    ("stops_enable", STOPS_ENABLE_FN),
    ("stops_add", STOPS_ADD_FN),
    ("stops_cancel", STOPS_CANCEL_FN),
    ("stops_read", QUOTES_FN),
]


class MeMatcher(C.Structure):
    """The HEAD of me_matcher: its members up to order_preview, the ones me_shard_ops shares. NEVER ALLOCATE IT:
    it is 32 bytes shorter than the C struct, which me_service_create_matcher reads and me_cluster_matcher clears
    in full. MeMatcherStops below is the whole struct; the prototypes take only that one."""
    _fields_ = [
        ("ctx", C.c_void_p),
        ("num_symbols", C.c_uint32),
        ("max_batch", C.c_uint32),
        ("max_resting", C.c_uint64),
        ("match", MATCH_FN),
        ("book", BOOK_FN),
        ("submit", SUBMIT_FN),
        ("collect", COLLECT_FN),
        ("quotes", QUOTES_FN),
    ] + PARITY_HOOKS


class MeMatcherStops(MeMatcher):
    """me_matcher as include/me_service.h declares it: MeMatcher's members (the struct up to order_preview, the
    members me_shard_ops shares), then the four stop hooks. ALLOCATE THIS ONE: me_cluster_matcher clears, and
    me_service_create_matcher reads, sizeof(me_matcher) bytes. A fresh instance is all zero: no stop orders."""
    _fields_ = STOP_HOOKS


# ---- include/me_cluster.h ---------------------------------------------------------------------
TRANSPORT_RCCL, TRANSPORT_TCP = 0, 1


class MeClusterConfig(C.Structure):
    _fields_ = [
        ("rank", C.c_uint32),
        ("world", C.c_uint32),
        ("num_symbols", C.c_uint32),
        ("max_batch", C.c_uint32),
        ("transport", C.c_int32),
        ("device", C.c_int32),
        ("addr", C.c_char_p),
        ("port", C.c_uint32),
        ("timeout_ms", C.c_uint32),
    ]


ADMIT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_int))
LEVELS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)


class MeShardOps(C.Structure):
    _fields_ = [
        ("ctx", C.c_void_p),
        ("max_resting", C.c_uint64),
        ("admit", ADMIT_FN),
        ("match", MATCH_FN),
        ("book", BOOK_FN),
        ("levels_all", LEVELS_FN),
        ("quotes", QUOTES_FN),
    ] + PARITY_HOOKS


PROTOTYPES.update({
    "me_service_create_matcher": (_P, [C.POINTER(MeMatcherStops), C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p]),
    "me_service_order_book": (C.c_int, [_P, C.c_char_p, C.c_uint32, C.POINTER(MeBookOrder), _SZ, C.POINTER(_SZ),
                                        C.POINTER(MeBookOrder), _SZ, C.POINTER(_SZ)]),
    "me_service_order_status": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_char_p), _SZ, C.POINTER(MeOrderStatus)]),
    "me_service_preview_order": (C.c_int, [_P, C.POINTER(MeOrderRequest), C.c_int32, _P]),
    "me_service_mass_cancel": (C.c_int, [_P, C.POINTER(C.c_char_p), _SZ, C.c_int32, C.POINTER(C.c_uint64)]),
    "me_service_cancel_order": (C.c_int, [_P, C.POINTER(MeCancelRequest), C.POINTER(MeOrderResponse)]),
    "me_service_reduce_order": (C.c_int, [_P, C.POINTER(MeReduceRequest), C.POINTER(MeOrderResponse)]),
    "me_service_market_data": (C.c_int, [_P, C.c_char_p, C.POINTER(MeMarketData)]),
    "me_service_market_subscribe": (C.c_int, [_P, C.c_int]),
    "me_service_market_stream": (C.c_int, [_P, C.c_char_p, C.POINTER(MeMarketUpdate), _SZ, C.POINTER(_SZ)]),
    "me_service_depth_subscribe": (C.c_int, [_P, C.c_uint32]),
    "me_service_depth_stream": (C.c_int, [_P, C.c_char_p, C.POINTER(MeDepthBook), _SZ, C.POINTER(_SZ)]),
    "me_service_trades_subscribe": (C.c_int, [_P, C.c_int]),
    "me_service_trades_stream": (C.c_int, [_P, C.c_char_p, C.POINTER(MeTradeUpdate), _SZ, C.POINTER(_SZ)]),
    "me_service_stops_enable": (C.c_int, [_P, C.c_uint64]),
    "me_service_submit_stop": (C.c_int, [_P, C.POINTER(MeStopRequest), C.POINTER(MeOrderResponse)]),
    "me_service_cancel_stop": (C.c_int, [_P, C.POINTER(MeStopCancelRequest), C.POINTER(MeOrderResponse)]),
    "me_service_stop_updates": (C.c_int, [_P, C.c_char_p, C.POINTER(MeStopUpdate), _SZ, C.POINTER(_SZ)]),
    "me_service_stops": (C.c_int, [_P, C.c_char_p, C.POINTER(MeStopUpdate), _SZ, C.POINTER(_SZ)]),
    "me_service_stop_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "me_cluster_quotes_enable": (C.c_int, [_P, C.c_uint64]),
    "me_cluster_quotes": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_cluster_depth_enable": (C.c_int, [_P, C.c_uint32, C.c_uint64]),
    "me_cluster_depth": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_cluster_trades_enable": (C.c_int, [_P, C.c_uint64]),
    "me_cluster_trades": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_cluster_order_query": (C.c_int, [_P, _P, _SZ, _P]),
    "me_cluster_order_preview": (C.c_int, [_P, C.POINTER(MeOrderSoa), _SZ, _P]),
    "me_service_updates": (C.c_int, [_P, C.c_char_p, C.POINTER(MeOrderUpdate), _SZ, C.POINTER(_SZ)]),
    "me_service_create": (_P, [_P, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p]),
    "me_service_destroy": (None, [_P]),
    "me_service_submit_order": (C.c_int, [_P, C.POINTER(MeOrderRequest), C.POINTER(MeOrderResponse)]),
    "me_service_submit_order_tif": (C.c_int, [_P, C.POINTER(MeOrderRequest), C.c_int32, C.POINTER(MeOrderResponse)]),
    "me_service_pending": (_SZ, [_P]),
    "me_service_next_oid": (C.c_uint64, [_P]),
    "me_service_flush": (C.c_int, [_P, _P, _SZ, C.POINTER(_SZ), _P, _P, _SZ, C.POINTER(_SZ)]),
    "me_service_book": (C.c_int, [_P, C.c_char_p, _P, _P, _SZ, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_service_last_error": (C.c_int, [_P, C.c_char_p, _SZ]),
    "me_service_unpersisted": (_SZ, [_P]),
    "me_service_submit_orders": (C.c_int, [_P, C.POINTER(MeOrderRequest), _SZ, C.POINTER(MeOrderResponse)]),
    "me_service_start": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "me_service_stop": (C.c_int, [_P]),
    "me_service_updates_dropped": (C.c_uint64, [_P]),
    "me_service_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "me_cluster_shard_symbols": (_SZ, [C.c_uint32, C.c_uint32, C.c_uint32, _P, _SZ]),
    "me_cluster_create": (_P, [C.POINTER(MeClusterConfig), C.POINTER(MeConfig), C.POINTER(MeShardOps)]),
    "me_cluster_stop": (C.c_int, [_P]),
    "me_cluster_destroy": (None, [_P]),
    "me_cluster_serve": (C.c_int, [_P]),
    "me_cluster_submit": (C.c_int, [_P, C.POINTER(MeOrderSoa), _SZ, C.POINTER(C.c_uint64)]),
    "me_cluster_collect": (C.c_int, [_P, C.c_uint64, C.POINTER(_P), C.POINTER(_SZ), C.POINTER(_P)]),
    "me_cluster_match": (C.c_int, [_P, C.POINTER(MeOrderSoa), _SZ, C.POINTER(_P), C.POINTER(_SZ), C.POINTER(_P)]),
    "me_cluster_book": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _SZ, C.POINTER(_SZ), _P, _SZ, C.POINTER(_SZ),
                                  _P, _P, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "me_cluster_snapshot": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "me_cluster_matcher": (C.c_int, [_P, C.POINTER(MeMatcherStops)]),
    "me_cluster_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "me_cluster_phases": (C.c_int, [_P, C.POINTER(C.c_double), _SZ]),
    "me_cluster_last_error": (C.c_int, [_P, C.c_char_p, _SZ]),
    "me_cluster_host_probe": (C.c_int, [C.c_uint32, C.c_uint32, _P, _SZ, C.c_double, C.c_uint32, _P]),
})
