"""Host-side mirror of the batched matching core (C-ABI include/me_engine.h).

``Engine`` is one shard (one GPU): HBM-resident books for ``num_symbols`` local symbols, driven
batch by batch. Every call goes through libme_engine.so; nothing here computes a match.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi
from ._abi import BOOK_ENTRY_DTYPE, FILL_DTYPE, LEVEL_DTYPE, RESULT_DTYPE, MeConfig, MeGenParams, MeOrderSoa, ptr


class EngineError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"me error {code}: {msg}")
        self.code = code


def _check(lib, handle, rc: int) -> None:
    if rc != _abi.ME_OK:
        buf = C.create_string_buffer(1024)
        lib.me_last_error(handle, buf, 1024)
        raise EngineError(rc, buf.value.decode(errors="replace"))


def _view(addr, n: int, dtype) -> np.ndarray:
    """numpy view of n records at a C address (no copy)."""
    if not n:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * dtype.itemsize)).from_address(addr)
    return np.frombuffer(buf, dtype=dtype, count=n)


def normalize_to_q4(price: int, scale: int) -> int:
    """include/domain/price.hpp:15-29 through the product library; raises like the reference."""
    lib = _abi.load()
    out = C.c_int64(0)
    rc = lib.me_normalize_to_q4(int(price), int(scale), C.byref(out))
    if rc == 1:
        raise ValueError("scale out of range")
    if rc == 2:
        raise OverflowError("overflow")
    if rc == 3:
        raise OverflowError("underflow")
    return out.value


@dataclass
class Batch:
    """One batch in SoA form (host numpy arrays), ascending seq."""

    seq: np.ndarray
    price_q4: np.ndarray
    qty: np.ndarray
    symbol: np.ndarray
    kind: np.ndarray

    def __post_init__(self):
        self.seq = np.ascontiguousarray(self.seq, dtype=np.uint64)
        self.price_q4 = np.ascontiguousarray(self.price_q4, dtype=np.int64)
        self.qty = np.ascontiguousarray(self.qty, dtype=np.int32)
        self.symbol = np.ascontiguousarray(self.symbol, dtype=np.uint32)
        self.kind = np.ascontiguousarray(self.kind, dtype=np.uint8)
        n = len(self.seq)
        assert all(len(a) == n for a in (self.price_q4, self.qty, self.symbol, self.kind))

    def __len__(self) -> int:
        return len(self.seq)

    def take(self, idx) -> "Batch":
        return Batch(self.seq[idx], self.price_q4[idx], self.qty[idx], self.symbol[idx], self.kind[idx])

    def soa(self) -> MeOrderSoa:
        return MeOrderSoa(ptr(self.seq), ptr(self.price_q4), ptr(self.qty), ptr(self.symbol), ptr(self.kind))


class DeviceBatch:
    """A batch copied once into HBM (me_device_alloc), for device-resident submission."""

    def __init__(self, engine: "Engine", b: Batch):
        self.engine = engine
        self.n = len(b)
        self.ptrs = []
        for a in (b.seq, b.price_q4, b.qty, b.symbol, b.kind):
            p = C.c_void_p()
            _check(engine.lib, engine.h, engine.lib.me_device_alloc(engine.h, max(a.nbytes, 1), C.byref(p)))
            if a.nbytes:
                _check(engine.lib, engine.h, engine.lib.me_memcpy_h2d(engine.h, p, ptr(a), a.nbytes))
            self.ptrs.append(p.value)
        self._soa = MeOrderSoa(*self.ptrs)

    def free(self):
        for p in self.ptrs:
            self.engine.lib.me_device_free(self.engine.h, p)
        self.ptrs = []


class Engine:
    """One shard of HBM-resident books (include/me_engine.h me_create ... me_destroy).

    `levels` is the depth of each symbol's on-chip window; `base_prices` only its initial position:
    any int64 price is accepted (far levels + re-centring) and any u64 seq (the seq ring, `seq_ring`
    entries, 0 = 2^28)."""

    def __init__(
        self,
        num_symbols: int,
        levels: int,
        base_prices,
        max_batch: int,
        max_resting: int,
        seq_ring: int = 0,
        max_chunks: int = 0,
        device: int = 0,
        symbol_ids=None,
        batches_per_launch: int = 0,
        far_levels: int = 0,
        host_slots: int = 0,
        host_tape_cap: int = 0,
    ):
        self.lib = _abi.load()
        self.num_symbols = int(num_symbols)
        self.levels = int(levels)
        self._base = np.ascontiguousarray(base_prices, dtype=np.int64)
        assert len(self._base) == num_symbols
        self._ids = None if symbol_ids is None else np.ascontiguousarray(symbol_ids, dtype=np.uint32)
        cfg = MeConfig(
            device,
            num_symbols,
            levels,
            max_batch,
            max_resting,
            max_chunks,
            seq_ring,
            self._base.ctypes.data_as(C.POINTER(C.c_int64)),
            None if self._ids is None else self._ids.ctypes.data_as(C.POINTER(C.c_uint32)),
            batches_per_launch,
            far_levels,
            host_slots,
            host_tape_cap,
        )
        self.max_batch = int(max_batch)
        self._depth = 0  # levels per side of the depth feed (depth_enable), 0 while it is off
        self._stops_cap = 0  # the trigger book's capacity (stops_enable), 0 while it is off
        h = self.lib.me_create(C.byref(cfg))
        if not h:
            buf = C.create_string_buffer(1024)
            self.lib.me_last_error(None, buf, 1024)
            raise EngineError(_abi.ME_E_HIP, buf.value.decode(errors="replace"))
        self.h = h

    # -- lifecycle
    def close(self):
        if getattr(self, "h", None):
            self.lib.me_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- batches
    def fill_bound(self, n: int) -> int:
        return int(self.lib.me_fill_bound(self.h, n))

    def submit_batch(self, b: Batch, want_fills: bool = True):
        """Host batch -> (results[n] RESULT_DTYPE, fills[k] FILL_DTYPE), synchronous."""
        n = len(b)
        res = np.zeros(n, dtype=RESULT_DTYPE)
        cap = self.fill_bound(n) if want_fills else 0
        fills = np.zeros(cap, dtype=FILL_DTYPE) if want_fills else None
        nf = C.c_size_t(0)
        soa = b.soa()
        rc = self.lib.me_submit_batch(
            self.h, C.byref(soa), n, ptr(fills) if want_fills else None, cap, C.byref(nf), ptr(res)
        )
        _check(self.lib, self.h, rc)
        return res, (fills[: nf.value].copy() if want_fills else nf.value)

    # -- pipelined host batches (me_submit_host / me_collect)
    def submit_host(self, b: Batch) -> int:
        """Enqueue a host batch (staged into the next pinned slot unless it already lives there, see
        host_inputs); returns its ticket at once."""
        t = C.c_uint64(0)
        soa = b.soa()
        _check(self.lib, self.h, self.lib.me_submit_host(self.h, C.byref(soa), len(b), C.byref(t)))
        return t.value

    def collect(self, ticket: int, copy: bool = True):
        """(results[n], fills[k]) of a ticket. copy=False returns views of the slot's pinned memory, valid
        until the next collect, or until a submit_host / host_inputs call that finds every other slot busy
        and takes the held slot back (me_collect's contract, include/me_engine.h)."""
        fp, rp = C.c_void_p(), C.c_void_p()
        nf, nr = C.c_size_t(0), C.c_size_t(0)
        _check(self.lib, self.h,
               self.lib.me_collect(self.h, ticket, C.byref(fp), C.byref(nf), C.byref(rp), C.byref(nr)))
        res = _view(rp.value, nr.value, RESULT_DTYPE)
        fills = _view(fp.value, nf.value, FILL_DTYPE)
        return (res.copy(), fills.copy()) if copy else (res, fills)

    def host_inputs(self, n: int) -> Batch:
        """Writable numpy views of the pinned arrays the next submit_host takes for an n-record batch
        (fill them in place, then submit_host the returned Batch: no staging copy)."""
        w = _abi.MeOrderSoaW()
        _check(self.lib, self.h, self.lib.me_host_inputs(self.h, n, C.byref(w)))
        arrs = [_view(getattr(w, f), n, np.dtype(t)) for f, t in
                (("seq", "<u8"), ("price_q4", "<i8"), ("qty", "<i4"), ("symbol", "<u4"), ("kind", "u1"))]
        return Batch(*arrs)

    def host_reserve(self, nslots: int = 0):
        """Allocate host slots now (0 = all) rather than on first use."""
        _check(self.lib, self.h, self.lib.me_host_reserve(self.h, nslots))

    def config(self) -> dict:
        cfg = MeConfig()
        _check(self.lib, self.h, self.lib.me_get_config(self.h, C.byref(cfg)))
        return {f: getattr(cfg, f) for f, _ in MeConfig._fields_ if f not in ("base_price", "symbol_ids")}

    def upload(self, b: Batch) -> DeviceBatch:
        return DeviceBatch(self, b)

    def submit_device(self, db: DeviceBatch):
        _check(self.lib, self.h, self.lib.me_submit_batch_device(self.h, C.byref(db._soa), db.n))

    def sync(self):
        _check(self.lib, self.h, self.lib.me_sync(self.h))

    def fetch_outputs(self, n: int):
        res = np.zeros(n, dtype=RESULT_DTYPE)
        nf = C.c_size_t(0)
        _check(self.lib, self.h, self.lib.me_fetch_outputs(self.h, None, 0, C.byref(nf), ptr(res), n))
        fills = np.zeros(nf.value, dtype=FILL_DTYPE)
        _check(self.lib, self.h, self.lib.me_fetch_outputs(self.h, ptr(fills), nf.value, C.byref(nf), None, 0))
        return res, fills

    def last_group_size(self) -> int:
        return int(self.lib.me_last_group_size(self.h))

    def fetch_group_outputs(self, k: int, n: int):
        """Outputs of the k-th batch (n records) of the most recent launch group."""
        res = np.zeros(n, dtype=RESULT_DTYPE)
        nf = C.c_size_t(0)
        _check(self.lib, self.h, self.lib.me_fetch_group_outputs(self.h, k, None, 0, C.byref(nf), ptr(res), n))
        fills = np.zeros(nf.value, dtype=FILL_DTYPE)
        _check(self.lib, self.h, self.lib.me_fetch_group_outputs(self.h, k, ptr(fills), nf.value, C.byref(nf),
                                                                 None, 0))
        return res, fills

    def copy_tape_device(self, dst_ptr: int, cap_fills: int) -> int:
        """Last batch's tape -> device buffer at dst_ptr (engine stream); returns its length."""
        nf = C.c_size_t(0)
        _check(self.lib, self.h, self.lib.me_copy_tape_device(self.h, dst_ptr, cap_fills, C.byref(nf)))
        return nf.value

    def copy_results_device(self, dst_ptr: int, n: int):
        """Last batch's n per-record results -> device buffer at dst_ptr (engine stream)."""
        _check(self.lib, self.h, self.lib.me_copy_results_device(self.h, dst_ptr, n))

    def set_stream(self, stream_handle: int | None):
        _check(self.lib, self.h, self.lib.me_set_stream(self.h, stream_handle))

    # -- book inspection
    def snapshot(self, symbol: int, depth: int = 10):
        bids = np.zeros(depth, dtype=LEVEL_DTYPE)
        asks = np.zeros(depth, dtype=LEVEL_DTYPE)
        nb, na = C.c_size_t(0), C.c_size_t(0)
        rc = self.lib.me_book_snapshot(self.h, symbol, ptr(bids), ptr(asks), depth, C.byref(nb), C.byref(na))
        _check(self.lib, self.h, rc)
        return bids[: nb.value], asks[: na.value]

    def book_orders(self, symbol: int, depth: int):
        """GetOrderBook per order from one device snapshot launch: (bids, asks) BOOK_ENTRY_DTYPE in
        priority order over the top `depth` levels per side, and (bid_levels, ask_levels)."""
        nb, na, nlb, nla = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        lb = np.zeros(max(depth, 1), dtype=LEVEL_DTYPE)
        la = np.zeros(max(depth, 1), dtype=LEVEL_DTYPE)
        _check(self.lib, self.h, self.lib.me_book_orders(self.h, symbol, depth, None, 0, C.byref(nb), None, 0,
                                                         C.byref(na), ptr(lb), ptr(la), C.byref(nlb), C.byref(nla)))
        bids = np.zeros(nb.value, dtype=BOOK_ENTRY_DTYPE)
        asks = np.zeros(na.value, dtype=BOOK_ENTRY_DTYPE)
        _check(self.lib, self.h, self.lib.me_book_orders(self.h, symbol, depth, ptr(bids), len(bids), C.byref(nb),
                                                         ptr(asks), len(asks), C.byref(na), None, None, None, None))
        return bids, asks, lb[: nlb.value], la[: nla.value]

    def levels_all(self, depth: int):
        """Top `depth` levels per side of every symbol (one launch): (levels[S, 2, depth], counts[S, 2])."""
        lv = np.zeros(self.num_symbols * 2 * depth, dtype=LEVEL_DTYPE)
        cnt = np.zeros(self.num_symbols * 2, dtype=np.uint32)
        _check(self.lib, self.h, self.lib.me_book_levels_all(self.h, depth, ptr(lv), ptr(cnt)))
        return lv.reshape(self.num_symbols, 2, depth), cnt.reshape(self.num_symbols, 2)

    def dump(self, symbol: int) -> np.ndarray:
        n = C.c_size_t(0)
        _check(self.lib, self.h, self.lib.me_book_dump(self.h, symbol, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=BOOK_ENTRY_DTYPE)
        _check(self.lib, self.h, self.lib.me_book_dump(self.h, symbol, ptr(out), n.value, C.byref(n)))
        return out

    def mass_cancel(self, symbols, sides=3):
        """me_mass_cancel: remove every resting order of `sides` (SIDE_BUY = 1, SIDE_SELL = 2, 3 = both; one value
        or one per symbol) of `symbols`. Returns (entries, counts): the removed orders in dump()'s dtype, request
        by request in dump()'s order, and counts[i] = (bids, asks) removed for symbols[i]."""
        sym = np.ascontiguousarray(symbols, dtype=np.uint32).reshape(-1)
        sd = np.ascontiguousarray(np.broadcast_to(np.asarray(sides, dtype=np.uint8), sym.shape))
        counts = np.zeros((len(sym), 2), dtype=np.uint64)
        n = C.c_size_t(0)
        out = np.zeros(0, dtype=BOOK_ENTRY_DTYPE)
        rc = self.lib.me_mass_cancel(self.h, ptr(sym), ptr(sd), len(sym), None, 0, C.byref(n), ptr(counts))
        if rc == _abi.ME_E_CAPACITY and n.value:  # sized from *n_out, once
            out = np.zeros(n.value, dtype=BOOK_ENTRY_DTYPE)
            rc = self.lib.me_mass_cancel(self.h, ptr(sym), ptr(sd), len(sym), ptr(out), len(out), C.byref(n), ptr(counts))
        _check(self.lib, self.h, rc)
        return out[:n.value], counts

    def order_query(self, seqs) -> np.ndarray:
        """me_order_query: one ORDER_INFO_DTYPE answer per seq (what the order still holds, its place in its
        level's FIFO, what rests at better prices of its side), from one launch on the current books."""
        q = np.ascontiguousarray(seqs, dtype=np.uint64).reshape(-1)
        out = np.zeros(len(q), dtype=_abi.ORDER_INFO_DTYPE)
        _check(self.lib, self.h, self.lib.me_order_query(self.h, ptr(q), len(q), ptr(out)))
        return out

    def order_preview(self, symbol, kind, price_q4, qty) -> np.ndarray:
        """me_order_preview: one PREVIEW_DTYPE answer per hypothetical NEW record (symbol, kind, price_q4, qty) —
        what it would execute against the books as they stand, from one read-only launch. Four equal-length
        arrays, or scalars (broadcast against the others). Nothing is submitted and nothing changes."""
        sy, kd, px, qt = np.broadcast_arrays(np.asarray(symbol, dtype=np.uint32), np.asarray(kind, dtype=np.uint8),
                                             np.asarray(price_q4, dtype=np.int64), np.asarray(qty, dtype=np.int32))
        sy, kd, px, qt = (np.ascontiguousarray(a).reshape(-1) for a in (sy, kd, px, qt))
        out = np.zeros(len(sy), dtype=_abi.PREVIEW_DTYPE)
        soa = MeOrderSoa(None, ptr(px), ptr(qt), ptr(sy), ptr(kd))
        _check(self.lib, self.h, self.lib.me_order_preview(self.h, C.byref(soa), len(sy), ptr(out)))
        return out

    def resting_count(self) -> int:
        v = C.c_uint64(0)
        _check(self.lib, self.h, self.lib.me_resting_count(self.h, C.byref(v)))
        return v.value

    def stats(self) -> dict:
        """Device event counters since creation (me_stats_read, me_hot_stats_read)."""
        h, hh = C.c_uint64(0), C.c_uint64(0)
        _check(self.lib, self.h, self.lib.me_stats_read(self.h, C.byref(h)))
        if hasattr(self.lib, "me_hot_stats_read"):  # (absent from an older build loaded through ME_ENGINE_LIB)
            _check(self.lib, self.h, self.lib.me_hot_stats_read(self.h, C.byref(hh)))
        return {"handoffs": h.value, "hot_handoffs": hh.value}

    def far_stats(self) -> dict:
        """The far arena (me_far_stats): sides moved to a larger region, collections, entries in use."""
        m, g, u = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(self.lib, self.h, self.lib.me_far_stats(self.h, C.byref(m), C.byref(g), C.byref(u)))
        return {"moves": m.value, "collections": g.value, "arena_used": u.value}

    def chunk_stats(self) -> dict:
        """The FIFO chunk pool (me_chunk_stats): reclamations, chunk ids ever handed out, pool size."""
        r, h, p = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(self.lib, self.h, self.lib.me_chunk_stats(self.h, C.byref(r), C.byref(h), C.byref(p)))
        return {"reclaims": r.value, "high_water": h.value, "pool": p.value}

    def paths(self) -> dict:
        """The matching paths running now (me_paths_read): grouped launches / hot symbols through the
        aggregate path (me_agg.hip)."""
        f = C.c_uint32(0)
        _check(self.lib, self.h, self.lib.me_paths_read(self.h, C.byref(f)))
        return {"grouped_agg": bool(f.value & 1), "hot_agg": bool(f.value & 2), "grouped_cancels": bool(f.value & 4)}

    def debug_export(self, which=None) -> dict:
        """DIAGNOSTIC (me_debug_layout / me_debug_export): the resident book's device arrays as the kernels
        left them, after everything enqueued was matched. Returns {"info": the me_debug_info fields, name:
        structured array ...} for the names in `which` (default: every array of _abi.DBG_ARRAYS); per-symbol
        arrays come back shaped [S][...]. Raises when a struct's size differs from its dtype's here."""
        info = _abi.MeDebugInfo()
        _check(self.lib, self.h, self.lib.me_debug_layout(self.h, C.byref(info)))
        inf = {n: int(getattr(info, n)) for n, _ in _abi.MeDebugInfo._fields_}
        for name, (_, dt, szf) in _abi.DBG_ARRAYS.items():
            if szf is not None and inf[szf] != dt.itemsize:
                raise RuntimeError(f"debug_export: {name}: the library's {szf} = {inf[szf]}, the dtype holds {dt.itemsize} B")
        if inf["chunk_slots"] != _abi.CHUNK_SLOTS or inf["fcache_row"] != 64:
            raise RuntimeError(f"debug_export: chunk_slots / fcache_row drifted: {inf}")
        S, L, W = inf["num_symbols"], inf["levels"], inf["level_words"]
        shapes = {"levels": (S, L), "occ": (S, W), "tend": (S, L), "fcache": (S, inf["fcache_row"]), "fdir": (S, 2)}
        out = {"info": inf}
        for name in (which if which is not None else _abi.DBG_ARRAYS):
            idx, dt, _ = _abi.DBG_ARRAYS[name]
            nb = C.c_size_t(0)
            _check(self.lib, self.h, self.lib.me_debug_export(self.h, idx, None, 0, C.byref(nb)))
            if nb.value % dt.itemsize:
                raise RuntimeError(f"debug_export: {name}: {nb.value} B is no multiple of {dt.itemsize}")
            a = np.zeros(nb.value // dt.itemsize, dtype=dt)
            _check(self.lib, self.h, self.lib.me_debug_export(self.h, idx, ptr(a), a.nbytes, C.byref(nb)))
            out[name] = a.reshape(shapes[name]) if name in shapes else a
        return out

    def admits(self, b: Batch) -> bool:
        """Would submit_batch(b) be admitted now (me_admission_check)? Nothing is enqueued."""
        n_rest = int(np.count_nonzero(((b.kind & 0x0C) == 0) & ((((b.kind >> 4) ^ (b.kind >> 5)) & 1) == 0)))
        ok = C.c_int(0)
        _check(self.lib, self.h, self.lib.me_admission_check(self.h, n_rest, C.byref(ok)))
        return bool(ok.value)

    def admission(self) -> dict:
        """Admission control (me_admission_read): device resting count after all enqueued work, the
        host's current bound, and how many submits had to take an exact count."""
        r, b, x = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(self.lib, self.h, self.lib.me_admission_read(self.h, C.byref(r), C.byref(b), C.byref(x)))
        return {"resting": r.value, "bound": b.value, "exact_counts": x.value}

    # -- the feeds' shared read side (me_quotes_* / me_depth_* / me_trades_*: one event-ring protocol, three event types)
    def _feed_read(self, fn, dtype, cap: int):
        out = np.zeros(cap, dtype=dtype)
        n, left = C.c_size_t(0), C.c_size_t(0)
        _check(self.lib, self.h, fn(self.h, ptr(out), cap, C.byref(n), C.byref(left)))
        return out[: n.value], left.value

    def _feed_drain(self, read) -> np.ndarray:
        parts = []
        while True:
            ev, left = read()
            parts.append(ev)
            if not left:
                return np.concatenate(parts)

    def _feed_stats(self, fn) -> dict:
        g, ev, d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(self.lib, self.h, fn(self.h, C.byref(g), C.byref(ev), C.byref(d)))
        return {"groups": g.value, "events": ev.value, "deferred": d.value}

    # -- top-of-book change feed (me_quotes_*)
    def quotes_enable(self, cap_events: int):
        """Turn the quote feed on with a log of cap_events events (raised to num_symbols), or off with 0.
        Enabling takes every symbol's quote once at this point of the stream."""
        _check(self.lib, self.h, self.lib.me_quotes_enable(self.h, int(cap_events)))

    def quotes_read(self, cap: int = 0):
        """(events QUOTE_DTYPE, left): up to `cap` logged events in order (0 = a buffer of num_symbols) and
        how many stay unread. Launches no partial group; see me_quotes_read for what is there when."""
        return self._feed_read(self.lib.me_quotes_read, _abi.QUOTE_DTYPE, int(cap) or self.num_symbols)

    def quotes_drain(self) -> np.ndarray:
        """Every logged event: reads until none is left (a deferred job's catch-up included)."""
        return self._feed_drain(self.quotes_read)

    def quotes_stats(self) -> dict:
        return self._feed_stats(self.lib.me_quotes_stats)

    # -- depth feed (me_depth_*)
    def depth_enable(self, depth: int, cap_events: int):
        """Turn the depth feed on: the `depth` best levels per side (<= 32), a log of cap_events events (raised
        to 4 * depth * num_symbols); depth or cap_events 0 turns it off. Enabling takes every view once at this
        point of the stream."""
        _check(self.lib, self.h, self.lib.me_depth_enable(self.h, int(depth), int(cap_events)))
        self._depth = int(depth) if cap_events else 0

    def depth_read(self, cap: int = 0):
        """(events DEPTH_DTYPE, left): up to `cap` logged events in order (0 = a buffer of one job's most) and
        how many stay unread. Launches no partial group; see me_depth_read for what is there when."""
        cap = int(cap) or max(1, 4 * self._depth * self.num_symbols)
        return self._feed_read(self.lib.me_depth_read, _abi.DEPTH_DTYPE, cap)

    def depth_drain(self) -> np.ndarray:
        """Every logged event: reads until none is left (a deferred job's catch-up included)."""
        return self._feed_drain(self.depth_read)

    def depth_stats(self) -> dict:
        return self._feed_stats(self.lib.me_depth_stats)

    # -- trade feed (me_trades_*)
    def trades_enable(self, cap_events: int):
        """Turn the trade feed on with a log of cap_events events (raised to num_symbols), or off with 0. Fills
        matched before this point of the stream are not counted."""
        _check(self.lib, self.h, self.lib.me_trades_enable(self.h, int(cap_events)))

    def trades_read(self, cap: int = 0):
        """(events TRADE_DTYPE, left): up to `cap` logged events in order (0 = a buffer of num_symbols) and
        how many stay unread. Launches no partial group; see me_trades_read for what is there when."""
        return self._feed_read(self.lib.me_trades_read, _abi.TRADE_DTYPE, int(cap) or self.num_symbols)

    def trades_drain(self) -> np.ndarray:
        """Every logged event: reads until none is left (a deferred job's catch-up included)."""
        return self._feed_drain(self.trades_read)

    def trades_stats(self) -> dict:
        return self._feed_stats(self.lib.me_trades_stats)

    # -- trigger book: stop and stop-limit orders (me_stops_*)
    def stops_enable(self, cap_stops: int):
        """Turn the trigger book on for at most cap_stops stops live or triggered-and-unread (<= 2^22), or off with
        0 (everything is dropped). Enabling again starts afresh."""
        _check(self.lib, self.h, self.lib.me_stops_enable(self.h, int(cap_stops)))
        self._stops_cap = int(cap_stops)

    def stops_add(self, stops):
        """me_stops_add: STOP_DTYPE records (id ascending, local symbol ids), all or nothing. Fills of batches
        submitted before this call never trigger them."""
        a = np.ascontiguousarray(stops, dtype=_abi.STOP_DTYPE).reshape(-1)
        _check(self.lib, self.h, self.lib.me_stops_add(self.h, ptr(a), len(a)))

    def stops_cancel(self, ids) -> np.ndarray:
        """me_stops_cancel: found (uint8) per id, strictly ascending ids; syncs first, so a stop the submitted
        batches trigger answers 0 and its event is readable."""
        q = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        found = np.zeros(len(q), dtype=np.uint8)
        _check(self.lib, self.h, self.lib.me_stops_cancel(self.h, ptr(q), len(q), ptr(found)))
        return found

    def stops_read(self, cap: int = 0):
        """(events STOP_EVENT_DTYPE, left): up to `cap` logged events in order (0 = a buffer of cap_stops, at most
        65,536) and how many stay unread. Launches no partial group and waits for nothing."""
        cap = int(cap) or max(1, min(self._stops_cap, 1 << 16))
        return self._feed_read(self.lib.me_stops_read, _abi.STOP_EVENT_DTYPE, cap)

    def stops_drain(self) -> np.ndarray:
        """Every logged event: reads until none is left."""
        return self._feed_drain(self.stops_read)

    def stops_stats(self) -> dict:
        """jobs run, events logged, stops live (exact after sync). Raises if a job ever found the ring full."""
        j, ev, lv = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(self.lib, self.h, self.lib.me_stops_stats(self.h, C.byref(j), C.byref(ev), C.byref(lv)))
        return {"jobs": j.value, "events": ev.value, "live": lv.value}

    def stops_dump(self) -> np.ndarray:
        """me_stops_dump: the live stops (STOP_DTYPE) in table order, after a sync: what a caller persists."""
        n = C.c_size_t(0)
        _check(self.lib, self.h, self.lib.me_stops_dump(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=_abi.STOP_DTYPE)
        if n.value:
            _check(self.lib, self.h, self.lib.me_stops_dump(self.h, ptr(out), len(out), C.byref(n)))
        return out[: n.value]

    # -- timing
    def timing_enable(self, period: int = 1):
        """HIP events on every `period`-th match launch (True = every launch, 0/False = off)."""
        _check(self.lib, self.h, self.lib.me_timing_enable(self.h, int(period)))

    def timing_read(self):
        m, p = C.c_double(0), C.c_double(0)
        k, f, o = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.me_timing_read(self.h, C.byref(m), C.byref(p), C.byref(k), C.byref(f), C.byref(o))
        _check(self.lib, self.h, rc)
        return {"match_ms": m.value, "pipeline_ms": p.value, "launches": k.value, "fills": f.value,
                "orders": o.value}


# ---------------------------------------------------------------------------------------------
# Synthetic streams (SURVEY.md §8(d) configurations)
@dataclass
class StreamConfig:
    config: int
    seed: int
    num_symbols: int
    levels: int
    spread_ticks: int = 32
    max_qty: int = 100
    market_pct: int = 20
    cancel_pct: int = 0
    zipf_s: float = 0.0
    market_qty_mult: int = 0
    batch: int = 65536
    batches: int = 1024
    seed_levels_per_side: int = 0
    seq_start: int = 0       # first seq (0 = 1); > 2^33 exercises OIDs far beyond any fixed table
    drift_step: int = 0      # > 0: each symbol's mid trends drift_step ticks every drift_every records
    drift_every: int = 0
    far_pct: int = 0         # % of LIMITs priced U[L, 64L] ticks away from the mid (outside the window)


def preset(config: int, **over) -> StreamConfig:
    """The five benchmark configurations of SURVEY.md §8(d) (override any field for small tests)."""
    base = {
        1: dict(config=1, seed=1, num_symbols=1, levels=128, batch=62500, batches=16),  # 1M orders on "SYM"
        2: dict(config=2, seed=2, num_symbols=1024, levels=128, batch=65536, batches=1024),
        3: dict(config=3, seed=3, num_symbols=100_000, levels=128, batch=1 << 20, batches=128),
        4: dict(config=4, seed=4, num_symbols=100_000, levels=32768, spread_ticks=5000, zipf_s=1.1,
                seed_levels_per_side=10_000, batch=65536, batches=256),
        5: dict(config=5, seed=5, num_symbols=1024, levels=128, cancel_pct=60, market_pct=15,
                market_qty_mult=20, batch=65536, batches=1024),
    }[config]
    base.update(over)
    return StreamConfig(**base)


class Stream:
    """Deterministic global order stream (me_gen_*), seq = 1, 2, ... across batches."""

    def __init__(self, sc: StreamConfig):
        self.lib = _abi.load()
        self.sc = sc
        p = MeGenParams(sc.config, sc.seed, sc.num_symbols, sc.levels, sc.spread_ticks, sc.max_qty,
                        sc.market_pct, sc.cancel_pct, float(sc.zipf_s), sc.market_qty_mult, sc.seq_start,
                        sc.drift_step, sc.drift_every, sc.far_pct)
        self.g = self.lib.me_gen_create(C.byref(p))
        if not self.g:
            raise ValueError(f"invalid stream config {sc}")

    def close(self):
        if self.g:
            self.lib.me_gen_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def base_prices(self) -> np.ndarray:
        out = np.zeros(self.sc.num_symbols, dtype=np.int64)
        self.lib.me_gen_base_prices(self.g, ptr(out))
        return out

    def next(self, n: int) -> Batch:
        a = [np.zeros(n, dtype=t) for t in (np.uint64, np.int64, np.int32, np.uint32, np.uint8)]
        self.lib.me_gen_next(self.g, n, *[ptr(x) for x in a])
        return Batch(*a)

    def seed_books(self, symbols, per_side: int) -> Batch:
        """Config 4 pre-seed: per_side resting orders per side for every symbol in `symbols`."""
        parts = []
        for s in symbols:
            m = 2 * per_side
            a = [np.zeros(m, dtype=t) for t in (np.uint64, np.int64, np.int32, np.uint8)]
            rc = self.lib.me_gen_seed_book(self.g, int(s), per_side, *[ptr(x) for x in a])
            if rc:
                raise ValueError("seed_book failed")
            parts.append(Batch(a[0], a[1], a[2], np.full(m, s, dtype=np.uint32), a[3]))
        return Batch(*[np.concatenate([getattr(p, f) for p in parts]) for f in
                       ("seq", "price_q4", "qty", "symbol", "kind")])


def stop_records(events, seq0: int) -> Batch:
    """The NEW records triggered stops become (STOP_EVENT_DTYPE events, in event order): seqs seq0, seq0 + 1, ...;
    price (limit_px_q4), qty, symbol and kind are the events'. The caller submits them in a later batch."""
    ev = np.asarray(events, dtype=_abi.STOP_EVENT_DTYPE).reshape(-1)
    seq = np.uint64(seq0) + np.arange(len(ev), dtype=np.uint64)
    return Batch(seq, ev["limit_px_q4"], ev["qty"], ev["symbol"], ev["kind"])


def shard_of(symbol: int, shards: int) -> int:
    return int(_abi.load().me_shard_of(symbol, shards))


def shard_table(num_symbols: int, shards: int):
    """global symbol -> (shard, local id); per shard the global ids in local-id order."""
    lib = _abi.load()
    shard = np.array([lib.me_shard_of(s, shards) for s in range(num_symbols)], dtype=np.uint32)
    local = np.zeros(num_symbols, dtype=np.uint32)
    members = []
    for r in range(shards):
        ids = np.nonzero(shard == r)[0].astype(np.uint32)
        local[ids] = np.arange(len(ids), dtype=np.uint32)
        members.append(ids)
    return shard, local, members
