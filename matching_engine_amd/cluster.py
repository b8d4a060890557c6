"""Sharded deployment — the Python view of include/me_cluster.h.

The cluster itself is C++ (csrc/me_cluster.cpp): one process per GPU, symbols hash-partitioned
(me_shard_of), RCCL over xGMI (or a TCP star: the CPU tests) only to scatter each slice's parts and to
bring tapes, results, books and level snapshots back to rank 0, where the SubmitOrder service runs
over ``Cluster.c_matcher()`` (me_cluster_matcher). This module creates it and exposes its entry points;
it moves no data itself.

``ShardOps`` adapts a Python book object to me_shard_ops (the CPU tests put the oracle behind it), and
``python_matcher`` a Python object to me_matcher (the single-book services the tests compare with).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import (BOOK_ENTRY_DTYPE, FILL_DTYPE, LEVEL_DTYPE, RESULT_DTYPE, MeClusterConfig, MeConfig, MeMatcher,
                   MeOrderSoa, MeShardOps, ptr)
from .engine import Batch, _view

TRANSPORTS = {"rccl": _abi.TRANSPORT_RCCL, "tcp": _abi.TRANSPORT_TCP}


class ClusterError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"cluster error {code}: {msg}")
        self.code = code


class SliceRefused(ClusterError):
    """A shard's admission control refused its part of a slice; no shard applied anything."""


def _batch_of(soa, n: int) -> Batch:
    s = soa.contents
    cols = [np.ctypeslib.as_array(C.cast(getattr(s, f), C.POINTER(t)), shape=(n,)).copy()
            for f, t in (("seq", C.c_uint64), ("price_q4", C.c_int64), ("qty", C.c_int32), ("symbol", C.c_uint32),
                         ("kind", C.c_uint8))]
    return Batch(*cols)


def _book_out(got, bids, bcap, nb, asks, acap, na, bl, al, nbl, nal):
    """me_book_orders' output contract from (bid entries, ask entries, bid levels, ask levels)."""
    eb, ea, lb, la = got
    for arr, p, cap, cnt in ((eb, bids, bcap, nb), (ea, asks, acap, na)):
        if cnt:
            cnt[0] = len(arr)
        if p and cap and len(arr):
            C.memmove(p, arr.ctypes.data, min(cap, len(arr)) * arr.itemsize)
    for arr, p, cnt in ((lb, bl, nbl), (la, al, nal)):
        if cnt:
            cnt[0] = len(arr)
        if p and len(arr):
            C.memmove(p, arr.ctypes.data, len(arr) * arr.itemsize)


def _quotes_cb(obj):
    """me_quotes_read's contract over obj.quotes(cap) -> (events QUOTE_DTYPE, events left unread)."""

    def quotes_cb(ctx, out, cap, n, left):
        try:
            ev, rest = obj.quotes(int(cap))
            ev = np.ascontiguousarray(ev, dtype=_abi.QUOTE_DTYPE)
            assert len(ev) <= cap
            if len(ev):
                C.memmove(out, ev.ctypes.data, ev.nbytes)
            if n:
                n[0] = len(ev)
            if left:
                left[0] = int(rest)
            return 0
        except Exception:
            return _abi.ME_E_STATE

    return quotes_cb


def _events_cb(read, dtype):
    """me_quotes_read's contract for another event type over read(cap) -> (events, events left unread)."""

    def events_cb(ctx, out, cap, n, left):
        if n:
            n[0] = 0
        if left:
            left[0] = 0
        try:
            ev, rest = read(int(cap))
            ev = np.ascontiguousarray(ev, dtype=dtype)
            assert len(ev) <= cap
            if len(ev):
                C.memmove(out, ev.ctypes.data, ev.nbytes)
            if n:
                n[0] = len(ev)
            if left:
                left[0] = int(rest)
            return 0
        except ValueError:  # the feed is off
            return _abi.ME_E_INVALID
        except Exception:
            return _abi.ME_E_STATE

    return events_cb


def _set_parity_hooks(struct, obj):
    """The optional hooks me_matcher and me_shard_ops share after `quotes`, each set only when obj has a method
    of that name (else NULL: the facility is absent, as before): depth_enable(depth, cap_events) and
    trades_enable(cap_events) (raise ValueError for me's ME_E_INVALID), depth(cap) / trades(cap) -> (events,
    left), order_query(seqs uint64[n]) -> ORDER_INFO_DTYPE[n], order_preview(symbol, kind, price_q4, qty arrays)
    -> PREVIEW_DTYPE[n]. Returns the callbacks, which must live as long as the struct."""
    keep = []

    def guard(fn):
        def cb(ctx, *a):
            try:
                fn(*a)
                return 0
            except ValueError:
                return _abi.ME_E_INVALID
            except Exception:
                return _abi.ME_E_STATE

        return cb

    def rows_out(out, rows, dtype, n):
        rows = np.ascontiguousarray(rows, dtype=dtype)
        assert len(rows) == n
        if n:
            C.memmove(out, rows.ctypes.data, rows.nbytes)

    def query(seqs, n, out):
        q = np.ctypeslib.as_array(seqs, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
        rows_out(out, obj.order_query(q), _abi.ORDER_INFO_DTYPE, n)

    def preview(soa, n, out):
        s = soa.contents
        cols = [np.ctypeslib.as_array(C.cast(getattr(s, f), C.POINTER(t)), shape=(n,)).copy()
                for f, t in (("symbol", C.c_uint32), ("kind", C.c_uint8), ("price_q4", C.c_int64), ("qty", C.c_int32))]
        rows_out(out, obj.order_preview(*cols), _abi.PREVIEW_DTYPE, n)

    hooks = {
        "depth_enable": lambda: _abi.DEPTH_ENABLE_FN(guard(lambda d, cap: obj.depth_enable(int(d), int(cap)))),
        "depth": lambda: _abi.QUOTES_FN(_events_cb(obj.depth, _abi.DEPTH_DTYPE)),
        "trades_enable": lambda: _abi.TRADES_ENABLE_FN(guard(lambda cap: obj.trades_enable(int(cap)))),
        "trades": lambda: _abi.QUOTES_FN(_events_cb(obj.trades, _abi.TRADE_DTYPE)),
        "order_query": lambda: _abi.ORDER_QUERY_FN(guard(query)),
        "order_preview": lambda: _abi.ORDER_PREVIEW_FN(guard(preview)),
    }
    for name, make in hooks.items():
        if hasattr(obj, name):
            fn = make()
            setattr(struct, name, fn)
            keep.append(fn)
    return tuple(keep)


def _set_stop_hooks(m, obj):
    """me_matcher's four stop hooks over stops_enable(cap), stops_add(recs STOP_DTYPE), stops_cancel(ids uint64[n])
    -> found uint8[n] and stops_read(cap) -> (events STOP_EVENT_DTYPE, left) — set when obj has all four, else
    all NULL (the matcher has no stop orders). ValueError is me's ME_E_INVALID, SliceRefused its ME_E_CAPACITY.
    Returns the callbacks, which must live as long as the struct."""
    names = ("stops_enable", "stops_add", "stops_cancel", "stops_read")
    if not all(hasattr(obj, n) for n in names):
        return ()

    def guard(fn):
        def cb(ctx, *a):
            try:
                fn(*a)
                return 0
            except ValueError:
                return _abi.ME_E_INVALID
            except SliceRefused:
                return _abi.ME_E_CAPACITY
            except Exception:
                return _abi.ME_E_STATE

        return cb

    def add(recs, n):
        a = np.zeros(n, dtype=_abi.STOP_DTYPE)
        if n:
            C.memmove(a.ctypes.data, recs, a.nbytes)
        obj.stops_add(a)

    def cancel(ids, n, found):
        q = np.ctypeslib.as_array(ids, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
        got = np.ascontiguousarray(obj.stops_cancel(q), dtype=np.uint8)
        assert len(got) == n
        for i in range(n):
            found[i] = int(got[i])

    m.stops_enable = _abi.STOPS_ENABLE_FN(guard(lambda cap: obj.stops_enable(int(cap))))
    m.stops_add = _abi.STOPS_ADD_FN(guard(add))
    m.stops_cancel = _abi.STOPS_CANCEL_FN(guard(cancel))
    m.stops_read = _abi.QUOTES_FN(_events_cb(obj.stops_read, _abi.STOP_EVENT_DTYPE))
    return (m.stops_enable, m.stops_add, m.stops_cancel, m.stops_read)


def python_matcher(obj) -> MeMatcher:
    """me_matcher over a Python object with match(batch) -> (results, tape), book_orders(symbol, depth)
    -> (bid entries, ask entries, bid levels, ask levels), num_symbols, max_batch, max_resting, and the optional
    hooks: quotes, _set_parity_hooks' six, and the four stop hooks (_set_stop_hooks: all four or none). Test
    infrastructure (a single book standing in for a backend); the callbacks run on the flushing thread."""
    keep = {}

    def match_cb(ctx, soa, n, fills, nf, results):
        try:
            res, tape = obj.match(_batch_of(soa, n))
            res, tape = np.ascontiguousarray(res), np.ascontiguousarray(tape)
            keep["out"] = (res, tape)
            fills[0] = tape.ctypes.data if len(tape) else None
            nf[0] = len(tape)
            results[0] = res.ctypes.data
            return 0
        except SliceRefused:
            return _abi.ME_E_CAPACITY
        except Exception:
            return _abi.ME_E_STATE

    def book_cb(ctx, symbol, depth, *out):
        try:
            _book_out(obj.book_orders(symbol, depth), *out)
            return 0
        except Exception:
            return _abi.ME_E_STATE

    m = _abi.MeMatcherStops()
    m.ctx = None
    m.num_symbols, m.max_batch, m.max_resting = obj.num_symbols, obj.max_batch, obj.max_resting
    m.match = _abi.MATCH_FN(match_cb)
    m.book = _abi.BOOK_FN(book_cb)
    m._keep = (m.match, m.book, keep)  # the callbacks live as long as the struct
    if hasattr(obj, "quotes"):  # the top-of-book change feed: quotes(cap) -> (events QUOTE_DTYPE, left)
        m.quotes = _abi.QUOTES_FN(_quotes_cb(obj))
        m._keep += (m.quotes,)
    m._keep += _set_parity_hooks(m, obj)
    m._keep += _set_stop_hooks(m, obj)
    return m


class ShardOps:
    """me_shard_ops over a Python book: admit(n_rest) -> bool (optional), match(batch) -> (results,
    tape), book_orders(local symbol, depth) -> (bid entries, ask entries, bid levels, ask levels),
    levels_all(depth) -> (levels [n, 2, depth], counts [n, 2])."""

    def __init__(self, book, max_resting: int):
        self.book = book
        self._out = None

        def admit_cb(ctx, n_rest, ok):
            try:
                ok[0] = 1 if (not hasattr(book, "admit") or book.admit(int(n_rest))) else 0
                return 0
            except Exception:
                return _abi.ME_E_STATE

        def match_cb(ctx, soa, n, fills, nf, results):
            try:
                res, tape = book.match(_batch_of(soa, n))
                self._out = (np.ascontiguousarray(res), np.ascontiguousarray(tape))
                fills[0] = self._out[1].ctypes.data if len(tape) else None
                nf[0] = len(tape)
                results[0] = self._out[0].ctypes.data
                return 0
            except Exception:
                return _abi.ME_E_STATE

        def book_cb(ctx, symbol, depth, *out):
            try:
                _book_out(book.book_orders(int(symbol), int(depth)), *out)
                return 0
            except Exception:
                return _abi.ME_E_STATE

        def levels_cb(ctx, depth, levels, counts):
            try:
                lv, cnt = book.levels_all(int(depth))
                lv, cnt = np.ascontiguousarray(lv, dtype=LEVEL_DTYPE), np.ascontiguousarray(cnt, dtype=np.uint32)
                C.memmove(levels, lv.ctypes.data, lv.nbytes)
                C.memmove(counts, cnt.ctypes.data, cnt.nbytes)
                return 0
            except Exception:
                return _abi.ME_E_STATE

        self.struct = MeShardOps(None, int(max_resting), _abi.ADMIT_FN(admit_cb), _abi.MATCH_FN(match_cb),
                                 _abi.BOOK_FN(book_cb), _abi.LEVELS_FN(levels_cb))
        if hasattr(book, "quotes"):  # quotes(cap) -> (events QUOTE_DTYPE with local ids, events left unread)
            self.struct.quotes = _abi.QUOTES_FN(_quotes_cb(book))
        self._hooks = _set_parity_hooks(self.struct, book)  # depth / trades / order_query / order_preview


def shard_symbols(num_symbols: int, world: int, rank: int) -> np.ndarray:
    """Global symbol ids of rank's shard (local id = position), me_cluster_shard_symbols."""
    lib = _abi.load()
    n = lib.me_cluster_shard_symbols(num_symbols, world, rank, None, 0)
    out = np.zeros(max(n, 1), dtype=np.uint32)
    lib.me_cluster_shard_symbols(num_symbols, world, rank, ptr(out), n)
    return out[:n]


class Cluster:
    """One rank of the sharded deployment (me_cluster_create is collective: every rank constructs it).

    The shard is an engine built from (levels, base_prices[num_symbols global], max_resting, engine
    options) — or, with ``shard_ops``, a ShardOps. Rank 0 issues submit / collect / match / book_orders
    / snapshot / stop; the other ranks call serve()."""

    def __init__(self, rank: int, world: int, num_symbols: int, max_batch: int, transport: str = "rccl",
                 addr: str = "127.0.0.1", port: int = 29610, device: int = 0, levels: int = 128, base_prices=None,
                 max_resting: int = 1 << 20, shard_ops: ShardOps | None = None, timeout_ms: int = 60000,
                 seq_ring: int = 0, batches_per_launch: int = 0, far_levels: int = 0):
        self.lib = _abi.load()
        self.rank, self.world, self.num_symbols, self.max_batch = rank, world, num_symbols, max_batch
        self._addr = addr.encode()
        cfg = MeClusterConfig(rank, world, num_symbols, max_batch, TRANSPORTS[transport], device, self._addr, port,
                              timeout_ms)
        self._ops = shard_ops
        ecfg = None
        if shard_ops is None:
            self._base = np.ascontiguousarray(base_prices, dtype=np.int64)
            assert len(self._base) == num_symbols
            ecfg = MeConfig(device, num_symbols, levels, max_batch, max_resting, 0, seq_ring,
                            self._base.ctypes.data_as(C.POINTER(C.c_int64)), None, batches_per_launch, far_levels,
                            0, 0)
        self.h = self.lib.me_cluster_create(C.byref(cfg), C.byref(ecfg) if ecfg is not None else None,
                                            C.byref(shard_ops.struct) if shard_ops is not None else None)
        if not self.h:
            raise ClusterError(_abi.ME_E_STATE, self._err(None))
        self._cm = None

    def _err(self, h) -> str:
        buf = C.create_string_buffer(1024)
        self.lib.me_cluster_last_error(h, buf, 1024)
        return buf.value.decode(errors="replace")

    def _check(self, rc: int):
        if rc == _abi.ME_E_CAPACITY:
            raise SliceRefused(rc, self._err(self.h))
        if rc != _abi.ME_OK:
            raise ClusterError(rc, self._err(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.me_cluster_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ranks != 0
    def serve(self):
        self._check(self.lib.me_cluster_serve(self.h))

    # -- rank 0
    def stop(self):
        self._check(self.lib.me_cluster_stop(self.h))

    def submit(self, b: Batch) -> int:
        t = C.c_uint64(0)
        soa = b.soa()
        self._check(self.lib.me_cluster_submit(self.h, C.byref(soa), len(b), C.byref(t)))
        return t.value

    def collect(self, ticket: int, n: int, copy: bool = True):
        """(results[n], tape) of the oldest ticket: copies, or (copy=False) views valid until the next call."""
        f, r, nf = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        self._check(self.lib.me_cluster_collect(self.h, ticket, C.byref(f), C.byref(nf), C.byref(r)))
        res, tape = _view(r.value, n, RESULT_DTYPE), _view(f.value, nf.value, FILL_DTYPE)
        return (res.copy(), tape.copy()) if copy else (res, tape)

    def match(self, b: Batch):
        return self.collect(self.submit(b), len(b))

    def book_orders(self, symbol: int, depth: int):
        nb, na, nbl, nal = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.me_cluster_book(self.h, symbol, depth, None, 0, C.byref(nb), None, 0, C.byref(na), None,
                                             None, C.byref(nbl), C.byref(nal)))
        eb, ea = np.zeros(max(nb.value, 1), BOOK_ENTRY_DTYPE), np.zeros(max(na.value, 1), BOOK_ENTRY_DTYPE)
        lb = np.zeros(max(depth, nbl.value, 1), LEVEL_DTYPE)
        la = np.zeros(max(depth, nal.value, 1), LEVEL_DTYPE)
        self._check(self.lib.me_cluster_book(self.h, symbol, depth, ptr(eb), len(eb), C.byref(nb), ptr(ea), len(ea),
                                             C.byref(na), ptr(lb), ptr(la), C.byref(nbl), C.byref(nal)))
        return eb[:nb.value], ea[:na.value], lb[:nbl.value if depth else 0], la[:nal.value if depth else 0]

    def snapshot(self, depth: int):
        """Top-`depth` levels of every global symbol: (levels [S, 2, depth], counts [S, 2])."""
        lv = np.zeros((self.num_symbols, 2, depth), dtype=LEVEL_DTYPE)
        cnt = np.zeros((self.num_symbols, 2), dtype=np.uint32)
        self._check(self.lib.me_cluster_snapshot(self.h, depth, ptr(lv), ptr(cnt)))
        return lv, cnt

    def quotes_enable(self, cap_events: int):
        """me_cluster_quotes_enable: every shard's quote feed on (a log of cap_events events) or off (0)."""
        self._check(self.lib.me_cluster_quotes_enable(self.h, int(cap_events)))

    def quotes(self, cap: int = 0):
        """me_cluster_quotes: (events QUOTE_DTYPE with global symbol ids, left). Drains every shard when all
        gathered events were handed out; `batches` is each shard's own count."""
        cap = int(cap) or max(self.num_symbols, 1)
        out = np.zeros(cap, dtype=_abi.QUOTE_DTYPE)
        n, left = C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.me_cluster_quotes(self.h, ptr(out), cap, C.byref(n), C.byref(left)))
        return out[: n.value], left.value

    def quotes_drain(self) -> np.ndarray:
        parts = []
        while True:
            ev, left = self.quotes()
            parts.append(ev)
            if not left:
                return np.concatenate(parts)

    def _feed(self, fn, dtype, cap: int):
        cap = int(cap) or max(4 * self.num_symbols, 1)
        out = np.zeros(cap, dtype=dtype)
        n, left = C.c_size_t(0), C.c_size_t(0)
        self._check(fn(self.h, ptr(out), cap, C.byref(n), C.byref(left)))
        return out[: n.value], left.value

    def _drain(self, read) -> np.ndarray:
        parts = []
        while True:
            ev, left = read()
            parts.append(ev)
            if not left:
                return np.concatenate(parts)

    def depth_enable(self, depth: int, cap_events: int):
        """me_cluster_depth_enable: every shard's depth feed on at `depth` levels per side (a log of cap_events
        events), or off with depth 0 or cap_events 0."""
        self._check(self.lib.me_cluster_depth_enable(self.h, int(depth), int(cap_events)))

    def depth(self, cap: int = 0):
        """me_cluster_depth: (events DEPTH_DTYPE with global symbol ids, left); `batches` is each shard's own count."""
        return self._feed(self.lib.me_cluster_depth, _abi.DEPTH_DTYPE, cap)

    def depth_drain(self) -> np.ndarray:
        return self._drain(self.depth)

    def trades_enable(self, cap_events: int):
        """me_cluster_trades_enable: every shard's trade feed on (a log of cap_events events) or off (0)."""
        self._check(self.lib.me_cluster_trades_enable(self.h, int(cap_events)))

    def trades(self, cap: int = 0):
        """me_cluster_trades: (events TRADE_DTYPE with global symbol ids, left)."""
        return self._feed(self.lib.me_cluster_trades, _abi.TRADE_DTYPE, cap)

    def trades_drain(self) -> np.ndarray:
        return self._drain(self.trades)

    def order_query(self, seqs) -> np.ndarray:
        """me_cluster_order_query: one ORDER_INFO_DTYPE answer per seq (global symbol ids), from the shard that
        holds it; found 0 when none does."""
        q = np.ascontiguousarray(seqs, dtype=np.uint64)
        out = np.zeros(len(q), dtype=_abi.ORDER_INFO_DTYPE)
        self._check(self.lib.me_cluster_order_query(self.h, ptr(q) if len(q) else None, len(q),
                                                    ptr(out) if len(q) else None))
        return out

    def order_preview(self, symbol, kind, price_q4, qty) -> np.ndarray:
        """me_cluster_order_preview: one PREVIEW_DTYPE answer per query (global symbol ids); no book changes."""
        sym = np.ascontiguousarray(symbol, dtype=np.uint32)
        kd = np.ascontiguousarray(kind, dtype=np.uint8)
        px = np.ascontiguousarray(price_q4, dtype=np.int64)
        qt = np.ascontiguousarray(qty, dtype=np.int32)
        n = len(sym)
        assert len(kd) == len(px) == len(qt) == n
        soa = MeOrderSoa()
        for f, a in (("price_q4", px), ("qty", qt), ("symbol", sym), ("kind", kd)):
            setattr(soa, f, a.ctypes.data)
        out = np.zeros(n, dtype=_abi.PREVIEW_DTYPE)
        self._check(self.lib.me_cluster_order_preview(self.h, C.byref(soa), n, ptr(out) if n else None))
        return out

    def c_matcher(self) -> MeMatcher:
        """me_cluster_matcher: the service on rank 0 is created over it (two slices in flight)."""
        if self._cm is None:
            m = _abi.MeMatcherStops()  # the whole struct: me_cluster_matcher clears it all and leaves the stop hooks NULL
            self._check(self.lib.me_cluster_matcher(self.h, C.byref(m)))
            self._cm = m
        return self._cm

    def stats(self) -> dict:
        s, b = C.c_uint64(0), C.c_uint64(0)
        self.lib.me_cluster_stats(self.h, C.byref(s), C.byref(b))
        return {"slices": s.value, "bytes": b.value}

    PHASES = ("split", "control", "scatter", "vote", "match", "collect", "gather", "merge", "split_count", "split_slot")

    def phases(self) -> dict:
        """Rank 0's seconds per protocol phase since create (me_cluster_phases)."""
        v = (C.c_double * len(self.PHASES))()
        self.lib.me_cluster_phases(self.h, v, len(self.PHASES))
        return dict(zip(self.PHASES, list(v)))
