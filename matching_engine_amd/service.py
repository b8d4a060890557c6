"""MatchingEngineService — Python view of include/me_service.h, the SubmitOrder drop-in
(src/server/matching_engine_service.cpp:41-121 re-hosted on the batched GPU core)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import (FILL_DTYPE, LEVEL_DTYPE, RESULT_DTYPE, MeBookOrder, MeCancelRequest, MeOrderRequest, MeReduceRequest,
                   MeOrderResponse, MeMarketData, MeMarketUpdate, MeDepthBook, MeTradeUpdate, MeOrderUpdate, ptr)


class ServiceError(RuntimeError):
    pass


class MatchingEngineService:
    """SubmitOrder / GetOrderBook over one engine shard; SQLite persistence when db_path is given."""

    def __init__(self, engine, symbols, db_path=None, matcher=None):
        """engine: the Engine the slices match on; or matcher: an object with c_matcher() -> MeMatcher —
        a cluster.Cluster (rank 0 of a sharded deployment, me_cluster_matcher) or a Python book behind
        cluster.python_matcher (tests) — for me_service_create_matcher."""
        self.lib = _abi.load()
        self.engine = engine
        self.matcher = matcher
        self.symbols = list(symbols)
        arr = (C.c_char_p * max(len(self.symbols), 1))(*[s.encode() for s in self.symbols])
        self._arr = arr
        if matcher is not None:
            self._cm = matcher.c_matcher()
            self.h = self.lib.me_service_create_matcher(C.byref(self._cm), arr, len(self.symbols),
                                                        db_path.encode() if db_path else None)
            if not self.h:
                raise ServiceError("me_service_create_matcher refused the matcher")
        else:
            self.h = self.lib.me_service_create(engine.h if engine is not None else None, arr, len(self.symbols),
                                                db_path.encode() if db_path else None)
        err = self.last_error()
        if db_path and err:
            raise ServiceError(err)

    def close(self):
        if getattr(self, "h", None):
            self.lib.me_service_destroy(self.h)
            self.h = None

    def start(self, interval_us: int = 1000, slice_orders: int = 0):
        """Background flusher: slices close at slice_orders records or interval_us age and are matched
        and persisted without a caller (errors: last_error())."""
        rc = self.lib.me_service_start(self.h, interval_us, slice_orders)
        if rc != 0:
            raise ServiceError(f"start failed ({rc}): {self.last_error()}")

    def stop(self):
        self.lib.me_service_stop(self.h)

    @property
    def unpersisted(self) -> int:
        """Matched records whose SQLite transaction has not committed yet."""
        return int(self.lib.me_service_unpersisted(self.h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        buf = C.create_string_buffer(1024)
        self.lib.me_service_last_error(self.h, buf, 1024)
        return buf.value.decode(errors="replace")

    def submit_order(self, client_id, symbol, order_type, side, price, scale, quantity, tif=0) -> dict:
        """OrderRequest -> OrderResponse fields + grpc status (0 OK, 2 UNKNOWN). tif: TIF_* (me_service_submit_order_tif;
        0 = the reference's SubmitOrder)."""
        req = MeOrderRequest(client_id.encode(), symbol.encode(), order_type, side, price, scale, quantity)
        resp = MeOrderResponse()
        self.lib.me_service_submit_order_tif(self.h, C.byref(req), tif, C.byref(resp))
        return {"order_id": resp.order_id.decode(), "success": bool(resp.success),
                "error_message": resp.error_message.decode(), "grpc_status": resp.grpc_status}

    def cancel_order(self, client_id, symbol, order_id) -> dict:
        """CancelOrder (build extension, me_service.h): queue a cancel of a resting order; the outcome
        arrives as an OrderUpdate after the flush."""
        req = MeCancelRequest(client_id.encode(), symbol.encode(), order_id.encode())
        resp = MeOrderResponse()
        self.lib.me_service_cancel_order(self.h, C.byref(req), C.byref(resp))
        return {"order_id": resp.order_id.decode(), "success": bool(resp.success),
                "error_message": resp.error_message.decode(), "grpc_status": resp.grpc_status}

    def reduce_order(self, client_id, symbol, order_id, quantity) -> dict:
        """ReduceOrder (build extension, me_service.h): queue a reduction of a resting order's quantity by
        `quantity`; the order keeps its place in the queue. The outcome arrives as an OrderUpdate after the
        flush: the target's own status with the smaller remaining_quantity, or CANCELED when `quantity`
        covers what was left."""
        req = MeReduceRequest(client_id.encode(), symbol.encode(), order_id.encode(), quantity)
        resp = MeOrderResponse()
        self.lib.me_service_reduce_order(self.h, C.byref(req), C.byref(resp))
        return {"order_id": resp.order_id.decode(), "success": bool(resp.success),
                "error_message": resp.error_message.decode(), "grpc_status": resp.grpc_status}

    def preview_order(self, client_id, symbol, order_type, side, price, scale, quantity, tif=0) -> np.ndarray:
        """PreviewOrder (build extension, me_service_preview_order): what submit_order with the same arguments
        would execute against the book now, as one PREVIEW_DTYPE row; nothing is submitted, no OID is taken. A
        request submit_order would refuse in-band raises ServiceError (code ME_E_INVALID) with its message; so
        does a service over a matcher without the order_preview hook."""
        req = MeOrderRequest(client_id.encode(), symbol.encode(), order_type, side, price, scale, quantity)
        out = np.zeros(1, dtype=_abi.PREVIEW_DTYPE)
        rc = self.lib.me_service_preview_order(self.h, C.byref(req), tif, ptr(out))
        if rc != 0:
            e = ServiceError(f"preview_order failed ({rc}): {self.last_error()}")
            e.code = rc
            raise e
        return out[0]

    def mass_cancel(self, symbols=None, sides=3) -> int:
        """me_service_mass_cancel: remove every resting order of `sides` (1 buy, 2 sell, 3 both) of the named
        symbols (None: every symbol that has a book); returns the number of orders removed. Each owner gets a
        CANCELED OrderUpdate per order, the rows are persisted, the emptied books count as idle."""
        n = C.c_uint64(0)
        if symbols is None:
            rc = self.lib.me_service_mass_cancel(self.h, None, 0, sides, C.byref(n))
        else:
            names = [x.encode() for x in symbols]
            arr = (C.c_char_p * max(len(names), 1))(*names)
            rc = self.lib.me_service_mass_cancel(self.h, arr, len(names), sides, C.byref(n))
        if rc != 0:
            e = ServiceError(f"mass_cancel failed ({rc}): {self.last_error()}")
            e.code = rc
            raise e
        return n.value

    def order_status(self, client_id, order_ids) -> list:
        """OrderStatus (build extension, me_service_order_status): one dict per id with state (OS_NOT_RESTING /
        OS_PENDING / OS_RESTING), side, quantity, price, scale and the queue position (qty_ahead, orders_ahead,
        level_qty, qty_better, levels_better), from one device query for all ids. Only the owner's resting
        orders answer RESTING. ServiceError (code ME_E_INVALID) on a matcher without the hook."""
        ids = [o.encode() for o in order_ids]
        n = len(ids)
        arr = (C.c_char_p * max(n, 1))(*ids)
        out = (_abi.MeOrderStatus * max(n, 1))()
        rc = self.lib.me_service_order_status(self.h, client_id.encode(), arr, n, out)
        if rc != 0:
            e = ServiceError(f"order_status failed ({rc}): {self.last_error()}")
            e.code = rc
            raise e
        return [{"order_id": o.order_id.decode(), "state": o.state, "side": o.side, "scale": o.scale,
                 "quantity": o.quantity, "price": o.price, "qty_ahead": o.qty_ahead, "level_qty": o.level_qty,
                 "qty_better": o.qty_better, "orders_ahead": o.orders_ahead, "levels_better": o.levels_better}
                for o in out[:n]]

    # ---- stop orders (me_service.h "stop and stop-limit orders") ----
    def _stop_call(self, what, rc):
        if rc != 0:
            e = ServiceError(f"{what} failed ({rc}): {self.last_error()}")
            e.code = rc
            raise e

    def stops_enable(self, cap_stops: int):
        """me_service_stops_enable: turn stop orders on with room for cap_stops stops (0: off), create the
        `stops` table and re-arm the stops the database shows ARMED. ServiceError (code ME_E_INVALID) on a
        matcher without the four stop hooks, ME_E_CAPACITY when the database holds more armed stops."""
        self._stop_call("stops_enable", self.lib.me_service_stops_enable(self.h, int(cap_stops)))

    def submit_stop(self, client_id, symbol, order_type, side, price, stop_price, scale, quantity, tif=0) -> dict:
        """me_service_submit_stop: a stop (order_type MARKET) or stop-limit (LIMIT, `price` its limit) that
        becomes an order of `side` once the symbol trades through stop_price. Answers like submit_order, with
        order_id = "SID-<n>"; ARMED / TRIGGERED / CANCELED arrive through stop_updates()."""
        req = _abi.MeStopRequest(client_id.encode(), symbol.encode(), order_type, side, price, stop_price, scale,
                                 quantity, tif)
        resp = MeOrderResponse()
        self.lib.me_service_submit_stop(self.h, C.byref(req), C.byref(resp))
        return {"order_id": resp.order_id.decode(), "success": bool(resp.success),
                "error_message": resp.error_message.decode(), "grpc_status": resp.grpc_status}

    def cancel_stop(self, client_id, stop_id) -> dict:
        """me_service_cancel_stop: queue a cancel of a stop; CANCELED or CANCEL_REJECTED arrives as a stop
        update once its boundary is applied."""
        req = _abi.MeStopCancelRequest(client_id.encode(), stop_id.encode())
        resp = MeOrderResponse()
        self.lib.me_service_cancel_stop(self.h, C.byref(req), C.byref(resp))
        return {"order_id": resp.order_id.decode(), "success": bool(resp.success),
                "error_message": resp.error_message.decode(), "grpc_status": resp.grpc_status}

    @staticmethod
    def _stop_dict(u) -> dict:
        return {"stop_id": u.stop_id.decode(), "order_id": u.order_id.decode(), "client_id": u.client_id.decode(),
                "symbol": u.symbol.decode(), "state": u.state, "scale": u.scale, "stop_price": u.stop_price,
                "limit_price": u.limit_price, "trigger_price": u.trigger_price, "quantity": u.quantity,
                "kind": u.kind}

    def stop_updates(self, client_id=None, cap=4096) -> list:
        """me_service_stop_updates: drain the queued stop updates (one client's, or all) as dicts with stop_id,
        order_id ("OID-<n>" once TRIGGERED), client_id, symbol, state (SS_*), scale, stop_price, limit_price,
        trigger_price, quantity, kind."""
        out = []
        buf = (_abi.MeStopUpdate * cap)()
        while True:
            n = C.c_size_t(0)
            self._stop_call("stop_updates", self.lib.me_service_stop_updates(
                self.h, client_id.encode() if client_id else None, buf, cap, C.byref(n)))
            out += [self._stop_dict(u) for u in buf[: n.value]]
            if n.value < cap:
                return out

    def stops(self, client_id=None) -> list:
        """me_service_stops: the client's (None: everybody's) QUEUED and ARMED stops in ascending stop id, as
        stop_updates() shapes them."""
        cid = client_id.encode() if client_id else None
        n = C.c_size_t(0)
        self._stop_call("stops", self.lib.me_service_stops(self.h, cid, None, 0, C.byref(n)))
        while True:
            cap = max(n.value, 1)
            buf = (_abi.MeStopUpdate * cap)()
            self._stop_call("stops", self.lib.me_service_stops(self.h, cid, buf, cap, C.byref(n)))
            if n.value <= cap:
                return [self._stop_dict(u) for u in buf[: n.value]]

    def stop_stats(self) -> dict:
        """me_service_stop_stats: stops QUEUED or ARMED now, events processed, stops re-armed from the database."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._stop_call("stop_stats", self.lib.me_service_stop_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"live": a.value, "triggered": b.value, "recovered": c.value}

    def order_updates(self, client_id=None, cap=1 << 16) -> list:
        """StreamOrderUpdates (proto:34,71-91): drain the queued OrderUpdate events (one client, or all)."""
        out = []
        buf = (MeOrderUpdate * cap)()
        while True:
            n = C.c_size_t(0)
            self.lib.me_service_updates(self.h, client_id.encode() if client_id else None, buf, cap, C.byref(n))
            for u in buf[: n.value]:
                out.append({"order_id": u.order_id.decode(), "client_id": u.client_id.decode(),
                            "symbol": u.symbol.decode(), "status": u.status, "fill_price": u.fill_price,
                            "scale": u.scale, "fill_quantity": u.fill_quantity,
                            "remaining_quantity": u.remaining_quantity})
            if n.value < cap:
                return out

    @property
    def pending(self) -> int:
        return int(self.lib.me_service_pending(self.h))

    @property
    def next_oid(self) -> int:
        return int(self.lib.me_service_next_oid(self.h))

    def flush(self, outputs: bool = True):
        """Match + persist every slice submitted so far -> (seq[n], results[n], fills[k]) of the records
        this call matched (outputs=False: nothing copied out, returns None)."""
        if not outputs:
            rc = self.lib.me_service_flush(self.h, None, 0, None, None, None, 0, None)
            if rc != 0:
                raise ServiceError(f"flush failed ({rc}): {self.last_error()}")
            return None
        n = self.pending
        res = np.zeros(max(n, 1), dtype=RESULT_DTYPE)
        seq = np.zeros(max(n, 1), dtype=np.uint64)
        if self.engine is not None:
            cap = self.engine.fill_bound(n) + 1
        else:
            cap = (self._cm.max_resting + 2 * n + 1) if self.matcher is not None else 1
        fills = np.zeros(cap, dtype=FILL_DTYPE)
        nf, nr = C.c_size_t(0), C.c_size_t(0)
        rc = self.lib.me_service_flush(self.h, ptr(fills), cap, C.byref(nf), ptr(res), ptr(seq), len(res),
                                       C.byref(nr))
        if rc != 0:
            raise ServiceError(f"flush failed ({rc}): {self.last_error()}")
        return seq[: nr.value].copy(), res[: nr.value].copy(), fills[: nf.value].copy()

    @property
    def updates_dropped(self) -> int:
        return int(self.lib.me_service_updates_dropped(self.h))

    def stats(self) -> dict:
        """Books handed over from idle symbols, resting orders replayed from the DB at create."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.lib.me_service_stats(self.h, C.byref(a), C.byref(b))
        return {"reclaimed_books": a.value, "recovered_orders": b.value}

    def market_data(self, symbol) -> dict:
        """MarketDataUpdate (proto:60-67) from the GPU book; a missing side has has_* False and 0s."""
        m = MeMarketData()
        rc = self.lib.me_service_market_data(self.h, symbol.encode(), C.byref(m))
        if rc != 0:
            raise ServiceError(self.last_error())
        return {"symbol": symbol, "best_bid": m.best_bid, "best_ask": m.best_ask, "scale": m.scale,
                "bid_size": m.bid_size, "ask_size": m.ask_size, "has_bid": bool(m.has_bid),
                "has_ask": bool(m.has_ask)}

    def depth_subscribe(self, depth: int):
        """The depth stream (me_service_depth_subscribe): enable the engine's depth feed at `depth` levels per
        side and queue the books as they stand; 0 turns it off. ServiceError (code ME_E_INVALID) on a matcher without the hook."""
        rc = self.lib.me_service_depth_subscribe(self.h, int(depth))
        if rc != 0:
            e = ServiceError(f"depth_subscribe failed ({rc}): {self.last_error()}")
            e.code = rc
            raise e

    def depth_stream(self, symbol=None, cap=256) -> list:
        """Drain the queued top-D books (one symbol's, or all in first-change order): dicts with symbol, scale,
        bids and asks as lists of (price, size), best first."""
        out = []
        buf = (MeDepthBook * cap)()
        while True:
            n = C.c_size_t(0)
            rc = self.lib.me_service_depth_stream(self.h, symbol.encode() if symbol else None, buf, cap, C.byref(n))
            if rc != 0:
                e = ServiceError(f"depth_stream failed ({rc}): {self.last_error()}")
                e.code = rc
                raise e
            for b in buf[: n.value]:
                out.append({"symbol": b.symbol.decode(), "scale": b.scale,
                            "bids": [(b.bids[i].price, b.bids[i].size) for i in range(b.n_bids)],
                            "asks": [(b.asks[i].price, b.asks[i].size) for i in range(b.n_asks)]})
            if n.value < cap:
                return out

    def trades_subscribe(self, on: bool = True):
        """The trade stream (me_service_trades_subscribe): enable the engine's trade feed; fills matched before
        are not counted. ServiceError (code ME_E_INVALID) on a matcher without the hook."""
        rc = self.lib.me_service_trades_subscribe(self.h, 1 if on else 0)
        if rc != 0:
            e = ServiceError(f"trades_subscribe failed ({rc}): {self.last_error()}")
            e.code = rc
            raise e

    def trades_stream(self, symbol=None, cap=4096) -> list:
        """Drain the queued trade summaries (one symbol's, or all in first-trade order): dicts with symbol,
        scale, last_price, last_size, open / high / low_price, volume, trades, cum_volume, cum_trades."""
        out = []
        buf = (MeTradeUpdate * cap)()
        names = [f for f, _ in MeTradeUpdate._fields_ if f != "symbol"]
        while True:
            n = C.c_size_t(0)
            rc = self.lib.me_service_trades_stream(self.h, symbol.encode() if symbol else None, buf, cap, C.byref(n))
            if rc != 0:
                e = ServiceError(f"trades_stream failed ({rc}): {self.last_error()}")
                e.code = rc
                raise e
            for u in buf[: n.value]:
                out.append({"symbol": u.symbol.decode(), **{f: getattr(u, f) for f in names}})
            if n.value < cap:
                return out

    def market_subscribe(self, on: bool = True):
        """StreamMarketData as a change stream (me_service_market_subscribe): enable the backend's quote
        feed and queue the books' current tops. ServiceError (code ME_E_INVALID) without a feed."""
        rc = self.lib.me_service_market_subscribe(self.h, 1 if on else 0)
        if rc != 0:
            e = ServiceError(f"market_subscribe failed ({rc}): {self.last_error()}")
            e.code = rc
            raise e

    def market_stream(self, symbol=None, cap=4096) -> list:
        """Drain the queued MarketDataUpdates (one symbol's, or all in first-change order): dicts shaped
        like market_data()'s."""
        out = []
        buf = (MeMarketUpdate * cap)()
        while True:
            n = C.c_size_t(0)
            rc = self.lib.me_service_market_stream(self.h, symbol.encode() if symbol else None, buf, cap, C.byref(n))
            if rc != 0:
                e = ServiceError(f"market_stream failed ({rc}): {self.last_error()}")
                e.code = rc
                raise e
            for u in buf[: n.value]:
                m = u.md
                out.append({"symbol": u.symbol.decode(), "best_bid": m.best_bid, "best_ask": m.best_ask,
                            "scale": m.scale, "bid_size": m.bid_size, "ask_size": m.ask_size,
                            "has_bid": bool(m.has_bid), "has_ask": bool(m.has_ask)})
            if n.value < cap:
                return out

    def get_order_book(self, symbol, depth=10):
        bids = np.zeros(depth, dtype=LEVEL_DTYPE)
        asks = np.zeros(depth, dtype=LEVEL_DTYPE)
        nb, na = C.c_size_t(0), C.c_size_t(0)
        rc = self.lib.me_service_book(self.h, symbol.encode(), ptr(bids), ptr(asks), depth, C.byref(nb),
                                      C.byref(na))
        if rc != 0:
            raise ServiceError(self.last_error())
        return bids[: nb.value], asks[: na.value]

    def order_book(self, symbol, depth=0):
        """GetOrderBook in the reference's shape (OrderBookResponse: repeated Order bids / asks, proto
        :16-23,57-60): lists of {order_id, client_id, price, scale, quantity, side} dicts, best price
        first, time order within a price; depth = price levels per side (0: the whole book)."""
        nb, na = C.c_size_t(0), C.c_size_t(0)
        rc = self.lib.me_service_order_book(self.h, symbol.encode(), depth, None, 0, C.byref(nb), None, 0, C.byref(na))
        if rc != 0:
            raise ServiceError(self.last_error())
        bids, asks = (MeBookOrder * max(nb.value, 1))(), (MeBookOrder * max(na.value, 1))()
        rc = self.lib.me_service_order_book(self.h, symbol.encode(), depth, bids, nb.value, C.byref(nb), asks,
                                            na.value, C.byref(na))
        if rc != 0:
            raise ServiceError(self.last_error())

        def conv(arr, n):
            return [{"order_id": o.order_id.decode(), "client_id": o.client_id.decode(), "price": o.price,
                     "scale": o.scale, "quantity": o.quantity, "side": o.side} for o in arr[:n]]

        return conv(bids, nb.value), conv(asks, na.value)
