"""Stop orders through the service — TEST INFRASTRUCTURE ONLY (tests/test_stops_service.py on a CPU,
tests/test_stops_service_gpu.py on the engine).

`StopMatcher` is tests/service_common.py's FeedMatcher with me_matcher's four stop hooks over
tests/stops_model.StopModel: every matched slice's fills are fed to the model and one job runs behind each match,
stamped with the slice number. `ServiceModel` replays the rules of include/me_service.h ("stop and stop-limit
orders") in plain Python over an OracleBook and a StopModel. The scripts drive a service and return everything
it showed, for a comparison between two backends."""
import sqlite3
from collections import deque

import numpy as np

from tests import stops_model as sm
from tests.service_common import FeedMatcher

BUY, SELL = 1, 2
LIMIT, MARKET = 0, 1
GTC, IOC, FOK, POST_ONLY = 0, 1, 2, 3
ARMED, TRIGGERED, CANCELED, CANCEL_REJECTED, QUEUED = 0, 1, 2, 3, 4
ST_NEW, ST_PARTIAL, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
MID = 1_000_000


def kind_of(side, otype=LIMIT, tif=GTC):
    return (side & 3) | ((otype & 1) << 2) | ((tif & 3) << 4)


def never_rests(kind):
    return bool((kind >> 2) & 1) or bool(((kind >> 4) ^ (kind >> 5)) & 1)


class StopMatcher(FeedMatcher):
    """FeedMatcher (no quote feed) plus stops_enable / stops_add / stops_cancel / stops_read."""

    def __init__(self, n, max_batch=4096):
        super().__init__(n, feed=False)
        self.max_batch = max_batch
        self.model, self.cap, self.ring, self.slices = None, 0, [], 0
        self.added = self.cancelled = self.read = 0

    def match(self, b):
        res, tape = super().match(b)
        self.slices += 1
        if self.model is not None:
            self.model.feed(tape)
            self.ring.extend(self.model.job(self.slices))
        return res, tape

    def stops_enable(self, cap):
        if cap > 1 << 22:
            raise ValueError("cap_stops above 2^22")
        self.model = sm.StopModel(self.num_symbols) if cap else None
        self.cap, self.ring = cap, []
        self.added = self.cancelled = self.read = 0

    def stops_add(self, recs):
        from matching_engine_amd import _abi
        from matching_engine_amd.cluster import SliceRefused

        if self.model is None:
            raise ValueError("off")
        if self.added - self.cancelled - self.read + len(recs) > self.cap:
            raise SliceRefused(_abi.ME_E_CAPACITY, "stops refused")
        self.model.add(recs)
        self.added += len(recs)

    def stops_cancel(self, ids):
        if self.model is None:
            raise ValueError("off")
        assert all(int(a) < int(b) for a, b in zip(ids[:-1], ids[1:])), "ids must ascend strictly"
        found = self.model.cancel(ids)
        self.cancelled += int(found.sum())
        return found

    def stops_read(self, cap):
        if self.model is None:
            raise ValueError("off")
        ev, self.ring = self.ring[:cap], self.ring[cap:]
        self.read += len(ev)
        out = np.zeros(len(ev), dtype=sm.STOP_EVENT_DTYPE)
        for k, e in enumerate(ev):
            out[k] = e
        return out, len(self.ring)


class PlainMatcher(FeedMatcher):
    """A matcher without the stop hooks."""

    def __init__(self, n):
        super().__init__(n, feed=False)


# ---- the rules, replayed ------------------------------------------------------------------------------------
class ServiceModel:
    """include/me_service.h's stop rules over OracleBook + StopModel, one slice in flight (the stream's order)."""

    def __init__(self, symbols, cap_stops, slice_max):
        from oracle.oracle import OracleBook

        self.names = list(symbols)
        self.ob = OracleBook(len(symbols))
        self.tb = sm.StopModel(len(symbols))
        self.cap, self.slice_max = cap_stops, slice_max
        self.next_oid = self.next_sid = 1
        self.open, self.closed = {"recs": [], "pre": []}, deque()
        self.stops, self.accepted, self.done = {}, 0, 0
        self.slices, self.ring = 0, []
        self.live = {}
        self.order_updates, self.stop_updates, self.pairs, self.triggered = [], [], [], []

    # -- the request path
    def _close_open(self):
        if self.open["recs"] or self.open["pre"]:
            self.closed.append(self.open)
            self.open = {"recs": [], "pre": []}

    def _append(self, rec):
        self.open["recs"].append(rec)
        if len(self.open["recs"]) >= self.slice_max:
            self._close_open()

    def submit_order(self, client, sym, otype, side, px, qty, tif=GTC):
        oid = self.next_oid
        self.next_oid += 1
        k = kind_of(side, otype, tif)
        if not never_rests(k):
            self.live[oid] = [client, sym, qty, False]
        self._append(dict(seq=oid, px=px, qty=qty, sid=self.names.index(sym), kind=k, client=client, sym=sym))
        return f"OID-{oid}"

    def submit_stop(self, client, sym, otype, side, px, stop_px, qty, tif=GTC):
        if self.accepted - self.done + 1 > self.cap:
            return None
        sid = self.next_sid
        self.next_sid += 1
        st = dict(id=sid, client=client, sym=sym, sidx=self.names.index(sym), stop_px=stop_px,
                  limit_px=px if otype == LIMIT else 0, qty=qty, kind=kind_of(side, otype, tif), armed=False)
        self.stops[sid] = st
        self.accepted += 1
        self._boundary(dict(cancel=False, id=sid, client=client, stop=dict(st)))
        return f"SID-{sid}"

    def cancel_stop(self, client, sid):
        st = self.stops.get(sid)
        if st is not None and st["client"] != client:
            return False
        self._boundary(dict(cancel=True, id=sid, client=client, stop=dict(st) if st else None,
                            unknown=sid >= self.next_sid))
        return True

    def _boundary(self, op):
        if self.open["recs"]:
            self._close_open()
        self.open["pre"].append(op)

    @property
    def pending(self):
        return len(self.open["recs"]) + sum(len(s["recs"]) for s in self.closed)

    # -- the flush path
    def _stop_update(self, sid, client, st, state, oid="", trig=0):
        st = st or dict(sym="", stop_px=0, limit_px=0, qty=0, kind=0)
        self.stop_updates.append(dict(stop_id=f"SID-{sid}", order_id=oid, client_id=client, symbol=st["sym"],
                                      state=state, scale=4, stop_price=st["stop_px"], limit_price=st["limit_px"],
                                      trigger_price=trig, quantity=st["qty"], kind=st["kind"]))

    def _process(self):
        for ev in self.ring:
            st = self.stops.pop(int(ev["id"]))
            oid = self.next_oid
            self.next_oid += 1
            k = int(ev["kind"])
            if not never_rests(k):
                self.live[oid] = [st["client"], st["sym"], int(ev["qty"]), False]
            self._append(dict(seq=oid, px=int(ev["limit_px_q4"]), qty=int(ev["qty"]), sid=int(ev["symbol"]), kind=k,
                              client=st["client"], sym=st["sym"]))
            self.done += 1
            self.pairs.append((f"SID-{st['id']}", f"OID-{oid}"))
            self.triggered.append(st["id"])
            self._stop_update(st["id"], st["client"], st, TRIGGERED, f"OID-{oid}", int(ev["trigger_px_q4"]))
        self.ring = []

    def _apply(self, ops):
        i = 0
        while i < len(ops):
            j = i
            while j < len(ops) and ops[j]["cancel"] == ops[i]["cancel"]:
                j += 1
            run = ops[i:j]
            i = j
            if not run[0]["cancel"]:
                self.tb.add(sm.stops([(o["id"], o["stop"]["stop_px"], o["stop"]["limit_px"], o["stop"]["qty"],
                                       o["stop"]["sidx"], o["stop"]["kind"]) for o in run]))
                for o in run:
                    self.stops[o["id"]]["armed"] = True
                    self._stop_update(o["id"], o["client"], o["stop"], ARMED)
                continue
            ids = sorted({o["id"] for o in run if not o["unknown"]})
            found = dict(zip(ids, self.tb.cancel(ids)))
            self._process()
            seen = set()
            for o in run:
                hit = not o["unknown"] and o["id"] not in seen and found[o["id"]]
                seen.add(o["id"])
                if hit:
                    self.stops.pop(o["id"], None)
                    self.done += 1
                self._stop_update(o["id"], o["client"], o["stop"], CANCELED if hit else CANCEL_REJECTED)

    def _emit(self, recs, res, tape):
        up = self.order_updates

        def push(oid, client, sym, status, px, fq, rem):
            up.append(dict(order_id=f"OID-{oid}", client_id=client, symbol=sym, status=status, fill_price=px, scale=4,
                           fill_quantity=fq, remaining_quantity=rem))

        for r, o in zip(recs, res):
            rem = r["qty"]
            for f in tape[int(o["tape_offset"]): int(o["tape_offset"]) + int(o["fill_count"])]:
                mk = self.live.get(int(f["maker_seq"]))
                q, p = int(f["qty"]), int(f["price_q4"])
                if mk is not None:
                    mk[2] -= q
                    mk[3] = True
                    push(int(f["maker_seq"]), mk[0], mk[1], ST_PARTIAL if mk[2] > 0 else ST_FILLED, p, q, mk[2])
                    if mk[2] <= 0:
                        del self.live[int(f["maker_seq"])]
                rem -= q
                push(r["seq"], r["client"], r["sym"], ST_PARTIAL if rem > 0 else ST_FILLED, p, q, rem)
            status, left = int(o["status"]), int(o["remaining_qty"])
            if status in (ST_REJECTED, ST_CANCELED) or (int(o["fill_count"]) == 0 and status == ST_NEW):
                push(r["seq"], r["client"], r["sym"], status, 0, 0, left)
            if never_rests(r["kind"]):
                continue
            if left > 0 and status in (ST_NEW, ST_PARTIAL):
                self.live[r["seq"]] = [r["client"], r["sym"], left, int(o["fill_count"]) != 0]
            else:
                self.live.pop(r["seq"], None)

    def flush(self):
        """-> (seq list, results, fills) of the records this flush matched."""
        import matching_engine_amd as me

        self._close_open()
        total = sum(len(s["recs"]) for s in self.closed)
        taken, seqs, ress, tapes = 0, [], [], []
        while self.closed and (taken < total or not self.closed[0]["recs"]):
            sl = self.closed.popleft()
            taken += len(sl["recs"])
            self._apply(sl["pre"])
            recs = sl["recs"]
            if not recs:
                continue
            b = me.Batch(np.array([r["seq"] for r in recs], np.uint64), np.array([r["px"] for r in recs], np.int64),
                         np.array([r["qty"] for r in recs], np.int32), np.array([r["sid"] for r in recs], np.uint32),
                         np.array([r["kind"] for r in recs], np.uint8))
            res, tape = self.ob.submit(b)
            self.slices += 1
            self.tb.feed(tape)
            self.ring.extend(self.tb.job(self.slices))
            self._emit(recs, res, tape)
            seqs += [r["seq"] for r in recs]
            ress.append(res)
            tapes.append(tape)
            self._process()
        return seqs, ress, tapes

    def listed(self, client=None):
        return [(f"SID-{i}", ARMED if st["armed"] else QUEUED) for i, st in sorted(self.stops.items())
                if client is None or st["client"] == client]


# ---- helpers and scripts over a real service -----------------------------------------------------------------
def limit(svc, client, sym, side, px, q, tif=GTC):
    r = svc.submit_order(client, sym, LIMIT, side, px, 4, q, tif)
    assert r["success"], r
    return r["order_id"]


def stop(svc, client, sym, otype, side, px, stop_px, q, tif=GTC):
    r = svc.submit_stop(client, sym, otype, side, px, stop_px, 4, q, tif)
    assert r["success"], r
    return r["order_id"]


def flush_out(svc):
    seq, res, fills = svc.flush()
    return ([int(x) for x in seq],
            [tuple(int(r[f]) for f in ("filled_qty", "remaining_qty", "fill_count", "tape_offset", "status", "reason"))
             for r in res],
            [tuple(int(f[n]) for n in ("taker_seq", "maker_seq", "price_q4", "qty", "symbol")) for f in fills])


def stop_rows(db):
    con = sqlite3.connect(db)
    try:
        return list(con.execute("SELECT stop_id, client_id, symbol, side, order_type, tif, stop_price, limit_price, "
                                "quantity, status, order_id, trigger_price FROM stops ORDER BY stop_id"))
    finally:
        con.close()


def order_rows(db):
    con = sqlite3.connect(db)
    try:
        return list(con.execute("SELECT order_id, client_id, symbol, side, price, quantity, status, remaining_quantity "
                                "FROM orders ORDER BY CAST(SUBSTR(order_id, 5) AS INTEGER)"))
    finally:
        con.close()


def has_stops_table(db):
    con = sqlite3.connect(db)
    try:
        return bool(list(con.execute("SELECT name FROM sqlite_master WHERE type='table' AND name='stops'")))
    finally:
        con.close()


class Log:
    """Everything a service shows after each step, in order."""

    def __init__(self, svc, db=None):
        self.svc, self.db, self.steps = svc, db, []

    def step(self, what, flush=True):
        s = self.svc
        out = flush_out(s) if flush else None
        self.steps.append(dict(what=what, flush=out, pending=s.pending, next_oid=s.next_oid,
                               stop_updates=s.stop_updates(), order_updates=s.order_updates(), stops=s.stops(),
                               stats=s.stop_stats(), stop_rows=stop_rows(self.db) if self.db else None,
                               order_rows=order_rows(self.db) if self.db else None))
        return self.steps[-1]


def script_basic(svc, db=None):
    """Rest SELL 10 @ MID on A; a BUY stop-MARKET 5 at MID on A and a SELL stop at MID on B (which must not
    trigger); BUY 1 @ MID trades."""
    log = Log(svc, db)
    limit(svc, "maker", "A", SELL, MID, 10)
    log.step("rest")
    sa = stop(svc, "alice", "A", MARKET, BUY, 0, MID, 5)
    sb = stop(svc, "bob", "B", MARKET, SELL, 0, MID, 3)
    limit(svc, "carol", "A", BUY, MID, 1)
    log.step("trade")    # TRIGGERED, the MARKET pending
    log.step("market")   # its fills
    log.step("idle")
    return log.steps, (sa, sb)


def script_cascade(svc, db=None):
    """Three SELL stop-MARKETs at descending prices over a ladder of bids: each triggered sell trades one level
    lower and triggers the next. One step per flush."""
    log = Log(svc, db)
    for k in range(5):
        limit(svc, "maker", "A", BUY, MID - k, 2)
    log.step("ladder")
    for k in range(3):
        stop(svc, f"c{k}", "A", MARKET, SELL, 0, MID - k, 2 + k)
    limit(svc, "x", "A", SELL, MID, 1)  # trades at MID: the first stop goes
    n = 0
    while True:
        log.step(f"step {n}")
        n += 1
        if svc.pending == 0:
            break
        assert n < 10
    return log.steps, n


def script_cancel(svc, db=None):
    """Owner check, CANCELED, cancel after the trigger (TRIGGERED then CANCEL_REJECTED), an add and a cancel at one
    boundary, a duplicate cancel, an id from the future."""
    log = Log(svc, db)
    limit(svc, "maker", "A", SELL, MID, 10)
    s1 = stop(svc, "alice", "A", LIMIT, BUY, MID + 5, MID, 4)
    s2 = stop(svc, "alice", "A", MARKET, BUY, 0, MID + 50, 1)
    r = svc.cancel_stop("mallory", s1)
    assert not r["success"] and r["error_message"] == "stop belongs to another client", r
    log.step("armed")
    assert svc.cancel_stop("alice", s2)["success"]
    log.step("canceled")
    limit(svc, "carol", "A", BUY, MID, 1)   # triggers s1 ...
    assert svc.cancel_stop("alice", s1)["success"]  # ... and the cancel comes behind the trade
    log.step("trigger then reject")
    s3 = stop(svc, "bob", "B", MARKET, SELL, 0, MID, 2)   # one boundary: add, cancel, cancel again, a future id
    assert svc.cancel_stop("bob", s3)["success"]
    assert svc.cancel_stop("bob", s3)["success"]
    assert svc.cancel_stop("bob", "SID-999")["success"]
    log.step("one boundary")
    log.step("drain")
    return log.steps, (s1, s2, s3)


def script_restart(make, db, cap=8):
    """Persist, destroy, re-create over a fresh backend. make(db) -> (service, finish): a service over a fresh
    backend on the database, and the call that destroys both. Of four stops one triggers and its order is flushed,
    one triggers and its order is never flushed (it comes back ARMED), one is cancelled, one stays armed."""
    steps = []
    svc, finish = make(db)
    try:
        svc.stops_enable(cap)
        log = Log(svc, db)
        limit(svc, "maker", "A", SELL, MID, 10)
        limit(svc, "maker", "A", SELL, MID + 1, 10)
        s1 = stop(svc, "alice", "A", MARKET, BUY, 0, MID, 2)
        s2 = stop(svc, "alice", "A", LIMIT, BUY, MID + 2, MID + 1, 3, IOC)
        s3 = stop(svc, "bob", "B", MARKET, SELL, 0, MID, 4)
        s4 = stop(svc, "bob", "A", MARKET, BUY, 0, MID + 9, 5)
        limit(svc, "carol", "A", BUY, MID, 1)
        log.step("s1 triggers")
        assert svc.cancel_stop("bob", s3)["success"]
        log.step("s1's order fills, s3 is cancelled")
        limit(svc, "carol", "A", BUY, MID + 1, 8)  # 7 @ MID, 1 @ MID + 1
        log.step("s2 triggers, its order stays pending")
        steps += log.steps
    finally:
        finish()
    steps.append(dict(what="destroyed", stop_rows=stop_rows(db), order_rows=order_rows(db)))
    svc, finish = make(db)
    try:
        log = Log(svc, db)
        log.step("books rebuilt")
        svc.stops_enable(cap)
        log.step("re-armed", flush=False)
        stop(svc, "zed", "B", MARKET, BUY, 0, MID, 1)
        limit(svc, "carol", "A", BUY, MID + 1, 1)  # the next qualifying fill: s2 triggers again
        log.step("s2 triggers again")
        log.step("its order")
        log.step("idle")
        steps += log.steps
    finally:
        finish()
    steps.append(dict(what="destroyed again", stop_rows=stop_rows(db), order_rows=order_rows(db)))
    return steps, (s1, s2, s3, s4)


def script_two_in_flight(svc, db=None):
    """Several boundaries inside one flush: stops on both symbols, each armed in front of a slice that triggers
    it, so events of the later slice can be readable while the earlier one is still being collected."""
    log = Log(svc, db)
    for sym in ("A", "B"):
        limit(svc, "maker", sym, SELL, MID, 50)
        limit(svc, "maker", sym, BUY, MID - 10, 50)
    log.step("rest")
    for k in range(3):
        stop(svc, "alice", "A", MARKET, BUY, 0, MID, 1 + k)      # boundary
        limit(svc, "carol", "A", BUY, MID, 1)                    # slice: triggers it
        stop(svc, "bob", "B", LIMIT, SELL, MID - 10, MID, 2 + k)  # boundary
        limit(svc, "dave", "B", BUY, MID, 1)                     # slice: triggers it
    log.step("six slices")
    while svc.pending:
        log.step("more")
    return log.steps, None
