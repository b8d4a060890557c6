"""Model of the trigger book (DESIGN.md §2 "Stop orders", include/me_engine.h me_stop / me_stop_event) — TEST
INFRASTRUCTURE ONLY.

`StopModel.add` appends stops in table order (ascending id), `cancel` answers found per id, `feed` takes the tape
of every batch of the launch being formed (the CPU oracle's fills) and keeps each symbol's highest and lowest
fill price, and `job` is one device job: every live stop whose symbol traded in the launch and whose stop price
the launch's high (BUY) or low (SELL) reached leaves the table as one event, in table order; the launch's
extremes are then forgotten. The arithmetic is done on Python ints; comparisons with the engine's events are
exact array equality. `brute` is the same answer worked out the slow way, fill by fill.
"""
from __future__ import annotations

import numpy as np

STOP_DTYPE = np.dtype(
    [("id", "<u8"), ("stop_px_q4", "<i8"), ("limit_px_q4", "<i8"), ("qty", "<i4"), ("symbol", "<u4"), ("kind", "u1"),
     ("pad", "u1", (7,))]
)
STOP_EVENT_DTYPE = np.dtype(
    [("id", "<u8"), ("stop_px_q4", "<i8"), ("limit_px_q4", "<i8"), ("trigger_px_q4", "<i8"), ("batches", "<u8"),
     ("qty", "<i4"), ("symbol", "<u4"), ("kind", "u1"), ("pad", "u1", (15,))]
)
BUY, SELL = 1, 2
FIELDS = ("id", "stop_px_q4", "limit_px_q4", "qty", "symbol", "kind")


def stops(rows) -> np.ndarray:
    """STOP_DTYPE records from (id, stop_px, limit_px, qty, symbol, kind) tuples."""
    a = np.zeros(len(rows), dtype=STOP_DTYPE)
    for k, r in enumerate(rows):
        for name, v in zip(FIELDS, r):
            a[k][name] = v
    return a


class StopModel:
    def __init__(self, num_symbols):
        self.S = num_symbols
        self.table = []  # dicts of Python ints, ascending id; triggered and cancelled stops are removed
        self.hi = {}     # symbol -> highest fill price of the launch being formed (absent: no fill)
        self.lo = {}

    def add(self, recs):
        for r in np.asarray(recs, dtype=STOP_DTYPE).reshape(-1):
            d = {name: int(r[name]) for name in FIELDS}
            assert d["id"] > 0 and (not self.table or d["id"] > self.table[-1]["id"]) and d["symbol"] < self.S
            assert d["kind"] & 3 in (BUY, SELL) and d["qty"] > 0 and not d["kind"] & 8
            self.table.append(d)

    def cancel(self, ids):
        found = np.zeros(len(ids), dtype=np.uint8)
        for k, i in enumerate(ids):
            hit = [d for d in self.table if d["id"] == int(i)]
            if hit:
                self.table.remove(hit[0])
                found[k] = 1
        return found

    def feed(self, fills):
        """The tape of one batch of the launch being formed (FILL_DTYPE)."""
        for f in fills:
            s, p = int(f["symbol"]), int(f["price_q4"])
            self.hi[s] = max(self.hi.get(s, p), p)
            self.lo[s] = min(self.lo.get(s, p), p)

    def job(self, batches):
        """The events of the job behind the launch fed so far, stamped `batches`."""
        out, keep = [], []
        for d in self.table:
            s = d["symbol"]
            if s in self.hi:
                buy = d["kind"] & 3 == BUY
                px = self.hi[s] if buy else self.lo[s]
                if (px >= d["stop_px_q4"]) if buy else (px <= d["stop_px_q4"]):
                    out.append((d, px))
                    continue
            keep.append(d)
        self.table = keep
        self.hi, self.lo = {}, {}
        ev = np.zeros(len(out), dtype=STOP_EVENT_DTYPE)
        for k, (d, px) in enumerate(out):
            for name in FIELDS:
                ev[k][name] = d[name]
            ev[k]["trigger_px_q4"] = px
            ev[k]["batches"] = batches
        return ev

    def dump(self):
        return stops([tuple(d[name] for name in FIELDS) for d in self.table])


def brute(live, tapes):
    """Which of `live` (STOP_DTYPE, table order) one job triggers given the launch's tapes, fill by fill: a list
    of (index into live, trigger price). A BUY stop's trigger price is the highest fill price of its symbol, a
    SELL stop's the lowest, and it triggers iff some fill of its symbol is at or through its stop price."""
    out = []
    for k, r in enumerate(live):
        buy = int(r["kind"]) & 3 == BUY
        hit, best = False, None
        for t in tapes:
            for f in t:
                if int(f["symbol"]) != int(r["symbol"]):
                    continue
                p = int(f["price_q4"])
                hit = hit or (p >= int(r["stop_px_q4"]) if buy else p <= int(r["stop_px_q4"]))
                best = p if best is None else (max(best, p) if buy else min(best, p))
        if hit:
            out.append((k, best))
    return out
