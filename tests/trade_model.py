"""Model of the trade feed (DESIGN.md §2 "Trade feed", include/me_engine.h me_trade) — TEST INFRASTRUCTURE ONLY.

`TradeModel.feed` takes the tape of every batch (the CPU oracle's fills, in tape order) and folds it into a
pending summary per symbol; `expect` is one job: an event for every symbol with pending fills, ascending by
local symbol id, and the pending summaries are published (emptied). `peek` is the same without publishing (a
deferred job). The arithmetic is done on Python ints; comparisons with the engine's events are exact array
equality. `replay` checks the feed's invariant: events against the fold of every fill of the tapes.
"""
from __future__ import annotations

import numpy as np

TRADE_DTYPE = np.dtype(
    [("taker_seq", "<u8"), ("maker_seq", "<u8"), ("last_price_q4", "<i8"), ("open_price_q4", "<i8"),
     ("high_price_q4", "<i8"), ("low_price_q4", "<i8"), ("volume", "<i8"), ("trades", "<u8"), ("cum_volume", "<i8"),
     ("cum_trades", "<u8"), ("batches", "<u8"), ("last_qty", "<i4"), ("symbol", "<u4")]
)


def fold(fills):
    """The summary of a non-empty run of one symbol's fills in tape order, as a dict of Python ints."""
    px = [int(p) for p in fills["price_q4"]]
    last = fills[-1]
    return dict(taker_seq=int(last["taker_seq"]), maker_seq=int(last["maker_seq"]), last_price_q4=px[-1],
                open_price_q4=px[0], high_price_q4=max(px), low_price_q4=min(px),
                volume=sum(int(q) for q in fills["qty"]), trades=len(px), last_qty=int(last["qty"]))


def merge(a, b):
    """Summary a followed by summary b."""
    if a is None:
        return dict(b)
    m = dict(b)  # the last-fill fields are b's
    m["open_price_q4"] = a["open_price_q4"]
    m["high_price_q4"] = max(a["high_price_q4"], b["high_price_q4"])
    m["low_price_q4"] = min(a["low_price_q4"], b["low_price_q4"])
    m["volume"] = a["volume"] + b["volume"]
    m["trades"] = a["trades"] + b["trades"]
    return m


class TradeModel:
    """The feed of `num_symbols` symbols from the moment it is made (enable): nothing pending, counts zero."""

    def __init__(self, num_symbols, symbol_ids=None):
        self.S = num_symbols
        self.ids = None if symbol_ids is None else [int(g) for g in symbol_ids]
        self.row = None if symbol_ids is None else {int(g): i for i, g in enumerate(symbol_ids)}
        self.pending = [None] * num_symbols
        self.cum = [[0, 0] for _ in range(num_symbols)]
        self.nfed = [0] * num_symbols  # batches fed that held a fill of the symbol, since its last event

    def feed(self, fills):
        """The tape of one batch (FILL_DTYPE, tape order)."""
        if not len(fills):
            return
        for g in np.unique(fills["symbol"]):
            s = int(g) if self.row is None else self.row[int(g)]
            f = fold(fills[fills["symbol"] == g])
            self.pending[s] = merge(self.pending[s], f)
            self.cum[s][0] += f["volume"]
            self.cum[s][1] += f["trades"]
            self.nfed[s] += 1

    def _events(self, batches):
        rows = [s for s in range(self.S) if self.pending[s] is not None]
        ev = np.zeros(len(rows), dtype=TRADE_DTYPE)
        for k, s in enumerate(rows):
            for name, v in self.pending[s].items():
                ev[k][name] = v
            ev[k]["cum_volume"], ev[k]["cum_trades"] = self.cum[s]
            ev[k]["batches"] = batches
            ev[k]["symbol"] = s if self.ids is None else self.ids[s]
        return ev, rows

    def expect(self, batches):
        """The events of a job run now, stamped `batches`; publishes them."""
        ev, rows = self._events(batches)
        self.spans = {s: self.nfed[s] for s in rows}  # per event: the batches whose fills it covers
        for s in rows:
            self.pending[s] = None
            self.nfed[s] = 0
        return ev

    def peek(self):
        """The events a job run now would hold (stamp 0), without publishing: a deferred job."""
        return self._events(0)[0]


def replay(events, tapes, num_symbols, symbol_ids=None):
    """The invariant of the feed after a sync and a full drain. `events`: every event read since enable, in
    order; `tapes`: the tape of every batch since enable, in order. For every symbol: the sums of volume and
    trades over its events equal its last event's cumulative pair and the fold of all its fills; the last
    event's last-fill fields are its last fill; events chain (each cumulative pair is the previous one plus the
    event's own) and every event's high / low bracket its open and last. Raises AssertionError."""
    ids = list(range(num_symbols)) if symbol_ids is None else [int(g) for g in symbol_ids]
    fills = np.concatenate(tapes) if len(tapes) else np.zeros(0, dtype=[("symbol", "<u4")])
    for g in ids:
        ev = events[events["symbol"] == g]
        f = fills[fills["symbol"] == g] if len(fills) else fills
        if not len(f):
            assert not len(ev), f"symbol {g}: events without fills"
            continue
        assert len(ev), f"symbol {g}: {len(f)} fills and no event"
        want = fold(f)
        vol = sum(int(v) for v in ev["volume"])
        n = sum(int(v) for v in ev["trades"])
        last = ev[-1]
        assert (vol, n) == (int(last["cum_volume"]), int(last["cum_trades"])) == (want["volume"], want["trades"]), \
            f"symbol {g}: sums {(vol, n)}, last cumulative {(int(last['cum_volume']), int(last['cum_trades']))}, " \
            f"tapes {(want['volume'], want['trades'])}"
        for name in ("taker_seq", "maker_seq", "last_price_q4", "last_qty"):
            assert int(last[name]) == want[name], f"symbol {g}: last event's {name}"
        assert int(ev[0]["open_price_q4"]) == want["open_price_q4"], f"symbol {g}: first event's open"
        assert max(int(v) for v in ev["high_price_q4"]) == want["high_price_q4"], f"symbol {g}: high"
        assert min(int(v) for v in ev["low_price_q4"]) == want["low_price_q4"], f"symbol {g}: low"
        cv = cn = 0
        for e in ev:
            cv += int(e["volume"])
            cn += int(e["trades"])
            assert (cv, cn) == (int(e["cum_volume"]), int(e["cum_trades"])), f"symbol {g}: cumulative chain"
            assert int(e["trades"]) >= 1
            assert int(e["low_price_q4"]) <= min(int(e["open_price_q4"]), int(e["last_price_q4"]))
            assert int(e["high_price_q4"]) >= max(int(e["open_price_q4"]), int(e["last_price_q4"]))
