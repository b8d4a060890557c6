"""Model of the depth feed (include/me_engine.h me_depth_event) — TEST INFRASTRUCTURE ONLY.

The view of (symbol, side) at depth D is read from a book's `snapshot(s, D)` (the CPU oracle's, the
engine's, or anything with that method): the side's D best levels as (price, total), best first.
`DepthModel.expect` is "views now against the views last published": per changed side a SET (qty = the new
total) for every price that is new or has another total, a DELETE (qty 0) for every published price that
left, merged in priority order (descending price for bids, ascending for asks); sides ascend by symbol,
bids first; the published views move on. Comparisons with the engine's events are exact array equality.
"""
from __future__ import annotations

import numpy as np

DEPTH_DTYPE = np.dtype(
    [("price_q4", "<i8"), ("qty", "<i8"), ("batches", "<u8"), ("symbol", "<u4"), ("side", "u1"), ("pad", "u1", (3,))]
)
BUY, SELL = 1, 2


def views(book, S, D):
    """[[bids, asks]] per symbol, each side a list of (price, qty), best first, at most D long."""
    out = []
    for s in range(S):
        bids, asks = book.snapshot(s, D)
        out.append([[(int(x["price_q4"]), int(x["total_qty"])) for x in side][:D] for side in (bids, asks)])
    return out


def _side_events(new, pub, side):
    """The events that turn the published view `pub` into `new`, in priority order."""
    was, now = dict(pub), dict(new)
    ev = [(p, q) for p, q in new if was.get(p) != q] + [(p, 0) for p, _ in pub if p not in now]
    ev.sort(key=lambda e: -e[0] if side == 0 else e[0])
    return ev


class DepthModel:
    """The feed over `book` at depth D: the published views start empty."""

    def __init__(self, book, num_symbols, depth, symbol_ids=None):
        self.book, self.S, self.D, self.ids = book, num_symbols, depth, symbol_ids
        self.published = [[[], []] for _ in range(num_symbols)]

    def _diff(self, now, batches):
        rows = []
        for s in range(self.S):
            g = s if self.ids is None else int(self.ids[s])
            for side in (0, 1):
                for p, q in _side_events(now[s][side], self.published[s][side], side):
                    rows.append((p, q, batches, g, BUY if side == 0 else SELL, (0, 0, 0)))
        return np.array(rows, dtype=DEPTH_DTYPE) if rows else np.zeros(0, dtype=DEPTH_DTYPE)

    def expect(self, batches):
        """The events of a job run now, stamped `batches`; publishes the views."""
        now = views(self.book, self.S, self.D)
        ev = self._diff(now, batches)
        self.published = now
        return ev

    def peek(self):
        """The events a job run now would emit (stamp 0), without publishing (a deferred job)."""
        return self._diff(views(self.book, self.S, self.D), 0)


def empty_maps(S):
    return [[{}, {}] for _ in range(S)]


def replay(maps, events, symbol_ids=None):
    """Apply events in order to {price: qty} maps per (local symbol, side); returns the maps."""
    row = None if symbol_ids is None else {int(g): i for i, g in enumerate(symbol_ids)}
    for e in events:
        i = int(e["symbol"]) if row is None else row[int(e["symbol"])]
        m = maps[i][0 if int(e["side"]) == BUY else 1]
        if int(e["qty"]) > 0:
            m[int(e["price_q4"])] = int(e["qty"])
        else:
            m.pop(int(e["price_q4"]), None)
    return maps


def same_views(maps, vw):
    """The replayed maps hold exactly the views `vw` (of views())."""
    for m, v in zip(maps, vw):
        for side in (0, 1):
            if sorted(m[side].items(), reverse=side == 0) != list(v[side]):
                return False
    return len(maps) == len(vw)
