"""Model of the top-of-book change feed (include/me_engine.h me_quote) — TEST
INFRASTRUCTURE ONLY.

A symbol's quote is read from a book's `snapshot(s, 1)` (the CPU oracle's, or anything with that
method): per side the best level's price and total quantity, flags bit 0 has_bid / bit 1 has_ask, an
absent side price and quantity 0. `QuoteModel.expect` is "state now against last published": one event
per symbol whose quote differs, ascending by symbol, and the published table moves on. Comparisons with
the engine's events are exact array equality.
"""
from __future__ import annotations

import numpy as np

QUOTE_DTYPE = np.dtype(
    [("bid_price_q4", "<i8"), ("ask_price_q4", "<i8"), ("bid_qty", "<i8"), ("ask_qty", "<i8"), ("batches", "<u8"),
     ("symbol", "<u4"), ("flags", "<u4")]
)
HAS_BID, HAS_ASK = 1, 2
_FIELDS = ("bid_price_q4", "ask_price_q4", "bid_qty", "ask_qty", "flags")


def tops(book, num_symbols, symbol_ids=None):
    """The current quote of every symbol as QUOTE_DTYPE rows (batches 0), row = local symbol."""
    t = np.zeros(num_symbols, dtype=QUOTE_DTYPE)
    t["symbol"] = np.arange(num_symbols) if symbol_ids is None else symbol_ids
    for s in range(num_symbols):
        bids, asks = book.snapshot(s, 1)
        if len(bids):
            t[s]["bid_price_q4"], t[s]["bid_qty"] = bids[0]["price_q4"], bids[0]["total_qty"]
            t[s]["flags"] |= HAS_BID
        if len(asks):
            t[s]["ask_price_q4"], t[s]["ask_qty"] = asks[0]["price_q4"], asks[0]["total_qty"]
            t[s]["flags"] |= HAS_ASK
    return t


def differs(a, b):
    """Rows whose quote differs (the stamp does not count)."""
    d = np.zeros(len(a), dtype=bool)
    for f in _FIELDS:
        d |= a[f] != b[f]
    return d


class QuoteModel:
    """The feed over `book`: published starts as "both sides absent"."""

    def __init__(self, book, num_symbols, symbol_ids=None):
        self.book, self.S, self.ids = book, num_symbols, symbol_ids
        self.published = tops(_Empty(), num_symbols, symbol_ids)

    def expect(self, batches):
        """The events of a job run now, stamped `batches`; publishes them."""
        now = tops(self.book, self.S, self.ids)
        ev = now[differs(now, self.published)].copy()
        ev["batches"] = batches
        self.published = now
        return ev

    def peek(self):
        """The changed rows of a job run now, without publishing (a deferred job)."""
        now = tops(self.book, self.S, self.ids)
        return now[differs(now, self.published)]


class _Empty:
    def snapshot(self, s, depth):
        return (), ()


def replay(table, events, symbol_ids=None):
    """Apply events in order to a table of quotes (row = local symbol); returns the table."""
    row = None if symbol_ids is None else {int(g): i for i, g in enumerate(symbol_ids)}
    for e in events:
        i = int(e["symbol"]) if row is None else row[int(e["symbol"])]
        for f in _FIELDS:
            table[i][f] = e[f]
    return table


def same_quotes(a, b):
    return not differs(a, b).any()


class OracleFeed:
    """The quote feed of an oracle-backed matcher or shard (me_matcher.quotes / me_shard_ops.quotes): call
    matched() after every slice the book took; quotes(cap) is me_quotes_read's contract. Events carry local
    symbol ids and the count of slices as their stamp. lag=1 holds the newest slice's events back until the
    next slice is matched (events that reach the reader late, as those of a slice still in flight do)."""

    def __init__(self, book, num_symbols, lag=0):
        self.model = QuoteModel(book, num_symbols)
        self.n, self.lag = 0, lag
        self.pending = self.model.expect(0)

    def matched(self):
        self.n += 1
        self.pending = np.concatenate([self.pending, self.model.expect(self.n)])

    def quotes(self, cap):
        ready = int(np.count_nonzero(self.pending["batches"] + self.lag <= self.n)) if self.lag else len(self.pending)
        k = min(int(cap), ready)
        ev, self.pending = self.pending[:k], self.pending[k:]
        return ev, ready - k
