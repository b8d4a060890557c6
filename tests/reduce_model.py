"""Model of the REDUCE record (include/me_engine.h ME_KIND_REDUCE) — TEST INFRASTRUCTURE ONLY.

A batch record whose kind byte has bit 3 (CANCEL) and bit 2 (type) both set takes `qty` = d off the resting
order whose seq is in `price_q4`. Written from that paragraph over `tests.tif_model.TifBook`'s containers,
not from the kernels (the native oracle and oracle/pybook.py read 0x0D as a plain cancel):

  reject order   BAD_SYMBOL, then BAD_QTY (d <= 0, whether or not the target lives), then UNKNOWN_ORDER (the
                 cancel's rule: no live resting order of this symbol has that seq).
  d >= r         exactly a cancel: CANCELED, remaining_qty = r, the order leaves the book.
  d <  r         the order keeps its seq and its place in the FIFO and holds r - d: NEW, remaining_qty = r - d,
                 filled_qty 0, fill_count 0, reason NONE.
  side and time-in-force bits are ignored; tape_offset follows the general rule; a REDUCE never rests.

`ReduceBook.submit` notes what became of every REDUCE in `self.reduces` (index, target, d, r or None), which
the rewrite test (tests/test_reduce_model.py) uses to pin the model with the native oracle. The module also
holds the seeded stream generator the CPU and GPU suites share.
"""
from __future__ import annotations

import numpy as np

from oracle.pybook import BUY, RESULT_DTYPE, FILL_DTYPE, RJ_BAD_QTY, RJ_BAD_SYMBOL, RJ_UNKNOWN, ST_CANCELED, ST_NEW, \
    ST_REJECTED
from tests.tif_model import Arrays, TifBook, base_prices, tif_stream

KIND_REDUCE = 0x0D
INT32_MAX = 2**31 - 1


def is_reduce(kd):
    return (np.asarray(kd) & 0x0C) == 0x0C


def reduce_kind(rng=None):
    """0x0D with random side, time-in-force and reserved bits when an rng is given (all ignored)."""
    if rng is None:
        return KIND_REDUCE
    return 0x0C | int(rng.integers(4)) | (int(rng.integers(16)) << 4)


class ReduceBook(TifBook):
    """TifBook plus the REDUCE record. Same interface."""

    def __init__(self, num_symbols):
        super().__init__(num_symbols)
        self.reduces = []

    def _reduce(self, s, tgt, d, r):
        """One REDUCE on symbol s; fills result row r. Returns the target's quantity before (None: rejected)."""
        if s >= self.S:
            r["status"], r["reason"] = ST_REJECTED, RJ_BAD_SYMBOL
            return None
        if d <= 0:
            r["status"], r["reason"] = ST_REJECTED, RJ_BAD_QTY
            return None
        hit = self.live.get(tgt)
        if hit is None or hit[0] != s:
            r["status"], r["reason"] = ST_REJECTED, RJ_UNKNOWN
            return None
        _, tside, tprice, entry = hit
        had = entry[1]
        if d >= had:
            entry[1] = 0
            del self.live[tgt]
            (self.side[s][0] if tside == BUY else self.side[s][1]).drop_if_empty(tprice)
            r["status"], r["remaining_qty"] = ST_CANCELED, had
        else:
            entry[1] = had - d
            r["status"], r["remaining_qty"] = ST_NEW, had - d
        return had

    def submit(self, b):
        n = len(b.seq)
        red = np.nonzero(is_reduce(b.kind))[0]
        self.reduces = []
        if len(red) == 0:
            return super().submit(b)
        res = np.zeros(n, dtype=RESULT_DTYPE)
        tapes, ntape, verdicts = [], 0, [0] * n
        lo = 0
        for i in list(red) + [n]:
            if i > lo:  # the records between two reduces: TifBook's, their tape offsets moved along
                rr, ff = super().submit(Arrays(b.seq[lo:i], b.price_q4[lo:i], b.qty[lo:i], b.symbol[lo:i],
                                               b.kind[lo:i]))
                rr["tape_offset"] += ntape
                res[lo:i] = rr
                verdicts[lo:i] = self.verdicts
                tapes.append(ff)
                ntape += len(ff)
            if i < n:
                res[i]["tape_offset"] = ntape
                tgt, d = int(b.price_q4[i]), int(b.qty[i])
                had = self._reduce(int(b.symbol[i]), tgt, d, res[i])
                self.reduces.append((int(i), tgt, d, had))
            lo = i + 1
        self.verdicts = verdicts
        fills = np.concatenate(tapes) if tapes else np.zeros(0, dtype=FILL_DTYPE)
        return res, fills


# ---- seeded streams shared by the CPU and GPU suites ------------------------------------------------

def _draw_d(rng, r, max_qty, odd=True):
    """A quantity around r, the target's remaining quantity (None: not live)."""
    if r is None:
        return int(rng.integers(1, max_qty + 1))
    u = int(rng.integers(20 if odd else 16))
    if u < 8:
        return int(rng.integers(1, r)) if r > 1 else 1  # strictly partial
    if u < 10:
        return 1
    if u < 12:
        return max(r - 1, 1)
    if u < 13:
        return r
    if u < 14:
        return r + 1
    if u < 16:
        return r + int(rng.integers(1, max_qty + 1))
    return (0, -1, INT32_MAX, int(rng.integers(-5, 1)))[u - 16]


def reduce_stream(seed, num_symbols, levels, nbatches, batch, *, convert_pct=60, fresh_pct=8, drift=0, odd=True,
                  **kw):
    """A cancel-bearing `tif_stream` (keywords passed on) with convert_pct % of its cancels turned into reduces
    whose d is drawn around the target's remaining quantity at that record, and fresh reduces of recently
    rested orders making up fresh_pct % of every batch (which still holds `batch` records). drift: every
    symbol's LIMIT prices move drift ticks per batch in the symbol's own direction, so windows re-centre and
    earlier orders become far ones. Returns (base, batches). The book behind the draws is a ReduceBook: the
    stream depends on the model only for the choice of d, never for what the engine is checked against."""
    rng = np.random.default_rng(seed * 7919 + 13)
    max_qty = kw.get("max_qty", 60)
    n_fresh = batch * fresh_pct // 100
    base, plain = tif_stream(seed, num_symbols, levels, nbatches, batch - n_fresh, **kw)
    book = ReduceBook(num_symbols)
    recent = [[] for _ in range(num_symbols)]
    out = []
    last_seq = 0
    for k, b in enumerate(plain):
        sq, px, qt, sy, kd = (x.copy() for x in (b.seq, b.price_q4, b.qty, b.symbol, b.kind))
        if drift:
            lim = ((kd & 0x0C) == 0) & (sq != 0)
            px[lim] += (k * drift) * np.where(sy[lim] % 2 == 0, 1, -1)
        ins = np.sort(rng.integers(0, len(sq) + 1, n_fresh)) if n_fresh else np.zeros(0, dtype=np.int64)
        o = ([], [], [], [], [])
        run = ([], [], [], [], [])

        def flush():
            if run[0]:
                book.submit(Arrays(*run))
                for x in run:
                    x.clear()

        def emit(rec):
            for dst in (o, run):
                for j in range(5):
                    dst[j].append(rec[j])

        def left(s, tgt):
            flush()
            hit = book.live.get(tgt)
            return hit[3][1] if hit is not None and hit[0] == s else None

        ip = 0
        for i in range(len(sq) + 1):
            while ip < len(ins) and ins[ip] == i:
                ip += 1
                s = int(rng.integers(num_symbols))
                if last_seq == 0:  # no seq to repeat yet (a reduce takes none of its own): the batch is one short
                    continue
                if not recent[s]:
                    s = next((t for t in range(num_symbols) if recent[t]), None)
                    if s is None:  # nothing to name yet: an unknown target
                        emit((last_seq, 1 << 40, 1, int(rng.integers(num_symbols)), reduce_kind(rng)))
                        continue
                tgt = recent[s][int(rng.integers(len(recent[s])))]
                emit((last_seq, tgt, _draw_d(rng, left(s, tgt), max_qty, odd), s, reduce_kind(rng)))
            if i == len(sq):
                break
            rec = [int(sq[i]), int(px[i]), int(qt[i]), int(sy[i]), int(kd[i])]
            if rec[4] & 8:
                rec[4] &= ~4  # a plain cancel (tif_stream sets no type bit on one; kept explicit)
                if rng.integers(100) < convert_pct:
                    rec[2] = _draw_d(rng, left(rec[3], rec[1]), max_qty, odd)
                    rec[4] = reduce_kind(rng)
            elif not (rec[4] & 4) and (rec[4] >> 4) & 3 in (0, 3) and rec[0]:
                r = recent[rec[3]]
                r.append(rec[0])
                if len(r) > 400:
                    del r[:200]
            if rec[0]:
                last_seq = max(last_seq, rec[0])
            emit(tuple(rec))
        flush()
        out.append(Arrays(*o))
    check_seq_rule(out)
    return base, out


def check_seq_rule(batches):
    """The engine's precondition: a NEW record's seq is above every earlier record's, a CANCEL's or REDUCE's at
    least the previous record's."""
    prev = 0
    for k, b in enumerate(batches):
        for i in range(len(b)):
            cur = int(b.seq[i])
            assert cur > prev or (cur == prev and int(b.kind[i]) & 8) or (prev == 0 and cur == 0), (k, i, prev, cur)
            prev = cur
