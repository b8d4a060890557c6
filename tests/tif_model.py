"""Model of the time-in-force instructions — TEST INFRASTRUCTURE ONLY.

A plain-Python restatement of the table in DESIGN.md §2 / include/me_engine.h over `oracle.pybook.PyBook`'s
containers, written from the spec and not from the kernels: bits 4-5 of a record's kind byte carry
GTC (0), IOC (1), FOK (2) or POST_ONLY (3); bits 6-7 are ignored; CANCEL records ignore the bits.

  IOC        crosses as a LIMIT at its price; the remainder is discarded: FILLED, or CANCELED with
             remaining_qty = the discarded part. A no-op on a MARKET.
  FOK        fillable when the opposite side's resting quantity at prices within the limit (any price
             for a MARKET) is >= qty on the book as it stands at that record; then it executes like the
             IOC / MARKET and ends FILLED. Else killed: CANCELED, filled 0, remaining = qty, no fills.
  POST_ONLY  LIMIT only: REJECTED / WOULD_CROSS (filled 0, remaining = qty) when the opposite best price
             is within its limit, else it rests whole (NEW). On a MARKET: REJECTED / BAD_TIF.
  reject order: the existing reasons first, in their order, then BAD_TIF, then WOULD_CROSS.

`TifBook.submit` also records a verdict per record in `self.verdicts` (see V_*), which the rewrite test
(tests/test_tif_model.py) uses to turn a TIF stream into plain records for the native oracle. The module
also holds the seeded stream generator the CPU and GPU suites share.
"""
from __future__ import annotations

import numpy as np

from oracle.pybook import (BUY, FILL_DTYPE, RESULT_DTYPE, RJ_BAD_QTY, RJ_BAD_SEQ, RJ_BAD_SIDE, RJ_BAD_SYMBOL, RJ_NONE,
                           RJ_UNKNOWN, SELL, ST_CANCELED, ST_FILLED, ST_NEW, ST_PARTIAL, ST_REJECTED, PyBook)

TIF_GTC, TIF_IOC, TIF_FOK, TIF_POST_ONLY = 0, 1, 2, 3
RJ_WOULD_CROSS, RJ_BAD_TIF = 8, 9

# verdicts: what became of a record, for the rewrite into plain records
V_PLAIN = 0        # tif 0, a cancel, or a record rejected for an existing reason: unchanged
V_IOC = 1          # an IOC (or a fillable FOK) LIMIT: a LIMIT followed by a cancel of itself
V_DROP = 2         # a killed FOK, a rejected POST_ONLY, MARKET + POST_ONLY: no effect on the book
V_POST = 3         # an accepted POST_ONLY: a plain LIMIT
V_MARKET = 4       # a MARKET with IOC or a fillable MARKET FOK: a plain MARKET


def kind(side, otype=0, op=0, tif=0):
    return (side & 3) | ((otype & 1) << 2) | ((op & 1) << 3) | ((tif & 3) << 4)


class TifBook(PyBook):
    """PyBook with the time-in-force bits. Same interface (submit / dump) plus resting()."""

    def __init__(self, num_symbols):
        super().__init__(num_symbols)
        self.verdicts = []

    def resting(self):
        return len(self.live)

    def _liquidity(self, opp, side, market, px, want):
        """Resting quantity of the opposite side at prices within the limit, summed best price first
        until it reaches `want` (reads only)."""
        total = 0
        for k, fifo in opp.levels.items():
            p = -k if opp.bids else k
            if not market and (p > px if side == BUY else p < px):
                break
            total += sum(e[1] for e in fifo if e[1] > 0)
            if total >= want:
                break
        return total

    def _take(self, opp, side, anyprice, px, seq, s, rem, tape):
        while rem > 0:
            p = opp.best()
            if p is None or (not anyprice and (p > px if side == BUY else p < px)):
                break
            fifo = opp.fifo(p)
            while rem > 0 and fifo:
                e = fifo[0]
                if e[1] == 0:
                    fifo.popleft()
                    continue
                t = min(rem, e[1])
                tape.append((seq, e[0], p, t, s))
                e[1] -= t
                rem -= t
                if e[1] == 0:
                    fifo.popleft()
                    del self.live[e[0]]
            opp.drop_if_empty(p)
        return rem

    def submit(self, b):
        n = len(b.seq)
        res = np.zeros(n, dtype=RESULT_DTYPE)
        tape = []
        self.verdicts = [V_PLAIN] * n
        for i in range(n):
            seq, px, q = int(b.seq[i]), int(b.price_q4[i]), int(b.qty[i])
            s, kd = int(b.symbol[i]), int(b.kind[i])
            side, market, cancel, tif = kd & 3, bool(kd & 4), bool(kd & 8), (kd >> 4) & 3
            r = res[i]
            r["tape_offset"] = len(tape)
            if s >= self.S:
                r["status"], r["reason"] = ST_REJECTED, RJ_BAD_SYMBOL
                continue
            if cancel:  # the bits are ignored
                hit = self.live.get(px)
                if hit is None or hit[0] != s:
                    r["status"], r["reason"] = ST_REJECTED, RJ_UNKNOWN
                    continue
                _, tside, tprice, entry = hit
                got = entry[1]
                entry[1] = 0
                del self.live[px]
                (self.side[s][0] if tside == BUY else self.side[s][1]).drop_if_empty(tprice)
                r["status"], r["remaining_qty"] = ST_CANCELED, got
                continue
            if q <= 0:
                r["status"], r["reason"] = ST_REJECTED, RJ_BAD_QTY
                continue
            r["remaining_qty"] = q
            if side not in (BUY, SELL):
                r["status"], r["reason"] = ST_REJECTED, RJ_BAD_SIDE
                continue
            if seq == 0:
                r["status"], r["reason"] = ST_REJECTED, RJ_BAD_SEQ
                continue
            own, opp = (self.side[s][0], self.side[s][1]) if side == BUY else (self.side[s][1], self.side[s][0])
            if tif == TIF_POST_ONLY:
                if market:
                    r["status"], r["reason"] = ST_REJECTED, RJ_BAD_TIF
                    self.verdicts[i] = V_DROP
                    continue
                best = opp.best()
                if best is not None and (best <= px if side == BUY else best >= px):
                    r["status"], r["reason"] = ST_REJECTED, RJ_WOULD_CROSS
                    self.verdicts[i] = V_DROP
                    continue
                self.verdicts[i] = V_POST
            if tif == TIF_FOK and self._liquidity(opp, side, market, px, q) < q:
                r["status"], r["reason"] = ST_CANCELED, RJ_NONE  # killed: filled 0, remaining = qty
                self.verdicts[i] = V_DROP
                continue
            never_rests = market or tif in (TIF_IOC, TIF_FOK)
            if tif in (TIF_IOC, TIF_FOK):
                self.verdicts[i] = V_MARKET if market else V_IOC
            t0 = len(tape)
            rem = self._take(opp, side, market, px, seq, s, q, tape)
            filled = q - rem
            r["filled_qty"], r["remaining_qty"], r["fill_count"] = filled, rem, len(tape) - t0
            if never_rests:
                r["status"] = ST_FILLED if rem == 0 else ST_CANCELED
                continue
            if rem > 0:
                entry = [seq, rem]
                own.fifo(px, create=True).append(entry)
                self.live[seq] = (s, side, px, entry)
            r["status"] = ST_FILLED if rem == 0 else (ST_PARTIAL if filled else ST_NEW)
        fills = np.array(tape, dtype=FILL_DTYPE) if tape else np.zeros(0, dtype=FILL_DTYPE)
        return res, fills


# ---- seeded streams shared by the CPU and GPU suites ------------------------------------------------

class Arrays:
    """A batch as five numpy arrays (the fields PyBook / OracleBook / the engine's Batch read)."""

    def __init__(self, seq, price_q4, qty, symbol, kind):
        self.seq = np.ascontiguousarray(seq, dtype=np.uint64)
        self.price_q4 = np.ascontiguousarray(price_q4, dtype=np.int64)
        self.qty = np.ascontiguousarray(qty, dtype=np.int32)
        self.symbol = np.ascontiguousarray(symbol, dtype=np.uint32)
        self.kind = np.ascontiguousarray(kind, dtype=np.uint8)

    def __len__(self):
        return len(self.seq)


def base_prices(num_symbols, levels):
    """Window base of symbol s: its mid is base + levels / 2."""
    return np.array([1_000_000 + 10_000 * s for s in range(num_symbols)], dtype=np.int64)


def tif_stream(seed, num_symbols, levels, nbatches, batch, *, spread=12, max_qty=60, far_pct=0, bad_pct=1,
               mix=(35, 20, 10, 10, 10, 15), seq_start=1, skew=False,
               market_tifs=(0, 0, 0, 1, 2, 2, 3)):
    """Seeded random stream. mix: % GTC LIMIT, IOC, FOK, POST_ONLY, MARKET, cancel. LIMIT prices are
    mid +- spread ticks (far_pct % of them levels..8 x levels away, outside the window); MARKETs carry a
    random tif of market_tifs (IOC: a no-op, FOK, POST_ONLY: BAD_TIF); bad_pct % of the NEW records have a
    bad qty, side or (rarely) seq 0. skew: half of the records go to symbol 0 (runs of more than 64)."""
    rng = np.random.default_rng(seed)
    base = base_prices(num_symbols, levels)
    cum = np.cumsum(mix)
    assert cum[-1] == 100
    seq = seq_start
    issued = [[] for _ in range(num_symbols)]  # LIMIT seqs a cancel may name
    out = []
    for _ in range(nbatches):
        sq, px, qt, sy, kd = [], [], [], [], []
        for _ in range(batch):
            s = 0 if (skew and rng.random() < 0.5) else int(rng.integers(num_symbols))
            u = int(rng.integers(100))
            side = BUY if rng.random() < 0.5 else SELL
            mid = int(base[s]) + levels // 2
            p = mid + int(rng.integers(-spread, spread + 1))
            if far_pct and rng.integers(100) < far_pct:
                p = mid + int(rng.choice((-1, 1))) * int(rng.integers(levels, 8 * levels))
            q = int(rng.integers(1, max_qty + 1))
            if u >= cum[4]:  # cancel: repeats the last seq, names an issued LIMIT (live or not)
                if issued[s] and seq > seq_start:
                    tgt = issued[s][int(rng.integers(len(issued[s])))] if rng.random() < 0.9 else seq + 1000
                    sq.append(seq - 1)
                    px.append(tgt)
                    qt.append(0)
                    sy.append(s)
                    kd.append(kind(BUY, 0, 1, int(rng.integers(4))))  # the bits are ignored on a cancel
                    continue
                u = 0
            if u < cum[0]:
                k = kind(side, 0, 0, TIF_GTC)
            elif u < cum[1]:
                k = kind(side, 0, 0, TIF_IOC)
            elif u < cum[2]:
                k = kind(side, 0, 0, TIF_FOK)
                q = int(rng.integers(1, 3 * max_qty))  # some need several levels, some cannot fill
            elif u < cum[3]:
                k = kind(side, 0, 0, TIF_POST_ONLY)
                p += -2 if side == BUY else 2  # mostly passive
            else:
                mt = int(rng.choice(market_tifs))
                k = kind(side, 1, 0, mt)
                p = 0
                q = int(rng.integers(1, 2 * max_qty))
            this = seq
            if bad_pct and rng.integers(100) < bad_pct:
                w = int(rng.integers(8))
                if w < 3:
                    q = 0 if w else -5
                elif w < 6:
                    k = (k & ~3) | (0 if w == 3 else 3)
                elif seq == seq_start:
                    this = 0  # seq 0 only where it keeps the stream ascending
            if this:
                seq += 1
            if not (k & 4) and (k >> 4) & 3 in (TIF_GTC, TIF_POST_ONLY) and this:
                issued[s].append(this)
            sq.append(this)
            px.append(p)
            qt.append(q)
            sy.append(s)
            kd.append(k | (int(rng.integers(4)) << 6 if rng.random() < 0.05 else 0))  # bits 6-7: ignored
        out.append(Arrays(sq, px, qt, sy, kd))
    return base, out
