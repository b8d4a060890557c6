"""Books and query sets of the order-preview tests — TEST INFRASTRUCTURE ONLY.

A Case is a list of batches that builds books, and after every batch a set of queries (symbol, kind, price_q4,
qty) derived from the model's books at that point: quantities on every maker, chunk and level boundary, limits
at, one tick inside and one tick beyond every level. After each batch the tests also submit ONE of the
previewed records for real, as the next record of the stream. For that the scripts' seqs are spread (a NEW seq a
becomes 4 a, a cancel or reduce repeats whatever came last), which leaves room for one record behind every
batch; cancel and reduce targets move with the seqs.

tests/test_preview_model.py checks the model on these cases and asserts that the query sets hold at least one
of each kind of answer (tags); tests/test_preview_gpu.py runs the same cases through the engine.
"""
from __future__ import annotations

import zlib

import numpy as np

from tests import big_qty, price_edges
from tests import preview_model as pm
from tests import tif_model as tm
from tests.big_qty import Script
from tests.preview_model import BUY, I64_MAX, I64_MIN, SELL, TIF_FOK, TIF_GTC, TIF_IOC, TIF_POST_ONLY
from tests.tif_model import Arrays, kind

MAX = (1 << 31) - 1
CHUNK = 16
LS = (128, 256, 1024, 2048)  # the window depths of tests/gpu_harness.PATHS


def kd(side, market=False, tif=0, hi=0):
    return kind(side, 1 if market else 0, 0, tif) | (hi << 6)


def clip(p):
    return max(I64_MIN, min(I64_MAX, p))


def spread(batches):
    """(batches with spread seqs, the seq left free behind each batch)."""
    out, free, last = [], [], 0
    for a in batches:
        seq = []
        px = a.price_q4.copy()
        for i in range(len(a)):
            s4 = 4 * int(a.seq[i])
            if int(a.kind[i]) & 8:  # repeats whatever came last, unless it takes a seq of its own
                px[i] = 4 * int(px[i])
                last = max(last, s4)
                seq.append(last)
            else:  # (seq 0: a BAD_SEQ record of the seeded streams, left as it is)
                assert s4 == 0 or s4 > last
                last = max(last, s4)
                seq.append(s4)
        out.append(Arrays(seq, px, a.qty, a.symbol, a.kind))
        last += 1
        free.append(last)
    return out, free


def one(seq, q):
    """The query q as a one-record batch with seq `seq`."""
    s, k, px, qty = q
    return Arrays([seq], [px], [qty], [s], [k])


class Case:
    def __init__(self, name, S, L, base, batches, queries, window=None, **kw):
        self.name, self.S, self.L, self.base = name, S, L, np.asarray(base, dtype=np.int64)
        self.batches, self.free = spread(batches)
        self.queries = queries  # (model, k) -> the queries behind batch k
        self.window = window    # {symbol: window base} where the script keeps it in place (None: not known)
        self.kw = kw            # Engine keywords

    def real(self, k, exp):
        """Which query behind batch k is then submitted for real: one with fills three times out of four."""
        rng = np.random.default_rng(zlib.crc32(self.name.encode()) + k)
        hit = np.nonzero(exp["fill_count"] > 0)[0]
        pool = hit if len(hit) and rng.random() < 0.75 else np.arange(len(exp))
        return int(pool[rng.integers(len(pool))])


# ---- queries around a book's boundaries ---------------------------------------------------------------------------------

def around(model, s, cap=10):
    """Queries against both sides of symbol s: per level (the `cap` - 2 best and the two worst) the running
    quantity up to and including it and that +- 1 as LIMIT at its price (GTC, IOC, FOK) and as MARKET; the same
    quantity with the limit one tick inside and one tick beyond; POST_ONLYs at and just short of it; maker
    boundaries of the best level (1, a chunk, the level: each +- 1); the whole side, one more, INT32_MAX."""
    lv = pm.levels_of(model, s)
    out = []
    for side in (BUY, SELL):
        opp = lv[SELL if side == BUY else BUY]
        worse = 1 if side == BUY else -1  # the direction in which prices get worse for the taker
        far_limit = I64_MAX if side == BUY else I64_MIN
        if not opp:
            out += [(s, kd(side, True), 0, 7), (s, kd(side), far_limit, 7), (s, kd(side, tif=TIF_FOK), far_limit, 1),
                    (s, kd(side, tif=TIF_IOC), far_limit, 3), (s, kd(side, tif=TIF_POST_ONLY), far_limit, 2)]
            continue
        cums, c = [], 0
        for _, fifo in opp:
            c += sum(q for _, q in fifo)
            cums.append(c)
        pick = range(len(opp)) if len(opp) <= cap else list(range(cap - 2)) + [len(opp) - 2, len(opp) - 1]
        for n, i in enumerate(pick):
            p, c = opp[i][0], cums[i]
            for d in (-1, 0, 1):
                if not 0 < c + d <= MAX:
                    continue
                for tif in (TIF_GTC, TIF_IOC, TIF_FOK):
                    out.append((s, kd(side, tif=tif), p, c + d))
                out.append((s, kd(side, True, (TIF_GTC, TIF_FOK, TIF_IOC)[n % 3]), 0, c + d))
            for e in (-1, 1):
                pe = clip(p + e * worse)
                out.append((s, kd(side, tif=(TIF_GTC, TIF_IOC)[n % 2]), pe, min(c, MAX)))
                out.append((s, kd(side, tif=TIF_FOK), pe, min(c, MAX)))
                out.append((s, kd(side), pe, MAX))
            out.append((s, kd(side, tif=TIF_POST_ONLY), p, 5))
            out.append((s, kd(side, tif=TIF_POST_ONLY), clip(p - worse), 5))
        fifo, run = opp[0][1], 0
        for j, (_, q) in enumerate(fifo, 1):
            run += q
            if j in (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, len(fifo) - 1, len(fifo)) and run < MAX:
                for d in (-1, 0, 1):
                    if run + d > 0:
                        out.append((s, kd(side, True), 0, run + d))
                        out.append((s, kd(side, tif=TIF_FOK), opp[0][0], run + d))
        for q in (cums[-1], cums[-1] + 1, MAX):
            if 0 < q <= MAX:
                out += [(s, kd(side, True), 0, q), (s, kd(side, True, TIF_FOK), 0, q), (s, kd(side), far_limit, q),
                        (s, kd(side, tif=TIF_FOK), far_limit, q)]
    return out


def tags(lv, q, row, window=None):
    """The kinds of answer `row` (to query q on the levels lv = levels_of(model, symbol)) is an example of."""
    s, k, px, qty = q
    side, market, tif = k & 3, bool(k & 4), (k >> 4) & 3
    st, rj, fc = int(row["status"]), int(row["reason"]), int(row["fill_count"])
    t = set()
    if rj == pm.RJ_WOULD_CROSS:
        t.add("would_cross")
    if st == pm.ST_REJECTED:
        return t
    if tif == TIF_POST_ONLY:
        t.add("post_rests")
    if tif == TIF_FOK:
        t.add("fok_filled" if st == pm.ST_FILLED else "fok_killed")
    if not fc:
        return t
    opp = lv[SELL if side == BUY else BUY]
    n = int(row["levels"])
    totals = [sum(x for _, x in fifo) for _, fifo in opp]
    at_last = int(row["filled_qty"]) - sum(totals[:n - 1])
    whole = at_last == totals[n - 1]
    t.add("boundary" if whole else "partial")
    if window is not None and s in window:
        inwin = [window[s][0] <= p < window[s][0] + window[s][1] for p, _ in opp[:n]]
        if not any(inwin):
            t.add("far_only")
        elif not all(inwin):
            t.add("reaches_far")
    if not market and whole and int(row["remaining_qty"]) > 0 and n < len(opp):
        a, b = sorted((opp[n - 1][0], opp[n][0]))
        if a < px < b:
            t.add("between")
    ntl = pm.notional(row)
    if ntl < 0:
        t.add("neg_notional")
    if abs(ntl) > 1 << 64:
        t.add("big_notional")
    return t


# ---- the scripts ----------------------------------------------------------------------------------------------------------

def _win(base, L, syms):
    return {s: (int(base[s]), L) for s in syms}


def chunks(L):
    """Forty bids of 10 at one price (chunks of 16) and two worse levels; then the third maker, the whole middle
    chunk and the last maker are cancelled. Symbol 1 holds one order a side."""
    S = 2
    base = tm.base_prices(S, L)
    p, m1 = int(base[0]) + L // 2 - 3, int(base[1]) + L // 2
    sc = Script()
    o = [None] + [sc.new(0, BUY, p, 10) for _ in range(40)]
    for _ in range(2):
        sc.new(0, BUY, p - 2, 7)
    sc.new(0, BUY, p - 5, 9)
    sc.new(1, SELL, m1 + 1, 5)
    sc.new(1, BUY, m1 - 1, 5)
    b0 = sc.take()
    sc.cancel(0, o[3])
    for j in range(17, 33):
        sc.cancel(0, o[j])
    sc.cancel(0, o[40])
    b1 = sc.take()

    def queries(model, k):
        q = around(model, 0) + around(model, 1)
        # behind the cancels: the first chunk's live sum 150, the level's total 220, the whole side 243
        for qty in (1, 149, 150, 151, 219, 220, 221, 243, 244, MAX):
            q += [(0, kd(SELL, True), 0, qty), (0, kd(SELL), p, qty), (0, kd(SELL, tif=TIF_IOC), p - 2, qty),
                  (0, kd(SELL, tif=TIF_FOK), p - 5, qty), (0, kd(SELL, tif=TIF_FOK), p, qty),
                  (0, kd(SELL, True, TIF_FOK), 0, qty)]
        return q

    return Case(f"chunks{L}", S, L, base, [b0, b1], queries, window=_win(base, L, (0, 1)))


def window_levels(L):
    return [l for l in sorted({3, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192, L - 65, L - 64, L - 3}) if 2 <= l <= L - 3]


def window_order(L):
    """Symbol 0: asks at window levels on both sides of every 64-level boundary the window has, at the first and
    the last bit of occupancy words, and more than 64 levels apart; symbol 1: bids at the same levels."""
    S = 2
    base = tm.base_prices(S, L)
    lv = window_levels(L)
    sc = Script()
    sc.new(0, BUY, int(base[0]) + 1, 2)
    sc.new(1, SELL, int(base[1]) + L - 2, 2)
    for i, l in enumerate(lv):
        for _ in range(2 if i % 3 == 0 else 1):
            sc.new(0, SELL, int(base[0]) + l, 3 + i)
            sc.new(1, BUY, int(base[1]) + l, 4 + i)
    return Case(f"order{L}", S, L, base, [sc.take()], lambda model, k: around(model, 0, 20) + around(model, 1, 20),
                window=_win(base, L, (0, 1)))


def far(L):
    """Symbol 0: asks on far levels only (a window bid keeps the window in place). Symbol 1: window and far levels
    on both sides. Symbol 2: 70 far bid levels. The second batch cancels far levels between live ones."""
    S = 3
    base = tm.base_prices(S, L)
    b = [int(x) for x in base]
    sc = Script()
    sc.new(0, BUY, b[0] + L // 2 - 2, 5)
    fa0 = []
    for k in range(6):
        fa0.append(sc.new(0, SELL, b[0] + L - 1 + 10 * (k + 1), 30 + k))
        if k % 2:
            sc.new(0, SELL, b[0] + L - 1 + 10 * (k + 1), 4)
    m = b[1] + L // 2
    for px, q in ((m - 1, 5), (m - 1, 6), (m - 4, 7)):
        sc.new(1, BUY, px, q)
    for px, q in ((m + 1, 8), (m + 3, 9)):
        sc.new(1, SELL, px, q)
    fb1, fa1 = [], []
    for k in range(5):
        fb1.append(sc.new(1, BUY, b[1] - 10 * (k + 1), 20 + k))
        fa1.append(sc.new(1, SELL, b[1] + L - 1 + 10 * (k + 1), 25 + k))
    sc.new(2, BUY, b[2] + L // 2 - 1, 3)
    sc.new(2, SELL, b[2] + L // 2 + 2, 4)
    fb2 = [sc.new(2, BUY, b[2] - 3 * (k + 1), k % 5 + 1) for k in range(70)]
    b0 = sc.take()
    for t in (fa0[2], fb1[1], fa1[3], fb2[1], fb2[40], fb2[65]):
        sc.cancel(0 if t == fa0[2] else (2 if t in fb2 else 1), t)
    b1 = sc.take()

    def queries(model, k):
        q = around(model, 0, 12) + around(model, 1, 12) + around(model, 2, 12)
        for n in price_edges.ALIAS_N:  # limits at the alias distances from a far price
            q += [(0, kd(BUY), b[0] + L - 1 + 10 + (1 << n), MAX), (0, kd(BUY, tif=TIF_FOK), b[0] + L - 1 + 10 - (1 << n), 30),
                  (1, kd(SELL), b[1] - 10 - (1 << n), MAX), (1, kd(SELL, tif=TIF_IOC), b[1] - 10 + (1 << n), MAX)]
        return q

    return Case(f"far{L}", S, L, base, [b0, b1], queries, window=_win(base, L, (0, 1, 2)), far_levels=4)


def wide(L):
    """Levels whose totals pass 2^31 and a side whose sum passes 2^32: asks of INT32_MAX, three on the best level,
    two on the next, two on a far level; the second batch takes one lot off the first maker."""
    S = 2
    base = tm.base_prices(S, L)
    mid = int(base[0]) + L // 2
    prices = (mid + 1, mid + 1, mid + 1, mid + 2, mid + 2, int(base[0]) + 2 * L, int(base[0]) + 2 * L)
    sc = Script()
    sc.new(0, BUY, mid - 3, 5)
    sc.new(1, SELL, int(base[1]) + L // 2, 5)
    for px in prices:
        sc.new(0, SELL, px, MAX)
    b0 = sc.take()
    sc.new(0, BUY, 0, 1, market=True)
    b1 = sc.take()

    def queries(model, k):
        q = around(model, 0) + around(model, 1)
        for px in sorted(set(prices)):
            for qty in (1, MAX - 1, MAX):
                q += [(0, kd(BUY), px, qty), (0, kd(BUY, tif=TIF_FOK), px, qty), (0, kd(BUY, tif=TIF_IOC), px - 1, qty)]
        return q

    return Case(f"wide{L}", S, L, base, [b0, b1], queries, window=_win(base, L, (0, 1)), max_resting=4096)


def fok(L):
    """tests/big_qty.fok_case: behind every batch, the records of the next one (FOKs of INT32_MAX one lot short
    and exactly covered, across 2^31 and 2^32 and into far levels) and the boundaries around the book."""
    c = big_qty.fok_case(L)
    nxt = c.batches[1:] + [c.batches[-1]]

    def queries(model, k):
        a = nxt[k]
        q = [(int(a.symbol[i]), int(a.kind[i]), int(a.price_q4[i]), int(a.qty[i])) for i in range(len(a)) if not int(a.kind[i]) & 8]
        return q + around(model, 0)

    return Case(f"fok{L}", c.S, L, c.base, c.batches, queries, max_resting=4096)


EDGE_CASES = ("clamps_min", "clamps_top", "aliases_min", "aliases_top", "window_edges_max_clamped", "adjacent_far_zero",
              "recentre_up_m31")


def edges(L, name):
    """A script of tests/price_edges (windows at INT64_MIN and at the top base, orders at both ends of int64);
    behind every batch the boundaries around symbol 0's book and LIMITs at the int64 extremes on both sides."""
    c = price_edges.script_cases(L)[name]()

    def queries(model, k):
        q = around(model, 0, 8)
        for side in (BUY, SELL):
            for px in price_edges.EXTREMES:
                for tif in (TIF_GTC, TIF_IOC, TIF_FOK, TIF_POST_ONLY):
                    q += [(0, kd(side, tif=tif), px, 1), (0, kd(side, tif=tif), px, 6)]
                q.append((0, kd(side), px, MAX))
            q.append((0, kd(side, True), 0, MAX))
        return q

    return Case(f"{name}{L}", c.S, L, c.base, c.batches, queries)


def mixed(L):
    """Every side x type x tif, good and bad quantities and symbols, on one two-sided book."""
    S = 2
    base = tm.base_prices(S, L)
    mid = int(base[0]) + L // 2
    sc = Script()
    for px, q in ((mid - 1, 10), (mid - 1, 5), (mid - 3, 7)):
        sc.new(0, BUY, px, q)
    for px, q in ((mid + 1, 6), (mid + 1, 4), (mid + 2, 9)):
        sc.new(0, SELL, px, q)
    sc.new(1, BUY, int(base[1]) + 3, 5)
    q, n = [], 0
    for side in range(4):
        for market in (False, True):
            for tif in range(4):
                for px in (mid - 3, mid - 1, mid, mid + 1, mid + 2):
                    for qty in (0, -1, 5, 12, 1000):
                        n += 1
                        q.append((0, kd(side, market, tif, n % 4 if n % 5 == 0 else 0), px, qty))
    for s in (S, S + 7, 0xFFFFFFFF):
        q += [(s, kd(BUY), mid, 5), (s, kd(0, True, TIF_POST_ONLY), mid, 0), (s, kd(SELL, tif=TIF_FOK), mid, -3)]
    return Case(f"mixed{L}", S, L, base, [sc.take()], lambda model, k: q, window=_win(base, L, (0, 1)))


def seeded(L, seed=0, per=192):
    """One tif_stream draw (books of a hundred orders or more, some far levels) and 64 random queries behind every
    batch: sides, types, tifs, prices near and far, quantities from one lot to a sweep, a few bad records."""
    S, nb = 4, 4
    base, arrays = tm.tif_stream(52_000 + L + seed, S, L, nb, per, far_pct=4, skew=True, mix=(70, 4, 3, 6, 5, 12), spread=5)

    def queries(model, k):
        rng = np.random.default_rng(1000 * L + 10 * seed + k)
        q = []
        for _ in range(64):
            s = int(rng.integers(S + 1)) if rng.random() < 0.03 else int(rng.integers(S))
            side = int(rng.integers(4)) if rng.random() < 0.04 else int(rng.integers(1, 3))
            market, tif = rng.random() < 0.2, int(rng.integers(4))
            mid = int(base[min(s, S - 1)]) + L // 2
            px = mid + int(rng.integers(-8, 9))
            u = rng.random()
            if u < 0.2:
                px = mid + int(rng.choice((-1, 1))) * int(rng.integers(L, 9 * L))
            elif u < 0.25:
                px = int(rng.choice(price_edges.EXTREMES))
            qty = int(rng.choice((1, int(rng.integers(1, 60)), int(rng.integers(60, 600)), int(rng.integers(600, 20000)), MAX)))
            if rng.random() < 0.03:
                qty = int(rng.choice((0, -4)))
            q.append((s, kd(side, market, tif, int(rng.integers(4)) if rng.random() < 0.1 else 0), px, qty))
        return q

    return Case(f"seeded{L}_{seed}_{per}", S, L, base, arrays, queries)


def scripted(L):
    """Every directed case at window depth L."""
    return [chunks(L), window_order(L), far(L), wide(L), fok(L), mixed(L)] + [edges(L, n) for n in EDGE_CASES]
