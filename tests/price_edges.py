"""Streams and scripts with prices at the ends of int64 and on the window's boundaries — TEST INFRASTRUCTURE ONLY.

A record's price is a wire int64: every value is legal. The engine keeps that promise through a per-symbol window
[base, base + L), far levels outside it, recentre_base and a hand-written in-window test `(u64)price - (u64)base
< L` ("price range"); this module builds the inputs that reach those places:

  edge_stream   a seeded stream with tif_stream's kinds (about 60 % of its cancels REDUCEs, as reduce_stream's)
                whose symbols start at the ends of int64, across 0, +-2^31 and 2^32, and whose prices are drawn
                around a mid that jumps between such places: alias draws (mid +- k * 2^n + jitter), the four
                extreme prices, bad records at those prices.
  coverage      counters, from the model and the draws alone, of the events the GPU tests rely on the stream to
                contain (tests/test_price_edges_model.py asserts the floors).
  window_edges, adjacent_far, recentres, clamps, aliases
                the directed cases as record scripts with their fills and final books written out by hand, shared
                by the model test (which pins the model to them) and the GPU test.
  Mod32Book, SentinelBook   two deliberately wrong models: the inputs must tell them from the right one.

As in reduce_stream a ReduceBook beside the draws decides only the draws (a REDUCE's d), never what an engine is
checked against. Prices are Python ints throughout.
"""
from __future__ import annotations

import functools

import numpy as np

from tests.big_qty import Case, Script
from tests.reduce_model import ReduceBook, _draw_d, check_seq_rule, is_reduce, reduce_kind
from tests.tif_model import TIF_FOK, TIF_GTC, TIF_IOC, TIF_POST_ONLY, Arrays, kind

BUY, SELL = 1, 2
ST_NEW, ST_PARTIAL, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
RJ_NONE, RJ_BAD_QTY, RJ_BAD_SIDE, RJ_BAD_SEQ, RJ_WOULD_CROSS = 0, 1, 2, 6, 8
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
EXTREMES = (I64_MIN, I64_MIN + 1, I64_MAX - 1, I64_MAX)
ALIAS_N = (15, 16, 31, 32, 48, 62)


def clip(p):
    return max(I64_MIN, min(I64_MAX, p))


def top_base(L):
    """The highest window base: base + L - 1 is INT64_MAX."""
    return I64_MAX - L + 1


def anchors(L):
    return (I64_MIN, top_base(L), I64_MAX, -(L // 2), (1 << 32) - L // 2, -(1 << 31) - L // 2, 1_000_000, 1 << 62)


def bases(S, L):
    """Symbol s starts at anchor s % 8 (the engine must clamp the third one to top_base)."""
    return np.array([anchors(L)[s % 8] for s in range(S)], dtype=np.int64)


# ---- the stream ----------------------------------------------------------------------------------------------------

NORMAL, ALIAS, EXTREME = 0, 1, 2  # how a record's price was drawn (Draw.tags)


class Draw:
    """What edge_stream drew besides the records: per batch and record how its price was drawn, and the jumps."""

    def __init__(self):
        self.tags, self.jumps = [], 0


def edge_stream(seed, S, L, nbatches, batch, *, spread=12, max_qty=60, bad_pct=1, special_bad_pct=20,
                mix=(30, 18, 9, 9, 12, 22), convert_pct=60, alias_pct=6.0, extreme_pct=3.0, jump_pct=0.4,
                skew=False, market_tifs=(0, 0, 0, 1, 2, 2, 3), draw=None):
    """(base, batches). mix: % GTC LIMIT, IOC, FOK, POST_ONLY, MARKET, cancel; convert_pct % of the cancels are
    REDUCEs with d drawn around the target's remaining quantity. A LIMIT's price is drawn around its symbol's
    mid (a Python int, clipped to int64):

      mostly        mid +- spread;
      alias_pct %   mid +- k * 2^n + jitter, n of ALIAS_N, k of (1, 2), |jitter| <= spread; 70 % on the passive
                    side (they rest as far levels), the others aggressive (they sweep far levels and their rest
                    forces a re-centre);
      extreme_pct % one of EXTREMES, 65 % on the passive side (they rest at the end of int64 and stay), the
                    others aggressive (they take whatever rests, the other extreme included);
      jump_pct %    of the records move their symbol's mid first: to INT64_MIN + L/2, INT64_MAX - L/2, 0 or
                    mid +- 2^33; the symbol's next 12 records are GTC LIMITs around the new mid (they cross
                    what stands in the way and rest there).

    bad_pct % of the NEW records (special_bad_pct % of those with an alias or extreme price) have a bad qty or
    side; the very first record may have seq 0. skew: half of the records are symbol 0's. draw: a Draw to fill."""
    rng = np.random.default_rng(seed * 15485863 + 29)
    base = bases(S, L)
    mid = [clip(min(int(b), top_base(L)) + L // 2) for b in base]
    burst = [0] * S
    book = ReduceBook(S)
    issued = [[] for _ in range(S)]
    cum = np.cumsum(mix)
    assert cum[-1] == 100
    seq = 1
    out = []
    draw = draw if draw is not None else Draw()
    for _ in range(nbatches):
        recs, tags = [], []
        while len(recs) < batch:
            s = 0 if (skew and rng.random() < 0.5) else int(rng.integers(S))
            if rng.random() * 100 < jump_pct:
                w = int(rng.integers(5))
                mid[s] = clip((I64_MIN + L // 2, I64_MAX - L // 2, 0, mid[s] + (1 << 33), mid[s] - (1 << 33))[w])
                burst[s] = 12
                draw.jumps += 1
            m = mid[s]
            u = int(rng.integers(100))
            if burst[s]:
                burst[s] -= 1
                u = 0
            side = BUY if rng.random() < 0.5 else SELL
            sg = -1 if side == BUY else 1  # the passive direction
            q = int(rng.integers(1, max_qty + 1))
            tag = NORMAL
            v = rng.random() * 100
            if v < alias_pct:
                n, k = int(rng.choice(ALIAS_N)), 1 + int(rng.integers(2))
                d = sg if rng.random() < 0.7 else -sg
                p = clip(m + d * (k << n) + int(rng.integers(-spread, spread + 1)))
                tag = ALIAS
            elif v < alias_pct + extreme_pct:
                far_side = side if rng.random() < 0.65 else 3 - side  # BUY: the bottom pair is the passive one
                p = EXTREMES[(0 if far_side == BUY else 2) + int(rng.integers(2))]
                tag = EXTREME
            else:
                p = clip(m + int(rng.integers(-spread, spread + 1)))
            if u >= cum[4] and issued[s] and seq > 1:  # cancel or REDUCE: repeats the last seq
                lst = issued[s]
                if rng.random() < 0.9:
                    tgt = lst[-1 - int(rng.integers(min(len(lst), 60)))] if rng.random() < 0.7 else \
                        lst[int(rng.integers(len(lst)))]
                else:
                    tgt = seq + 1000
                if rng.integers(100) < convert_pct:
                    hit = book.live.get(tgt)
                    left = hit[3][1] if hit is not None and hit[0] == s else None
                    rec = (seq - 1, tgt, _draw_d(rng, left, max_qty), s, reduce_kind(rng))
                else:
                    rec = (seq - 1, tgt, 0, s, kind(BUY, 0, 1, int(rng.integers(4))))
                tag = NORMAL
            else:
                if u >= cum[4]:
                    u = 0
                if u < cum[0]:
                    kd = kind(side, 0, 0, TIF_GTC)
                elif u < cum[1]:
                    kd = kind(side, 0, 0, TIF_IOC)
                elif u < cum[2]:
                    kd = kind(side, 0, 0, TIF_FOK)
                    q = int(rng.integers(1, 3 * max_qty))
                elif u < cum[3]:
                    kd = kind(side, 0, 0, TIF_POST_ONLY)
                    if tag == NORMAL:
                        p = clip(p + 2 * sg)  # mostly passive
                else:
                    kd = kind(side, 1, 0, int(rng.choice(market_tifs)))
                    p, tag = 0, NORMAL
                    q = int(rng.integers(1, 2 * max_qty))
                this = seq
                if rng.integers(100) < (special_bad_pct if tag != NORMAL else bad_pct):
                    w = int(rng.integers(5))
                    if w < 2:
                        q = (0, -5)[w]
                    elif w < 4:
                        kd = (kd & ~3) | (0, 3)[w - 2]
                    elif seq == 1:
                        this = 0  # seq 0 only where it keeps the stream ascending
                if this:
                    seq += 1
                if not (kd & 4) and (kd >> 4) & 3 in (TIF_GTC, TIF_POST_ONLY) and this:
                    issued[s].append(this)
                if rng.random() < 0.05:
                    kd |= int(rng.integers(4)) << 6  # bits 6-7: ignored
                rec = (this, p, q, s, kd)
            book.submit(Arrays(*[[x] for x in rec]))
            recs.append(rec)
            tags.append(tag)
        out.append(Arrays(*[[x[i] for x in recs] for i in range(5)]))
        draw.tags.append(np.array(tags, dtype=np.uint8))
    check_seq_rule(out)
    return base, out


def coverage(base, arrays, levels, draw):
    """Counters from the model and the draws alone:
      fills_extreme    fills at one of EXTREMES
      fills_exact      fills at INT64_MIN or INT64_MAX themselves
      rest_extreme     orders resting at INT64_MIN or INT64_MAX after the last record
      span63           symbols whose final book spans 2^63 or more (highest minus lowest resting price)
      jumps            moves of a symbol's mid
      alias_rest       records with an alias price that rested
      special_rejects  records with an alias or extreme price rejected for a bad qty, side or seq
      reduce_share     REDUCEs / records
      reduces_partial  executed partial REDUCEs
      neg_fills, fills   fills at a negative price, all fills
      far_fills        fills at a price outside the symbol's initial window
    """
    S = len(base)
    b0 = [min(int(b), top_base(levels)) for b in base]
    model = ReduceBook(S)
    c = dict(fills_extreme=0, fills_exact=0, rest_extreme=0, span63=0, jumps=draw.jumps, alias_rest=0, special_rejects=0,
             reduce_share=0.0, reduces_partial=0, neg_fills=0, fills=0, far_fills=0)
    nred = ntot = 0
    for a, tags in zip(arrays, draw.tags):
        res, fills = model.submit(a)
        px = [int(x) for x in fills["price_q4"]]
        c["fills"] += len(px)
        c["fills_extreme"] += sum(p in EXTREMES for p in px)
        c["fills_exact"] += sum(p in (I64_MIN, I64_MAX) for p in px)
        c["neg_fills"] += sum(p < 0 for p in px)
        c["far_fills"] += sum(not (b0[int(s)] <= p < b0[int(s)] + levels) for p, s in zip(px, fills["symbol"]))
        red = is_reduce(a.kind)
        nred += int(red.sum())
        ntot += len(a)
        c["reduces_partial"] += int((red & (res["status"] == ST_NEW)).sum())
        new = (a.kind & 8) == 0
        rested = new & ((res["status"] == ST_NEW) | (res["status"] == ST_PARTIAL)) & (((a.kind >> 4) & 3) != TIF_IOC)
        c["alias_rest"] += int((rested & (tags == ALIAS)).sum())
        bad = (res["status"] == ST_REJECTED) & np.isin(res["reason"], (RJ_BAD_QTY, RJ_BAD_SIDE, RJ_BAD_SEQ))
        c["special_rejects"] += int((new & bad & (tags != NORMAL)).sum())
    c["reduce_share"] = nred / ntot
    for s in range(S):
        d = model.dump(s)
        if len(d):
            p = [int(x) for x in d["price_q4"]]
            c["span63"] += max(p) - min(p) >= 1 << 63
            c["rest_extreme"] += sum(x in (I64_MIN, I64_MAX) for x in p)
    return c


def forced_moves(base, levels, model):
    """{symbol: least distance} for the symbols whose book cannot lie around their initial window (invariant I:
    every bid below base + L, every ask at or above base): the engine's base must have moved at least that far."""
    out = {}
    for s in range(len(base)):
        b0 = min(int(base[s]), top_base(levels))
        bb, ba = model.side[s][0].best(), model.side[s][1].best()
        if bb is not None and bb >= b0 + levels:
            out[s] = bb - (b0 + levels) + 1
        elif ba is not None and ba < b0:
            out[s] = b0 - ba
    return out


# ---- the streams the GPU tests run (tests/test_price_edges_model.py asserts their floors) --------------------------

S_EDGE = 8
DRAWS = (0, 1)
# name: (levels, batches, records per batch, skew, seeds of the two draws)
STREAMS = {
    "l128": (128, 6, 600, False, (2, 4)),
    "l128_dev": (128, 8, 1200, False, (10, 14)),  # one device-batch launch group of eight
    "l256": (256, 6, 600, False, (1, 19)),
    "l1024": (1024, 6, 600, False, (16, 15)),
    "l1024_hot": (1024, 6, 600, True, (3, 9)),
    "l2048_hot": (2048, 6, 600, True, (7, 22)),
}
PATH_STREAM = {"reg": "l128", "gwalk": "l128", "gwalk_cx": "l128", "deep256": "l256", "deep": "l1024",
               "hot_agg": "l1024_hot", "hot": "l2048_hot"}


@functools.lru_cache(maxsize=None)
def stream(name, d):
    """(base, batches, [(results, fills)] of the model, the model after the last batch, the Draw). Shared: nobody
    changes the arrays or steps the model."""
    L, nb, n, skew, seeds = STREAMS[name]
    draw = Draw()
    base, arrays = edge_stream(seeds[d], S_EDGE, L, nb, n, skew=skew, draw=draw)
    model = ReduceBook(S_EDGE)
    exp = [model.submit(a) for a in arrays]
    return base, arrays, exp, model, draw


# ---- two wrong models ------------------------------------------------------------------------------------------------

def _narrow_gt(a, b):
    """a > b as code would decide it that narrows the difference to 32 bits first."""
    d = (a - b) & 0xFFFFFFFF
    return 0 < d < 1 << 31


class _ByLevel(ReduceBook):
    """ReduceBook with the taker's loop split in two: `_crosses` decides, `_level` takes one level."""

    def _crosses(self, p, px, side):
        raise NotImplementedError

    def _take(self, opp, side, anyprice, px, seq, s, rem, tape):
        while rem > 0:
            p = opp.best()
            if p is None or not self._crosses(p, None if anyprice else px, side):
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


class Mod32Book(_ByLevel):
    """Wrong on purpose: a taker's limit is compared with the best opposite price modulo 2^32."""

    def _crosses(self, p, px, side):
        return px is None or not (_narrow_gt(p, px) if side == BUY else _narrow_gt(px, p))


class SentinelBook(_ByLevel):
    """Wrong on purpose: a best price of INT64_MAX or INT64_MIN reads as "this side is empty"."""

    def _crosses(self, p, px, side):
        if p in (I64_MIN, I64_MAX):
            return False
        return px is None or not (p > px if side == BUY else p < px)


def differs(model_cls, S, arrays, exp):
    """Does model_cls give other results or tapes than `exp` (the right model's) on these batches?"""
    m = model_cls(S)
    for a, (ro, fo) in zip(arrays, exp):
        r, f = m.submit(a)
        if r.tobytes() != ro.tobytes() or f.tobytes() != fo.tobytes():
            return True
    return False


# ---- the directed cases ------------------------------------------------------------------------------------------------
# A Case holds the batches of symbol 0's script (symbol 1 only holds one bid), `want`: per batch the fills as
# (taker, maker, price, qty), `rest`: symbol 0's final book as (seq, price, qty, side) in dump order, `status`:
# {(batch, index): (status, reason, filled, remaining)} of the records worth naming, and `bases`: per batch the
# window base of symbol 0 the engine must show after it (None: not pinned). All written out by hand.
# Every batch carries NOISE + NOISE in-window IOCs of symbol 0 that fill nothing, so that the hot paths take it.

NOISE = 35
OTHER = 1_000_000  # symbol 1's base


class _Sc(Script):
    """Script plus the expectations gathered while it is written."""

    def __init__(self):
        super().__init__()
        self.batches, self.want, self.status, self.bases = [], [], {}, []
        self.fills = []

    def noise(self, side, px, n=NOISE):
        for _ in range(n):
            self.new(0, side, px, 1, tif=TIF_IOC)

    def expect(self, st, reason, filled, remaining):
        """of the record just appended"""
        self.status[(len(self.batches), len(self.r) - 1)] = (st, reason, filled, remaining)

    def fill(self, taker, maker, price, qty):
        self.fills.append((taker, maker, price, qty))

    def end(self, base=None):
        self.batches.append(self.take())
        self.want.append(self.fills)
        self.fills = []
        self.bases.append(base)

    def case(self, L, b0, rest, **info):
        check_seq_rule(self.batches)
        return Case(2, L, np.array([b0, OTHER], dtype=np.int64), self.batches, want=self.want, rest=rest,
                    status=self.status, bases=self.bases, **info)


def edge_levels(L):
    return sorted({l for l in (0, 1, 62, 63, 64, 65, L - 2, L - 1) if 0 <= l < L})


def window_edges(L, b0):
    """Window [b0, b0 + L) (b0 may be INT64_MAX: the engine clamps it). Bids, then crossing sells, at the edge
    and occupancy-word levels; an ask at level 0 and a bid at level L - 1; MARKETs sweeping the occupied edge and
    word-boundary levels from one end to the other in both directions. Nothing rests outside the window: the
    base stays where it is."""
    w0 = min(b0, top_base(L))
    lv = edge_levels(L)
    P = lambda l: w0 + l  # noqa: E731
    nz = P(30)
    assert 30 not in lv
    sc = _Sc()
    sc.new(1, BUY, OTHER + 1, 5)
    sc.noise(BUY, nz)
    B = {l: sc.new(0, BUY, P(l), 10 + i) for i, l in enumerate(lv)}
    sc.noise(BUY, nz)
    sc.end(w0)
    sc.noise(BUY, nz)
    for i, l in reversed(list(enumerate(lv))):
        t = sc.new(0, SELL, P(l), 10 + i)
        sc.expect(ST_FILLED, RJ_NONE, 10 + i, 0)
        sc.fill(t, B[l], P(l), 10 + i)
    sc.noise(BUY, nz)
    sc.end(w0)
    sc.noise(SELL, nz)
    a0 = sc.new(0, SELL, P(0), 7)
    sc.noise(SELL, nz, 3)
    t = sc.new(0, BUY, P(0), 2, tif=TIF_IOC)
    sc.fill(t, a0, P(0), 2)
    sc.cancel(0, a0)
    sc.expect(ST_CANCELED, RJ_NONE, 0, 5)
    bl = sc.new(0, BUY, P(L - 1), 9)
    sc.noise(BUY, nz, 3)
    t = sc.new(0, SELL, P(L - 1), 4, tif=TIF_IOC)
    sc.fill(t, bl, P(L - 1), 4)
    sc.cancel(0, bl)
    sc.expect(ST_CANCELED, RJ_NONE, 0, 5)
    sc.noise(BUY, nz)
    sc.end(w0)
    sc.noise(SELL, nz)
    A = {l: sc.new(0, SELL, P(l), 1 + i) for i, l in enumerate(lv)}
    sc.noise(SELL, nz, 3)
    total = sum(1 + i for i in range(len(lv)))
    t = sc.new(0, BUY, 0, total, market=True)
    sc.expect(ST_FILLED, RJ_NONE, total, 0)
    for i, l in enumerate(lv):
        sc.fill(t, A[l], P(l), 1 + i)
    sc.noise(BUY, nz, 3)
    C = {l: sc.new(0, BUY, P(l), 1 + i) for i, l in enumerate(lv)}
    sc.noise(BUY, nz, 3)
    t = sc.new(0, SELL, 0, total + 5, market=True)
    sc.expect(ST_CANCELED, RJ_NONE, total, 5)
    for i, l in reversed(list(enumerate(lv))):
        sc.fill(t, C[l], P(l), 1 + i)
    sc.noise(SELL, nz)
    sc.end(w0)
    return sc.case(L, b0, [], levels_used=lv)


def adjacent_far(L, b0):
    """A bid at base - 1 and an ask at base + L (far levels next to the window; neither forces a re-centre, and
    the window holds an order whenever one of them rests): sweeps from the window into each, a REDUCE and a cancel
    on each, a FOK one lot short and a FOK exactly filled across each boundary, a POST_ONLY that would cross only
    the adjacent far level. The base stays where it is."""
    assert b0 - 1 >= I64_MIN and b0 + L <= I64_MAX
    h = L // 2
    P = lambda l: b0 + l  # noqa: E731
    nz = P(h)
    sc = _Sc()
    sc.new(1, BUY, OTHER + 1, 5)
    sc.noise(BUY, nz)
    wb, wa = sc.new(0, BUY, P(h - 2), 5), sc.new(0, SELL, P(h + 2), 5)
    fb1, fb2 = sc.new(0, BUY, P(-1), 8), sc.new(0, BUY, P(-1), 6)
    fa1, fa2 = sc.new(0, SELL, P(L), 8), sc.new(0, SELL, P(L), 6)
    sc.noise(BUY, nz)
    sc.end(b0)
    sc.noise(BUY, nz)
    t = sc.new(0, SELL, P(-1), 8)
    sc.expect(ST_FILLED, RJ_NONE, 8, 0)
    sc.fill(t, wb, P(h - 2), 5)
    sc.fill(t, fb1, P(-1), 3)
    t = sc.new(0, BUY, P(L), 8)
    sc.expect(ST_FILLED, RJ_NONE, 8, 0)
    sc.fill(t, wa, P(h + 2), 5)
    sc.fill(t, fa1, P(L), 3)
    sc.reduce(0, fb1, 2)
    sc.expect(ST_NEW, RJ_NONE, 0, 3)
    sc.reduce(0, fa1, 2)
    sc.expect(ST_NEW, RJ_NONE, 0, 3)
    sc.cancel(0, fb2)
    sc.expect(ST_CANCELED, RJ_NONE, 0, 6)
    sc.cancel(0, fa2)
    sc.expect(ST_CANCELED, RJ_NONE, 0, 6)
    sc.noise(BUY, nz)
    sc.end(b0)
    sc.noise(BUY, nz)
    wa2 = sc.new(0, SELL, P(L - 1), 4)
    sc.new(0, BUY, P(L), 8, tif=TIF_FOK)  # 4 + 3 within the limit: one lot short
    sc.expect(ST_CANCELED, RJ_NONE, 0, 8)
    t = sc.new(0, BUY, P(L), 7, tif=TIF_FOK)
    sc.expect(ST_FILLED, RJ_NONE, 7, 0)
    sc.fill(t, wa2, P(L - 1), 4)
    sc.fill(t, fa1, P(L), 3)
    wb2 = sc.new(0, BUY, P(0), 4)
    sc.new(0, SELL, P(-1), 8, tif=TIF_FOK)
    sc.expect(ST_CANCELED, RJ_NONE, 0, 8)
    t = sc.new(0, SELL, P(-1), 7, tif=TIF_FOK)
    sc.expect(ST_FILLED, RJ_NONE, 7, 0)
    sc.fill(t, wb2, P(0), 4)
    sc.fill(t, fb1, P(-1), 3)
    sc.noise(BUY, nz)
    sc.end(b0)
    sc.noise(BUY, nz)
    wb3 = sc.new(0, BUY, P(h - 2), 5)
    fa3 = sc.new(0, SELL, P(L), 2)
    sc.new(0, BUY, P(L), 1, tif=TIF_POST_ONLY)  # the window holds no ask: it would cross fa3 alone
    sc.expect(ST_REJECTED, RJ_WOULD_CROSS, 0, 1)
    wa3 = sc.new(0, SELL, P(h + 2), 5)
    sc.cancel(0, wb3)
    sc.expect(ST_CANCELED, RJ_NONE, 0, 5)
    fb3 = sc.new(0, BUY, P(-1), 2)
    sc.new(0, SELL, P(-1), 1, tif=TIF_POST_ONLY)  # the window holds no bid: it would cross fb3 alone
    sc.expect(ST_REJECTED, RJ_WOULD_CROSS, 0, 1)
    sc.new(0, BUY, P(L - 1), 1, tif=TIF_POST_ONLY)  # one tick below fa3, above wa3: it would cross wa3
    sc.expect(ST_REJECTED, RJ_WOULD_CROSS, 0, 1)
    p4 = sc.new(0, BUY, P(h), 1, tif=TIF_POST_ONLY)
    sc.expect(ST_NEW, RJ_NONE, 0, 1)
    sc.noise(BUY, nz)
    sc.end(b0)
    rest = [(p4, P(h), 1, BUY), (fb3, P(-1), 2, BUY), (wa3, P(h + 2), 5, SELL), (fa3, P(L), 2, SELL)]
    return sc.case(L, b0, rest)


def recentres(L, b0, up):
    """A mandatory re-centre by one tick past the edge: an ask that rests at base - 1 (`up` false) or a bid that
    rests at base + L. On its way it takes the order in the middle and the one on the near edge; the order that
    sat on the other old edge leaves the window or stays and still fills last, in price order."""
    assert b0 - 1 - L // 2 >= I64_MIN and b0 + L + L // 2 <= I64_MAX
    h = L // 2
    P = lambda l: b0 + l  # noqa: E731
    nz = P(h)
    sc = _Sc()
    sc.new(1, BUY, OTHER + 1, 5)
    sc.noise(BUY, nz)
    e0, e1 = sc.new(0, BUY, P(0), 5), sc.new(0, SELL, P(L - 1), 5)
    wb, wa = sc.new(0, BUY, P(h - 2), 5), sc.new(0, SELL, P(h + 2), 5)
    sc.noise(BUY, nz)
    sc.end(b0)
    sc.noise(BUY, nz)
    if up:
        r1 = sc.new(0, BUY, P(L), 12)
        sc.expect(ST_PARTIAL, RJ_NONE, 10, 2)
        sc.fill(r1, wa, P(h + 2), 5)
        sc.fill(r1, e1, P(L - 1), 5)
        sc.noise(BUY, nz)  # (no ask is left)
        sc.end(b0 + h)  # recentre_base: target - L/2 = b0 + L - L/2; the best bid wb allows it
        sc.noise(BUY, nz)
        t = sc.new(0, SELL, 0, 12, market=True)
        sc.expect(ST_FILLED, RJ_NONE, 12, 0)
        sc.fill(t, r1, P(L), 2)
        sc.fill(t, wb, P(h - 2), 5)
        sc.fill(t, e0, P(0), 5)
    else:
        r1 = sc.new(0, SELL, P(-1), 12)
        sc.expect(ST_PARTIAL, RJ_NONE, 10, 2)
        sc.fill(r1, wb, P(h - 2), 5)
        sc.fill(r1, e0, P(0), 5)
        sc.noise(SELL, nz)  # (no bid is left)
        sc.end(b0 - 1 - h)
        sc.noise(SELL, nz)
        t = sc.new(0, BUY, 0, 12, market=True)
        sc.expect(ST_FILLED, RJ_NONE, 12, 0)
        sc.fill(t, r1, P(-1), 2)
        sc.fill(t, wa, P(h + 2), 5)
        sc.fill(t, e1, P(L - 1), 5)
    sc.noise(SELL if not up else BUY, nz)
    sc.end(None)
    return sc.case(L, b0, [])


def clamps(L, b0):
    """On a symbol whose window starts at INT64_MIN or at the top base: a bid rests at INT64_MAX and is taken by
    a LIMIT and a MARKET; an ask rests at INT64_MIN (the window goes from one end of int64 to the other) and is
    taken likewise; then an order rests at each extreme while the market sits at the other end: the book spans
    2^64 - 1, a MARKET sweeps from one end to the other, FOKs count across it."""
    lo, hi = I64_MIN, top_base(L)
    assert b0 in (lo, hi)
    nz = b0 + L // 2
    sc = _Sc()
    sc.new(1, BUY, OTHER + 1, 5)
    sc.noise(BUY, nz)
    x = sc.new(0, BUY, I64_MAX, 9)
    sc.expect(ST_NEW, RJ_NONE, 0, 9)
    sc.noise(BUY, nz, 3)
    t = sc.new(0, SELL, I64_MAX, 4)
    sc.expect(ST_FILLED, RJ_NONE, 4, 0)
    sc.fill(t, x, I64_MAX, 4)
    t = sc.new(0, SELL, 0, 3, market=True)
    sc.fill(t, x, I64_MAX, 3)
    sc.cancel(0, x)
    sc.expect(ST_CANCELED, RJ_NONE, 0, 2)
    sc.noise(BUY, nz)
    sc.end(hi)
    sc.noise(SELL, nz)
    y = sc.new(0, SELL, I64_MIN, 9)
    sc.expect(ST_NEW, RJ_NONE, 0, 9)
    sc.noise(SELL, nz, 3)
    t = sc.new(0, BUY, I64_MIN, 4)
    sc.expect(ST_FILLED, RJ_NONE, 4, 0)
    sc.fill(t, y, I64_MIN, 4)
    t = sc.new(0, BUY, 0, 3, market=True)
    sc.fill(t, y, I64_MIN, 3)
    sc.reduce(0, y, 1)
    sc.expect(ST_NEW, RJ_NONE, 0, 1)
    sc.cancel(0, y)
    sc.expect(ST_CANCELED, RJ_NONE, 0, 1)
    sc.noise(SELL, nz)
    sc.end(lo)
    sc.noise(BUY, nz)
    z1 = sc.new(0, BUY, I64_MIN, 5)
    z2 = sc.new(0, SELL, I64_MAX, 5)  # a far ask 2^64 - 1 above the base
    sc.noise(BUY, nz, 3)
    z3 = sc.new(0, BUY, I64_MAX - 5, 3)  # the market moves to the top; z1 is now a far bid
    sc.expect(ST_NEW, RJ_NONE, 0, 3)
    sc.noise(BUY, nz, 3)
    t = sc.new(0, SELL, I64_MAX - 5, 1, tif=TIF_IOC)
    sc.fill(t, z3, I64_MAX - 5, 1)
    t = sc.new(0, BUY, 0, 2, market=True)
    sc.fill(t, z2, I64_MAX, 2)
    t = sc.new(0, SELL, 0, 4, market=True)
    sc.expect(ST_FILLED, RJ_NONE, 4, 0)
    sc.fill(t, z3, I64_MAX - 5, 2)
    sc.fill(t, z1, I64_MIN, 2)
    sc.noise(BUY, nz)
    sc.end(hi)
    sc.noise(SELL, nz)
    z4 = sc.new(0, SELL, I64_MIN + 5, 3)  # the market moves to the bottom; z2 is a far ask again
    sc.expect(ST_NEW, RJ_NONE, 0, 3)
    sc.noise(SELL, nz, 3)
    t = sc.new(0, BUY, I64_MIN + 5, 1, tif=TIF_IOC)
    sc.fill(t, z4, I64_MIN + 5, 1)
    sc.new(0, BUY, I64_MAX, 6, tif=TIF_FOK)  # 2 + 3 in the whole book
    sc.expect(ST_CANCELED, RJ_NONE, 0, 6)
    t = sc.new(0, BUY, I64_MAX, 5, tif=TIF_FOK)
    sc.expect(ST_FILLED, RJ_NONE, 5, 0)
    sc.fill(t, z4, I64_MIN + 5, 2)
    sc.fill(t, z2, I64_MAX, 3)
    sc.new(0, SELL, I64_MIN, 1, tif=TIF_POST_ONLY)
    sc.expect(ST_REJECTED, RJ_WOULD_CROSS, 0, 1)
    sc.noise(SELL, nz)
    sc.end(lo)
    return sc.case(L, b0, [(z1, I64_MIN, 3, BUY)])


def aliases(L, b0):
    """With nothing resting at window level l, for every n of ALIAS_N in turn (where those prices exist): an ask
    rests at base + l + 2^n, a buy at base + l fills nothing, a buy at the alias price fills that order. Then the
    same below the window with bids at base + l' - 2^n. An order at INT64_MAX (INT64_MIN) ends each half. The
    window holds an order throughout, so no far rest moves it."""
    w0 = min(b0, top_base(L))
    h = L // 2
    P = lambda l: w0 + l  # noqa: E731
    nz = P(h)
    la, lb = h + 5, h - 8
    do_asks = P(la) + (1 << 62) <= I64_MAX
    do_bids = P(lb) - (1 << 62) >= I64_MIN
    assert do_asks or do_bids
    sc = _Sc()
    sc.new(1, BUY, OTHER + 1, 5)
    sc.noise(BUY, nz)
    wb = sc.new(0, BUY, P(h - 3), 5) if do_asks else None
    wa = None if do_asks else sc.new(0, SELL, P(h + 3), 5)
    sc.noise(BUY, nz)
    sc.end(w0)
    if do_asks:
        sc.noise(BUY, nz)
        for i, n in enumerate(ALIAS_N + (None,)):
            px = I64_MAX if n is None else P(la) + (1 << n)
            q = sc.new(0, SELL, px, 3 + i)
            sc.new(0, BUY, P(la), 50, tif=TIF_IOC)
            sc.expect(ST_CANCELED, RJ_NONE, 0, 50)
            t = sc.new(0, BUY, px, 3 + i, tif=TIF_IOC)
            sc.expect(ST_FILLED, RJ_NONE, 3 + i, 0)
            sc.fill(t, q, px, 3 + i)
        if do_bids:
            wa = sc.new(0, SELL, P(h + 3), 5)
            sc.cancel(0, wb)
            sc.expect(ST_CANCELED, RJ_NONE, 0, 5)
        sc.noise(BUY, nz)
        sc.end(w0)
    if do_bids:
        sc.noise(BUY, nz)
        for i, n in enumerate(ALIAS_N + (None,)):
            px = I64_MIN if n is None else P(lb) - (1 << n)
            q = sc.new(0, BUY, px, 3 + i)
            sc.new(0, SELL, P(lb), 50, tif=TIF_IOC)
            sc.expect(ST_CANCELED, RJ_NONE, 0, 50)
            t = sc.new(0, SELL, px, 3 + i, tif=TIF_IOC)
            sc.expect(ST_FILLED, RJ_NONE, 3 + i, 0)
            sc.fill(t, q, px, 3 + i)
        sc.noise(BUY, nz)
        sc.end(w0)
    rest = [(wa, P(h + 3), 5, SELL)] if do_bids else [(wb, P(h - 3), 5, BUY)]
    return sc.case(L, b0, rest)


def script_cases(L):
    """{name: builder} of every directed case at window size L."""
    lo, hi, h = I64_MIN, top_base(L), L // 2
    out = {}
    for tag, b in (("min", lo), ("top", hi), ("max_clamped", I64_MAX), ("zero", -h), ("plain", 1_000_000)):
        out[f"window_edges_{tag}"] = functools.partial(window_edges, L, b)
    for tag, b in (("zero", -h), ("p32", (1 << 32) - h), ("plain", 1_000_000)):
        out[f"adjacent_far_{tag}"] = functools.partial(adjacent_far, L, b)
    for tag, b in (("zero", -h), ("m31", -(1 << 31) - h), ("p32", (1 << 32) - h)):
        out[f"recentre_up_{tag}"] = functools.partial(recentres, L, b, True)
        out[f"recentre_down_{tag}"] = functools.partial(recentres, L, b, False)
    for tag, b in (("min", lo), ("top", hi)):
        out[f"clamps_{tag}"] = functools.partial(clamps, L, b)
    for tag, b in (("min", lo), ("top", hi), ("zero", -h), ("plain", 1_000_000)):
        out[f"aliases_{tag}"] = functools.partial(aliases, L, b)
    return out


CASE_NAMES = tuple(script_cases(128))
