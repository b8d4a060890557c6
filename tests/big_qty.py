"""Streams and scripts with quantities up to INT32_MAX and book sums past 2^31 — TEST INFRASTRUCTURE ONLY.

A record's qty is a wire int32: everything up to 2^31 - 1 is legal. The kernels hold some quantities in 32 bits
behind bounds ("quantity widths"); this module builds the inputs that reach those bounds:

  big_stream   a seeded stream like reduce_model.reduce_stream's whose quantities come from a mixture up to
               2^31 - 1 and whose symbols are steered, by a ReduceBook kept beside the draws, back and forth
               across a book sum of 2^31 (the ladder walks' LW_CAP) and up past 2^32.
  trace        per symbol and record, the model's book sum before the record.
  coverage     counters, from the model alone, of the events the GPU tests rely on the stream to contain.
  Script, ...  the directed cases (saturating chunk ranking, FOK across 2^31, REDUCE at width) as record
               scripts, shared by the model test (which pins their outcomes) and the GPU test.

As in reduce_stream the model decides only the draws, never what an engine is checked against.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import cancel_targets as ct
from tests.reduce_model import INT32_MAX, KIND_REDUCE, ReduceBook, check_seq_rule, _draw_d
from tests.tif_model import TIF_FOK, TIF_GTC, TIF_IOC, TIF_POST_ONLY, Arrays, base_prices, kind

BUY, SELL = 1, 2
ST_NEW, ST_PARTIAL, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
CAP31, CAP32 = 1 << 31, 1 << 32
LO, HI = CAP31 - (1 << 27), CAP32 + (1 << 28)  # the controller's thresholds on a symbol's book sum
Q28 = 1 << 28
CONSTS = ((1 << 24) - 1, 1 << 24, INT32_MAX - 1, INT32_MAX)
CHUNK = 16  # slots per FIFO chunk (matching_engine_amd._abi.CHUNK_SLOTS)


class Script:
    """Records appended in stream order; a cancel or reduce repeats the last seq."""

    def __init__(self, seq0=1):
        self.next = seq0
        self.r = []

    def new(self, s, side, px, q, market=False, tif=0):
        self.r.append((self.next, px, q, s, kind(side, 1 if market else 0, 0, tif)))
        self.next += 1
        return self.next - 1

    def cancel(self, s, target, q=0):
        self.r.append((max(self.next - 1, 1), ct.to_i64(target), q, s, kind(BUY, 0, 1)))

    def reduce(self, s, target, d, kd=KIND_REDUCE):
        self.r.append((max(self.next - 1, 1), ct.to_i64(target), d, s, kd))
        return len(self.r) - 1

    def take(self):
        a = Arrays(*[[x[i] for x in self.r] for i in range(5)])
        self.r = []
        return a


# ---- the model beside the draws ------------------------------------------------------------------------------------

def _one(book, rec):
    """One record through the model: (result row, fills, change of the symbol's book sum)."""
    res, fills = book.submit(Arrays(*[[x] for x in rec]))
    r = res[0]
    seq, _, q, s, kd = rec
    st = int(r["status"])
    if kd & 8:
        if st == ST_CANCELED:
            return r, fills, -int(r["remaining_qty"])
        if st == ST_NEW and (kd & 4):  # a partial reduce
            return r, fills, -q
        return r, fills, 0
    d = -int(r["filled_qty"])
    hit = book.live.get(seq)
    if st != ST_REJECTED and hit is not None and hit[0] == s:
        d += hit[3][1]
    return r, fills, d


def model_snapshot(book, s, depth):
    """(bids, asks) of a PyBook-family model as the engine's snapshot gives them: price, total, count."""
    from matching_engine_amd import LEVEL_DTYPE

    out = []
    for sd in book.side[s]:
        rows = []
        for k, fifo in sd.levels.items():
            if len(rows) == depth:
                break
            live = [e[1] for e in fifo if e[1] > 0]
            rows.append((-k if sd.bids else k, sum(live), len(live)))
        a = np.zeros(len(rows), dtype=LEVEL_DTYPE)
        for i, (p, t, c) in enumerate(rows):
            a[i]["price_q4"], a[i]["total_qty"], a[i]["order_count"] = p, t, c
        out.append(a)
    return out[0], out[1]


class Snap:
    """A model with the snapshot() method the feed models read."""

    def __init__(self, book):
        self.book = book

    def snapshot(self, s, depth):
        return model_snapshot(self.book, s, depth)


# ---- the stream ----------------------------------------------------------------------------------------------------

def _qty(rng, mode):
    """The mixture: [1, 60], [2^20, 2^26], [2^28, 2^31 - 1] and the constants; `mode` sets the weights: "large",
    "mixed", or "calm" (nothing above 2^26)."""
    u = int(rng.integers(100))
    a, b, c = {"large": (8, 18, 80), "mixed": (35, 60, 85), "calm": (55, 90, 0)}[mode]
    if u < a:
        return int(rng.integers(1, 61))
    if u < b:
        return int(rng.integers(1 << 20, (1 << 26) + 1))
    if u < c:
        return int(rng.integers(Q28, CAP31))
    return int(CONSTS[int(rng.integers(2 if mode == "calm" else len(CONSTS)))])


FILL, DRAIN, CALM = 0, 1, 2


def big_stream(seed, num_symbols, levels, nbatches, batch, *, group, far_pct=0, skew=False):
    """(base, batches): GTC / IOC / FOK / POST_ONLY LIMITs, MARKETs, cancels (their ignored qty field 0, -1 or
    INT32_MAX), reduces (d around the target's remaining quantity) and ~1 % bad records. Every symbol goes
    through phases that follow its own book sum, record by record, so their changes fall anywhere in a batch and
    a launch group (`group` only names the grouping the stream is meant for; coverage() counts against it):

      filling   mostly passive large LIMITs, most of them at one price so that a level passes 2^32, until the
                sum passes HI = 2^32 + 2^28;
      draining  large takers, cancels and reduces of the largest resting orders, until the sum is below
                LO = 2^31 - 2^27;
      calm      60 to 140 of the symbol's records with quantities of at most 2^26, nearly all of kinds the fast
                walks cover (GTC, IOC, MARKET; few cancels), the largest resting orders cancelled first: the book
                falls well below 2^31 and the walks run records of their own against 32-bit totals of up to 2^30.
                Every other time the draining goes on down to 2^29 and the calm phase (100 to 220 records) holds
                only covered kinds: the walks run whole blocks until a block's quantities take the bound to
                2^31 — in a batch's later block or a group's later batch. Then filling again.

    skew: half of the records are symbol 0's."""
    rng = np.random.default_rng(seed * 104729 + 71)
    S, L = num_symbols, levels
    base = base_prices(S, L)
    book = ReduceBook(S)
    sums = [0] * S
    phase = [FILL] * S
    calm_left = [0] * S
    pure = [False] * S
    heavy = [(BUY if rng.random() < 0.5 else SELL, 1 + int(rng.integers(3))) for _ in range(S)]
    rested = [[] for _ in range(S)]
    seq = 1
    out = []
    # per phase: % cancel or reduce, % passive LIMIT (the rest: takers), targets sampled, quantity modes
    MIX = {FILL: (14, 70, 1, "large", "mixed"), DRAIN: (34, 12, 8, "mixed", "large"), CALM: (10, 45, 8, "calm", "calm")}

    def live_targets(s, k):
        """up to k live resting orders of s, as (remaining, seq)"""
        got, lst = [], rested[s]
        for _ in range(min(3 * k, len(lst))):
            if not lst or len(got) == k:
                break
            j = int(rng.integers(len(lst)))
            hit = book.live.get(lst[j])
            if hit is None:
                lst[j] = lst[-1]
                lst.pop()
            else:
                got.append((hit[3][1], lst[j]))
        return got

    for _ in range(nbatches):
        recs = []
        while len(recs) < batch:
            s = 0 if (skew and rng.random() < 0.5) else int(rng.integers(S))
            mid = int(base[s]) + L // 2
            if phase[s] == FILL and sums[s] > HI:
                phase[s] = DRAIN
                pure[s] = rng.random() < 0.5
            elif phase[s] == DRAIN and sums[s] < (1 << 29 if pure[s] else LO):
                phase[s], calm_left[s] = CALM, int(rng.integers(100, 221)) if pure[s] else int(rng.integers(60, 141))
            elif phase[s] == CALM:
                calm_left[s] -= 1
                if calm_left[s] < 0:
                    phase[s] = FILL
                    heavy[s] = (BUY if rng.random() < 0.5 else SELL, 1 + int(rng.integers(3)))
            ph = phase[s]
            pcx, ppass, ntgt, qpass, qtake = MIX[ph]
            calm = ph == CALM
            clean = calm and pure[s]
            if clean:
                pcx = 0
            u = int(rng.integers(100))
            side = BUY if rng.random() < 0.5 else SELL
            sg = -1 if side == BUY else 1
            rec = None
            if seq > 1 and u >= 100 - pcx:  # cancel / reduce
                t = live_targets(s, ntgt)
                red = rng.random() < (0.15 if calm else 0.5)
                if t and rng.random() < 0.9:
                    r, tgt = max(t)
                else:
                    r, tgt = None, (seq + 1000 if rng.random() < 0.5 else max(1, seq - 1 - int(rng.integers(50))))
                    hit = book.live.get(tgt)
                    r = hit[3][1] if hit is not None and hit[0] == s else None
                if red:
                    rec = (seq - 1, tgt, min(_draw_d(rng, r, INT32_MAX), INT32_MAX), s, 0x0C | int(rng.integers(4)))
                else:
                    rec = (seq - 1, tgt, (0, -1, INT32_MAX)[int(rng.integers(3))], s, kind(BUY, 0, 1, int(rng.integers(4))))
            elif u < ppass:  # passive LIMIT
                if ph == FILL and rng.random() < 0.7:
                    side, k = heavy[s]
                    sg = -1 if side == BUY else 1
                else:
                    k = 1 + int(rng.integers(4))
                p = mid + sg * k
                if far_pct and not calm and rng.integers(100) < far_pct:
                    p = mid + sg * int(rng.integers(L, 8 * L))
                tif = TIF_POST_ONLY if rng.random() < (0 if clean else 0.03 if calm else 0.15) else TIF_GTC
                if tif == TIF_POST_ONLY:
                    best = book.side[s][1 if side == BUY else 0].best()
                    if best is not None and (best <= p if side == BUY else best >= p):
                        tif = TIF_GTC
                rec = (seq, p, _qty(rng, qpass), s, kind(side, 0, 0, tif))
            else:  # a taker: MARKET, IOC, FOK or a crossing LIMIT
                q = _qty(rng, qtake)
                w = int(rng.integers(4))
                p = mid - sg * (1 + int(rng.integers(5)))
                if far_pct and not calm and rng.integers(100) < 4 * far_pct:
                    p = mid - sg * 8 * L  # reaches every far level
                if calm and w == 2 and (clean or rng.random() < 0.9):
                    w = 1  # (few FOKs: the walks hand a FOK off)
                if w == 0:
                    rec = (seq, 0, q, s, kind(side, 1, 0, (0, 0, 1, 1 if calm else 2)[int(rng.integers(4))]))
                else:
                    rec = (seq, p, q, s, kind(side, 0, 0, (TIF_IOC, TIF_FOK, TIF_GTC)[w - 1]))
            if not (rec[4] & 8) and rng.integers(100) < 1:  # a bad record
                w = int(rng.integers(4))
                rec = (rec[0], rec[1], (0, -5)[w] if w < 2 else rec[2], rec[3], rec[4] if w < 2 else (rec[4] & ~3) | (0, 3)[w - 2])
            if not (rec[4] & 8):
                seq += 1
            r, _, d = _one(book, rec)
            sums[s] += d
            hit = book.live.get(rec[0])
            if not (rec[4] & 8) and hit is not None and hit[0] == s and int(r["status"]) != ST_REJECTED:
                rested[s].append(rec[0])
            recs.append(rec)
        out.append(Arrays(*[[x[i] for x in recs] for i in range(5)]))
    check_seq_rule(out)
    return base, out


# ---- what a stream contains ----------------------------------------------------------------------------------------

def _walk(batches, S):
    """(k, i, record, result row, fills, sum before, sum after, book) for every record, the model stepping."""
    book = ReduceBook(S)
    sums = [0] * S
    for k, b in enumerate(batches):
        for i in range(len(b)):
            rec = (int(b.seq[i]), int(b.price_q4[i]), int(b.qty[i]), int(b.symbol[i]), int(b.kind[i]))
            s = rec[3]
            before = sums[s] if s < S else 0
            pre = _pre(book, rec) if s < S else None
            r, f, d = _one(book, rec)
            if s < S:
                sums[s] += d
            yield k, i, rec, r, f, before, before + d, book, pre


def _pre(book, rec):
    """What a taker faces, read before it runs: (live quantities of the opposite best level's head chunk run,
    quantity available within its limit, the opposite side's whole quantity)."""
    seq, px, q, s, kd = rec
    side = kd & 3
    if kd & 8 or side not in (BUY, SELL) or q <= 0:
        return None
    opp = book.side[s][1 if side == BUY else 0]
    best = opp.best()
    market = bool(kd & 4)
    if best is None or (not market and (best > px if side == BUY else best < px)):
        return None
    fifo = opp.fifo(best)
    head = next(e for e in fifo if e[1] > 0)
    pos = _POS.get(head[0], 0) % CHUNK
    run, started = [], False
    for e in fifo:
        if e is head:
            started = True
        if started:
            if len(run) == CHUNK - pos:
                break
            run.append(e[1])
    avail = whole = 0
    for k, ff in opp.levels.items():
        p = -k if opp.bids else k
        t = sum(e[1] for e in ff)
        whole += t
        if market or not (p > px if side == BUY else p < px):
            avail += t
    return run, avail, whole


_POS = {}  # seq -> position in its level's FIFO counted from the level's creation (coverage() fills it)


def trace(batches, num_symbols):
    """Per symbol, [(batch, index in the batch, the model's book sum before the record)]."""
    out = [[] for _ in range(num_symbols)]
    for k, i, rec, _, _, before, _, _, _ in _walk(batches, num_symbols):
        if rec[3] < num_symbols:
            out[rec[3]].append((k, i, before))
    return out


def coverage(batches, num_symbols, group, levels=None):
    """Counters from the model alone:
      up, down       per symbol: records that took the symbol's book sum from below 2^31 to 2^31 or more / back
      mid_batch      crossings whose record is not the first of its symbol in its batch
      group_over     (launch group, symbol) pairs: the symbol has records in the group and starts it at >= 2^31
      level_over     rests that left their level's total above 2^32
      sat_chunk      takes whose first level's head chunk run (the live quantities from the head order to the
                     end of its 16-slot chunk, slots counted from the level's creation) sums to >= 2^32
      fok_filled     FOKs that filled with >= 2^31 available within their limit
      fok_killed     FOKs killed (less than qty <= 2^31 - 1 within their limit, so that sum cannot pass 2^31)
                     while the opposite side as a whole held >= 2^31: the running sum over levels is large, the
                     limit cuts it short
      big_reduce     executed reduces with d >= 2^28
      far_big_fill   fills of >= 2^28 (so a maker of at least that) at a price outside the initial window;
                     needs `levels`
      walk_big, walk_big_cx      records with a quantity >= 2^20 that the plain / the cancel grouped walk runs
                     itself, by lw_cases' rule with the model's sum for B: per (launch group, symbol) the records
                     before the first one the walk does not cover (FOK, POST_ONLY, REDUCE, a far price; a cancel
                     on the plain walk) and before the first block that takes the bound to 2^31
      refused_later, refused_later_cx   (launch group, symbol) pairs the bound stopped after the walk ran
                     records of the group: `adm` false in a later block or batch
      rejects, news  REJECTED records among the NEW ones, and the NEW ones
      sum_end        per symbol, the book sum after the last record
    """
    S = num_symbols
    base = base_prices(S, levels) if levels else None
    c = dict(up=[0] * S, down=[0] * S, mid_batch=0, group_over=0, level_over=0, sat_chunk=0, fok_filled=0,
             fok_killed=0, big_reduce=0, far_big_fill=0, rejects=0, news=0, sum_end=[0] * S, walk_big=0, walk_big_cx=0,
             refused_later=0, refused_later_cx=0)
    per = {}  # (group, symbol) -> [sum at its start, {batch: [(qty, kind, far price)]}]
    _POS.clear()
    count = {}  # (s, side, price) -> orders appended since the level was created
    seen_batch, seen_group = set(), set()
    for k, i, rec, r, f, before, after, book, pre in _walk(batches, S):
        seq, px, q, s, kd = rec
        if s >= S:
            if not (kd & 8):
                c["news"] += 1
                c["rejects"] += 1
            continue
        first = (k, s) not in seen_batch
        seen_batch.add((k, s))
        if (k // group, s) not in seen_group:
            seen_group.add((k // group, s))
            c["group_over"] += before >= CAP31
            per[(k // group, s)] = [before, {}]
        far = base is not None and not (kd & 12) and not (int(base[s]) <= px < int(base[s]) + levels)
        per[(k // group, s)][1].setdefault(k, []).append((q, kd, far))
        if before < CAP31 <= after:
            c["up"][s] += 1
            c["mid_batch"] += not first
        elif after < CAP31 <= before:
            c["down"][s] += 1
            c["mid_batch"] += not first
        c["sum_end"][s] = after
        st = int(r["status"])
        if kd & 8:
            if (kd & 4) and st != ST_REJECTED and q >= Q28:
                c["big_reduce"] += 1
            continue
        c["news"] += 1
        c["rejects"] += st == ST_REJECTED
        hit = book.live.get(seq)
        if st != ST_REJECTED and hit is not None and hit[0] == s:  # it rests
            sd = book.side[s][0 if hit[1] == BUY else 1]
            fifo = sd.fifo(hit[2])
            key = (s, hit[1], hit[2])
            if len(fifo) == 1:  # (an emptied level is dropped: a FIFO of one is a new level)
                count[key] = 0
            _POS[seq] = count.get(key, 0)
            count[key] = count.get(key, 0) + 1
            c["level_over"] += sum(e[1] for e in fifo) > CAP32
        if pre is not None and len(f):
            run, avail, whole = pre
            c["sat_chunk"] += sum(run) >= CAP32
        if pre is not None and (kd >> 4) & 3 == TIF_FOK:
            run, avail, whole = pre
            if st == ST_FILLED and avail >= CAP31:
                c["fok_filled"] += 1
        if (kd >> 4) & 3 == TIF_FOK and st == ST_CANCELED and int(r["filled_qty"]) == 0:
            side = kd & 3
            opp = book.side[s][1 if side == BUY else 0]
            if sum(e[1] for ff in opp.levels.values() for e in ff) >= CAP31:
                c["fok_killed"] += 1
        if base is not None:
            lo = int(base[s])
            for x in f:
                if not (lo <= int(x["price_q4"]) < lo + levels) and int(x["qty"]) >= Q28:
                    c["far_big_fill"] += 1
    for cx, tag in ((False, ""), (True, "_cx")):
        for start, by_batch in per.values():
            ub, walked, going = start, 0, start < CAP31
            for k in sorted(by_batch):
                rs = by_batch[k]
                for lo in range(0, len(rs), 64):
                    if not going:
                        break
                    blk = rs[lo:lo + 64]
                    ub += sum(0 if (cx and kd & 8) else max(q, 0) for q, kd, _ in blk)
                    if ub >= CAP31:
                        c["refused_later" + tag] += walked > 0
                        going = False
                        break
                    for q, kd, far in blk:
                        if far or (kd >> 4) & 3 in (TIF_FOK, TIF_POST_ONLY) and not kd & 8 or \
                                (kd & 12) == 12 or (kd & 8 and not cx):
                            going = False
                            break
                        walked += 1
                        c["walk_big" + tag] += q >= 1 << 20 and not kd & 8
    return c


def plain_subset(batches, map_qty=None, far_free=None):
    """The GTC LIMITs and MARKETs of a stream (TIF bits clear, no cancels, no reduces), seqs kept; map_qty maps
    every quantity; far_free = (base, levels) also drops LIMITs priced outside the initial window."""
    out = []
    for b in batches:
        keep = ((b.kind & 0x08) == 0) & (((b.kind >> 4) & 3) == 0)
        if far_free is not None:
            base, L = far_free
            lo = base[np.minimum(b.symbol, len(base) - 1)]
            keep &= ((b.kind & 4) != 0) | ((b.price_q4 >= lo) & (b.price_q4 < lo + L))
        q = b.qty[keep]
        if map_qty is not None:
            q = np.where(q > 0, map_qty(q.astype(np.int64)), q)
        out.append(Arrays(b.seq[keep], b.price_q4[keep], q, b.symbol[keep], b.kind[keep] & 0x0F))
    out = [a for a in out if len(a)]
    check_seq_rule(out)
    return out


# ---- the streams the GPU tests run (tests/test_big_qty_model.py asserts their coverage) -----------------------------

STREAMS = {
    # name: (seed, symbols, levels, batches, records per batch, group, keywords)
    "grouped_far": (1, 16, 128, 12, 1024, 4, dict(far_pct=3)),
    "grouped": (2, 16, 128, 12, 1024, 4, dict()),
    "deep256_far": (3, 8, 256, 8, 1500, 1, dict(far_pct=3)),
    "deep256": (4, 8, 256, 8, 1500, 1, dict()),
    "deep_far": (5, 8, 1024, 8, 1500, 1, dict(far_pct=3)),
    "deep": (6, 8, 1024, 8, 1500, 1, dict()),
    "hot1024_far": (7, 8, 1024, 8, 1500, 1, dict(far_pct=3, skew=True)),
    "hot1024": (8, 8, 1024, 8, 1500, 1, dict(skew=True)),
    "hot2048_far": (9, 8, 2048, 8, 1500, 1, dict(far_pct=3, skew=True)),
    "hot2048": (10, 8, 2048, 8, 1500, 1, dict(skew=True)),
}
PATH_STREAMS = {"reg": ("grouped_far", "grouped"), "gwalk": ("grouped_far", "grouped"),
                "gwalk_cx": ("grouped_far", "grouped"), "deep256": ("deep256_far", "deep256"),
                "deep": ("deep_far", "deep"), "hot_agg": ("hot1024_far", "hot1024"),
                "hot": ("hot2048_far", "hot2048")}


FEEDS = {"reg": ("grouped_far", 256), "deep": ("deep_far", 300)}  # path: (stream, records per launch)


def slices(batches, n):
    """The stream in batches of at most n records (more launches: more points at which a feed is compared)."""
    return [Arrays(b.seq[lo:lo + n], b.price_q4[lo:lo + n], b.qty[lo:lo + n], b.symbol[lo:lo + n], b.kind[lo:lo + n])
            for b in batches for lo in range(0, len(b), n)]


@functools.lru_cache(maxsize=None)
def stream(name):
    """(base, batches, [(results, fills)] of the model, the model after the last batch). Shared: nobody changes
    the arrays or steps the model."""
    seed, S, L, nb, n, group, kw = STREAMS[name]
    base, batches = big_stream(seed, S, L, nb, n, group=group, **kw)
    model = ReduceBook(S)
    exp = [model.submit(a) for a in batches]
    return base, batches, exp, model


# ---- the directed cases ------------------------------------------------------------------------------------------------
# Each builder returns a Case: the batches in order (grouped into launch groups where that matters) and what
# the model test pins about them. HOT_PAD records keep symbol 0 above ME_HOT_MIN = 64 on the hot paths.

MAX = INT32_MAX
HOT_PAD = 70
PATTERNS = ("max", "q28", "hole", "pow2")


class Case:
    def __init__(self, S, L, base, batches, **info):
        self.S, self.L, self.base, self.batches = S, L, base, batches
        self.__dict__.update(info)


def _pad_bids(sc, mid, n):
    """n passive one-lot bids of symbol 0 well below everything else"""
    for j in range(n):
        sc.new(0, BUY, mid - 30 - j % 8, 1)


def pattern_quantities(pattern, n):
    one = {"max": [MAX] * CHUNK,
           "q28": [Q28] * (CHUNK - 1) + [Q28 + 5],
           "hole": [MAX, MAX, 1] + [MAX] * (CHUNK - 3),
           "pow2": [1 << (15 + j) for j in range(CHUNK)]}[pattern]
    return [one[j % CHUNK] for j in range(n)]


def chunk_case(where, pattern, nmakers, one_batch):
    """`nmakers` asks of symbol 0 at one price (16: exactly one chunk; 33: three), quantities of `pattern`; then
    the buys MARKET INT32_MAX, IOC 1, LIMIT INT32_MAX - 1, FOK INT32_MAX — each in its own batch or all in one
    (batches[1:named_end]) — then a batch of MARKETs of INT32_MAX while at least 2 x INT32_MAX stay and a last
    batch of MARKETs that drains the level.
    where: "reg" / "hot" (a window level, L = 128 / 2,048, the hot batches padded past ME_HOT_MIN) or "far" (a
    price outside the window, L = 128)."""
    L = 2048 if where == "hot" else 128
    S = 2
    base = base_prices(S, L)
    mid = int(base[0]) + L // 2
    price = int(base[0]) + 3 * L if where == "far" else mid + 2
    pad = HOT_PAD // 2 if where == "hot" else 0
    qs = pattern_quantities(pattern, nmakers)
    sc = Script()
    sc.new(1, SELL, int(base[1]) + L // 2 + 1, 5)
    sc.new(0, BUY, mid - 3, 5)
    _pad_bids(sc, mid, pad)
    makers = [sc.new(0, SELL, price, q) for q in qs]
    _pad_bids(sc, mid, pad)
    batches = [sc.take()]
    takers = [dict(q=MAX, market=True), dict(q=1, tif=TIF_IOC), dict(q=MAX - 1), dict(q=MAX, tif=TIF_FOK)]
    left = sum(qs) - (MAX + 1 + MAX - 1 + MAX)  # (when the FOK fills; a killed one leaves more: fine)
    more = [dict(q=MAX, market=True)] * max(0, left // MAX - 2)
    tseq = []

    def put(t):
        _pad_bids(sc, mid, pad)
        tseq.append(sc.new(0, BUY, 0 if t.get("market") else price, t["q"], market=t.get("market", False),
                           tif=t.get("tif", 0)))
        _pad_bids(sc, mid, pad)

    if one_batch:
        for t in takers:
            put(t)
        batches.append(sc.take())
    else:
        for t in takers:
            put(t)
            batches.append(sc.take())
    named_end = len(batches)
    if more:
        for t in more:
            put(t)
        batches.append(sc.take())
    ndrain = (sum(qs) + MAX - 1) // MAX + 1
    _pad_bids(sc, mid, pad)
    for _ in range(ndrain):
        tseq.append(sc.new(0, BUY, 0, MAX, market=True))
    _pad_bids(sc, mid, pad)
    batches.append(sc.take())
    check_seq_rule(batches)
    return Case(S, L, base, batches, makers=makers, qs=qs, price=price, takers=tseq, named_end=named_end)


def fok_case(path_levels, hot=False):
    """Five window ask levels and two far ones of INT32_MAX each (one order per level: a1..a7), then, one record
    per batch, buys of symbol 0:
      0 MARKET 1                         a1: 1
      1 FOK MAX, limit level 1           MAX - 1 there: one lot too little, killed
      2 (a SELL of 1 rests at level 1: a8)
      3 FOK MAX, limit level 1           exactly enough: a1 MAX - 1, a8 1
      4 MARKET 1                         a2: 1
      5 FOK MAX, limit level 3           2 x MAX - 1 within the limit (the running sum passes 2^31): a2 MAX - 1, a3 1
      6 FOK MAX, limit the first far     window levels, then a far one (> 2^32 within the limit): a3 MAX - 1, a4 1
      7 FOK MAX, limit the second far    a4 MAX - 1, a5 1
      8 MARKET FOK MAX                   needs a far level: a5 MAX - 1, a6 1
      9 MARKET FOK MAX                   far levels only: a6 MAX - 1, a7 1
     10 MARKET FOK MAX                   MAX - 1 left in the book: one lot too little, killed
    """
    L, S = path_levels, 2
    base = base_prices(S, L)
    mid = int(base[0]) + L // 2
    pad = HOT_PAD // 2 if hot else 0
    sc = Script()
    sc.new(1, SELL, int(base[1]) + L // 2 + 1, 5)
    sc.new(0, BUY, mid - 3, 5)
    prices = [mid + 1 + j for j in range(5)] + [int(base[0]) + 2 * L, int(base[0]) + 3 * L]
    _pad_bids(sc, mid, pad)
    a = [None] + [sc.new(0, SELL, p, MAX) for p in prices]
    _pad_bids(sc, mid, pad)
    batches = [sc.take()]
    steps = [dict(q=1, market=True), dict(q=MAX, px=prices[0], tif=TIF_FOK), dict(sell=1, px=prices[0]),
             dict(q=MAX, px=prices[0], tif=TIF_FOK), dict(q=1, market=True), dict(q=MAX, px=prices[2], tif=TIF_FOK),
             dict(q=MAX, px=prices[5], tif=TIF_FOK), dict(q=MAX, px=prices[6], tif=TIF_FOK),
             dict(q=MAX, market=True, tif=TIF_FOK), dict(q=MAX, market=True, tif=TIF_FOK),
             dict(q=MAX, market=True, tif=TIF_FOK)]
    seqs = []
    for t in steps:
        _pad_bids(sc, mid, pad)
        if "sell" in t:
            seqs.append(sc.new(0, SELL, t["px"], t["sell"]))
        else:
            seqs.append(sc.new(0, BUY, t.get("px", 0), t["q"], market=t.get("market", False), tif=t.get("tif", 0)))
        _pad_bids(sc, mid, pad)
        batches.append(sc.take())
    check_seq_rule(batches)
    a.append(seqs[2])  # a8
    want = {0: [(a[1], 1)], 1: [], 3: [(a[1], MAX - 1), (a[8], 1)], 4: [(a[2], 1)], 5: [(a[2], MAX - 1), (a[3], 1)],
            6: [(a[3], MAX - 1), (a[4], 1)], 7: [(a[4], MAX - 1), (a[5], 1)], 8: [(a[5], MAX - 1), (a[6], 1)],
            9: [(a[6], MAX - 1), (a[7], 1)], 10: []}
    return Case(S, L, base, batches, pad=pad, want=want, killed=(1, 10), a=a)


def reduce_case(path_levels):
    """Bids of symbol 0. Level p: A (MAX), B (5). Level p - 1: C (MAX). Level p - 2: five orders of MAX (more than
    2^33 of queue), X (MAX), Y (1). Batches: [the book], [reduce A by MAX - 1 (one lot rests, ahead of B), a SELL
    of 3: A 1, B 2], [reduce C by MAX: a cancel], [reduce X by 2^31 - 2: one lot rests behind the queue], [SELLs
    that take B's 3 and the five orders, then a SELL of 2: X 1, Y 1]."""
    L, S = path_levels, 2
    base = base_prices(S, L)
    mid = int(base[0]) + L // 2
    p = mid - 1
    sc = Script()
    sc.new(1, SELL, int(base[1]) + L // 2 + 1, 5)
    A, B = sc.new(0, BUY, p, MAX), sc.new(0, BUY, p, 5)
    C = sc.new(0, BUY, p - 1, MAX)
    Q = [sc.new(0, BUY, p - 2, MAX) for _ in range(5)]
    X, Y = sc.new(0, BUY, p - 2, MAX), sc.new(0, BUY, p - 2, 1)
    batches = [sc.take()]
    sc.reduce(0, A, MAX - 1)
    t1 = sc.new(0, SELL, p, 3)
    batches.append(sc.take())
    sc.reduce(0, C, MAX)
    batches.append(sc.take())
    sc.reduce(0, X, MAX - 1)
    batches.append(sc.take())
    sc.new(0, SELL, 0, 3, market=True)
    for _ in range(5):
        sc.new(0, SELL, 0, MAX, market=True)
    t2 = sc.new(0, SELL, 0, 2, market=True)
    batches.append(sc.take())
    check_seq_rule(batches)
    return Case(S, L, base, batches, A=A, B=B, C=C, Q=Q, X=X, Y=Y, t1=t1, t2=t2)


# LW_CAP: one symbol; a case is a list of launch groups (G batches each) with the hand-offs each must add.
P31 = 1 << 31
LW_Q = 1000


def lw_cases(path):
    """{name: (G, [(batches of the group, hand-offs it adds, why)])} for `path` in gwalk / gwalk_cx / hot_agg.
    The counts follow from the code's comparisons, with B the symbol's window sum at the group's start and Q the
    quantities of the blocks up to and including the one in question (me_agg.hip):

      grouped walks (k_agg_gwalk<CX>): lok = lw_init() = `w.ub < LW_CAP` with ub = B; per block
        `lw.ub += qsum; adm = lw.ub < LW_CAP`, qsum = gw_prepare's sum of `(uint32_t)max(oq, 0)` over the block's
        records — a cancel's ignored qty included on the plain walk, counted as 0 on the cancel walk
        (gw_prepare_cx: `cxr ? 0 : ...`). !lok or !adm clears the block's fast mask, lw_block walks 0 records
        and a_ghand hands the symbol off: one hand-off per group, however many blocks follow. So a group adds a
        hand-off iff B >= 2^31 or B + Q >= 2^31 at some block (or a record is one the walk does not cover: on
        the plain walk every cancel, a_classify's `uncovered`).
      hot aggregate walk (k_agg_hot): `ladder = lw_init()`; a book the ladder cannot hold (B >= 2^31) runs the
        64-bit list walk (a_block), no hand-off; on the ladder `adm = lw_admit(lw, oq)` per block with the same
        clamp and every record's qty (cancels included), and !adm hands off (hot_handoffs), once per batch.

    Rejected pad records (qty 0) add nothing to Q; on hot_agg every batch is padded to HOT_PAD records."""
    hot = path == "hot_agg"
    cx = path == "gwalk_cx"
    L = 1024 if hot else 128
    base = base_prices(1, L)
    mid = int(base[0]) + L // 2
    cases = {}

    def mk(G, groups):
        """groups: [([batch as list of ops], delta, why)]; an op is a tuple for Script"""
        sc = Script()
        out = []
        for blist, delta, why in groups:
            assert len(blist) == G
            arrs = []
            for ops, before in blist:
                n = 0
                for _ in range(before):
                    sc.new(0, BUY, mid - 10, 0)
                    n += 1
                for op in ops:
                    if op[0] == "ask":
                        sc.new(0, SELL, mid + op[2] if len(op) > 2 else mid + 2, op[1])
                    elif op[0] == "bid":
                        sc.new(0, BUY, mid - 2, op[1])
                    elif op[0] == "mkt":
                        sc.new(0, BUY, 0, op[1], market=True)
                    elif op[0] == "bad":
                        sc.new(0, BUY, mid - 2, op[1])
                    elif op[0] == "cancel":
                        sc.cancel(0, op[1], op[2])
                    n += 1
                while hot and n < HOT_PAD:
                    sc.new(0, BUY, mid - 10, 0)
                    n += 1
                arrs.append(sc.take())
            out.append((arrs, delta, why))
        check_seq_rule([a for g in out for a in g[0]])
        return G, out

    def one(ops, before=0):
        return [(ops, before)]

    pad = ([("bad", 0)], 0)
    q = LW_Q
    build = [("ask", 1 << 30), ("ask", (1 << 30) - 1 - q)]  # B = 2^31 - 1 - q
    drain = (one([("mkt", 1 << 30)]), 0 if hot else 1,
             "B = 2^31 at the start: the grouped walks' lok is false (a hand-off); the hot walk runs its list walk")
    after = (one([("bid", 5), ("mkt", 3)]), 0, "B = 2^30: back on the walk")
    for name, before in (("i", 0), ("ii", 64)):
        cases[name + "_keep"] = mk(1, [(one(build), 0, "Q = 2^31 - 1 - q"),
                                      (one([("bid", q)], before), 0, "B + Q = 2^31 - 1")])
        cases[name + "_over"] = mk(1, [(one(build), 0, "Q = 2^31 - 1 - q"),
                                      (one([("bid", q + 1)], before), 1, "B + Q = 2^31"), drain, after])
    if not hot:
        t1, t2 = 1 << 29, 1 << 28
        qs = P31 - 1 - ((1 << 30) + t1 + t2)
        for name, qq, delta in (("iii_keep", qs, 0), ("iii_over", qs + 1, 1)):
            cases[name] = mk(3, [([([("ask", 1 << 30)], 0), pad, pad], 0, "Q = 2^30"),
                                 ([([("mkt", t1)], 0), ([("mkt", t2)], 0), ([("bid", qq)], 0)], delta,
                                  "ub = 2^30 + 2^29 + 2^28 + q while the true sum fell to 2^28 + q"),
                                 ([([("bid", 5)], 0), ([("mkt", 3)], 0), pad], 0, "B < 2^30: on the walk")])
    cases["iv_below"] = mk(1, [(one([("ask", 1 << 30), ("ask", (1 << 30) - 1)]), 0, "Q = 2^31 - 1"),
                               (one([("bad", 0)]), 0, "B = 2^31 - 1, Q = 0")])
    cases["iv_at"] = mk(1, [(one([("ask", 1 << 30), ("ask", 1 << 30)]), 1, "Q = 2^31 on an empty book"),
                            (one([("bad", 0)]), 0 if hot else 1, "B = 2^31, Q = 0: lok false / the list walk"),
                            drain, after])
    # (v) seq 1 is the cancel's target: 7 lots alone on its level
    book = [("ask", 7, 3), ("ask", 1 << 30), ("ask", (1 << 30) - 2 - 7)]  # B = 2^31 - 2
    if cx:
        cases["v"] = mk(1, [(one(book), 0, "Q = 2^31 - 2"),
                            (one([("cancel", 1, MAX), ("bad", -5), ("bid", 1)]), 0,
                             "Q = 0 (cxr) + 0 (max(-5, 0)) + 1: B + Q = 2^31 - 1")])
    else:
        cases["v"] = mk(1, [(one(book), 0, "Q = 2^31 - 2"),
                            (one([("bad", -5), ("bid", 1)]), 0, "Q = 0 (max(-5, 0)) + 1: B + Q = 2^31 - 1"),
                            (one([("cancel", 1, MAX)]), 1,
                             "a cancel is not covered (a_classify) whatever Q; its qty would also take Q past the bound")])
    return L, base, cases
