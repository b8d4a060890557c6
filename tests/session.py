"""Composed sessions: one engine's whole life as a script — TEST INFRASTRUCTURE ONLY.

`plan(case)` composes the models the single-feature suites stand on (ReduceBook, QuoteModel, DepthModel,
TradeModel, StopModel, the mass-cancel equivalent, the order query's and the preview's answers) over one
`reduce_stream`, with all four device feeds on, stops armed, and the between-launch calls drawn at every stretch
boundary. Every expected output is in the plan: tests/test_session_gpu.py only replays and compares,
tests/test_session_model.py checks on the CPU what the plans reach. `PARAMS` is the one list of cases both use.

What the plan has to know about the engine, each read in me_engine.cpp:
  * a launch is what one match launch takes: the batches of the open group when it closes (batches_per_launch of
    them) or is cut. `Pipe` restates the three-stage pipeline (bucket, match, tape) as far as cuts go: a collect of
    a ticket whose group has not reached its tape job, me_sync, and every call that goes through me_sync or
    flush_pipeline (stops_add once it is past its capacity check, stops_cancel, stops_dump, mass_cancel,
    order_query, order_preview) send the open group out as it is;
  * every feed's job runs behind a match launch and stamps its events with the batches matched so far; a purge
    that removes something runs the quote and depth jobs once more under the unchanged stamp;
  * a feed job that does not fit its ring's free room logs nothing and is caught up by the read that empties
    the ring (`Ring`, the rule tests/test_feed_ring_gpu.py states); the trigger book never defers because
    stops_add refuses while added - cancelled - read + n > cap_stops.
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass, field

import numpy as np

from oracle.pybook import RJ_BAD_QTY, RJ_BAD_SEQ, RJ_BAD_SIDE, RJ_BAD_SYMBOL, ST_CANCELED, ST_NEW, \
    ST_PARTIAL, ST_REJECTED
from tests import depth_model as dm
from tests import mass_cancel_model as mc
from tests import order_query_model as oq
from tests import preview_model as pv
from tests import quote_model as qm
from tests import stops_model as sm
from tests import trade_model as tm
from tests.big_qty import Snap
from tests.gpu_harness import PATHS
from tests.reduce_model import ReduceBook, is_reduce, reduce_stream
from tests.tif_model import Arrays, kind

BUY, SELL = 1, 2
TIF_IOC, TIF_FOK, TIF_POST = 1, 2, 3
RJ_WOULD_CROSS, RJ_BAD_TIF = 8, 9
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
S = 16
D = 4             # the depth feed's levels per side
CAP_STOPS = 256   # the trigger book's capacity, and the seq gap left behind every batch for injected records
DEEP_BOOKS = dict(mix=(70, 4, 3, 6, 5, 12), spread=5)  # tests/test_order_query_gpu.py's: levels of several chunks
VARIANTS = ("host", "device", "tight", "lagcut", "wrap")
WRONG = ("stretch_extremes", "add_sees_earlier_fills", "purge_clears_stops", "inject_at_stop_px")


@dataclass(frozen=True)
class Case:
    seed: int
    path: str
    group: int
    variant: str = "host"

    @property
    def id(self):
        return f"{self.path}-G{self.group}-{self.variant}-s{self.seed}"


def cases(nseeds=2):
    """The sessions the GPU suite runs: `nseeds` seeds on each of the seven rows (G = 1 and 4 on the grouped
    ones), the device-group form at G = 8 on the L = 128 rows, the tight rings on gwalk_cx / reg / deep, a lag
    below the group on the grouped rows, the small wrapping seq ring under seqs above 2^40 on gwalk_cx / deep."""
    out = []
    for p, row in PATHS.items():
        for g in ((1, 4) if row[3] else (1,)):
            out += [Case(s, p, g) for s in range(nseeds)]
    out += [Case(10, p, 8, "device") for p in PATHS if PATHS[p][3]]
    out += [Case(20, "gwalk_cx", 4, "tight"), Case(21, "reg", 1, "tight"), Case(22, "deep", 1, "tight")]
    out += [Case(30, p, 4, "lagcut") for p in PATHS if PATHS[p][3]]
    out += [Case(40, "gwalk_cx", 4, "wrap"), Case(41, "deep", 1, "wrap")]
    return out


# ME_FUZZ_SEEDS=N widens the seed range for soak runs, as in tests/test_gpu_fuzz.py; the default stays as listed
PARAMS = cases(int(os.environ.get("ME_FUZZ_SEEDS", "0")) or 2)


class Pipe:
    """Which batches each match launch takes (me_engine.cpp enqueue_batch / pipe_launch / flush_pipeline /
    me_collect), tickets = positions in the stretch. On a path without launch groups a batch is a launch."""

    def __init__(self, group, grouped):
        self.G, self.grouped = group, grouped
        self.open, self.match, self.tape = [], None, None
        self.taped = set()
        self.launches = []  # in match order
        self.cuts = 0

    def _launch(self, nb):
        if self.match:
            self.launches.append(self.match)
        self.taped.update(self.tape or ())
        self.tape, self.match = self.match, nb

    def submit(self, t):
        if not self.grouped:
            self.launches.append([t])
            self.taped.add(t)
            return
        self.open.append(t)
        if len(self.open) == self.G:
            self._launch(self.open)
            self.open = []

    def flush(self):
        """-> whether a partial group went out."""
        cut = bool(self.open)
        if self.open:
            self._launch(self.open)
            self.open = []
        while self.match or self.tape:
            self._launch(None)
        self.cuts += cut
        return cut

    def collect(self, t):
        return self.flush() if t not in self.taped else False


class Ring:
    """The event-ring protocol over a feed model: a job that does not fit cap - (tail - consumed) logs nothing
    and leaves a deferral pending (`peek`); a read that empties the ring with one pending runs one catch-up job
    (`expect`), whose events follow in the same read as far as the room goes."""

    def __init__(self, cap, model, dtype, room):
        self.cap, self.model, self.room = cap, model, room
        self.logged = np.zeros(0, dtype=dtype)
        self.tail = self.consumed = self.deferred = 0
        self.pending = False

    def job(self, stamp):
        if len(self.model.peek()) <= self.cap - (self.tail - self.consumed):
            self.logged = np.concatenate([self.logged, self.model.expect(stamp)])
            self.tail = len(self.logged)
            self.pending = False
        else:
            self.deferred += 1
            self.pending = True

    def read(self, stamp):
        lo = self.consumed
        self.consumed += min(self.tail - self.consumed, self.room)
        if self.consumed == self.tail and self.pending:
            self.job(stamp)
            assert not self.pending  # (an empty log holds any one job)
            self.consumed += min(self.tail - self.consumed, self.room - (self.consumed - lo))
        return self.logged[lo:self.consumed], self.tail - self.consumed

    def drain(self, stamp):
        parts = []
        while True:
            ev, left = self.read(stamp)
            parts.append(ev)
            if not left:
                return np.concatenate(parts)


class Books:
    """The books of a checkpoint as the book checks read a model: dump(s) and resting()."""

    def __init__(self, book, n):
        self.dumps = [book.dump(s) for s in range(n)]

    def dump(self, s):
        return self.dumps[s]

    def resting(self):
        return sum(len(d) for d in self.dumps)


@dataclass
class Plan:
    case: Case
    levels: int
    grouped: bool
    base: np.ndarray
    knobs: dict           # what the seed drew
    engine_kw: dict = field(default_factory=dict)
    caps: dict = field(default_factory=dict)     # quotes / depth / trades / stops
    first_stops: np.ndarray = None
    steps: list = field(default_factory=list)
    counts: dict = field(default_factory=dict)
    spans: list = field(default_factory=list)    # seq span of every launch
    tapes: list = field(default_factory=list)    # every batch's tape, in order
    stream: list = field(default_factory=list)   # every batch submitted, in order


def _renumber(batches):
    """The stream with a gap of CAP_STOPS seqs behind every batch; CANCEL / REDUCE targets move with their orders.
    Seqs only have to ascend."""
    firsts = []
    for b in batches:
        new = b.seq[((b.kind & 8) == 0) & (b.seq != 0)]
        firsts.append(int(new.min()) if len(new) else (firsts[-1] if firsts else 0))
    assert firsts == sorted(firsts)
    edges = np.array(firsts, dtype=np.uint64)

    def move(v):
        v = np.asarray(v, dtype=np.uint64)
        k = np.maximum(np.searchsorted(edges, v, side="right"), 1) - 1
        return np.where(v == 0, v, v + np.uint64(CAP_STOPS) * k.astype(np.uint64))

    out = []
    for b in batches:
        px = b.price_q4.copy()
        c = ((b.kind & 8) != 0) & (px > 0)
        px[c] = move(px[c].astype(np.uint64)).astype(np.int64)
        out.append(Arrays(move(b.seq), px, b.qty, b.symbol, b.kind))
    return out


class _Builder:
    def __init__(self, case, wrong):
        self.c, self.wrong = case, wrong
        L, _, _, grouped = PATHS[case.path]
        self.L, self.grouped, self.G = L, grouped, case.group if grouped else 1
        rng = self.rng = np.random.default_rng([case.seed, list(PATHS).index(case.path), case.group,
                                                VARIANTS.index(case.variant)])
        hot = case.path in ("hot", "hot_agg")
        wrap = case.variant == "wrap"
        k = dict(far_pct=int(rng.choice((0, 2, 5))), drift=int(rng.choice((0, 3))),
                 skew=bool(hot or rng.integers(2)), seq_start=(1 << 40) + 3 if wrap or rng.integers(2) else 1,
                 deep_books=bool(case.seed % 2), small_ring=bool(wrap or rng.integers(2)))
        self.tight = case.variant == "tight"
        self.n_launches = int(rng.integers(8, 11))
        self.batch = 768 if not grouped else (512 if self.G == 1 else 384)
        kw = dict(far_pct=k["far_pct"], drift=k["drift"], skew=k["skew"], seq_start=k["seq_start"])
        if k["deep_books"]:
            kw.update(DEEP_BOOKS)
        nb = self.n_launches * self.G
        base, raw = reduce_stream(7_000 + case.seed, S, L, nb, self.batch, **kw)
        self.feedstock = _renumber(raw)
        self.p = Plan(case, L, grouped, base, k)
        self.book = ReduceBook(S)
        snap = Snap(self.book)
        self.trades, self.stops = tm.TradeModel(S), sm.StopModel(S)
        q, d = qm.QuoteModel(snap, S), dm.DepthModel(snap, S, D)
        if self.tight:  # each deferring feed at its minimum capacity
            caps = dict(quotes=S, depth=4 * D * S, trades=S)
        else:
            caps = dict(quotes=16 * S, depth=16 * 4 * D * S, trades=16 * S)
        caps["stops"] = CAP_STOPS
        self.p.caps = caps
        self.rings = {"quotes": Ring(caps["quotes"], q, qm.QUOTE_DTYPE, S),
                      "depth": Ring(caps["depth"], d, dm.DEPTH_DTYPE, 4 * D * S),
                      "trades": Ring(caps["trades"], self.trades, tm.TRADE_DTYPE, S)}
        for name in ("quotes", "depth"):  # enabling takes the (empty) books once; the trade feed starts silent
            self.rings[name].job(0)
        self.nm = 0            # batches matched
        self.prev = 0          # the last seq of the stream so far
        self.next_stream = 0
        self.stop_ev = []      # stop events logged and not read
        self.sc = dict(added=0, cancelled=0, read=0, events=0)
        self.next_id = 1
        self.triggered, self.issued, self.injected = [], [], set()
        self.peak = 0
        self.cn = self.p.counts
        for name in ("stop_events", "stop_jobs", "inj_fill", "inj_rest", "cascade", "refused", "cancelled_live",
                     "purges", "purged_orders", "purged_far", "fok_kill", "post_reject", "reduce_partial",
                     "reduce_cover", "bad", "all_three", "cuts", "launches", "mid_adds", "mid_purges"):
            self.cn[name] = 0

    # ---- the books' side -------------------------------------------------------------------------------
    def _mid(self, s):
        """(bid, ask) of symbol s, an absent side a tick from the initial mid."""
        bids, asks = Snap(self.book).snapshot(s, 1)
        mid = int(self.p.base[s]) + self.L // 2
        return (int(bids[0]["price_q4"]) if len(bids) else mid - 1, int(asks[0]["price_q4"]) if len(asks) else mid + 1)

    def _count_kinds(self, b, res):
        kd, st, rj = b.kind.astype(np.int64), res["status"], res["reason"]
        new, tif = (kd & 8) == 0, (kd >> 4) & 3
        red = is_reduce(kd)
        self.cn["fok_kill"] += int((new & ((kd & 4) == 0) & (tif == TIF_FOK) & (st == ST_CANCELED) & (res["filled_qty"] == 0)).sum())
        self.cn["post_reject"] += int((new & (rj == RJ_WOULD_CROSS)).sum())
        self.cn["reduce_partial"] += int((red & (st == ST_NEW)).sum())
        self.cn["reduce_cover"] += int((red & (st == ST_CANCELED)).sum())
        self.cn["bad"] += int(((st == ST_REJECTED) & np.isin(rj, (RJ_BAD_QTY, RJ_BAD_SIDE, RJ_BAD_SYMBOL, RJ_BAD_SEQ,
                                                                  RJ_BAD_TIF))).sum())

    def _launch(self, batches, last_of_stretch, before_jobs=None):
        """One match launch through every model; -> ([(results, tape)] per batch, the tapes)."""
        outs, tapes = [], []
        for b in batches:
            res, fills = self.book.submit(b)
            self.peak = max(self.peak, self.book.resting())
            self._count_kinds(b, res)
            self.trades.feed(fills)
            self.stops.feed(fills)
            outs.append((res, fills))
            tapes.append(fills)
            self.p.tapes.append(fills)
            self.p.stream.append(b)
            new = b.seq[((b.kind & 8) == 0) & (b.seq != 0)]
            self.issued.extend(int(x) for x in new[:: max(1, len(new) // 24)])
        if before_jobs:
            before_jobs(tapes)
        self.nm += len(batches)
        seqs = np.concatenate([b.seq[b.seq != 0] for b in batches])
        self.p.spans.append(int(seqs.max()) - int(seqs.min()) + 1)
        emits = [len(r.model.peek()) > 0 for r in self.rings.values()]
        for r in self.rings.values():
            r.job(self.nm)
        if self.wrong == "stretch_extremes" and not last_of_stretch:
            ev = np.zeros(0, dtype=sm.STOP_EVENT_DTYPE)  # (the extremes are kept for the stretch's last job)
        else:
            ev = self.stops.job(self.nm)
        if len(ev):
            self.cn["stop_jobs"] += 1
            self.cn["stop_events"] += len(ev)
            self.sc["events"] += len(ev)
            self.stop_ev.append(ev)
            self.triggered.extend(int(x) for x in ev["id"])
            fl = np.concatenate(tapes)
            fl = fl[np.isin(fl["taker_seq"], np.fromiter(self.injected, dtype=np.uint64, count=len(self.injected)))]
            for e in ev:  # a stop a fill of an injected record reaches: a cascade of depth >= 2
                px = fl["price_q4"][fl["symbol"] == e["symbol"]]
                buy = int(e["kind"]) & 3 == BUY
                if len(px) and ((px >= e["stop_px_q4"]).any() if buy else (px <= e["stop_px_q4"]).any()):
                    self.cn["cascade"] += 1
        if all(emits) and len(ev):
            self.cn["all_three"] += 1
        self.cn["launches"] += 1
        return outs, tapes

    # ---- the steps between launches ----------------------------------------------------------------------
    def _pending(self):
        return self.sc["added"] - self.sc["cancelled"] - self.sc["read"]

    def _ids(self, n):
        ids = []
        for _ in range(n):
            self.next_id += int(self.rng.integers(1, 4))
            ids.append(self.next_id)
        return ids

    def _add(self, rows, refused=False):
        st = sm.stops(rows)
        room = self._pending() + len(st) <= CAP_STOPS
        assert room != refused, "the plan's own capacity arithmetic"
        if not refused:
            self.stops.add(st)
            self.sc["added"] += len(st)
        return {"op": "stops_add", "stops": st, "refused": refused}

    def _ladder(self, nsym):
        """Fresh stops at and a few ticks through the market of `nsym` symbols, every kind among them."""
        rng, rows = self.rng, []
        for s in rng.choice(S, nsym, replace=False):
            s = int(s)
            bid, ask = self._mid(s)
            side = SELL if rng.integers(2) else BUY  # one side per symbol: a triggered stop's fills reach the next
            for j, off in enumerate((0, 1, 2, 4)):
                sp = bid - off if side == SELL else ask + off
                u = 0 if j < 2 else int(rng.integers(4))
                q = int(rng.integers(80, 400)) if u == 0 else int(rng.integers(1, 120))
                if u == 0:    # stop: a MARKET, large enough to trade through a few levels
                    kd, lp = kind(side, 1), 0
                elif u == 1:  # stop-limit through the market: takes
                    kd, lp = kind(side), sp + (6 if side == BUY else -6)
                elif u == 2:  # stop-limit behind the market: rests
                    kd, lp = kind(side), sp - (5 if side == BUY else -5)
                else:
                    kd, lp = kind(side, 0, 0, TIF_IOC), sp + (3 if side == BUY else -3)
                rows.append((sp, lp, q, s, kd))
        return rows

    def stops_add(self):
        """One add that fits (the ladders, one stop at INT64_MIN, one at INT64_MAX) and one that is refused."""
        rng = self.rng
        rows = self._ladder(int(rng.integers(3, 6)))
        for edge in (I64_MIN, I64_MAX):
            s, side = int(rng.integers(S)), BUY if rng.integers(2) else SELL
            bid, ask = self._mid(s)
            rows.append((edge, bid if side == BUY else ask, int(rng.integers(1, 9)), s, kind(side)))
        room = CAP_STOPS - self._pending()
        rows = rows[-min(len(rows), max(room, 0)):]
        out = []
        if rows:
            out.append(self._add([(i,) + r for i, r in zip(self._ids(len(rows)), rows)]))
        over = CAP_STOPS - self._pending() + 1  # one more than fits
        ids = [self.next_id + 1 + j for j in range(over)]
        out.append(self._add([(i, I64_MAX, 0, 1, int(i % S), kind(BUY, 1)) for i in ids], refused=True))
        self.cn["refused"] += 1
        return out

    def stops_cancel(self):
        rng = self.rng
        live = [d["id"] for d in self.stops.table]
        ids = set(int(x) for x in rng.choice(live, min(len(live), int(rng.integers(3, 7))), replace=False)) if live else set()
        if self.triggered:
            ids.update(int(x) for x in rng.choice(self.triggered, min(len(self.triggered), 3), replace=False))
        known = set(live) | set(self.triggered)
        ids.update(i for i in (int(x) for x in rng.integers(1, self.next_id + 50, 6)) if i not in known)
        ids.update((self.next_id + 7, (1 << 64) - 1))
        ids = sorted(ids)
        found = self.stops.cancel(ids)
        n = int(found.sum())
        self.sc["cancelled"] += n
        self.cn["cancelled_live"] += n
        return [{"op": "stops_cancel", "ids": np.array(ids, dtype=np.uint64), "found": found}]

    def _far(self, s, sides=3):
        """The orders of symbol s (of `sides`) at least a window away from its market: on far levels."""
        bid, ask = self._mid(s)
        d = self.book.dump(s)
        d = d[(d["side"] & sides) != 0]
        return int((np.abs(d["price_q4"] - np.where(d["side"] == BUY, bid, ask)) >= self.L).sum())

    def mass_cancel(self, nsym=None):
        rng = self.rng
        n = int(rng.integers(1, 4)) if nsym is None else nsym
        holders = [s for s in range(S) if self._far(s)]
        syms = [int(s) for s in rng.choice(S, n, replace=False)]
        sides = [int(x) for x in rng.choice((1, 2, 3, 3), len(syms))]
        if holders and not any(self._far(s, sd) for s, sd in zip(syms, sides)):
            s = int(rng.choice(holders))  # a symbol that holds an order far from its market
            syms = [s] + [x for x in syms if x != s][:n - 1]
            sides[0] = 3
        elif nsym is None:  # the fullest book, both sides
            s = max(range(S), key=lambda x: len(self.book.dump(x)))
            syms = [s] + [x for x in syms if x != s][:n - 1]
            sides[0] = 3
        far = sum(self._far(s, sd) for s, sd in zip(syms, sides))
        ent, counts = mc.apply(self.book, syms, sides, self.prev)
        if self.wrong == "purge_clears_stops":
            self.stops.table = [d for d in self.stops.table if d["symbol"] not in syms]
        if len(ent):  # the quote and depth jobs behind the purge, under the unchanged stamp; no trade, no stop job
            self.rings["quotes"].job(self.nm)
            self.rings["depth"].job(self.nm)
        self.cn["purges"] += 1
        self.cn["purged_orders"] += len(ent)
        self.cn["purged_far"] += far
        return [{"op": "mass_cancel", "symbols": syms, "sides": sides, "entries": ent, "counts": counts}]

    def order_query(self):
        rng = self.rng
        live = list(self.book.live)
        seqs = [int(x) for x in rng.choice(live, min(len(live), 24), replace=False)] if live else []
        seqs += [q for q, hit in self.book.live.items() if abs(hit[2] - int(self.p.base[hit[0]]) - self.L // 2) >= self.L][:6]
        seqs += [int(x) for x in rng.choice(self.issued, min(len(self.issued), 20), replace=False)]
        seqs += self.issued[:6] + sorted(self.injected)[-4:]  # the oldest: behind the horizon of a small ring
        seqs += [0, self.prev + 1, self.prev + 1000, (1 << 64) - 1]
        while len(seqs) < 64:
            seqs.append(int(rng.integers(1, self.prev + 1)))
        seqs = seqs[:64]
        return [{"op": "order_query", "seqs": np.array(seqs, dtype=np.uint64), "answers": oq.expected(self.book, S, seqs)}]

    def order_preview(self):
        rng, qs = self.rng, []
        for i in range(32):
            s = int(rng.integers(S)) if i != 31 else S + 3
            bid, ask = self._mid(min(s, S - 1))
            side = (BUY, SELL, BUY, SELL, 0, 3)[i % 6] if i >= 26 else (BUY, SELL)[i % 2]
            kd = kind(side, int(i % 5 == 4), 0, (i // 2) % 4)
            px = (bid + ask) // 2 + int(rng.integers(-15, 16))
            if i % 8 == 5:
                px += int(rng.choice((-1, 1))) * 5 * self.L  # outside the window
            qs.append((s, kd, px, 0 if i == 30 else int(rng.integers(1, 300))))
        a = np.array(qs, dtype=np.int64)
        return [{"op": "order_preview", "queries": a, "answers": pv.expected(self.book, S, qs)}]

    # ---- stretches and checkpoints ---------------------------------------------------------------------
    def _take(self, n):
        out = []
        while n > 0 and self.next_stream < len(self.feedstock):
            b = self.feedstock[self.next_stream]
            self.next_stream += 1
            sq = b.seq.copy()
            c = (b.kind & 8) != 0  # a CANCEL / REDUCE repeats the seq in front of it: an injected record's, if one is
            sq[c] = np.maximum(sq[c], np.uint64(self.prev))
            b = Arrays(sq, b.price_q4, b.qty, b.symbol, b.kind)
            self.prev = max(self.prev, int(sq.max()))
            out.append(b)
            n -= 1
        return out

    def _inject(self, events):
        from matching_engine_amd import stop_records

        if self.wrong == "inject_at_stop_px":
            events = events.copy()
            events["limit_px_q4"] = events["stop_px_q4"]
        rec = stop_records(events, self.prev + 1)
        b = Arrays(rec.seq, rec.price_q4, rec.qty, rec.symbol, rec.kind)
        self.injected.update(int(x) for x in b.seq)
        self.prev = int(b.seq.max())
        return b

    def stretch(self, n_launches, form, lag, inject, mid):
        """`n_launches` launches' worth of batches, the injected batch first: submitted as the GPU test will,
        the launches as `Pipe` cuts them."""
        if self.next_stream >= len(self.feedstock):
            return 0
        want = n_launches * self.G
        seq0 = self.prev + 1
        batches = [self._inject(inject)] if inject is not None and len(inject) else []
        inj = bool(batches)
        batches += self._take(max(want - len(batches), 1))  # (in groups of one the injected batch is a launch)
        if inj:  # the gap behind the last batch holds them
            nxt = batches[1].seq[((batches[1].kind & 8) == 0) & (batches[1].seq != 0)]
            assert int(batches[0].seq.max()) < int(nxt.min()) and len(inject) <= CAP_STOPS
        pipe = Pipe(self.G, self.grouped)
        mid_at = self.G // 2 if mid and self.G >= 2 and form == "host" and len(batches) > self.G // 2 else None
        mid_launches, tickets, cuts = None, [], 0
        for k in range(len(batches)):
            if k == mid_at:
                pipe.flush()
                mid_launches = len(pipe.launches)
            pipe.submit(k)
            if form == "host":
                tickets.append(k)
                while len(tickets) > lag:
                    cuts += pipe.collect(tickets.pop(0))  # (a collect that sends a partial group out)
        for t in tickets:
            pipe.collect(t)
        pipe.flush()  # the checkpoint's sync
        assert [k for g in pipe.launches for k in g] == list(range(len(batches)))
        step = {"op": "stretch", "form": form, "lag": lag, "batches": batches, "inject_seq0": seq0 if inj else None,
                "mid_at": mid_at, "mid": None, "launches": pipe.launches, "stamps": [], "outs": [None] * len(batches)}

        def mid_step(tapes):
            if mid == "add":
                rows = self._mid_rows(tapes)
                step["mid"] = self._add([(i,) + r for i, r in zip(self._ids(len(rows)), rows)]) if rows else None
                self.cn["mid_adds"] += 1
            else:
                step["mid"] = self.mass_cancel(2)[0]
                self.cn["mid_purges"] += 1

        early = self.wrong == "add_sees_earlier_fills" and mid == "add"
        tapes = None
        for j, g in enumerate(pipe.launches):
            if j == mid_launches and not early:
                mid_step(tapes)
            # the wrong composition: the add's stops are in the table when the cut launch's own fills are judged
            hook = mid_step if early and j + 1 == mid_launches else None
            outs, tapes = self._launch([batches[k] for k in g], j == len(pipe.launches) - 1, hook)
            for k, o in zip(g, outs):
                step["outs"][k] = o
            step["stamps"].append(self.nm)
        if inj:
            res, kd = step["outs"][0][0], batches[0].kind
            self.cn["inj_fill"] += int((res["filled_qty"] > 0).sum())
            self.cn["inj_rest"] += int((((kd & 4) == 0) & (((kd >> 4) & 3) == 0) & (res["remaining_qty"] > 0) &
                                        np.isin(res["status"], (ST_NEW, ST_PARTIAL))).sum())
        self.cn["cuts"] += cuts
        self.p.steps.append(step)
        return -(-len(batches) // self.G) - (inj and self.G == 1)  # (in groups of one the injected launch is extra)

    def _mid_rows(self, tapes):
        """Stops the cut launch's own fills would trigger, had they counted: per traded symbol (four at most) a BUY
        stop at the launch's high and a SELL stop-limit at its low."""
        fl = np.concatenate(tapes)
        rows = []
        for s in np.unique(fl["symbol"])[:4]:
            p = fl["price_q4"][fl["symbol"] == s]
            rows.append((int(p.max()), 0, 1 + int(s) % 5, int(s), kind(BUY, 1)))
            rows.append((int(p.min()), int(p.min()) - 4, 2 + int(s) % 7, int(s), kind(SELL)))
        return rows[:max(CAP_STOPS - self._pending(), 0)]

    def checkpoint(self, tag):
        q, d, t = (self.rings[n].drain(self.nm) for n in ("quotes", "depth", "trades"))
        ev = np.concatenate(self.stop_ev) if self.stop_ev else np.zeros(0, dtype=sm.STOP_EVENT_DTYPE)
        self.stop_ev = []
        self.sc["read"] += len(ev)
        self.p.steps.append({"op": "checkpoint", "tag": tag, "quotes": q, "depth": d, "trades": t, "stops": ev,
                             "deferred": {n: r.deferred for n, r in self.rings.items()},
                             "logged": {n: r.tail for n, r in self.rings.items()},
                             "stop_events": self.sc["events"], "stop_live": len(self.stops.table),
                             "stop_dump": self.stops.dump(), "books": Books(self.book, S), "last_seq": self.prev,
                             "batches": self.nm})
        return ev


def _first_stops(b):
    """Eight stops per symbol at mid +- 2, 4, 7, 12: BUY stops above, SELL stops below, every kind among them."""
    rows = []
    for s in range(S):
        mid = int(b.p.base[s]) + b.L // 2
        for j, off in enumerate((2, 4, 7, 12)):
            for side in (BUY, SELL):
                sp = mid + off if side == BUY else mid - off
                u = (s + j + side) % 4 if j else 0  # the nearest is a MARKET: its fills reach the next
                q = 5 + 37 * ((s + 3 * j + side) % 5)
                if u == 0:  # (large enough to trade through to the next stop)
                    kd, lp, q = kind(side, 1), 0, 3 * q
                elif u == 1:
                    kd, lp = kind(side), sp + (4 if side == BUY else -4)
                elif u == 2:
                    kd, lp = kind(side), sp - (6 if side == BUY else -6)
                else:
                    kd, lp = kind(side, 0, 0, TIF_IOC), sp + (2 if side == BUY else -2)
                rows.append((sp, lp, q, s, kd))
    order = b.rng.permutation(len(rows))  # table order is not symbol order
    return [(i,) + rows[k] for i, k in zip(b._ids(len(rows)), order)]


@functools.lru_cache(maxsize=None)
def plan(case, wrong=None):
    """The session of `case` (a Case), computed from the models alone. `wrong` names one deliberately wrong
    composition (WRONG) for the CPU tests."""
    assert wrong is None or wrong in WRONG
    b = _Builder(case, wrong)
    rng, p, G = b.rng, b.p, b.G
    p.first_stops = b._add(_first_stops(b))["stops"]
    variant = case.variant
    bag, events = [], None
    k = done = 0  # stretches; launches' worth of batches submitted (a cut makes two launches of one)
    while done < b.n_launches:
        n = int(rng.integers(3, 5)) if b.tight else int(rng.choice((1, 1, 1, 2, 2, 3)))
        n = min(n, b.n_launches - done)
        form = "device" if variant == "device" and b.grouped and k % 2 == 0 else "host"
        if form == "device":
            n, lag = 1, 0
        elif variant == "lagcut":
            lag = max(G // 2, 1)
        elif b.grouped:
            lag = 3 * G - 1 + int(rng.integers(3))  # a ticket's group has had its tape job: no collect cuts
        else:
            lag = int(rng.integers(1, 4))
        mid = ("add", "purge")[(k // 2 + case.seed) % 2] if k else "add"
        n = b.stretch(n, form, lag, events, mid)
        if not n:
            break
        done += n
        events = b.checkpoint(f"stretch {k}")
        # one to three of the six between-launch steps. The injection is drawn on its own (always behind the first
        # two stretches: cascades need steps); the others come from a bag that refills, as many as the stretch had
        # launches, so that every step comes round within six launches
        inject = k < 2 or rng.random() < 0.75
        for _ in range(3 if b.tight else min(n, 2 if inject else 3)):
            if not bag:
                bag = [str(x) for x in rng.permutation(["stops_add", "stops_cancel", "mass_cancel", "mass_cancel",
                                                        "order_query", "order_preview"])]
            p.steps.extend(getattr(b, bag.pop())())
        if not inject:
            events = None
        k += 1
    b.checkpoint("end")  # (the steps after the last stretch)
    span = max(p.spans)
    small = 1 << int(2 * span - 1).bit_length()
    p.knobs["ring"] = small if p.knobs["small_ring"] else 1 << 20
    maxb = max(len(x) for x in p.stream)
    p.engine_kw = dict(max_batch=maxb, max_resting=b.peak + G * maxb + 4096, seq_ring=p.knobs["ring"])
    return p


def diff(a, b):
    """What the first expected output is that differs between two plans (None: none does)."""
    for i, (x, y) in enumerate(zip(a.steps, b.steps)):
        if x["op"] != y["op"]:
            return f"step {i}: {x['op']} / {y['op']}"
        if x["op"] == "stretch":
            if len(x["batches"]) != len(y["batches"]):
                return f"step {i}: batches of the stretch"
            for k, (p, q) in enumerate(zip(x["batches"], y["batches"])):
                for f in ("seq", "price_q4", "qty", "symbol", "kind"):
                    if not np.array_equal(getattr(p, f), getattr(q, f)):
                        return f"step {i}: batch {k} {f}" + (" (injected)" if k == 0 and x["inject_seq0"] else "")
            if x["launches"] != y["launches"]:
                return f"step {i}: launches"
            for k, (p, q) in enumerate(zip(x["outs"], y["outs"])):
                if not np.array_equal(p[0], q[0]) or not np.array_equal(p[1], q[1]):
                    return f"step {i}: outputs of batch {k}"
            continue
        for f, v in x.items():
            w = y[f]
            if f == "books":
                same = all(np.array_equal(v.dump(s), w.dump(s)) for s in range(S))
            elif isinstance(v, (np.ndarray, list)):
                same = np.array_equal(np.asarray(v), np.asarray(w))
            else:
                same = v == w
            if not same:
                return f"step {i}: {x['op']} {x.get('tag', '')}: {f}"
    return None if len(a.steps) == len(b.steps) else "number of steps"
