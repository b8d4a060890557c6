"""Seq-repeating cancels at stream-position boundaries — TEST INFRASTRUCTURE ONLY (numpy and the models).

A CANCEL or REDUCE record may repeat the previous record's seq instead of taking one (include/me_engine.h,
`seq_follows` in me_layout.hpp); every cancel the service sends does. A cancel of the most recently accepted
order therefore carries a seq equal to its target's. The three target lookups each have code that
depends on where such a record sits: at a launch group's start (`gw_prepare_cx`'s `T >= gmin` test, `k_seq_sweep`'s
new horizon), at a batch start inside a group (`cut`, the rest-info route), at a 64-record block start of the
symbol's bucket (`reg_cancel`'s ring hint). This module builds the inputs that put one there:

  scripted(L)      the directed cases, each with its outcomes and final books WRITTEN BY HAND: the builders
                   give every record its expected (status, reason, remaining_qty) as they emit it and keep a
                   ledger of what rests; no model is asked. Families: group_start, group_start_run,
                   group_start_limit, batch_start_in_group, block_start, sweep_start, span_edge; every case in
                   the forms "cancel", "d1" (REDUCE by 1), "dr" (REDUCE by all that is left), "d0" (REDUCE by 0).
  boundary_stream  a seeded `reduce_stream` with runs of 1-4 seq-repeating CANCEL / REDUCE records inserted at
                   every batch start and at every multiple of 64 of a symbol's bucket, their targets drawn by
                   class from a `ReduceBook` stepped beside the draws; with per-record labels.
  GroupFirstSeq, BlockSnapshot   two deliberately wrong models (tests/test_seq_edges_model.py).
  sweep_states     `k_seq_sweep`'s horizon / span arithmetic restated over the groups' seqs.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from tests import cancel_targets as ct
from tests import tif_model as tm
from tests.big_qty import Script
from tests.reduce_model import KIND_REDUCE, ReduceBook, check_seq_rule, reduce_stream, _draw_d
from tests.tif_model import TIF_FOK, TIF_IOC, Arrays, kind

BUY, SELL = 1, 2
ST_NEW, ST_PARTIAL, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
RJ_NONE, RJ_BAD_QTY, RJ_UNKNOWN = 0, 1, 5
UNK = (ST_REJECTED, RJ_UNKNOWN, 0)
BADQ = (ST_REJECTED, RJ_BAD_QTY, 0)
FORMS = ("cancel", "d1", "dr", "d0")
FAMILIES = ("group_start", "group_start_run", "group_start_limit", "batch_start_in_group", "block_start",
            "sweep_start", "span_edge")
BIG_RING = 1 << 20
SEQ_HIGH = (1 << 63) - 4096

# name, family, form; base prices, batches, groups (batches per launch group, in order), expected (per batch, per
# record: status, reason, remaining_qty), books (per symbol: seq, price, qty, side in dump order), fills (batch ->
# [(maker seq, qty)]), queries (group -> [(seq, None | (qty, orders_ahead))]), handoff (on the cancel walk: False
# none may happen, True at least one must, None not asserted), ring, pre (the boundary target is live and lies before its
# cancel's launch group), block (the family-(b) boundary), boundary (index of the group that holds the boundary)
Case = namedtuple("Case", "name family form S base batches groups expected books fills queries handoff ring pre "
                          "block boundary")


class Ctx:
    """A script and, beside it, what its author expects: every record's outcome and the ledger of resting
    orders (arrival order; `left` is written by hand wherever a record changes an order)."""

    def __init__(self, L, S=3, seq0=1):
        self.S = S
        self.base = tm.base_prices(S, L)
        self.m = [int(b) + L // 2 for b in self.base]
        self.sc = Script(seq0)
        self.exp, self.batches, self.expected, self.groups, self._g = [], [], [], [], 0
        self.ledger = {}  # seq -> [price, qty, side, symbol]
        self.fills, self.queries = {}, {}

    @property
    def n(self):
        """The last seq handed out."""
        return self.sc.next - 1

    def new(self, s, side, px, q, exp=None, rest=None, **kw):
        """A NEW record; by default a LIMIT that rests whole. exp / rest: its outcome and what it leaves resting."""
        seq = self.sc.new(s, side, px, q, **kw)
        self.exp.append(exp if exp is not None else (ST_NEW, RJ_NONE, q))
        rest = (q if exp is None else 0) if rest is None else rest
        if rest:
            self.ledger[seq] = [px, rest, side, s]
        return seq

    def cancel(self, s, target, exp):
        self.sc.cancel(s, target)
        self.exp.append(exp)

    def reduce(self, s, target, d, exp):
        self.sc.reduce(s, target, d)
        self.exp.append(exp)

    def left(self, seq, q):
        self.ledger[seq][1] = q

    def batch(self):
        self.batches.append(self.sc.take())
        self.expected.append(self.exp)
        self.exp = []
        self._g += 1

    def group(self):
        if self.sc.r:
            self.batch()
        assert self._g
        self.groups.append(self._g)
        self._g = 0

    def ask(self, seq, want):
        """After the group being built: order_query(seq) must answer want (None: not found; (qty, orders_ahead))."""
        self.queries.setdefault(len(self.groups), []).append((seq, want))

    def book(self, s):
        """The ledger as dump() orders it: bids best first, then asks best first, arrival order inside a level."""
        rows = [(q, e) for q, e in self.ledger.items() if e[3] == s and e[1] > 0]
        bids = sorted((r for r in rows if r[1][2] == BUY), key=lambda r: (-r[1][0], r[0]))
        asks = sorted((r for r in rows if r[1][2] == SELL), key=lambda r: (r[1][0], r[0]))
        return [(q, e[0], e[1], e[2]) for q, e in bids + asks]

    def case(self, name, family, form, handoff, ring=BIG_RING, pre=False, block=False, boundary=1):
        if self.sc.r or self._g:
            self.group()
        check_seq_rule(self.batches)
        return Case(name, family, form, self.S, self.base, self.batches, self.groups, self.expected,
                    {s: self.book(s) for s in range(self.S)}, self.fills, self.queries, handoff, ring, pre, block,
                    boundary)


def X(c, s, t, form, r):
    """The boundary record in its form, naming t, which holds r now (0 / None: not live for symbol s).
    Returns what t holds afterwards."""
    if form == "cancel":
        c.cancel(s, t, (ST_CANCELED, RJ_NONE, r) if r else UNK)
        return 0
    if form == "d0":
        c.reduce(s, t, 0, BADQ)
        return r or 0
    if not r:
        c.reduce(s, t, 1 if form == "d1" else 7, UNK)
        return 0
    if form == "d1":
        assert r > 1
        c.reduce(s, t, 1, (ST_NEW, RJ_NONE, r - 1))
        return r - 1
    c.reduce(s, t, r, (ST_CANCELED, RJ_NONE, r))
    return 0


def _ho(form, base=False):
    """Hand-off expectation of a case on the cancel walk: a REDUCE hands its symbol off by design."""
    return True if form != "cancel" else base


def pre(c):
    """B0 (10, symbol 0, at the price A will take, so ahead of it), B1 (20, symbol 1), B2 (30, symbol 2)."""
    m = c.m
    c.B0 = c.new(0, BUY, m[0] - 2, 10)
    c.B1 = c.new(1, BUY, m[1] - 3, 20)
    c.B2 = c.new(2, SELL, m[2] + 3, 30)


def rest_a(c):
    c.A = c.new(0, BUY, c.m[0] - 2, 7)
    return c.A


RUNS = ("single", "other_first", "twice", "wrong_right", "B_n_B", "five")  # runs of 1, 2, 2, 2, 3 and 5 records


def run(c, how, form):
    """The boundary run, all of it repeating seq n = A (7, symbol 0, behind B0). Sets the ledger by hand."""
    A = c.A
    if how == "single":
        c.left(A, X(c, 0, A, form, 7))
    elif how == "other_first":  # the target equal to the run's seq is not the run's first record
        c.cancel(1, c.B1, (ST_CANCELED, RJ_NONE, 20))
        c.left(c.B1, 0)
        c.left(A, X(c, 0, A, form, 7))
    elif how == "twice":
        r = X(c, 0, A, form, 7)
        c.left(A, X(c, 0, A, form, r))
    elif how == "wrong_right":
        X(c, 1, A, form, None)
        c.left(A, X(c, 0, A, form, 7))
    elif how == "B_n_B":
        c.cancel(0, c.B0, (ST_CANCELED, RJ_NONE, 10))
        c.left(c.B0, 0)
        c.left(A, X(c, 0, A, form, 7))
        c.cancel(0, c.B0, UNK)
    elif how == "five":  # three older targets' descriptors and two repeats through the walk's "named before" pass
        c.cancel(1, c.B1, (ST_CANCELED, RJ_NONE, 20))
        c.left(c.B1, 0)
        c.cancel(0, c.B0, (ST_CANCELED, RJ_NONE, 10))
        c.left(c.B0, 0)
        r = X(c, 0, A, form, 7)
        c.left(A, X(c, 0, A, form, r))
        c.cancel(0, c.B0, UNK)
    elif how == "mixed":  # the REDUCE hands symbol 1 off, the cancel's symbol stays on the walk
        c.reduce(1, c.B1, 5, (ST_NEW, RJ_NONE, 15))
        c.left(c.B1, 15)
        c.cancel(0, A, (ST_CANCELED, RJ_NONE, 7))
        c.left(A, 0)
    else:
        raise ValueError(how)
    q = c.ledger[A][1]
    c.ask(A, (q, 1 if c.ledger[c.B0][1] else 0) if q else None)


def taker(c, k):
    """A SELL of 12 at A's price after the boundary: B0 (10, if it rests) fills first, then what A holds."""
    b0, a = c.ledger[c.B0][1], c.ledger[c.A][1]
    got = min(12, b0 + a)
    exp = (ST_FILLED, 0, 0) if got == 12 else ((ST_PARTIAL, 0, 12 - got) if got else (ST_NEW, 0, 12))
    c.new(0, SELL, c.m[0] - 2, 12, exp=exp, rest=12 - got)
    fb = min(12, b0)
    c.fills[k] = [(q, t) for q, t in ((c.B0, fb), (c.A, got - fb)) if t]
    c.left(c.B0, b0 - fb)
    c.left(c.A, a - (got - fb))


# ---- the families --------------------------------------------------------------------------------------------------

def group_start(L, form):
    out = []
    # a one-record batch
    c = Ctx(L)
    pre(c)
    rest_a(c)
    c.group()
    run(c, "single", form)
    out.append(c.case(f"group_start one {form}", "group_start", form, _ho(form), pre=True))
    # followed by 70 ordinary records: the symbol's bucket spans two 64-blocks
    c = Ctx(L)
    pre(c)
    c.batch()
    rest_a(c)
    c.group()
    run(c, "single", form)
    for j in range(70):
        if j % 16:
            c.new(0, BUY, c.m[0] - 8 - j % 2, 1 + j % 3)
        else:
            s = 1 + (j // 16) % 2
            c.new(s, BUY if s == 1 else SELL, c.m[s] + (-8 if s == 1 else 8), 2)
    c.batch()
    c.new(1, BUY, c.m[1] - 8, 2)
    out.append(c.case(f"group_start seventy {form}", "group_start", form, _ho(form), pre=True))
    # followed by a taker at A's price
    c = Ctx(L)
    pre(c)
    rest_a(c)
    c.group()
    run(c, "single", form)
    c.group()
    taker(c, 2)
    out.append(c.case(f"group_start taker {form}", "group_start", form, _ho(form), pre=True))
    return out


NEVER = ("market", "ioc", "fok", "filled", "rejected")


def group_start_run(L, form):
    out = []
    for how in RUNS[1:]:
        c = Ctx(L)
        pre(c)
        rest_a(c)
        c.group()
        run(c, how, form)
        c.group()
        taker(c, 2)
        out.append(c.case(f"group_start_run {how} {form}", "group_start_run", form, _ho(form), pre=True))
    for what in NEVER:  # seq n never rested: UNKNOWN every time
        c = Ctx(L)
        pre(c)
        m0 = c.m[0]
        if what == "market":
            t = c.new(0, SELL, 0, 4, exp=(ST_FILLED, 0, 0), market=True)
            c.left(c.B0, 6)
        elif what == "ioc":
            t = c.new(0, BUY, m0 - 6, 5, exp=(ST_CANCELED, 0, 5), tif=TIF_IOC)
        elif what == "fok":
            t = c.new(0, SELL, m0 - 2, 50, exp=(ST_CANCELED, 0, 50), tif=TIF_FOK)
        elif what == "filled":
            t = c.new(0, SELL, m0 - 2, 3, exp=(ST_FILLED, 0, 0))
            c.left(c.B0, 7)
        else:
            t = c.new(0, BUY, m0 - 1, 0, exp=BADQ)
        c.group()
        X(c, 0, t, form, None)
        c.ask(t, None)
        # (the FOK hands symbol 0 off in the first group: the counter is read around the boundary group only)
        out.append(c.case(f"group_start_run never {what} {form}", "group_start_run", form, _ho(form)))
    if form == "cancel":
        c = Ctx(L)
        pre(c)
        rest_a(c)
        c.group()
        run(c, "mixed", form)
        out.append(c.case("group_start_run mixed", "group_start_run", "mixed", True, pre=True))
    return out


def group_start_limit(L, form):
    out = []
    c = Ctx(L)
    pre(c)
    rest_a(c)
    c.group()
    N = c.new(0, BUY, c.m[0] - 1, 5)
    c.left(N, X(c, 0, N, form, 5))
    c.ask(N, (c.ledger[N][1], 0) if c.ledger[N][1] else None)
    c.ask(c.A, (7, 1))
    out.append(c.case(f"group_start_limit same {form}", "group_start_limit", form, _ho(form)))
    # the group's first record is another symbol's LIMIT; this symbol's first record repeats its seq, so the
    # two have one record number in their symbols' buckets
    c = Ctx(L)
    pre(c)
    rest_a(c)
    c.group()
    N = c.new(0, BUY, c.m[0] - 1, 5)
    c.cancel(1, c.B1, (ST_CANCELED, RJ_NONE, 20))
    c.left(c.B1, 0)
    X(c, 1, N, form, None)
    c.ask(N, (5, 0))
    out.append(c.case(f"group_start_limit other_symbol {form}", "group_start_limit", form, _ho(form)))
    return out


def _in_group(L, form, G, b, how):
    """A group of G batches; A is the last record of batch b (b = -1: of the group before, whose place a
    batch of one cancel takes), batch b + 1 starts with the run; then the cancels of the symbol-0 orders the
    group's earlier batches rested (one, two, three ... batches back)."""
    c = Ctx(L)
    pre(c)
    if b < 0:
        rest_a(c)
    c.group()
    cs = []
    if b < 0:
        c.cancel(2, c.B2, (ST_CANCELED, RJ_NONE, 30))
        c.left(c.B2, 0)
        c.batch()
    for k in range(b + 1):
        cs.append(c.new(0, SELL, c.m[0] + 4 + k, 3))
        c.new(1, BUY, c.m[1] - 8, 2)
        if k == b:
            rest_a(c)
        c.batch()
    run(c, how, form)
    for t in cs:
        c.cancel(0, t, (ST_CANCELED, RJ_NONE, 3))
        c.left(t, 0)
    c.new(2, SELL, c.m[2] + 8, 2)
    c.batch()
    while c._g < G:
        c.new(1, BUY, c.m[1] - 8, 2)
        c.batch()
    c.group()
    taker(c, len(c.batches))
    return c.case(f"batch_start_in_group G={G} b={b} {how} {form}", "batch_start_in_group", form, _ho(form),
                  pre=b < 0)


def batch_start_in_group(L, form):
    return [_in_group(L, form, G, b, how) for G in (4, 8) for b in (-1, 0, 1, G - 2) for how in RUNS]


def block_start(L, form):
    """In one batch A is symbol 0's P-th record and the boundary record its (P + 1)-th."""
    out = []
    for P in (64, 63, 127):
        for mixed in (False, True):
            c = Ctx(L)
            pre(c)
            c.group()
            for j in range(P - 1):
                c.new(0, BUY if j % 2 else SELL, c.m[0] + (-8 - j % 3 if j % 2 else 8 + j % 3), 1 + j % 3)
                if mixed:
                    s = 1 + j % 2
                    c.new(s, BUY if s == 1 else SELL, c.m[s] + (-8 if s == 1 else 8), 2)
            rest_a(c)
            run(c, "single", form)
            for j in range(3):
                c.new(1, BUY, c.m[1] - 12, 2)
            c.group()
            taker(c, 2)
            out.append(c.case(f"block_start P={P}{' interleaved' if mixed else ''} {form}", "block_start", form,
                              _ho(form), block=True))
    return out


SWEEP_R = 64


def _fill16(c, n=16):
    for j in range(n):
        s = j % 3
        c.new(s, BUY if j % 2 else SELL, c.m[s] + (-9 - j % 4 if j % 2 else 9 + j % 4), 1 + j % 3)


def sweep_start(L, form):
    """seq_ring = 64, batches of 16 records, one per launch group. A is the last record of a batch whose
    successor forces k_seq_sweep's rebuild, so the new horizon is the boundary cancel's seq and target."""
    out = []
    for old in (False, True):
        c = Ctx(L, seq0=SEQ_HIGH)
        pre(c)
        _fill16(c, 13)
        c.group()
        for _ in range(14 if old else 2):
            _fill16(c)
            c.group()
        _fill16(c, 15)
        rest_a(c)
        c.group()
        if old:  # B0 is more than three rings old: the old-order table; the run's other cancel names gmin
            assert c.A - c.B0 > 3 * SWEEP_R
            c.cancel(0, c.B0, (ST_CANCELED, RJ_NONE, 10))
            c.left(c.B0, 0)
        c.left(c.A, X(c, 0, c.A, form, 7))
        c.ask(c.A, (c.ledger[c.A][1], 0 if old else 1) if c.ledger[c.A][1] else None)
        _fill16(c, 15)
        c.group()
        taker(c, len(c.batches))
        out.append(c.case(f"sweep_start {'old ' if old else ''}{form}", "sweep_start", form, _ho(form), ring=SWEEP_R,
                          pre=True, boundary=len(c.groups) - 1))
    return out


def span_edge(L, form):
    """A group that opens with the repeating cancel and spans exactly seq_ring - 1 seqs from the repeated one."""
    c = Ctx(L, seq0=(1 << 40) + 7)
    pre(c)
    rest_a(c)
    c.group()
    run(c, "single", form)
    _fill16(c, 15)
    c.batch()
    for _ in range(3):
        _fill16(c)
        c.batch()
    c.group()
    assert c.n - c.A == SWEEP_R - 1
    taker(c, len(c.batches))
    return [c.case(f"span_edge {form}", "span_edge", form, _ho(form), ring=SWEEP_R, pre=True)]


BUILDERS = {"group_start": group_start, "group_start_run": group_start_run, "group_start_limit": group_start_limit,
            "batch_start_in_group": batch_start_in_group, "block_start": block_start, "sweep_start": sweep_start,
            "span_edge": span_edge}


@functools.lru_cache(maxsize=None)
def scripted(L):
    """Every scripted case at window depth L (the base prices depend on it). Shared: nobody changes the arrays."""
    return tuple(cs for fam in FAMILIES for form in FORMS for cs in BUILDERS[fam](L, form))


def sweep_states(groups_seqs, R, horizon=0):
    """k_seq_sweep's arithmetic over the launch groups' (first seq, last seq): per group (sweep due, span
    accepted, the horizon the group's matching reads)."""
    out = []
    for gmin, gmax in groups_seqs:
        need = gmax - horizon >= R
        horizon = gmin if need else horizon
        out.append((need, gmax - gmin < R, horizon))
    return out


def group_seqs(case):
    """(first seq, last seq) of every launch group of a case."""
    out, k = [], 0
    for g in case.groups:
        out.append((int(case.batches[k].seq[0]), int(case.batches[k + g - 1].seq[-1])))
        k += g
    return out


# ---- the two wrong models ---------------------------------------------------------------------------------------

class _PerRecord(ReduceBook):
    """ReduceBook stepped record by record, a subclass deciding per CANCEL / REDUCE whether it sees its target."""

    def at(self, s, kd):
        pass

    def sees(self, s, tgt):
        return True

    def note(self, seq, s, kd, rested):
        pass

    def submit(self, b):
        res, tapes, nt = [], [], 0
        for i in range(len(b.seq)):
            one = ct.one(b, i)
            s, kd, tgt = int(b.symbol[i]), int(b.kind[i]), int(b.price_q4[i]) & ((1 << 64) - 1)
            self.at(s, kd)
            if (kd & 8) and s < self.S and not self.sees(s, tgt):
                one = Arrays(one.seq, [ct.to_i64((1 << 64) - 3)], one.qty, one.symbol, one.kind)  # (never an order's seq)
            r, f = super().submit(one)
            r["tape_offset"] += nt
            nt += len(f)
            res.append(r)
            tapes.append(f)
            if not (kd & 8):
                self.note(int(b.seq[i]), s, kd, int(b.seq[i]) in self.live)
        return np.concatenate(res), np.concatenate(tapes)


class GroupFirstSeq(_PerRecord):
    """Wrong model (a): a target T >= the first seq of the current launch group is looked up only among that
    group's earlier records. `start_group(first_seq)` before every launch group."""

    def __init__(self, S):
        super().__init__(S)
        self.gmin, self.mine = 0, set()

    def start_group(self, first_seq):
        self.gmin, self.mine = int(first_seq), set()

    def sees(self, s, tgt):
        return tgt < self.gmin or tgt in self.mine

    def note(self, seq, s, kd, rested):
        self.mine.add(seq)


class BlockSnapshot(_PerRecord):
    """Wrong model (b): the block-start snapshot, taken one record early. A cancel at position p >= 63 of its
    symbol's bucket sees only orders that rested before bucket position 64 * ((p - 1) // 64) of its batch;
    buckets shorter than a block are exact. `start_batch()` before every batch.

    The literal model — a cancel sees only orders that rested before its symbol's current 64-record block —
    fails the families both ways: with the target the bucket's 64th record and its cancel the 65th the target
    lies in the block before and is seen, so the model agrees with ReduceBook on that block_start case; and it
    hides every target of the cancel's own block, so it differs on group_start_limit, whose LIMIT and cancel
    are records 0 and 1 of one bucket. Taking the snapshot one record early catches the first; leaving buckets
    of fewer than 63 records exact spares the second."""

    def __init__(self, S):
        super().__init__(S)
        self.start_batch()

    def start_batch(self):
        self.pos = {}    # symbol -> records of the batch so far
        self.where = {}  # seq -> bucket position of the batch's records
        self.p = 0

    def at(self, s, kd):
        self.p = self.pos.get(s, 0)
        self.pos[s] = self.p + 1

    def sees(self, s, tgt):
        if self.p < 63 or tgt not in self.where:
            return True
        return self.where[tgt] < 64 * ((self.p - 1) // 64)

    def note(self, seq, s, kd, rested):
        self.where[seq] = self.p


def run_model(model, case):
    """A case through a model, launch group by launch group: per batch (results, fills)."""
    out, k = [], 0
    for g in case.groups:
        if hasattr(model, "start_group"):
            model.start_group(case.batches[k].seq[0])
        for b in case.batches[k:k + g]:
            if hasattr(model, "start_batch"):
                model.start_batch()
            out.append(model.submit(b))
        k += g
    return out


def outcomes(res):
    return [(int(r["status"]), int(r["reason"]), int(r["remaining_qty"])) for r in res]


def book_rows(dump):
    return [(int(e["seq"]), int(e["price_q4"]), int(e["qty"]), int(e["side"])) for e in dump]


# ---- the seeded overlay ------------------------------------------------------------------------------------------

# the overlay's shape in the CPU and the GPU tests: symbols, batches, stream records per batch, stream keywords
# (more resting LIMITs than tif_stream's default mix, close to the mid; no skew and no far LIMITs, so that nearly
# every symbol's bucket passes 64 records and hardly one passes the walks' 128)
OS, ONB, ON = 8, 16, 768
OVERLAY_KW = dict(mix=(60, 8, 4, 8, 5, 15), spread=5)


OVERLAY_HIGH = (1 << 40) + 3


def overlay_seed(L, seed):
    return 9100 + 10 * L + seed


@functools.lru_cache(maxsize=None)
def overlay_stream(L, seed, plain=False, high=False):
    """(base, batches, labels) of the overlay as the GPU tests run it (high: seqs from OVERLAY_HIGH, for the small
    ring). Shared: nobody changes the arrays."""
    kw = dict(OVERLAY_KW, seq_start=OVERLAY_HIGH) if high else OVERLAY_KW
    return boundary_stream(overlay_seed(L, seed), OS, L, ONB, ON, 1, plain=plain, **kw)


KINDS = ("batch_start", "block_start")
TARGETS = ("own_seq", "older_same", "other_symbol", "dead", "twice")
NLAB = len(KINDS) * len(TARGETS)


def label(kd, tg):
    return KINDS.index(kd) * len(TARGETS) + TARGETS.index(tg)


def boundary_stream(seed, S, L, nbatches, batch, group, plain=False, **kw):
    """(base, batches, labels): the records of `reduce_stream(seed, S, L, nbatches, batch, **kw)` with runs of
    1-4 CANCEL / REDUCE records that repeat the last seq inserted at every batch start and before every record
    that would take a position of its symbol's bucket that is a multiple of 64 (the run takes those positions).
    A ReduceBook is stepped beside the draws.

    Batches are cut anew: each ends at the first NEW record at or past `batch` stream records that leaves an order
    of at least 2 resting (so that the run's first two own_seq records both succeed), so the run that opens the next batch (and the next launch group) can name an order whose seq it
    repeats. Such a run is [own_seq, one of older_same / other_symbol / dead in turn, own_seq, twice]: REDUCEs
    by 1 while the order holds more, a CANCEL last, the last record dropped three times in ten — the floors of
    tests/test_seq_edges_model.py need two to three successes per batch start. A block-start run draws its
    length, classes and forms; its symbol is the bucket's, except that own_seq takes the last NEW record's.

    Target classes, judged at the record: own_seq (the last NEW record's seq), older_same (another live order
    of the symbol), other_symbol (a live order of another symbol), dead (not live: cancelled, filled or never
    rested), twice (the run's previous target again). labels: per batch an int8 array, -1 on the stream's own
    records, else label(boundary kind, target class). `group` only names the grouping the stream is meant for
    (boundary_successes counts against it). plain: no REDUCE and no time-in-force bits anywhere, every boundary
    record a CANCEL — the vocabulary OracleBook and PyBook share, and streams whose symbols the cancel walk keeps."""
    rng = np.random.default_rng(seed * 104729 + 71)
    if plain:
        kw = dict(kw, convert_pct=0, fresh_pct=0)
    base, src = reduce_stream(seed, S, L, nbatches, batch, **kw)
    cols = [np.concatenate([getattr(b, f) for b in src]) for f in ("seq", "price_q4", "qty", "symbol", "kind")]
    if plain:
        cols[4] = cols[4] & 0x0F
    book = ReduceBook(S)
    max_qty = kw.get("max_qty", 60)
    dead = [1 << 50]  # seqs that are not live
    st = {"last_new": 0, "last_sym": 0, "turn": 0}
    out, labels = [], []
    o, lab, cnt = ([], [], [], [], []), [], [0] * S
    pend = ([], [], [], [], [])

    def flush():
        if pend[0]:
            book.submit(Arrays(*pend))
            for x in pend:
                x.clear()

    def emit(rec, lb):
        for dst in (o, pend):
            for k in range(5):
                dst[k].append(rec[k])
        lab.append(lb)
        if rec[3] < S:
            cnt[rec[3]] += 1

    def held(t, sym):
        flush()
        hit = book.live.get(t)
        return hit[3][1] if hit is not None and hit[0] == sym else None

    def pick(cls, s, prev):
        """(class, target, symbol) — `dead` where the class has no candidate."""
        last = st["last_new"]
        t, sym = None, s
        if cls == "own_seq":
            t, sym = last, st["last_sym"] if st["last_sym"] < S else s
        elif cls == "older_same":
            old = [q for q, h in book.live.items() if h[0] == s and q != last]
            t = old[int(rng.integers(len(old)))] if old else None
        elif cls == "other_symbol":
            oth = [q for q, h in book.live.items() if h[0] != s]
            t = oth[int(rng.integers(len(oth)))] if oth else None
        elif cls == "twice" and prev:
            t, sym = prev
        if t is None:
            cls, t = "dead", dead[int(rng.integers(max(len(dead) - 50, 0), len(dead)))]
        return cls, t, sym

    def one(kd, cls, s, prev, d=None):
        flush()
        cls, t, sym = pick(cls, s, prev)
        r = held(t, sym)
        if plain:
            red = False
        elif d is None:
            d = _draw_d(rng, r, max_qty) if rng.integers(100) < 40 else 0
            red = d != 0 or bool(rng.integers(2))
        else:
            red = d > 0
        emit((st["last_new"], ct.to_i64(t), d if red else 0, sym, KIND_REDUCE if red else kind(BUY, 0, 1)),
             label(kd, cls))
        if r is not None and held(t, sym) is None:
            dead.append(t)
        return t, sym

    def insert(kd, s):
        if not st["last_new"]:
            return
        if kd == "batch_start":
            own = lambda last: 1 if not last and (held(st["last_new"], s) or 0) > 1 else -1  # noqa: E731  (-1: a CANCEL)
            drop = rng.random() < 0.3
            prev = one(kd, "own_seq", s, None, own(False))
            prev = one(kd, ("older_same", "other_symbol", "dead")[st["turn"] % 3], s, prev)
            st["turn"] += 1
            prev = one(kd, "own_seq", s, prev, own(drop))
            if not drop:
                one(kd, "twice", s, prev, -1)
            return
        prev = None
        for _ in range(int(rng.integers(1, 5))):
            prev = one(kd, TARGETS[int(rng.choice(len(TARGETS), p=(0.3, 0.2, 0.15, 0.15, 0.2)))], s, prev)

    def cut():
        flush()
        out.append(Arrays(*o))
        labels.append(np.array(lab, dtype=np.int8))
        for x in o:
            x.clear()
        lab.clear()
        for k in range(S):
            cnt[k] = 0

    n, taken = len(cols[0]), 0
    for i in range(n):
        rec = tuple(int(c[i]) for c in cols)
        s = rec[3]
        if not o[0] and out:  # a batch start: the run names the order the last batch ended with
            insert("batch_start", st["last_sym"])
        if s < S and cnt[s] and cnt[s] % 64 == 0:
            insert("block_start", s)
        emit(rec, -1)
        taken += 1
        if not (rec[4] & 8) and rec[0]:
            flush()
            if st["last_new"] and st["last_new"] not in book.live:
                dead.append(st["last_new"])
            st["last_new"], st["last_sym"] = rec[0], s
            if taken >= batch and len(out) + 1 < nbatches and s < S and (held(rec[0], s) or 0) >= 2:
                cut()
                taken = 0
    if o[0]:
        cut()
    check_seq_rule(out)
    return base, out, labels


def boundary_successes(batches, labels, group, S, per_start=False):
    """From ReduceBook alone: how many boundary records of a draw succeed (CANCELED, or NEW for a partial
    REDUCE) with target == own seq == the first seq of their launch group at group size `group`. per_start: the
    list of these counts per launch group after the first (whose opening run has no earlier order to name)."""
    book, per = ReduceBook(S), []
    for k, (b, lab) in enumerate(zip(batches, labels)):
        res, _ = book.submit(b)
        if k % group == 0:
            gmin = int(b.seq[0])
            per.append(0)
        for i in np.nonzero(lab >= 0)[0]:
            t = int(b.price_q4[i]) & ((1 << 64) - 1)
            if t == int(b.seq[i]) == gmin and int(res[i]["status"]) in (ST_CANCELED, ST_NEW):
                per[-1] += 1
    return per[1:] if per_start else sum(per)
