"""me_order_query (k_order_query) on every matching path against the model
(tests/order_query_model.py): after every synchronous batch, every seq the stream has used so far plus the dead
ones is queried and every field of every answer compared. Needs an MI355X. Everything is exact.

The query kernel itself is the same on every path; what differs is who wrote the book it reads (the register
window kernel, the grouped walks and their resolve, the deep generic kernel, the hot walks) and the window
depth: L <= 128 adds up level totals, deeper windows go through the occupancy words.
"""
import collections
import functools

import numpy as np
import pytest

from tests import book_audit
from tests import order_query_model as oq
from tests import reduce_model as rm
from tests import tif_model as tm
from tests._parity import assert_books_equal, assert_fills_equal, assert_results_equal
from tests.big_qty import Script
from tests.gpu_harness import PATHS, as_batch, engine_on
from tests.reduce_model import INT32_MAX, ReduceBook
from tests.tif_model import TIF_IOC, kind

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
ALL = tuple(PATHS)
GROUPED = tuple(p for p in PATHS if PATHS[p][3])
U64_MAX = 2**64 - 1
# tif_stream keywords: mostly GTC LIMITs within five ticks of the mid, so that books grow to a few hundred orders
# and levels to more than one chunk (the default mix leaves some 60 orders resting, five to a level at most)
DEEP_BOOKS = dict(mix=(70, 4, 3, 6, 5, 12), spread=5)


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _kw(path, group=1):
    return {"batches_per_launch": group} if PATHS[path][3] else {}


def _dead(last):
    """Seqs no order ever had: 0, the stream's next, a few beyond, 2^63 and its neighbours, 2^64 - 1."""
    return [0, last + 1, last + 64, last + 12345, 1 << 63, (1 << 63) + 5, U64_MAX - 1, U64_MAX]


def _ask(eng, model, S, seqs, ctx, symbol_ids=None):
    q = np.array([int(x) for x in seqs], dtype=np.uint64)
    got = eng.order_query(q)
    oq.assert_answers_equal(got, oq.expected(model, S, q, symbol_ids), ctx)
    return {int(r["seq"]): r for r in got}


class Run:
    """An engine and the model beside it; step() is one synchronous batch, checked, then the query of every seq
    used so far plus the dead ones."""

    def __init__(self, me, eng, S, model=None, symbol_ids=None):
        self.me, self.eng, self.S = me, eng, S
        self.model = model or ReduceBook(S)
        self.ids = symbol_ids
        self.used = set()

    def step(self, a, ctx, extra=()):
        r, f = self.eng.submit_batch(as_batch(self.me, a))
        ro, fo = self.model.submit(a)
        assert_results_equal(r, ro, ctx)
        assert_fills_equal(f, fo, ctx)
        self.used.update(int(x) for x in a.seq)
        return ro, self.ask(ctx, extra)

    def ask(self, ctx, extra=()):
        last = max(self.used)
        return _ask(self.eng, self.model, self.S, sorted(self.used) + _dead(last) + list(extra), ctx, self.ids)

    def books(self, ctx):
        assert_books_equal(self.eng, self.model, range(self.S), ctx)
        v, _ = book_audit.audit(self.eng.debug_export(), last_seq=max(self.used))
        assert not v, f"{ctx}: {v[:3]}"


def _own_seq_cancel(sc, s, target):
    """A cancel record that takes a seq of its own (a cancel's seq may also exceed the previous record's)."""
    sc.r.append((sc.next, int(target), 0, s, kind(BUY, 0, 1)))
    sc.next += 1
    return sc.next - 1


def _pos(r):
    return (int(r["found"]), int(r["qty"]), int(r["qty_ahead"]), int(r["orders_ahead"]), int(r["level_qty"]))


# ---- chunks: the walk back through a level's FIFO -------------------------------------------------------------------

@pytest.mark.parametrize("path", ALL)
def test_chunks_and_dead_seqs(me, path):
    L, S = PATHS[path][0], 4
    base = tm.base_prices(S, L)
    p = int(base[0]) + L // 2 - 3
    m1 = int(base[1]) + L // 2
    sc = Script()
    o = [None] + [sc.new(0, BUY, p, 10) for _ in range(40)]  # o[1..40]: chunks 1-16, 17-32, 33-40
    low = [sc.new(0, BUY, p - 2, 7) for _ in range(2)]
    s1_ask, s1_bid = sc.new(1, SELL, m1 + 1, 5), sc.new(1, BUY, m1 - 1, 5)
    for s in (2, 3):
        sc.new(s, SELL, int(base[s]) + L // 2 + 1, 5)
        sc.new(s, BUY, int(base[s]) + L // 2 - 1, 6)
    mkt = sc.new(1, BUY, 0, 2, market=True)          # takes 2 of s1_ask: found, holding 3
    ioc = sc.new(1, BUY, m1 - 5, 3, tif=TIF_IOC)      # crosses nothing: discarded
    script = [sc.take()]
    sc.cancel(0, o[3])
    for j in range(17, 33):
        sc.cancel(0, o[j])                             # the middle chunk is unlinked
    sc.cancel(0, o[40])
    cx_seq = _own_seq_cancel(sc, 0, o[39])             # a cancel record with a seq of its own
    script.append(sc.take())
    sc.reduce(0, o[5], 4)
    script.append(sc.take())
    taker = sc.new(0, SELL, p, 15)                     # o[1] 10 (filled), o[2] 5 of 10
    script.append(sc.take())
    sc.reduce(0, o[6], 100)                            # reduced to nothing
    script.append(sc.take())
    with engine_on(me, path, S, base, script, **_kw(path)) as eng:
        run = Run(me, eng, S)
        _, a0 = run.step(script[0], f"chunks {path} build")
        assert [_pos(a0[o[j]]) for j in (1, 16, 17, 33, 40)] == [
            (1, 10, 0, 0, 400), (1, 10, 150, 15, 400), (1, 10, 160, 16, 400), (1, 10, 320, 32, 400), (1, 10, 390, 39, 400)]
        assert (int(a0[low[1]]["levels_better"]), int(a0[low[1]]["qty_better"]), int(a0[low[1]]["qty_ahead"])) == (1, 400, 7)
        assert _pos(a0[s1_ask])[:2] == (1, 3) and int(a0[s1_ask]["symbol"]) == 1 and int(a0[s1_ask]["side"]) == SELL
        assert not int(a0[mkt]["found"]) and not int(a0[ioc]["found"])
        _, a1 = run.step(script[1], f"chunks {path} cancels")
        # 40 - 1 - 16 - 1 - 1 = 21 orders: head chunk 1, 2, 4..16, tail chunk 33..38
        assert [_pos(a1[o[j]]) for j in (2, 4, 16, 33, 38)] == [
            (1, 10, 10, 1, 210), (1, 10, 20, 2, 210), (1, 10, 140, 14, 210), (1, 10, 150, 15, 210), (1, 10, 200, 20, 210)]
        assert not any(int(a1[x]["found"]) for x in [o[3], o[40], o[39], cx_seq] + o[17:33])
        _, a2 = run.step(script[2], f"chunks {path} reduce")
        assert _pos(a2[o[5]]) == (1, 6, 30, 3, 206)
        for j in [4] + list(range(7, 17)) + list(range(33, 39)):  # behind it: exactly d less ahead, as many orders
            d = 0 if j == 4 else 4
            assert int(a2[o[j]]["qty_ahead"]) == int(a1[o[j]]["qty_ahead"]) - d, j
            assert int(a2[o[j]]["orders_ahead"]) == int(a1[o[j]]["orders_ahead"]), j
        _, a3 = run.step(script[3], f"chunks {path} partial fill")
        assert not int(a3[o[1]]["found"]) and not int(a3[taker]["found"])
        assert _pos(a3[o[2]]) == (1, 5, 0, 0, 191) and _pos(a3[o[4]]) == (1, 10, 5, 1, 191)
        _, a4 = run.step(script[4], f"chunks {path} reduced to nothing")
        assert not int(a4[o[6]]["found"]) and _pos(a4[o[7]]) == (1, 10, 21, 3, 181)
        run.books(f"chunks {path}")


# ---- the number of queries --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["reg", "deep"])
def test_query_counts_and_arguments(me, path):
    L, S = PATHS[path][0], 8
    base, arrays = rm.reduce_stream(777, S, L, 3, 512, far_pct=3, skew=True, **DEEP_BOOKS)
    model = ReduceBook(S)
    with engine_on(me, path, S, base, arrays, **_kw(path)) as eng:
        for a in arrays:
            eng.submit_batch(as_batch(me, a))
            model.submit(a)
        used = sorted({int(x) for a in arrays for x in a.seq})
        pool = np.array(used + _dead(used[-1]) + [used[-1] + 2 + 3 * i for i in range(32)], dtype=np.uint64)
        rng = np.random.default_rng(5)
        assert model.resting() > 100
        for n in (1, 3, 5, 64, 257, 70_000):
            q = pool[rng.integers(0, len(pool), n)]
            got = eng.order_query(q)
            oq.assert_answers_equal(got, oq.expected(model, S, q), f"counts {path} n={n}")
            if n >= 257:
                assert 0 < int(got["found"].sum()) < n
        assert len(eng.order_query([])) == 0
        lib, h = eng.lib, eng.h
        assert lib.me_order_query(h, None, 0, None) == me.ME_OK
        one = np.array([used[0]], dtype=np.uint64)
        out = np.zeros(1, dtype=me.ORDER_INFO_DTYPE)
        assert lib.me_order_query(h, None, 1, out.ctypes.data) == me.ME_E_INVALID
        assert lib.me_order_query(h, one.ctypes.data, 1, None) == me.ME_E_INVALID
        assert lib.me_order_query(h, one.ctypes.data, (1 << 24) + 1, out.ctypes.data) == me.ME_E_INVALID
        # none of that failed the engine
        oq.assert_answers_equal(eng.order_query(one), oq.expected(model, S, one), f"counts {path} after the refusals")
        assert_books_equal(eng, model, range(S), f"counts {path}")


# ---- far levels and a re-centre ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ALL)
def test_far_levels_and_a_recentre(me, path):
    L, S = PATHS[path][0], 2
    base = tm.base_prices(S, L)
    b0 = int(base[0])
    m = b0 + L // 2
    sc = Script()
    fb, fa = [], []
    for k in range(10):  # ten prices beyond the window on each side, two orders on every other one
        fb.append(sc.new(0, BUY, b0 - 10 * (k + 1), 20 + k))
        fa.append(sc.new(0, SELL, b0 + L - 1 + 10 * (k + 1), 30 + k))
        if k % 2:
            fb.append(sc.new(0, BUY, b0 - 10 * (k + 1), 3))
            fa.append(sc.new(0, SELL, b0 + L - 1 + 10 * (k + 1), 4))
    wb = [sc.new(0, BUY, m - 1, 5), sc.new(0, BUY, m - 1, 6), sc.new(0, BUY, m - 4, 7)]
    wa = [sc.new(0, SELL, m + 1, 8), sc.new(0, SELL, m + 3, 9)]
    sc.new(1, BUY, int(base[1]) + 3, 5)
    build = sc.take()
    # a bid above the window: it takes both window asks (17) and rests 3 at a price below the first far ask, so
    # the window re-centres around it; the old window's bids become far levels, far asks come into the window
    mover = sc.new(0, BUY, b0 + L + 5, 20)
    move = sc.take()
    with engine_on(me, path, S, base, [build, move], far_levels=4, **_kw(path)) as eng:
        run = Run(me, eng, S)
        _, a0 = run.step(build, f"far {path} build")
        assert eng.far_stats()["moves"] > 0  # ten levels in regions of four: the sides moved to the arena
        # a far order counts every window level of its side as better
        r = a0[fb[0]]
        assert (int(r["side"]), int(r["price_q4"]), int(r["levels_better"]), int(r["qty_better"])) == (BUY, b0 - 10, 2, 18)
        r = a0[fa[3]]  # the third far ask level (two orders on the second)
        assert (int(r["side"]), int(r["price_q4"]), int(r["levels_better"]), int(r["qty_better"]), int(r["level_qty"])) == \
            (SELL, b0 + L - 1 + 30, 4, 8 + 9 + 30 + 31 + 4, 32)
        r = a0[fb[2]]  # the second order of the second far bid level
        assert (int(r["qty_ahead"]), int(r["orders_ahead"]), int(r["level_qty"]), int(r["levels_better"])) == (21, 1, 24, 3)
        assert (int(a0[wb[2]]["levels_better"]), int(a0[wb[2]]["qty_better"])) == (1, 11)
        raw0 = eng.debug_export()
        _, a1 = run.step(move, f"far {path} re-centre")
        raw1 = eng.debug_export()
        assert int(raw1["sym"]["base"][0]) != int(raw0["sym"]["base"][0]), "the window did not move"
        assert int(a1[mover]["found"]) and int(a1[mover]["qty"]) == 3 and not int(a1[wa[0]]["found"])
        for x in fa:  # the asks: both window levels are gone, nothing else changed
            assert int(a1[x]["levels_better"]) == int(a0[x]["levels_better"]) - 2
            assert int(a1[x]["qty_better"]) == int(a0[x]["qty_better"]) - 17
            assert _pos(a1[x]) == _pos(a0[x])
        for x in fb + wb:  # the bids: one better level more, the same places
            assert int(a1[x]["levels_better"]) == int(a0[x]["levels_better"]) + 1
            assert int(a1[x]["qty_better"]) == int(a0[x]["qty_better"]) + 3
            assert _pos(a1[x]) == _pos(a0[x])
        run.books(f"far {path}")


# ---- the seq ring and the old-order table -------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ALL)
def test_ring_and_old_table(me, path):
    """seq_ring = 64, seqs just below 2^63: orders rest, the stream moves on by several rings (16 records per
    batch, so a launch group spans fewer than 64 seqs), and a later order takes the ring entry of a live older one."""
    L, S, R = PATHS[path][0], 2, 64
    base = tm.base_prices(S, L)
    m0, m1 = int(base[0]) + L // 2, int(base[1]) + L // 2
    sc = Script((1 << 63) - 4096)
    A, A2 = sc.new(0, BUY, m0 - 5, 9), sc.new(0, SELL, m0 + 5 * L, 12)  # (A2 on a far level)
    P = sc.new(1, BUY, m1 - 7, 11)
    script = [sc.take()]

    def fillers(n):
        for j in range(n):
            sc.new(1 if j % 4 else 0, BUY if j % 2 else SELL, (m1 if j % 4 else m0) + (-2 if j % 2 else 2), 1 + j % 3)

    while sc.next + 16 <= P + 3 * R:
        fillers(16)
        script.append(sc.take())
    fillers(P + 3 * R - sc.next)
    Q = sc.new(1, BUY, m1 - 7, 13)  # the same ring entry as P, the same level, behind it
    assert Q == P + 3 * R and (Q & (R - 1)) == (P & (R - 1))
    script.append(sc.take())
    pair_at = len(script) - 1
    sc.cancel(1, P)
    script.append(sc.take())
    sc.cancel(1, Q)
    script.append(sc.take())
    for _ in range(6):  # and on: the table is rebuilt again with A, A2 and the fillers in it
        fillers(16)
        script.append(sc.take())
    sc.reduce(0, A, 4)
    sc.reduce(0, A2, 11)
    script.append(sc.take())
    with engine_on(me, path, S, base, script, ring=R, **_kw(path)) as eng:
        run = Run(me, eng, S)
        for k, a in enumerate(script):
            _, ans = run.step(a, f"ring {path} batch {k}", extra=[P + R, P + 2 * R, A + 7 * R])
            if k == pair_at:  # both live: P through the table, Q through the ring
                assert _pos(ans[P]) == (1, 11, 0, 0, 24) and _pos(ans[Q]) == (1, 13, 11, 1, 24)
            if k == pair_at + 1:
                assert not int(ans[P]["found"]) and _pos(ans[Q]) == (1, 13, 0, 0, 13)
            if k == pair_at + 2:
                assert not int(ans[P]["found"]) and not int(ans[Q]["found"])
        assert _pos(ans[A])[:2] == (1, 5) and _pos(ans[A2])[:2] == (1, 1)
        raw = eng.debug_export()
        sq = raw["sq"][raw["info"]["sq_idx"]]
        assert int(sq["horizon"]) > A2 and int(sq["epoch"]) > 1, "the old-order table was never rebuilt"
        run.books(f"ring {path}")


# ---- int64 quantities, symbol ids ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ALL)
def test_int64_quantities_and_symbol_ids(me, path):
    L, S = PATHS[path][0], 3
    base = tm.base_prices(S, L)
    ids = [70_000, 5, 4_000_000_000]
    p = int(base[2]) + L // 2 - 2
    sc = Script()
    hi = [sc.new(2, BUY, p, INT32_MAX) for _ in range(3)]
    lo = [sc.new(2, BUY, p - 1, INT32_MAX) for _ in range(3)]
    far = sc.new(2, BUY, int(base[2]) - 3 * L, INT32_MAX)
    sc.new(0, SELL, int(base[0]) + 9, 1)
    sc.new(1, BUY, int(base[1]) + 9, 2)
    a = sc.take()
    with engine_on(me, path, S, base, [a], max_resting=4096, symbol_ids=ids, **_kw(path)) as eng:
        run = Run(me, eng, S, symbol_ids=ids)
        _, ans = run.step(a, f"int64 {path}")
        assert int(ans[hi[2]]["qty_ahead"]) == 4_294_967_294
        r = ans[lo[2]]
        assert (int(r["qty_ahead"]), int(r["qty_better"]), int(r["level_qty"])) == (2 * INT32_MAX, 3 * INT32_MAX, 3 * INT32_MAX)
        assert int(ans[far]["qty_better"]) == 6 * INT32_MAX > 1 << 33 and int(ans[far]["levels_better"]) == 2
        assert {int(r["symbol"]) for r in ans.values() if int(r["found"])} == set(ids)
        assert int(ans[far]["symbol"]) == 4_000_000_000


# ---- randomized streams -------------------------------------------------------------------------------------------------

RS, RNB, RN, RSUB = 8, 6, 512, 64
DRAWS = range(10)


@functools.lru_cache(maxsize=8)
def _draw(L, draw, per):
    """(base, arrays, checkpoints): six batches of 512 records cut into batches of `per`, and after every one of
    them the model's outputs and the answers owed for every seq used so far, the dead ones and 64 that never
    were. Shared between the tests: nobody changes the arrays."""
    base, big = rm.reduce_stream(31_000 + 10 * L + draw, RS, L, RNB, RN, convert_pct=50, fresh_pct=6,
                                 drift=(0, 3, 7)[draw % 3], far_pct=3, skew=True, **DEEP_BOOKS)
    cols = [np.concatenate([getattr(a, f) for a in big]) for f in ("seq", "price_q4", "qty", "symbol", "kind")]
    n = len(cols[0])
    arrays = [tm.Arrays(*[c[i:i + per] for c in cols]) for i in range(0, n, per)]
    rm.check_seq_rule(arrays)
    model = ReduceBook(RS)
    used, cps, longest = set(), [], 0
    rng = np.random.default_rng(draw)
    for a in arrays:
        ro, fo = model.submit(a)
        used.update(int(x) for x in a.seq)
        last = max(used)
        never = [last + 2 + int(x) for x in rng.integers(0, 1 << 40, 64)]
        q = np.array(sorted(used) + _dead(last) + never, dtype=np.uint64)
        cps.append((ro, fo, q, oq.expected(model, RS, q)))
        longest = max(longest, max(collections.Counter(hit[:3] for hit in model.live.values()).values(), default=0))
    assert int(cps[-1][3]["found"].sum()) == model.resting() > 150
    assert longest > 10, "no level ever held more than ten orders: the walks stay inside one chunk"
    dumps = [model.dump(s) for s in range(RS)]
    return base, arrays, cps, dumps


def _books_equal(eng, dumps, ctx):
    for s, e in enumerate(dumps):
        g = eng.dump(s)
        assert len(g) == len(e) and np.all(g == e), f"{ctx}: book of symbol {s} differs"


@pytest.mark.parametrize("path", ALL)
@pytest.mark.parametrize("draw", DRAWS)
def test_random_streams(me, path, draw):
    L = PATHS[path][0]
    base, arrays, cps, dumps = _draw(L, draw, RN)
    with engine_on(me, path, RS, base, arrays, **_kw(path)) as eng:
        for k, (a, (ro, fo, q, want)) in enumerate(zip(arrays, cps)):
            ctx = f"random L={L} #{draw} {path} batch {k}"
            r, f = eng.submit_batch(as_batch(me, a))
            assert_results_equal(r, ro, ctx)
            assert_fills_equal(f, fo, ctx)
            oq.assert_answers_equal(eng.order_query(q), want, ctx)
        _books_equal(eng, dumps, f"random {path} #{draw}")
        st = eng.stats()
        if path in ("hot", "hot_agg"):
            assert st["hot_handoffs"] > 0


@pytest.mark.parametrize("path", GROUPED)
@pytest.mark.parametrize("group", [1, 8, 32])
@pytest.mark.parametrize("draw", DRAWS)
def test_random_streams_in_device_groups(me, path, group, draw):
    """The same streams as device batches of 64 records, `group` of them per launch; queried after every group."""
    L = PATHS[path][0]
    base, arrays, cps, dumps = _draw(L, draw, RSUB)
    total = sum(len(a) for a in arrays)
    with engine_on(me, path, RS, base, arrays, max_resting=2 * total + 1024, batches_per_launch=group) as eng:
        dbs = [eng.upload(as_batch(me, a)) for a in arrays]
        try:
            for g0 in range(0, len(dbs), group):
                g1 = min(g0 + group, len(dbs))
                for db in dbs[g0:g1]:
                    eng.submit_device(db)
                ctx = f"groups L={L} #{draw} {path} G={group} batches {g0}..{g1 - 1}"
                _, _, q, want = cps[g1 - 1]
                oq.assert_answers_equal(eng.order_query(q), want, ctx)  # (the query flushes the group itself)
                assert eng.last_group_size() == g1 - g0
                r, f = eng.fetch_group_outputs(g1 - g0 - 1, len(arrays[g1 - 1]))
                assert_results_equal(r, cps[g1 - 1][0], ctx)
                assert_fills_equal(f, cps[g1 - 1][1], ctx)
        finally:
            for db in dbs:
                db.free()
        _books_equal(eng, dumps, f"groups {path} #{draw} G={group}")


# ---- nothing is disturbed -------------------------------------------------------------------------------------------------

def _feeds_run(me, path, draw, queries):
    """The draw's 512-record batches as pipelined host batches with both feeds on; with `queries`, order queries
    between the batches, between submit_host and collect included. Returns (outputs, quote events, depth
    events, final dumps, the engine's last export)."""
    L = PATHS[path][0]
    base, arrays, cps, _ = _draw(L, draw, RN)
    batches = [as_batch(me, a) for a in arrays]
    quotes, depth, outs = [], [], [None] * len(batches)
    with engine_on(me, path, RS, base, arrays, **_kw(path, 1)) as eng:
        eng.quotes_enable(1 << 14)
        eng.depth_enable(5, 1 << 15)
        quotes.append(eng.quotes_drain())
        depth.append(eng.depth_drain())
        tickets = []
        for k, b in enumerate(batches):
            tickets.append((k, eng.submit_host(b)))
            if queries:  # the batch is submitted, not collected: the query brings the pipeline to this point
                oq.assert_answers_equal(eng.order_query(cps[k][2]), cps[k][3], f"undisturbed {path} after submit {k}")
            if len(tickets) > 1:
                j, t = tickets.pop(0)
                outs[j] = eng.collect(t)
                if queries:
                    oq.assert_answers_equal(eng.order_query(cps[k][2][::3]), cps[k][3][::3],
                                            f"undisturbed {path} after collect {j}")
        for j, t in tickets:
            outs[j] = eng.collect(t)
        eng.sync()
        quotes.append(eng.quotes_drain())
        depth.append(eng.depth_drain())
        dumps = [eng.dump(s) for s in range(RS)]
        raw = eng.debug_export()
    return outs, np.concatenate(quotes), np.concatenate(depth), dumps, raw


@pytest.mark.parametrize("path", ALL)
def test_queries_disturb_nothing(me, path):
    L = PATHS[path][0]
    _, arrays, cps, want_dumps = _draw(L, 0, RN)
    plain = _feeds_run(me, path, 0, False)
    asked = _feeds_run(me, path, 0, True)
    for k, (ro, fo, _, _) in enumerate(cps):
        for name, run in (("plain", plain), ("asked", asked)):
            assert_results_equal(run[0][k][0], ro, f"undisturbed {path} {name} batch {k}")
            assert_fills_equal(run[0][k][1], fo, f"undisturbed {path} {name} batch {k}")
    for s in range(RS):
        assert np.array_equal(asked[3][s], want_dumps[s]) and np.array_equal(plain[3][s], want_dumps[s]), s
    last = max(int(x) for a in arrays for x in a.seq)
    v, _ = book_audit.audit(asked[4], last_seq=last)
    assert not v, v[:3]
    # every batch is a launch of its own in both runs, so the feeds' jobs fall at the same points of the stream:
    # the very same events
    assert len(plain[1]) > 0 and len(plain[2]) > 0
    assert np.array_equal(plain[1], asked[1]), f"{path}: quote events differ"
    assert np.array_equal(plain[2], asked[2]), f"{path}: depth events differ"
