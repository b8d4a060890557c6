"""me_mass_cancel (k_purge) against the CPU oracle. Needs an MI355X. Everything is exact.

The oracle has no mass cancel: its equivalent (tests/mass_cancel_model.py) is one batch of CANCEL records, one
per entry of the oracle's own dump filtered by side, fed at the same point of the stream. After every engine call
the device book is audited (tests/book_audit.py: totals, occ, chunk zeroing, free lists, resting, far counts)
and every symbol's dump compared; after a purge every removed seq is queried (found = 0) and the stream goes on
against the oracle bit-exact.
"""
import ctypes as C

import numpy as np
import pytest

from tests import book_audit
from tests import mass_cancel_model as mc
from tests import tif_model as tm
from tests._parity import assert_books_equal, assert_fills_equal, assert_results_equal
from tests.big_qty import Script
from tests.gpu_harness import PATHS, as_batch, engine_on

pytestmark = pytest.mark.gpu

BUY, SELL, BOTH = 1, 2, 3
ST_REJECTED, RJ_UNKNOWN = 4, 5
CHUNK = 16
PURGE_PASS = 2048  # levels one pass of k_purge takes (me_snapshot.hip PURGE_P)
PLAIN = dict(mix=(84, 0, 0, 0, 4, 12), market_tifs=(0,), bad_pct=0, spread=12, max_qty=20)  # GTC LIMITs, MARKETs, cancels


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _kw(path):
    return {"batches_per_launch": 1} if PATHS[path][3] else {}


class Run:
    """An engine and the oracle beside it. step() is one synchronous batch, purge() one mass cancel and its
    equivalent; both compare outputs, every book, the counters and the audit."""

    def __init__(self, me, eng, S):
        from oracle.oracle import OracleBook

        self.me, self.eng, self.S = me, eng, S
        self.orc = OracleBook(S)
        self.last = 0
        self.purged = set()

    def step(self, a, ctx, check=True):
        r, f = self.eng.submit_batch(as_batch(self.me, a))
        ro, fo = self.orc.submit(a)
        assert_results_equal(r, ro, ctx)
        assert_fills_equal(f, fo, ctx)
        self.last = max(self.last, int(a.seq.max()))
        if check:
            self.check(ctx)
        return ro, fo

    def check(self, ctx):
        assert_books_equal(self.eng, self.orc, range(self.S), ctx)
        assert self.eng.resting_count() == self.eng.admission()["resting"] == self.orc.resting(), f"{ctx}: resting counters"
        v, books = book_audit.audit(self.eng.debug_export(), last_seq=self.last)
        assert not v, f"{ctx}: {v[:3]}"
        return books

    def purge(self, symbols, sides, ctx, base_check=True):
        base0 = self.eng.debug_export(["sym"])["sym"]["base"].copy() if base_check else None  # (the export flushes)
        want = mc.apply(self.orc, symbols, sides, self.last)
        got = self.eng.mass_cancel(symbols, sides)
        mc.assert_removed_equal(got, want, ctx)
        assert not got[0]["pad"].any()
        self.check(ctx)
        if base_check:
            assert np.array_equal(self.eng.debug_export(["sym"])["sym"]["base"], base0), f"{ctx}: a window base moved"
        if len(got[0]):
            ans = self.eng.order_query(got[0]["seq"])
            assert not ans["found"].any(), f"{ctx}: a removed order is still found"
        self.purged.update(int(x) for x in got[0]["seq"])
        return got


# ---- the shapes of a book -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["reg", "gwalk_cx", "deep"])
def test_book_shapes_sides_and_symbol_lists(me, path):
    """Symbol 0 around price 0 (negative prices, price 0): a level of 40 orders with dead slots in its head and
    middle chunks, other levels, inline far levels on both sides. Symbol 1: both sides, far asks. Symbol 2:
    emptied by cancels. Symbol 3: never used. Symbol 4: both sides. sides 1, 2 and 3; lists in any order."""
    L, S = PATHS[path][0], 5
    base = tm.base_prices(S, L)
    base[0] = -(L // 2)
    sc = Script()
    o = [None] + [sc.new(0, BUY, -3, 10 + j % 5) for j in range(40)]  # chunks 1-16, 17-32, 33-40
    for p, q in ((-1, 5), (-1, 6), (-2, 7), (-7, 8)):
        sc.new(0, BUY, p, q)
    for p, q in ((0, 4), (0, 3), (2, 9), (5, 1)):
        sc.new(0, SELL, p, q)
    for k in range(3):  # beyond the window: far levels in the inline regions
        sc.new(0, BUY, -L - 10 * k, 11 + k)
        sc.new(0, BUY, -L - 10 * k, 2)
        sc.new(0, SELL, L + 7 * k, 21 + k)
    m1 = int(base[1]) + L // 2
    for j in range(20):
        sc.new(1, BUY, m1 - 1 - j % 4, 3 + j)
        sc.new(1, SELL, m1 + 1 + j % 3, 2 + j)
    sc.new(1, SELL, m1 + 3 * L, 50)
    m2 = int(base[2]) + L // 2
    gone = [sc.new(2, BUY, m2 - 1, 5), sc.new(2, SELL, m2 + 1, 5), sc.new(2, SELL, m2 + 2 * L, 5)]
    m4 = int(base[4]) + L // 2
    for j in range(10):
        sc.new(4, BUY, m4 - 2 - j, 4)
        sc.new(4, SELL, m4 + 2 + j, 6)
    build = sc.take()
    for j in (1, 2, 20, 21, 25, 40):
        sc.cancel(0, o[j])
    for t in gone:
        sc.cancel(2, t)
    cancels = sc.take()
    # afterwards: cancels of purged orders (rejected), the purged books trade again
    sc.cancel(0, o[5])
    sc.cancel(4, gone[0])
    a1 = sc.new(0, SELL, 1, 10)
    sc.new(0, BUY, 1, 4)
    sc.new(0, BUY, -3, 8)
    sc.new(1, BUY, m1 + 1, 1000, market=True)
    sc.new(1, SELL, m1 - 9, 1000, market=True)
    sc.new(4, BUY, m4 - 2, 5)
    sc.cancel(0, a1)
    after = sc.take()
    with engine_on(me, path, S, base, [build, cancels, after], ring=1 << 16, **_kw(path)) as eng:
        run = Run(me, eng, S)
        run.step(build, f"shapes {path} build")
        run.step(cancels, f"shapes {path} cancels")
        nb1 = int((run.orc.dump(1)["side"] == BUY).sum())
        e, c = run.purge([1], SELL, f"shapes {path} one side")
        assert c.tolist() == [[0, 21]] and len(eng.dump(1)) == nb1
        e, c = run.purge([4, 2, 3, 0], [BUY, BOTH, BOTH, BOTH], f"shapes {path} list")
        assert c.tolist() == [[10, 0], [0, 0], [0, 0], [34 + 4 + 6, 4 + 3]]
        assert [int(x) for x in e["price_q4"][10:14]] == [-1, -1, -2, -3] and int(e["seq"][13]) == o[3]
        assert len(eng.dump(0)) == 0 and len(eng.dump(4)) == 10
        e, c = run.purge([0, 3], BOTH, f"shapes {path} empty books")
        assert len(e) == 0 and not c.any()
        e, c = run.purge([1], BUY, f"shapes {path} other side")
        assert c.tolist() == [[nb1, 0]] and len(eng.dump(1)) == 0
        ro, _ = run.step(after, f"shapes {path} afterwards")
        assert [(int(r["status"]), int(r["reason"])) for r in ro[:2]] == [(ST_REJECTED, RJ_UNKNOWN)] * 2
        run.purge(list(range(S - 1, -1, -1)), BOTH, f"shapes {path} everything")
        assert book_audit.is_drained(eng.debug_export()) == []


def test_more_levels_than_one_pass(me):
    """A 4,096-level window with PURGE_PASS + 1 occupied bid levels (and a level of three chunks among them), a
    few asks and far levels: the bid side takes two passes, through the occupancy words."""
    L, S = 4096, 2
    base = tm.base_prices(S, L)
    b0 = int(base[0])
    sc = Script()
    for j in range(PURGE_PASS + 1):
        sc.new(0, BUY, b0 + 3 + j, 1 + j % 9)
    for j in range(2 * CHUNK + 5):
        sc.new(0, BUY, b0 + 700, 2)
    for j in range(12):
        sc.new(0, SELL, b0 + 3000 + 5 * j, 7)
    sc.new(0, BUY, b0 - 50, 3)
    sc.new(0, SELL, b0 + L + 50, 3)
    sc.new(1, BUY, int(base[1]) + 100, 5)
    build = sc.take()
    sc.new(0, SELL, b0 + 1000, 30)
    sc.new(0, BUY, b0 + 1000, 10)
    sc.cancel(0, 5)
    after = sc.take()
    with me.Engine(S, L, base, max_batch=len(build), max_resting=len(build) + 64, seq_ring=1 << 16) as eng:
        run = Run(me, eng, S)
        run.step(build, "passes build")
        e, c = run.purge([0], BUY, "passes bids")
        assert c.tolist() == [[PURGE_PASS + 1 + 2 * CHUNK + 5 + 1, 0]]
        assert int(e["price_q4"][0]) == b0 + 3 + PURGE_PASS and int(e["price_q4"][-1]) == b0 - 50
        ro, _ = run.step(after, "passes afterwards")
        assert (int(ro[2]["status"]), int(ro[2]["reason"])) == (ST_REJECTED, RJ_UNKNOWN)
        run.purge([1, 0], BOTH, "passes the rest")
        assert eng.resting_count() == 0


@pytest.mark.parametrize("path", ["reg", "deep"])
def test_far_side_moved_into_the_arena(me, path):
    """far_levels = 4 and nine far bid levels: the side lives in the arena. The purge leaves its directory entry
    alone; far bids rest there again afterwards."""
    L, S = PATHS[path][0], 2
    base = tm.base_prices(S, L)
    b0 = int(base[0])
    m = b0 + L // 2
    sc = Script()
    for k in range(9):
        sc.new(0, BUY, b0 - 10 * (k + 1), 20 + k)
        if k % 2:
            sc.new(0, BUY, b0 - 10 * (k + 1), 3)
    for k in range(3):
        sc.new(0, SELL, b0 + L + 10 * k, 30 + k)
    sc.new(0, BUY, m - 1, 5)
    sc.new(0, SELL, m + 1, 8)
    sc.new(1, BUY, int(base[1]) + 3, 5)
    build = sc.take()
    for k in range(6):
        sc.new(0, BUY, b0 - 15 * (k + 1), 9)
    sc.new(0, SELL, b0 - 100, 25)  # takes the window bid, then far bids
    after = sc.take()
    with engine_on(me, path, S, base, [build, after], ring=1 << 16, far_levels=4, **_kw(path)) as eng:
        run = Run(me, eng, S)
        run.step(build, f"arena {path} build")
        assert eng.far_stats()["moves"] > 0
        fdir0 = eng.debug_export(["fdir"])["fdir"].copy()
        e, c = run.purge([0], BUY, f"arena {path} bids")
        assert c.tolist() == [[9 + 4 + 1, 0]]
        assert np.array_equal(eng.debug_export(["fdir"])["fdir"], fdir0)
        run.step(after, f"arena {path} afterwards")
        run.purge([0, 1], BOTH, f"arena {path} the rest")


# ---- the stream goes on -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["gwalk_cx", "gwalk", "reg", "deep", "hot_agg", "hot"])
def test_the_stream_goes_on(me, path):
    """Six batches of 1,024 records on four symbols (256 per symbol and batch; on the hot paths half of them
    symbol 0's), purges after the third: the same symbols trade on, cancels of purged orders are rejected."""
    L, S = PATHS[path][0], 4
    base, arrays = tm.tif_stream(4200 + L, S, L, 6, 1024, far_pct=2, skew=path in ("hot", "hot_agg"), **PLAIN)
    with engine_on(me, path, S, base, arrays, ring=1 << 16, **_kw(path)) as eng:
        run = Run(me, eng, S)
        for k in range(3):
            run.step(arrays[k], f"goes on {path} batch {k}", check=k == 2)
        assert run.orc.resting() > 200
        e, c = run.purge([2, 0], BOTH, f"goes on {path} purge")
        assert c.min() > 10
        run.purge([1], SELL, f"goes on {path} one side")
        hits = 0
        for k in range(3, 6):
            ro, _ = run.step(arrays[k], f"goes on {path} batch {k}", check=k == 5)
            cx = (arrays[k].kind & 8) != 0
            named = np.isin(arrays[k].price_q4[cx].astype(np.uint64), np.fromiter(run.purged, dtype=np.uint64))
            assert (ro["status"][cx][named] == ST_REJECTED).all() and (ro["reason"][cx][named] == RJ_UNKNOWN).all()
            hits += int(named.sum())
        assert hits > 0, "no later cancel named a purged order"
        run.purge([3, 2, 1, 0], BOTH, f"goes on {path} everything")
        assert book_audit.is_drained(eng.debug_export()) == []


def test_freed_chunks_are_reclaimed_and_reused(me, monkeypatch):
    """max_resting = 250, so the pool holds 250 + 32 S + 64 = 442 chunks. 240 orders on 240 levels of symbols 0
    and 1 (one chunk each) are purged; 240 on symbols 2 and 3 follow, then 240 on 0 and 1 again: the pool cannot
    hold the sum, so the reclamation takes the purged chains' chunks back and the next groups reuse them."""
    monkeypatch.setenv("ME_REG_AGG", "0")
    L, S, R = 128, 4, 250
    base = tm.base_prices(S, L)
    sc = Script()

    def fill(pair):
        for s in pair:
            for j in range(60):
                sc.new(s, BUY, int(base[s]) + 59 - j, 3)
                sc.new(s, SELL, int(base[s]) + 64 + j, 4)
        return sc.take()

    with me.Engine(S, L, base, max_batch=256, max_resting=R, seq_ring=1 << 16, batches_per_launch=1) as eng:
        assert eng.chunk_stats()["pool"] == R + 32 * S + 64
        run = Run(me, eng, S)
        run.step(fill((0, 1)), "chunks first")
        r0 = eng.chunk_stats()["reclaims"]
        e, c = run.purge([1, 0], BOTH, "chunks purge 1")
        assert len(e) == 240
        run.step(fill((2, 3)), "chunks second")
        run.purge([2, 3], BOTH, "chunks purge 2")
        run.step(fill((0, 1)), "chunks third")
        cs = eng.chunk_stats()
        assert cs["reclaims"] > r0 and cs["high_water"] <= cs["pool"], cs


def test_a_refused_batch_is_admitted_after_the_purge(me):
    S, L, R = 4, 128, 512
    base = tm.base_prices(S, L)
    sc = Script()
    for i in range(R):
        s = i % S
        mid = int(base[s]) + L // 2
        buy = (i // S) % 2
        sc.new(s, BUY if buy else SELL, mid + (-1 - i % 7 if buy else 1 + i % 7), 10)
    fill = sc.take()
    for i in range(150):
        sc.new(i % S, BUY, int(base[i % S]) + 10 + i % 3, 1)
    more = sc.take()
    with me.Engine(S, L, base, max_batch=1024, max_resting=R, seq_ring=1 << 16) as eng:
        run = Run(me, eng, S)
        run.step(fill, "admission fill")
        assert eng.admission()["resting"] == R
        assert not eng.admits(as_batch(me, more))
        with pytest.raises(me.EngineError) as ei:
            eng.submit_batch(as_batch(me, more))
        assert ei.value.code == me.ME_E_CAPACITY
        e, c = run.purge([3, 1], [BOTH, BUY], "admission purge")
        assert len(e) == R // 4 + R // 8
        adm = eng.admission()
        assert adm["resting"] == adm["bound"] == R - len(e)
        assert eng.admits(as_batch(me, more))
        run.step(more, "admission admitted")


def test_host_tickets_held_across_a_purge(me):
    """Three host batches submitted and not collected, a purge, then the three collects: the oracle's outputs."""
    L, S = 128, 4
    base, arrays = tm.tif_stream(977, S, L, 4, 512, **PLAIN)
    with me.Engine(S, L, base, max_batch=512, max_resting=4096, seq_ring=1 << 16, batches_per_launch=4) as eng:
        run = Run(me, eng, S)
        tickets = [eng.submit_host(as_batch(me, a)) for a in arrays[:3]]
        exp = [run.orc.submit(a) for a in arrays[:3]]
        run.last = max(int(a.seq.max()) for a in arrays[:3])
        assert run.orc.resting() > 100
        run.purge([0, 3], BOTH, "tickets purge", base_check=False)  # the call itself flushes the group
        for k, t in enumerate(tickets):
            r, f = eng.collect(t)
            assert_results_equal(r, exp[k][0], f"tickets batch {k}")
            assert_fills_equal(f, exp[k][1], f"tickets batch {k}")
        run.step(arrays[3], "tickets afterwards")


# ---- the contract's edges -------------------------------------------------------------------------------------------------

def test_capacity_and_invalid_arguments_change_nothing(me):
    L, S = 128, 3
    base, arrays = tm.tif_stream(31, S, L, 2, 512, **PLAIN)
    with me.Engine(S, L, base, max_batch=512, max_resting=4096, seq_ring=1 << 16) as eng:
        run = Run(me, eng, S)
        run.step(arrays[0], "edges build")
        lib, h = eng.lib, eng.h
        dumps = [eng.dump(s) for s in range(S)]
        need = len(dumps[0]) + len(dumps[2])
        assert need > 20

        def call(sym, sides, cap, n=None, out=True, counts=True):
            sy = np.array(sym, dtype=np.uint32)
            sd = np.array(sides, dtype=np.uint8)
            buf = np.zeros(max(cap, 1), dtype=me.BOOK_ENTRY_DTYPE)
            cnt = np.full((max(len(sy), 1), 2), 99, dtype=np.uint64)
            k = C.c_size_t(12345)
            rc = lib.me_mass_cancel(h, sy.ctypes.data, sd.ctypes.data, len(sy) if n is None else n,
                                    buf.ctypes.data if out else None, cap, C.byref(k), cnt.ctypes.data if counts else None)
            return rc, k.value, buf, cnt

        def unchanged(ctx):
            for s in range(S):
                assert np.array_equal(eng.dump(s), dumps[s]), f"{ctx}: symbol {s} changed"
            run.check(ctx)

        rc, k, _, _ = call([2, 0], [3, 3], need - 1)
        assert (rc, k) == (me.ME_E_CAPACITY, need)
        unchanged("cap one short")
        rc, k, _, _ = call([2, 0], [3, 3], need, out=False)
        assert (rc, k) == (me.ME_E_CAPACITY, need)
        for sym, sides in (([0, 0], [3, 3]), ([1, 2, 1], [1, 2, 2]), ([0], [0]), ([0], [4]), ([1, S], [3, 3]),
                           ([0xFFFFFFFF], [3]), ([0, 1, 2, 0], [3, 3, 3, 3])):
            rc, k, _, _ = call(sym, sides, 4096)
            assert (rc, k) == (me.ME_E_INVALID, 0), (sym, sides)
        assert lib.me_mass_cancel(h, None, None, 2, None, 0, None, None) == me.ME_E_INVALID
        assert lib.me_mass_cancel(h, None, None, 0, None, 0, None, None) == me.ME_OK
        unchanged("refusals")
        # the engine is still usable: the same call with room succeeds, with or without counts
        want = mc.apply(run.orc, [2, 0], 3, run.last)
        rc, k, buf, cnt = call([2, 0], [3, 3], need)
        assert rc == me.ME_OK and k == need
        mc.assert_removed_equal((buf[:k], cnt), want, "exact cap")
        run.check("exact cap")
        want = mc.apply(run.orc, [1], 3, run.last)
        rc, k, buf, _ = call([1], [3], len(dumps[1]), counts=False)
        assert rc == me.ME_OK and np.array_equal(buf[:k], want[0])
        run.step(arrays[1], "edges afterwards")


# ---- the feeds ------------------------------------------------------------------------------------------------------------

def _replay_depth(state, ev):
    for e in ev:
        key = (int(e["symbol"]), int(e["side"]))
        if int(e["qty"]) == 0:
            state.setdefault(key, {}).pop(int(e["price_q4"]), None)
        else:
            state.setdefault(key, {})[int(e["price_q4"])] = int(e["qty"])


@pytest.mark.parametrize("path", ["reg", "deep256"])
def test_quote_and_depth_feeds_follow_a_purge(me, path):
    L, S, D = PATHS[path][0], 4, 4
    base, arrays = tm.tif_stream(555, S, L, 3, 512, far_pct=2, **PLAIN)
    with engine_on(me, path, S, base, arrays, ring=1 << 16, **_kw(path)) as eng:
        run = Run(me, eng, S)
        eng.quotes_enable(1 << 12)
        eng.depth_enable(D, 1 << 13)
        quotes, views = [eng.quotes_drain()], {}
        _replay_depth(views, eng.depth_drain())
        for k in range(2):
            run.step(arrays[k], f"feeds {path} batch {k}", check=False)
        eng.sync()
        quotes.append(eng.quotes_drain())
        _replay_depth(views, eng.depth_drain())
        assert len(views[(0, BUY)]) == D and len(views[(0, SELL)]) == D and len(views[(2, SELL)]) == D
        assert int(quotes[-1]["batches"].max()) == 2
        run.purge([2, 0], [SELL, BOTH], f"feeds {path} purge")
        q, d = eng.quotes_drain(), eng.depth_drain()
        # the purged sides: a quote with the flag clear, DELETEs of the published view; stamped with the unchanged count
        assert sorted(int(x) for x in q["symbol"]) == [0, 2]
        by = {int(x["symbol"]): x for x in q}
        assert int(by[0]["flags"]) == 0 and int(by[2]["flags"]) == me.QUOTE_HAS_BID
        assert (q["batches"] == 2).all() and (d["batches"] == 2).all()
        assert len(d) == 3 * D and not d["qty"].any()
        assert sorted({(int(x["symbol"]), int(x["side"])) for x in d}) == [(0, BUY), (0, SELL), (2, SELL)]
        quotes.append(q)
        _replay_depth(views, d)
        run.step(arrays[2], f"feeds {path} batch 2")
        eng.sync()
        quotes.append(eng.quotes_drain())
        _replay_depth(views, eng.depth_drain())
        # replaying every event gives the top of every book
        lv, cnt = eng.levels_all(D)
        for s in range(S):
            for k, side in ((0, BUY), (1, SELL)):
                want = {int(x["price_q4"]): int(x["total_qty"]) for x in lv[s, k, : cnt[s, k]]}
                assert views.get((s, side), {}) == want, (s, side)
        last = {}
        for e in np.concatenate(quotes):
            last[int(e["symbol"])] = e
        lv1, cnt1 = eng.levels_all(1)
        for s in range(S):
            e = last[s]
            for k, (flag, pf, qf) in enumerate(((1, "bid_price_q4", "bid_qty"), (2, "ask_price_q4", "ask_qty"))):
                assert bool(int(e["flags"]) & flag) == bool(cnt1[s, k])
                if cnt1[s, k]:
                    assert (int(e[pf]), int(e[qf])) == (int(lv1[s, k, 0]["price_q4"]), int(lv1[s, k, 0]["total_qty"]))
