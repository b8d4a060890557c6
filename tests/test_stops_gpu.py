"""The trigger book (me_stops_*, DESIGN.md §2 "Stop orders") on every matching path against the model
(tests/stops_model.py fed the CPU oracle's tapes): exact array equality of every job's events and of the dump.
Needs an MI355X.

The ring never defers by construction; me_stops_stats answers ME_E_STATE if a job ever found it full, and every
test ends on `_no_deferral`, which also holds the job and event counts against the model's.
"""
import functools

import numpy as np
import pytest

from tests import stops_model as sm
from tests.feed_common import BUY, SELL, Rows, _c5_stream, _same
from tests.gpu_harness import FEED_PATHS as PATHS, SMALL, feed_engine

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
TIF_IOC = 1


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle

    return oracle


def _no_deferral(eng, jobs=None, events=None, live=None):
    st = eng.stops_stats()  # raises EngineError (ME_E_STATE) had any job been deferred: deferred == 0
    for name, want in (("jobs", jobs), ("events", events), ("live", live)):
        if want is not None:
            assert st[name] == want, (name, st)
    return st


def _trade(rows, s, px, q=1):
    """One fill of symbol s at px: a resting sell and the buy that takes it."""
    rows.limit(s, SELL, px, q)
    rows.limit(s, BUY, px, q)


def _stop_array(ids, stop_px, limit_px, qty, symbol, kind):
    a = np.zeros(len(ids), dtype=sm.STOP_DTYPE)
    for name, v in zip(sm.FIELDS, (ids, stop_px, limit_px, qty, symbol, kind)):
        a[name] = v
    return a


# ---- 1. every path and group size --------------------------------------------------------------------
S_PATHS = 128
SHAPE = {1: (5, 400), 8: (12, 200), 32: (36, 100)}  # tests/test_trades_gpu.py's shapes
SHAPE_DEEP = (4, 1500)


@functools.lru_cache(maxsize=None)
def _path_case(me, orc, L, nb, batch, group):
    """Computed once per shape from the oracle alone and shared: the stream, the stops built from every symbol's
    highs and lows per job, the model's events per job, its final dump and the guards."""
    base, batches = _c5_stream(me, S_PATHS, L, nb, batch)
    ob = orc.OracleBook(S_PATHS)
    bounds = list(range(group, nb, group)) + [nb]
    jobs, done = [], 0  # per job: the tapes of its batches
    for x in bounds:
        jobs.append([ob.submit(b)[1] for b in batches[done:x]])
        done = x
    hi = [dict() for _ in jobs]
    lo = [dict() for _ in jobs]
    for j, tapes in enumerate(jobs):
        for t in tapes:
            for s in np.unique(t["symbol"]):
                p = t["price_q4"][t["symbol"] == s]
                hi[j][int(s)] = max(hi[j].get(int(s), int(p.max())), int(p.max()))
                lo[j][int(s)] = min(lo[j].get(int(s), int(p.min())), int(p.min()))
    traded = sorted(set().union(*[set(h) for h in hi]))
    # five stops per traded symbol, ids type-major: table order is not symbol order
    kinds = [me.kind(BUY, 1), me.kind(BUY, 0, 0, TIF_IOC), me.kind(SELL, 1), me.kind(SELL), me.kind(BUY)]
    rows, nid = [], 100
    for t in range(5):
        for s in traded:
            top = max(h[s] for h in hi if s in h)
            bot = min(l[s] for l in lo if s in l)
            first = next(h[s] for h in hi if s in h)
            px = (top, top + 1, bot, bot - 1, first)[t]  # equality, never, equality, never, the first traded job
            rows.append((nid, px, px + 7 * t, 1 + s % 9, s, kinds[t]))
            nid += 1 + (s + t) % 3
    stops = sm.stops(rows)
    model = sm.StopModel(S_PATHS)
    model.add(stops)
    exp, two = [], False
    for j, tapes in enumerate(jobs):
        for t in tapes:
            model.feed(t)
        ev = model.job(bounds[j])
        exp.append(ev)
        src = set()  # the batches of the launch holding a fill at an event's trigger price
        for e in ev:
            src.add(next(k for k, t in enumerate(tapes)
                         if ((t["symbol"] == e["symbol"]) & (t["price_q4"] == e["trigger_px_q4"])).any()))
        two = two or len(src) >= 2
    return base, batches, bounds, stops, exp, model.dump(), len(traded), two


@pytest.mark.parametrize("path,group", [(p, g) for p in SMALL for g in (1, 8, 32)] +
                         [(p, 1) for p in PATHS if p not in SMALL])
def test_events_of_every_group_on_every_path(me, orc, path, group):
    """A config-5-style stream; per traded symbol a BUY stop at its highest fill (equality), one a tick above
    (never), a SELL stop at its lowest fill, one a tick below (never) and a BUY stop at its first traded job's
    high, all added before the first batch. The events of every job and the dump at the end equal the model's."""
    L, grouped = PATHS[path][0], PATHS[path][3]
    nb, batch = SHAPE[group] if grouped else SHAPE_DEEP
    base, batches, bounds, stops, exp, dump, traded, two = _path_case(me, orc, L, nb, batch, group if grouped else 1)
    # a silent feed cannot pass: on the oracle's side alone
    assert traded >= S_PATHS // 2, traded
    assert sum(len(e) for e in exp) == 3 * traded and len(dump) == 2 * traded == len(stops) - 3 * traded
    assert two or group == 1
    total = nb * batch
    kw = {"batches_per_launch": group} if grouped else {}
    with feed_engine(me, path, S_PATHS, base, batch, 2 * total + 1024, **kw) as eng:
        eng.stops_enable(len(stops))
        eng.stops_add(stops)
        _no_deferral(eng, jobs=0, events=0, live=len(stops))
        got = []
        if grouped:
            dbs = [eng.upload(b) for b in batches]
            try:
                for db in dbs:
                    eng.submit_device(db)
                eng.sync()
            finally:
                for db in dbs:
                    db.free()
            ev = eng.stops_drain()
            for x in bounds:  # the jobs by their stamps
                got.append(ev[ev["batches"] == x])
            assert sum(len(g) for g in got) == len(ev)
        else:
            for b in batches:
                eng.submit_batch(b)
                got.append(eng.stops_drain())
        for k in range(len(bounds)):
            _same(got[k], exp[k], f"{path} G={group} job {k}")
        _same(eng.stops_dump(), dump, f"{path} G={group} dump")
        _no_deferral(eng, jobs=len(bounds), events=3 * traded, live=2 * traded)
        if path == "reg":
            assert eng.stats()["handoffs"] > 0
        if path in ("hot_agg", "hot"):
            assert eng.stats()["hot_handoffs"] > 0


# ---- 2. table sizes at the mask words' edges ---------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 1030, 70_000])
def test_table_sizes(me, orc, N):
    """N BUY stops on five symbols. The first job triggers the first, the last and the middle entry and every
    97th in between (the first, the last and the middle mask words among them; at 70,000 entries the 1,094 words
    are more than the emit workgroup's 1,024 threads prefix in one step), the second all the rest."""
    S, L = 5, 128
    base = np.array([10_000 + 1_000 * s for s in range(S)], dtype=np.int64)
    i = np.arange(N)
    first = (i == 0) | (i == N - 1) | (i == N // 2) | (i % 97 == 50)
    sym = (i * 3 + i // 64) % S
    stops = _stop_array(1 + 2 * i, base[sym] + np.where(first, 10, 11), base[sym] - i, 1 + i % 5, sym,
                        np.where(i % 2 == 0, me.kind(BUY, 1), me.kind(BUY)))
    ob = orc.OracleBook(S)
    model = sm.StopModel(S)
    model.add(stops)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20) as eng:
        eng.stops_enable(N)
        eng.stops_add(stops)
        rows = Rows(me)
        for n, off in enumerate((10, 11)):
            for s in range(S):
                _trade(rows, s, int(base[s]) + off)
            b = rows.batch()
            eng.submit_batch(b)
            model.feed(ob.submit(b)[1])
            ev = eng.stops_drain()
            exp = model.job(n + 1)
            assert len(exp) == (int(first.sum()) if n == 0 else N - int(first.sum()))
            _same(ev, exp, f"N={N} job {n}")
            _same(eng.stops_dump(), model.dump(), f"N={N} dump {n}")
        # (the second launch ran a job only if a stop was left for it)
        _no_deferral(eng, jobs=2 if first.sum() < N else 1, events=N, live=0)


# ---- 3. price edges ----------------------------------------------------------------------------------
def test_price_edges(me, orc):
    S, L = 2, 128
    base = np.array([-64, 1_000], dtype=np.int64)
    b, s_ = me.kind(BUY, 1), me.kind(SELL, 1)
    stops = sm.stops([(1, I64_MIN, 0, 1, 0, b), (2, I64_MAX, 0, 1, 0, s_), (3, I64_MAX, I64_MAX, 1, 0, b),
                      (4, I64_MIN, I64_MIN, 1, 0, s_), (5, 0, 0, 1, 0, b), (6, -1, 0, 1, 0, s_), (7, -1, 0, 1, 0, b),
                      (8, 0, 0, 1, 0, s_), (9, 1_010, 0, 1, 1, b)])
    ob = orc.OracleBook(S)
    model = sm.StopModel(S)
    model.add(stops)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20) as eng:
        eng.stops_enable(16)
        eng.stops_add(stops)
        rows = Rows(me)
        # symbol 0 does not trade: a BUY stop at INT64_MIN and a SELL stop at INT64_MAX stay; then fills at -5; at 0
        for n, (s, px, ids) in enumerate([(1, 1_010, [9]), (0, -5, [1, 2, 6, 8]), (0, 0, [5, 7])]):
            _trade(rows, s, px)
            bt = rows.batch()
            eng.submit_batch(bt)
            f = ob.submit(bt)[1]
            assert len(f) == 1 and int(f[0]["price_q4"]) == px
            model.feed(f)
            ev = eng.stops_drain()
            _same(ev, model.job(n + 1), f"edges job {n}")
            assert ev["id"].tolist() == ids and (ev["trigger_px_q4"] == px).all()
        d = eng.stops_dump()
        _same(d, model.dump(), "edges dump")
        assert d["id"].tolist() == [3, 4] and d["limit_px_q4"].tolist() == [I64_MAX, I64_MIN]
        _no_deferral(eng, jobs=3, events=7, live=2)


# ---- 4. stream position ------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [4, 1], ids=["open_partial_group", "bucketed_unmatched"])
def test_a_stop_sees_only_batches_submitted_after_it(me, orc, group):
    """Batch A's fill at P would satisfy a stop added after A was submitted: with groups of 4 A still sits in the
    open partial group at the add, with groups of 1 it is bucketed and waits for its match launch. The add sends
    A out first; A's job judges the table without the new stop (and triggers the control stop added before A).
    The same fill in batch B triggers it."""
    S, L, P = 2, 128, 10_020
    base = np.array([10_000, 20_000], dtype=np.int64)
    model = sm.StopModel(S)
    ob = orc.OracleBook(S)
    with feed_engine(me, "reg", S, base, 64, 1024, batches_per_launch=group) as eng:
        eng.stops_enable(8)
        before = sm.stops([(1, P, 0, 1, 0, me.kind(BUY, 1)), (2, P + 50, 0, 1, 0, me.kind(BUY, 1))])
        eng.stops_add(before)
        model.add(before)
        rows = Rows(me)
        dbs = []
        try:
            _trade(rows, 0, P)
            a = rows.batch()
            dbs.append(eng.upload(a))
            eng.submit_device(dbs[-1])  # no sync: A is submitted, not matched
            late = sm.stops([(3, P, 0, 1, 0, me.kind(BUY, 1)), (4, P, 0, 1, 0, me.kind(SELL))])
            eng.stops_add(late)
            model.feed(ob.submit(a)[1])
            exp_a = model.job(1)  # (the model judges A before it learns of the late stops)
            model.add(late)
            eng.sync()
            ev = eng.stops_drain()
            _same(ev, exp_a, "A's job")
            assert ev["id"].tolist() == [1]
            _same(eng.stops_dump(), model.dump(), "after A")
            _trade(rows, 0, P)
            b = rows.batch()
            dbs.append(eng.upload(b))
            eng.submit_device(dbs[-1])
            model.feed(ob.submit(b)[1])
            eng.sync()
            ev = eng.stops_drain()
            _same(ev, model.job(2), "B's job")
            assert ev["id"].tolist() == [3, 4]
        finally:
            for db in dbs:
                db.free()
        assert eng.stops_dump()["id"].tolist() == [2]
        _no_deferral(eng, jobs=2, events=3, live=1)


# ---- 5. cancel ---------------------------------------------------------------------------------------
def test_cancel(me, orc):
    S, L = 2, 128
    base = np.array([10_000, 20_000], dtype=np.int64)
    top = 2 ** 64 - 1
    model = sm.StopModel(S)
    ob = orc.OracleBook(S)
    k = me.kind(BUY, 1)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20) as eng:
        eng.stops_enable(16)
        first = sm.stops([(10, 10_010, 0, 1, 0, k), (20, 10_020, 0, 1, 0, k), (30, 10_030, 0, 1, 0, k),
                          (40, 10_040, 0, 1, 0, k)])
        eng.stops_add(first)
        model.add(first)
        # below the range, the first id, between two, the last id, above the range
        ids = [5, 10, 25, 40, 50]
        f = eng.stops_cancel(ids)
        assert f.tolist() == [0, 1, 0, 1, 0] == model.cancel(ids).tolist()
        _same(eng.stops_dump(), model.dump(), "after the first cancel")
        more = sm.stops([(60, 20_010, 0, 1, 1, k), (top, 20_020, 0, 1, 1, k)])
        eng.stops_add(more)
        model.add(more)
        rows = Rows(me)
        _trade(rows, 0, 10_020)  # triggers 20
        b = rows.batch()
        eng.submit_batch(b)
        model.feed(ob.submit(b)[1])
        ev = eng.stops_drain()
        _same(ev, model.job(1), "trigger 20")
        assert ev["id"].tolist() == [20]
        # a cancelled id, a triggered id, id 2^64 - 1
        ids = [10, 20, top]
        assert eng.stops_cancel(ids).tolist() == [0, 0, 1] == model.cancel(ids).tolist()
        # the still-unsynced last batch triggers 30: the cancel syncs first
        _trade(rows, 0, 10_030)
        b = rows.batch()
        db = eng.upload(b)
        try:
            eng.submit_device(db)
            model.feed(ob.submit(b)[1])
            exp = model.job(2)
            assert eng.stops_cancel([30]).tolist() == [0] == model.cancel([30]).tolist()
        finally:
            db.free()
        ev = eng.stops_drain()
        _same(ev, exp, "the unsynced batch's trigger")
        assert ev["id"].tolist() == [30]
        # unsorted ids: ME_E_INVALID, nothing changed
        for bad in ([60, 60], [top, 60]):
            with pytest.raises(me.EngineError) as ei:
                eng.stops_cancel(bad)
            assert ei.value.code == me.ME_E_INVALID
        _same(eng.stops_dump(), model.dump(), "after the refused cancels")
        assert eng.stops_dump()["id"].tolist() == [60]
        assert eng.stops_cancel([]).tolist() == []
        _no_deferral(eng, jobs=2, events=2, live=1)


# ---- 6. capacity, wrap and compaction ----------------------------------------------------------------
def test_capacity_wrap_and_compaction(me, orc):
    S, L, CAP = 2, 128, 8
    base = np.array([10_000, 20_000], dtype=np.int64)
    model = sm.StopModel(S)
    ob = orc.OracleBook(S)
    k = me.kind(BUY, 1)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20) as eng:
        eng.stops_enable(CAP)
        rows = Rows(me)
        nbat = 0

        def add(recs):
            eng.stops_add(recs)
            model.add(recs)

        def step(trades, want_ids, dump=True):
            nonlocal nbat
            for s, px in trades:
                _trade(rows, s, px)
            b = rows.batch()
            eng.submit_batch(b)
            model.feed(ob.submit(b)[1])
            nbat += 1
            ev = eng.stops_drain()
            _same(ev, model.job(nbat), f"batch {nbat}")
            assert ev["id"].tolist() == want_ids
            if dump:  # (the dump is the compaction pass: where an add is to be the one that compacts, none)
                _same(eng.stops_dump(), model.dump(), f"dump after batch {nbat}")

        add(sm.stops([(i, 10_000 + i, 0, 1, 0, k) for i in range(1, 9)]))  # the table is full
        ninth = sm.stops([(9, 10_003, 0, 1, 0, k)])
        with pytest.raises(me.EngineError) as ei:
            eng.stops_add(ninth)
        assert ei.value.code == me.ME_E_CAPACITY
        _same(eng.stops_dump(), model.dump(), "the refused add changed nothing")
        step([(0, 10_005)], [1, 2, 3, 4, 5], dump=False)  # the engine stays usable; events 0..4 read
        # five more: the append end is reached, the three live entries move to the front
        add(sm.stops([(i, 10_003, 0, 1, 0, k) for i in range(9, 14)]))
        with pytest.raises(me.EngineError) as ei:  # 3 + 5 live: full again
            eng.stops_add(sm.stops([(14, 10_003, 0, 1, 0, k)]))
        assert ei.value.code == me.ME_E_CAPACITY
        step([(0, 10_005)], [9, 10, 11, 12, 13], dump=False)  # events 5..9 of a ring of 8: they wrap
        # dead entries fill the table: cancel one more, and the next add compacts again
        assert eng.stops_cancel([7]).tolist() == [1] == model.cancel([7]).tolist()
        add(sm.stops([(14, 20_001, 0, 1, 1, k), (15, 20_001, 0, 1, 1, me.kind(SELL)), (16, 20_009, 0, 1, 1, k)]))
        d = eng.stops_dump()
        _same(d, model.dump(), "after the second compaction")
        assert d["id"].tolist() == [6, 8, 14, 15, 16]
        assert eng.stops_cancel([8]).tolist() == [1] == model.cancel([8]).tolist()  # found where it moved to
        step([(1, 20_001), (0, 10_006)], [6, 14, 15])  # id order across symbols
        assert eng.stops_dump()["id"].tolist() == [16]
        _no_deferral(eng, jobs=3, events=13, live=1)


# ---- 7. a cascade, end to end ------------------------------------------------------------------------
def test_cascade(me):
    """Bids of one lot at 100, 99, 98, 97, 96 and a ladder of SELL stops under them: each triggered sell trades one
    level lower and triggers the next stop, one job per step. Every job's events go through stop_records into the
    next batch; the same batches go to the model book."""
    from tests.reduce_model import ReduceBook  # (the model book that knows IOC)
    from tests.tif_model import Arrays

    S, L = 2, 128
    base = np.array([50, 1_000], dtype=np.int64)
    ladder = sm.stops([(1, 100, 0, 1, 0, me.kind(SELL, 1)), (2, 99, 0, 1, 0, me.kind(SELL, 1)),
                       (3, 98, 97, 1, 0, me.kind(SELL, 0, 0, TIF_IOC)), (4, 97, 90, 3, 0, me.kind(SELL))])
    ob = ReduceBook(S)
    model = sm.StopModel(S)
    model.add(ladder)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20) as eng:
        eng.stops_enable(8)
        eng.stops_add(ladder)
        rows = Rows(me)
        for px in (100, 99, 98, 97, 96):
            rows.limit(0, BUY, px, 1)
        rows.market(0, SELL, 1)  # the first trade, at 100
        b = rows.batch()
        seq, steps, all_ev = rows.seq, 0, []
        while len(b):
            res, fills = eng.submit_batch(b)
            mres, mfills = ob.submit(Arrays(b.seq, b.price_q4, b.qty, b.symbol, b.kind))
            for name in ("status", "reason", "filled_qty", "remaining_qty", "fill_count"):
                assert np.array_equal(res[name], mres[name]), f"step {steps}: {name}"
            assert np.array_equal(fills, mfills), f"step {steps}"
            model.feed(mfills)
            steps += 1
            ev = eng.stops_drain()
            _same(ev, model.job(steps), f"cascade step {steps}")
            all_ev.append(ev)
            b = me.stop_records(ev, seq)
            seq += len(ev)
        ids = [e["id"].tolist() for e in all_ev]
        assert ids == [[1], [2], [3], [4], []]  # one job per step
        assert [int(e[0]["trigger_px_q4"]) for e in all_ev[:4]] == [100, 99, 98, 97]
        for s in range(S):
            assert np.array_equal(eng.dump(s), ob.dump(s))
        d = eng.dump(0)  # the stop-limit at 90 took the last bid, at 96, and rests two lots
        assert len(d) == 1 and (int(d[0]["price_q4"]), int(d[0]["qty"]), int(d[0]["side"])) == (90, 2, SELL)
        assert len(eng.stops_dump()) == 0
        # (the fifth batch found no stop left: no job)
        _no_deferral(eng, jobs=4, events=4, live=0)


# ---- 8. independence ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["gwalk", "deep"])
def test_the_feeds_and_the_outputs_do_not_depend_on_it(me, path):
    """The same stream with the quote, depth and trade feeds on, once without the trigger book and once with
    stops pending (some trigger): results, tapes, book dumps and the three feeds' events are equal."""
    S, L, grouped = 24, PATHS[path][0], PATHS[path][3]
    nb, batch = 6, 300
    base, batches = _c5_stream(me, S, L, nb, batch)

    def run(stops):
        kw = {"batches_per_launch": 4} if grouped else {}
        with feed_engine(me, path, S, base, batch, 2 * nb * batch + 1024, **kw) as eng:
            eng.quotes_enable(64 * S)
            eng.depth_enable(4, 64 * 16 * S)
            eng.trades_enable(64 * S)
            if stops:
                eng.stops_enable(4 * S)
                eng.stops_add(sm.stops([(1 + s, int(base[s]) + (s % 5) * 20, 0, 1, s, me.kind(BUY, 1)) for s in range(S)] +
                                       [(100 + s, I64_MAX, 0, 1, s, me.kind(BUY)) for s in range(S)]))
            if grouped:
                ts = [eng.submit_host(b) for b in batches]
                outs = [eng.collect(t) for t in ts]
            else:
                outs = [eng.submit_batch(b) for b in batches]
            eng.sync()
            q, d, t = eng.quotes_drain(), eng.depth_drain(), eng.trades_drain()
            n = len(eng.stops_drain()) if stops else 0
            if stops:
                _no_deferral(eng, events=n, live=2 * S - n)
            dumps = [eng.dump(s) for s in range(S)]
            return outs, q, d, t, dumps, n

    a, b = run(False), run(True)
    assert 0 < b[5] <= S and len(a[1]) > 0 and len(a[2]) > 0 and len(a[3]) > 0
    for (ra, fa), (rb, fb) in zip(a[0], b[0]):
        assert np.array_equal(ra, rb) and np.array_equal(fa, fb)
    _same(b[1], a[1], f"{path}: quote events")
    _same(b[2], a[2], f"{path}: depth events")
    _same(b[3], a[3], f"{path}: trade events")
    for da, db in zip(a[4], b[4]):
        assert np.array_equal(da, db)


def test_enabled_and_empty_runs_no_job_and_off_is_invalid(me):
    S, L = 8, 128
    base, batches = _c5_stream(me, S, L, 3, 200)
    with me.Engine(S, L, base, max_batch=200, max_resting=4096, seq_ring=1 << 20) as eng:
        with pytest.raises(me.EngineError) as ei:  # never enabled
            eng.stops_stats()
        assert ei.value.code == me.ME_E_INVALID
        eng.stops_enable(16)
        n = 0
        for b in batches:
            n += len(eng.submit_batch(b)[1])
        assert n > 0
        _no_deferral(eng, jobs=0, events=0, live=0)
        assert len(eng.stops_drain()) == 0 and len(eng.stops_dump()) == 0
        with pytest.raises(me.EngineError) as ei:
            eng.stops_enable((1 << 22) + 1)
        assert ei.value.code == me.ME_E_INVALID
        with pytest.raises(me.EngineError) as ei:  # a failing enable leaves it off
            eng.stops_stats()
        assert ei.value.code == me.ME_E_INVALID
        eng.stops_enable(16)
        eng.stops_enable(0)
        for call in (eng.stops_read, eng.stops_stats, eng.stops_dump, lambda: eng.stops_cancel([1]),
                     lambda: eng.stops_add(sm.stops([(1, 0, 0, 1, 0, me.kind(BUY))]))):
            with pytest.raises(me.EngineError) as ei:
                call()
            assert ei.value.code == me.ME_E_INVALID
        eng.submit_batch(me.Batch([10 ** 9], [int(base[0])], [1], [0], [me.kind(BUY)]))  # the engine is fine
