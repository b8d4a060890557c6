"""The depth feed (me_depth_*) on every matching path against the model
(tests/depth_model.py over the CPU oracle): exact array equality of every job's events. Needs an MI355X.

Every test but the log-full one sizes the log so that no job defers, and asserts it: a deferral must not
be able to hide a missing event.
"""
import numpy as np
import pytest

from tests import depth_model as dm
from tests import quote_model as qm
from tests.feed_common import BIG, BUY, SELL, Rows, _c5_stream, _same
from tests.gpu_harness import FEED_PATHS as PATHS, SMALL, env, feed_engine

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle

    return oracle


def _no_deferral(eng, groups=None):
    st = eng.depth_stats()
    assert st["deferred"] == 0, st
    if groups is not None:
        assert st["groups"] == groups, st
    return st


def _pq(ev):
    return [(int(e["price_q4"]), int(e["qty"])) for e in ev]


def _step(eng, ob, rows):
    b = rows.batch()
    eng.submit_batch(b)
    ob.submit(b)


def _replays_to(eng, S, D, got, ids=None):
    return dm.same_views(dm.replay(dm.empty_maps(S), got, ids), dm.views(eng, S, D))


# ---- every path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,group", [(p, g) for p in SMALL for g in (1, 8, 32)] +
                         [(p, 1) for p in PATHS if p not in SMALL])
def test_events_of_every_group_on_every_path(me, orc, path, group):
    """A config-5-style stream (cancels, MARKET sweeps, 3 % far prices), D = 5. Bucketed paths: device batches
    in groups of G, all enqueued before one sync, a partial group last; deep paths: one synchronous batch per
    job. The events of every job equal the model's. On gwalk_cx the quote feed runs beside it, unchanged."""
    S, L, D = 12, PATHS[path][0], 5
    grouped = PATHS[path][3]
    nb, batch = (70, 60) if grouped else (4, 1500)
    base, batches = _c5_stream(me, S, L, nb, batch)
    total = nb * batch
    ob = orc.OracleBook(S)
    model = dm.DepthModel(ob, S, D)
    both = path == "gwalk_cx"
    qmodel = qm.QuoteModel(ob, S) if both else None
    kw = {"batches_per_launch": group} if grouped else {}
    with feed_engine(me, path, S, base, batch, 2 * total + 1024, **kw) as eng:
        if both:
            eng.quotes_enable(64 * S * (nb + 1))
        eng.depth_enable(D, 4 * D * S * (nb + 2))
        exp = [model.expect(0)]
        qexp = [qmodel.expect(0)] if both else None
        if grouped:
            dbs = [eng.upload(b) for b in batches]
            try:
                for db in dbs:
                    eng.submit_device(db)
                eng.sync()
            finally:
                for db in dbs:
                    db.free()
            bounds = list(range(group, nb, group)) + [nb]
        else:
            for b in batches:
                eng.submit_batch(b)
            bounds = list(range(1, nb + 1))
        done = 0
        for x in bounds:
            for b in batches[done:x]:
                ob.submit(b)
            done = x
            exp.append(model.expect(x))
            if both:
                qexp.append(qmodel.expect(x))
        got = eng.depth_drain()
        exp = np.concatenate(exp)
        assert len(exp) > len(bounds)  # (more events than jobs: the stream moves the views)
        _same(got, exp, f"{path} G={group}")
        _no_deferral(eng, groups=1 + len(bounds))
        assert _replays_to(eng, S, D, got)
        if both:
            qgot = eng.quotes_drain()
            assert np.array_equal(qgot, np.concatenate(qexp)), "the quote feed beside the depth feed"
            assert eng.quotes_stats() == {"groups": 1 + len(bounds), "events": len(qgot), "deferred": 0}


# ---- side counts and depths: partial waves, the prefix across workgroups ---------------------------
@pytest.mark.parametrize("S,D", [(1, 3), (33, 3), (65, 3), (1030, 3), (65, 1), (65, 32)])
def test_side_counts_and_depths(me, orc, S, D):
    L = 128
    base = np.array([10_000 + 1_000 * s for s in range(S)], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = dm.DepthModel(ob, S, D)
    with me.Engine(S, L, base, max_batch=2 * D * S + 8, max_resting=4 * D * S + 64, seq_ring=1 << 20) as eng:
        eng.depth_enable(D, 8 * D * S)
        _same(eng.depth_drain(), model.expect(0), "enable on empty books")
        rows = Rows(me)
        # every symbol changes: D levels per side
        for s in range(S):
            for i in range(D):
                rows.limit(s, BUY, int(base[s]) + 40 - i, 5 + s % 7)
                rows.limit(s, SELL, int(base[s]) + 60 + i, 3 + i)
        _step(eng, ob, rows)
        ev = eng.depth_drain()
        assert len(ev) == 2 * D * S and (ev["qty"] > 0).all()
        _same(ev, model.expect(1), "every symbol")
        got = [ev]
        # nothing changes: orders behind the D-th level, and a cancel of nothing
        for s in (0, S // 2, S - 1):
            rows.limit(s, BUY, int(base[s]) + 40 - D, 9)
            rows.limit(s, SELL, int(base[s]) + 60 + D, 9)
        rows.cancel(0, 1 << 40)
        _step(eng, ob, rows)
        before = _no_deferral(eng)
        ev = eng.depth_drain()
        assert len(ev) == 0 and len(model.expect(2)) == 0
        st = _no_deferral(eng, groups=3)
        assert st["events"] == before["events"] == 2 * D * S
        # only the last symbol's ask side changes
        rows.limit(S - 1, SELL, int(base[S - 1]) + 60, 2)
        _step(eng, ob, rows)
        ev = eng.depth_drain()
        assert len(ev) == 1 and ev[0]["symbol"] == S - 1 and ev[0]["side"] == SELL
        assert _pq(ev) == [(int(base[S - 1]) + 60, 5)]
        _same(ev, model.expect(3), "last symbol's asks")
        _no_deferral(eng, groups=4)
        assert _replays_to(eng, S, D, np.concatenate(got + [ev]))


class _Only:
    """The oracle's snapshots of the symbols a test touched; the others are empty without asking."""

    def __init__(self, ob, touched):
        self.ob, self.touched = ob, touched

    def snapshot(self, s, depth):
        return self.ob.snapshot(s, depth) if s in self.touched else ((), ())


def test_many_offset_rounds_and_long_emit_runs(me, orc):
    """S = 70,000: the offsets pass carries its running total through 137 rounds of 1,024 counts (S = 1,030
    above takes three), and an emit wave's run is 69 sides, more than one 64-count load (runs pass 64 sides
    only above S = 65,536). Every seventh symbol trades, which puts changed sides into the second load of
    many runs and leaves whole runs unchanged between them; the last symbol trades too."""
    S, L, D = 70_000, 128, 2
    assert -(-2 * S // 2048) > 64 and 2 * S > 100 * 1024
    base = np.full(S, 50_000, dtype=np.int64)
    touched = sorted(set(range(0, S, 7)) | {S - 1})
    ob = orc.OracleBook(S)
    model = dm.DepthModel(_Only(ob, set(touched)), S, D)
    with me.Engine(S, L, base, max_batch=2 * len(touched) + 8, max_resting=8 * len(touched), seq_ring=1 << 20) as eng:
        eng.depth_enable(D, 1)  # 4 * D * S
        assert len(eng.depth_drain()) == 0 and len(model.expect(0)) == 0
        rows = Rows(me)
        for s in touched:
            rows.limit(s, BUY, 50_040 - s % 3, 1 + s % 5)
            rows.limit(s, SELL, 50_060 + s % 4, 2 + s % 3)
        _step(eng, ob, rows)
        ev = eng.depth_drain()
        _same(ev, model.expect(1), "every seventh symbol")
        assert len(ev) == 2 * len(touched) and ev["symbol"][::2].tolist() == touched
        # sides 69 w + 64 .. 69 w + 68 are a run's second load: symbols that own one change again
        second = [s for s in touched if (2 * s) % 69 >= 64 or (2 * s + 1) % 69 >= 64]
        assert len(second) > 100
        again = sorted(set(second) | {S - 1})
        for s in again:
            rows.limit(s, BUY, 50_041, 3)           # a new best bid: one SET, the old best stays in view
            rows.limit(s, SELL, 50_060 + s % 4, 1)  # one more order on the best ask: one SET
        _step(eng, ob, rows)
        ev = eng.depth_drain()
        _same(ev, model.expect(2), "second loads")
        assert len(ev) == 2 * len(again) and ev["symbol"][::2].tolist() == again
        _no_deferral(eng, groups=3)


# ---- pushed out and back ---------------------------------------------------------------------------
def test_pushed_out_and_back(me, orc):
    S, L, D = 1, 128, 3
    base = np.array([1_000], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = dm.DepthModel(ob, S, D)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20) as eng:
        eng.depth_enable(D, 256)
        model.expect(0)
        rows = Rows(me)
        got = []

        def job(k, want):
            _step(eng, ob, rows)
            ev = eng.depth_drain()
            _same(ev, model.expect(k), f"job {k}")
            assert _pq(ev) == want and (ev["side"] == BUY).all()
            got.append(ev)

        a = rows.limit(0, BUY, 1_030, 5)
        b1 = rows.limit(0, BUY, 1_020, 6)
        b2 = rows.limit(0, BUY, 1_020, 1)
        rows.limit(0, BUY, 1_010, 7)
        job(1, [(1_030, 5), (1_020, 7), (1_010, 7)])
        rows.limit(0, BUY, 1_040, 4)  # a better level: the worst leaves the view although it still rests
        job(2, [(1_040, 4), (1_010, 0)])
        rows.market(0, SELL, 4)  # the best is taken: the pushed-out level is SET again
        job(3, [(1_040, 0), (1_010, 7)])
        rows.market(0, SELL, 2)  # a partial take: one SET with the smaller total
        job(4, [(1_030, 3)])
        rows.limit(0, BUY, 1_005, 9)  # behind the view
        job(5, [])
        rows.cancel(0, b1)  # cancels empty a middle level: it is deleted, the level behind moves in
        rows.cancel(0, b2)
        job(6, [(1_020, 0), (1_005, 9)])
        _no_deferral(eng, groups=7)
        assert _replays_to(eng, S, D, np.concatenate(got))
        assert a == 1


# ---- window plus far -------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [128, 1024])
def test_window_plus_far(me, orc, L):
    S, D = 3, 5
    base = np.array([1_000_000, 2_000_000, 3_000_000], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = dm.DepthModel(ob, S, D)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20, far_levels=4) as eng:
        eng.depth_enable(D, 1024)
        model.expect(0)
        b0 = int(base[1])
        mid = b0 + L // 2
        rows = Rows(me)
        got = []

        def job(k, n=None):
            _step(eng, ob, rows)
            ev = eng.depth_drain()
            _same(ev, model.expect(k), f"L={L} job {k}")
            assert n is None or len(ev) == n, ev
            assert (ev["symbol"] == 1).all()
            got.append(ev)
            assert _replays_to(eng, S, D, np.concatenate(got))
            return ev

        # asks: 2 window levels and 6 far levels (more than the inline region of 4): the view takes 2 + 3;
        # bids: a far-only side
        rows.limit(1, SELL, mid + 5, 10)
        rows.limit(1, SELL, mid + 6, 11)
        far_asks = [b0 + 6 * L + 10 * i for i in range(6)]
        for i, p in enumerate(far_asks):
            rows.limit(1, SELL, p, 20 + i)
        rows.limit(1, BUY, b0 - 3 * L, 7)
        rows.limit(1, BUY, b0 - 5 * L, 4)
        ev = job(1, 7)
        assert _pq(ev[ev["side"] == BUY]) == [(b0 - 3 * L, 7), (b0 - 5 * L, 4)]
        assert _pq(ev[ev["side"] == SELL]) == [(mid + 5, 10), (mid + 6, 11)] + [(p, 20 + i) for i, p in enumerate(far_asks[:3])]
        # a MARKET takes the best window ask: the fourth far level moves into the view
        rows.market(1, BUY, 10)
        ev = job(2, 2)
        assert _pq(ev) == [(mid + 5, 0), (far_asks[3], 23)]
        # an ask below the window re-centres it between jobs: levels move between window and far, prices
        # keep their place in the view, and only the new level and the one it pushes out are reported
        rows.limit(1, SELL, b0 - 2 * L, 3)
        ev = job(3, 2)
        assert _pq(ev) == [(b0 - 2 * L, 3), (far_asks[3], 0)]
        # and a bid above the far bids, inside the moved window
        rows.limit(1, BUY, b0 - 2 * L - 4, 8)
        ev = job(4, 1)
        assert _pq(ev) == [(b0 - 2 * L - 4, 8)]
        _no_deferral(eng, groups=5)


# ---- sparse deep window ----------------------------------------------------------------------------
def test_sparse_deep_window(me, orc):
    """L = 32,768: occupied levels more than 4,096 apart (a walk over several 64-word occ reads), at both
    window edges and at 64-level block boundaries; three idle symbols never yield an event."""
    S, L, D = 4, 32_768, 4
    base = np.array([1_000_000, 2_000_000, 3_000_000, 4_000_000], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = dm.DepthModel(ob, S, D)
    with env({"ME_HOT_MIN": "0"}):
        eng = me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20)
    with eng:
        eng.depth_enable(D, 1024)
        model.expect(0)
        rows = Rows(me)
        got = []
        b0 = int(base[0])

        def job(k):
            _step(eng, ob, rows)
            ev = eng.depth_drain()
            _same(ev, model.expect(k), f"job {k}")
            assert len(ev) > 0 and (ev["symbol"] == 0).all()
            got.append(ev)
            assert _replays_to(eng, S, D, np.concatenate(got))
            return ev

        bid = {l: rows.limit(0, BUY, b0 + l, 1 + l % 5) for l in (0, 63, 64)}
        ask = {l: rows.limit(0, SELL, b0 + l, 2 + l % 3) for l in (4_095, 4_096, 12_000, 20_000, L - 1)}
        ev = job(1)
        assert [p - b0 for p, _ in _pq(ev[ev["side"] == BUY])] == [64, 63, 0]
        assert [p - b0 for p, _ in _pq(ev[ev["side"] == SELL])] == [4_095, 4_096, 12_000, 20_000]
        rows.cancel(0, ask[4_095])
        rows.cancel(0, ask[4_096])
        ev = job(2)
        assert [(p - b0, q > 0) for p, q in _pq(ev)] == [(4_095, False), (4_096, False), (L - 1, True)]
        rows.cancel(0, ask[12_000])
        rows.cancel(0, ask[20_000])
        bid[9_000] = rows.limit(0, BUY, b0 + 9_000, 4)
        bid[20_000] = rows.limit(0, BUY, b0 + 20_000, 6)
        ev = job(3)
        assert [(p - b0, q > 0) for p, q in _pq(ev[ev["side"] == BUY])] == [(20_000, True), (9_000, True), (0, False)]
        assert [(p - b0, q > 0) for p, q in _pq(ev[ev["side"] == SELL])] == [(12_000, False), (20_000, False)]
        for l in (20_000, 9_000, 64):
            rows.cancel(0, bid[l])
        ev = job(4)
        assert [(p - b0, q > 0) for p, q in _pq(ev)] == [(20_000, False), (9_000, False), (64, False), (0, True)]
        _no_deferral(eng, groups=5)


# ---- values ----------------------------------------------------------------------------------------
def test_values_int64_totals_zero_and_negative_prices_emptied_books(me, orc):
    S, L, D = 4, 128, 2
    base = np.array([-64, -1_000, 5_000, 9_000], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = dm.DepthModel(ob, S, D)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20) as eng:
        eng.depth_enable(D, 256)
        model.expect(0)
        rows = Rows(me)
        ids = [rows.limit(0, BUY, 0, 5),       # price 0 is a price
               rows.limit(0, BUY, -1, 6),      # a negative one inside the view
               rows.limit(0, BUY, -2, 7)]      # and one outside it
        ids += [rows.limit(1, SELL, -990, 6), rows.limit(1, SELL, -980, 1)]
        ids += [rows.limit(2, BUY, 5_010, BIG), rows.limit(2, BUY, 5_010, BIG)]  # a level total above 2^31
        ids += [rows.limit(3, SELL, 9_050, 1)]
        _step(eng, ob, rows)
        ev = first = eng.depth_drain()
        _same(ev, model.expect(1), "values")
        assert ev["symbol"].tolist() == [0, 0, 1, 1, 2, 3]
        assert _pq(ev) == [(0, 5), (-1, 6), (-990, 6), (-980, 1), (5_010, 4_294_967_294), (9_050, 1)]
        assert not ev["pad"].any()
        # every book emptied whole: DELETEs only, in priority order (-2 was never in the view)
        for s, oid in zip((0, 0, 0, 1, 1, 2, 2, 3), ids):
            rows.cancel(s, oid)
        _step(eng, ob, rows)
        ev = eng.depth_drain()
        _same(ev, model.expect(2), "emptied")
        assert _pq(ev) == [(0, 0), (-1, 0), (-990, 0), (-980, 0), (5_010, 0), (9_050, 0)]
        _no_deferral(eng, groups=3)
        assert dm.replay(dm.empty_maps(S), np.concatenate([first, ev])) == dm.empty_maps(S)


def test_symbol_ids_name_the_events(me, orc):
    S, L, D = 70, 128, 2
    ids = np.arange(S, dtype=np.uint32) * 3 + 1000
    base = np.full(S, 50_000, dtype=np.int64)
    ob = orc.OracleBook(S)
    model = dm.DepthModel(ob, S, D, symbol_ids=ids)
    with me.Engine(S, L, base, max_batch=256, max_resting=1024, seq_ring=1 << 20, symbol_ids=ids) as eng:
        eng.depth_enable(D, 1)  # raised to 4 * D * num_symbols
        model.expect(0)
        rows = Rows(me)
        for s in range(S):
            rows.limit(s, SELL, 50_070 + s % 3, 2)
        _step(eng, ob, rows)
        ev = eng.depth_drain()
        _same(ev, model.expect(1), "symbol ids")
        assert ev["symbol"].tolist() == ids.tolist()
        _no_deferral(eng, groups=2)
        assert _replays_to(eng, S, D, ev, ids)


# ---- the host pipeline -----------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 4])
def test_host_pipeline_events_are_there_after_collect(me, orc, group):
    """submit_host with two tickets in flight. After collect(t) a read that launches and waits for nothing
    holds every event stamped <= t + 1 (t's ordinal): the events read so far replay to the books' views after
    some X >= t + 1 batches, and for every stamp X seen, the events up to it replay to the views after X."""
    S, L, D, nb, batch = 12, 128, 5, 13, 200
    base, batches = _c5_stream(me, S, L, nb, batch)
    ob = orc.OracleBook(S)
    after = [dm.views(ob, S, D)]
    for b in batches:
        ob.submit(b)
        after.append(dm.views(ob, S, D))
    cap = 4 * D * S * (nb + 2)
    with feed_engine(me, "reg", S, base, batch, nb * batch + 1024, batches_per_launch=group) as eng:
        eng.depth_enable(D, cap)
        got = np.zeros(0, dtype=dm.DEPTH_DTYPE)
        tickets = []

        def collected(t, submitted):
            nonlocal got
            eng.collect(t)
            ev, left = eng.depth_read(cap)
            assert left == 0
            got = np.concatenate([got, ev])
            maps = dm.replay(dm.empty_maps(S), got)
            assert any(dm.same_views(maps, after[x]) for x in range(t + 1, submitted + 1)), f"after collect({t})"

        for k, b in enumerate(batches):
            tickets.append(eng.submit_host(b))
            if len(tickets) > 2:
                collected(tickets.pop(0), k + 1)
        for t in tickets:
            collected(t, nb)
        assert np.all(np.diff(got["batches"].astype(np.int64)) >= 0)
        for x in np.unique(got["batches"]):
            maps = dm.replay(dm.empty_maps(S), got[got["batches"] <= x])
            assert dm.same_views(maps, after[int(x)]), f"events up to stamp {x}"
        eng.sync()
        assert len(eng.depth_drain()) == 0
        _no_deferral(eng)


# ---- the bounded log -------------------------------------------------------------------------------
def test_log_full_defers_and_catches_up(me, orc):
    S, L, D = 8, 128, 4
    base = np.full(S, 20_000, dtype=np.int64)
    ob = orc.OracleBook(S)
    model = dm.DepthModel(ob, S, D)
    with me.Engine(S, L, base, max_batch=4 * D * S, max_resting=64 * D * S, seq_ring=1 << 20) as eng:
        eng.depth_enable(D, 1)  # the minimum: 4 * D * S = 128 events
        exp = [model.expect(0)]
        rows = Rows(me)

        def all_levels_change():  # 2 D levels of every symbol: 64 events
            for s in range(S):
                for i in range(D):
                    rows.limit(s, BUY, 20_040 - i, 1 + s)
                    rows.limit(s, SELL, 20_060 + i, 2 + s)
            _step(eng, ob, rows)

        all_levels_change()
        exp.append(model.expect(1))
        all_levels_change()  # 128 events logged: the log is full
        exp.append(model.expect(2))
        assert eng.depth_stats() == {"groups": 3, "events": 128, "deferred": 0}
        all_levels_change()  # does not fit: deferred, nothing emitted, nothing published
        assert eng.depth_stats() == {"groups": 4, "events": 128, "deferred": 1}
        pending = model.peek()
        assert len(pending) == 64
        rows.limit(0, BUY, 20_040, 3)  # a second deferred job; its change conflates with the first's
        _step(eng, ob, rows)
        assert eng.depth_stats() == {"groups": 5, "events": 128, "deferred": 2}
        first, left = eng.depth_read(127)  # the log is not read empty yet: no catch-up
        assert len(first) == 127 and left == 1 and eng.depth_stats()["groups"] == 5
        rest = eng.depth_drain()  # reads the last one, then the catch-up job's events
        exp.append(model.expect(4))
        assert len(exp[-1]) == 64 and exp[-1][0]["qty"] == 3 * 1 + 3  # (one event per level: conflated)
        got = np.concatenate([first, rest])
        _same(got, np.concatenate(exp), "log full")
        assert eng.depth_stats() == {"groups": 6, "events": 128 + 64, "deferred": 2}
        assert dm.same_views(dm.replay(dm.empty_maps(S), got), dm.views(ob, S, D))
        assert _replays_to(eng, S, D, got)
        # a deferred change that a later job carries once the log has room again
        all_levels_change()  # 64 events beside nothing unread: fits
        all_levels_change()  # 128: full
        rows.limit(1, SELL, 20_059, 1)
        _step(eng, ob, rows)  # deferred
        assert eng.depth_stats()["deferred"] == 3
        ev, left = eng.depth_read(100)  # 28 stay unread: no catch-up
        assert len(ev) == 100 and left == 28
        got = np.concatenate([got, ev])
        rows.limit(2, BUY, 20_041, 1)
        _step(eng, ob, rows)  # 4 events: fits, and carries the deferred ones
        assert eng.depth_stats()["deferred"] == 3
        got = np.concatenate([got, eng.depth_drain()])
        assert (got[-4:]["symbol"] == [1, 1, 2, 2]).all() and (got[-4:]["batches"] == 8).all()
        assert dm.same_views(dm.replay(dm.empty_maps(S), got), dm.views(ob, S, D))


# ---- enabling mid-stream, invalid use --------------------------------------------------------------
@pytest.mark.parametrize("path", ["reg", "deep"])
def test_enable_mid_stream(me, orc, path):
    S, L, D = 65, PATHS[path][0], 4
    base, batches = _c5_stream(me, S, L, 3, 300)
    ob = orc.OracleBook(S)
    with feed_engine(me, path, S, base, 300, 2048) as eng:
        for b in batches[:2]:
            eng.submit_batch(b)
            ob.submit(b)
        eng.depth_enable(D, 8 * D * S)
        model = dm.DepthModel(ob, S, D)
        exp = model.expect(2)
        vw = dm.views(ob, S, D)
        assert 0 < len(exp) == sum(len(v[0]) + len(v[1]) for v in vw) and (exp["qty"] > 0).all()
        _same(eng.depth_drain(), exp, "first read after enabling")
        eng.submit_batch(batches[2])
        ob.submit(batches[2])
        _same(eng.depth_drain(), model.expect(3), "the batch after")
        _no_deferral(eng, groups=2)
        # enabling again, with another depth, starts afresh; 0 turns the feed off
        eng.depth_enable(2, 1)
        _same(eng.depth_drain(), dm.DepthModel(ob, S, 2).expect(3), "re-enabled at D = 2")
        _no_deferral(eng, groups=1)
        eng.depth_enable(0, 0)
        with pytest.raises(me.EngineError) as ei:
            eng.depth_read()
        assert ei.value.code == me.ME_E_INVALID


def test_invalid_use(me):
    with me.Engine(4, 128, [1000] * 4, 64, 1024, 1 << 20) as eng:
        for call in (eng.depth_read, eng.depth_stats,                 # the feed is off
                     lambda: eng.depth_enable(33, 1024),              # deeper than ME_DEPTH_MAX
                     lambda: eng.depth_enable(32, (1 << 26) + 1)):    # a log above 2^26 events
            with pytest.raises(me.EngineError) as ei:
                call()
            assert ei.value.code == me.ME_E_INVALID
        with pytest.raises(me.EngineError):  # none of them turned it on
            eng.depth_stats()
        eng.depth_enable(32, 1)
        assert eng.depth_stats() == {"groups": 1, "events": 0, "deferred": 0}
