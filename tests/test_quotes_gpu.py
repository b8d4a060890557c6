"""The top-of-book change feed (me_quotes_*) on every matching path against the model
(tests/quote_model.py over the CPU oracle): exact array equality of every job's events. Needs an MI355X.

Every test but the log-full one sizes the log so that no job defers, and asserts it: a deferral must not
be able to hide a missing event.
"""
import numpy as np
import pytest

from tests import quote_model as qm
from tests.feed_common import BIG, BUY, SELL, Rows, _c5_stream, _same
from tests.gpu_harness import FEED_PATHS as PATHS, SMALL, feed_engine

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
    st = eng.quotes_stats()
    assert st["deferred"] == 0, st
    if groups is not None:
        assert st["groups"] == groups, st
    return st


# ---- every path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,group", [(p, g) for p in SMALL for g in (1, 8, 32)] +
                         [(p, 1) for p in PATHS if p not in SMALL])
def test_events_of_every_group_on_every_path(me, orc, path, group):
    """A config-5-style stream (cancels, MARKET sweeps, 3 % far prices). Bucketed paths: device batches in
    groups of G, all enqueued before one sync (the pipeline runs as in production), a partial group last;
    deep paths: one synchronous batch per job. The events of every job equal the model's."""
    S, L = 12, PATHS[path][0]
    grouped = PATHS[path][3]
    nb, batch = (70, 60) if grouped else (4, 1500)
    base, batches = _c5_stream(me, S, L, nb, batch)
    total = nb * batch
    ob = orc.OracleBook(S)
    model = qm.QuoteModel(ob, S)
    kw = {"batches_per_launch": group} if grouped else {}
    with feed_engine(me, path, S, base, batch, 2 * total + 1024, **kw) as eng:
        eng.quotes_enable(64 * S * (nb + 1))
        exp = [model.expect(0)]
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
        got = eng.quotes_drain()
        exp = np.concatenate(exp)
        assert len(exp) > len(bounds)  # (the stream moves the tops)
        _same(got, exp, f"{path} G={group}")
        _no_deferral(eng, groups=1 + len(bounds))
        if path in ("hot_agg", "hot"):  # (a hot symbol was picked, and its cancels left the walk)
            assert eng.stats()["hot_handoffs"] > 0
        # and the feed agrees with the engine's own snapshot
        assert qm.same_quotes(qm.replay(qm.tops(qm._Empty(), S), got), qm.tops(eng, S))


# ---- symbol counts: partial waves, the cross-wave prefix ------------------------------------------
@pytest.mark.parametrize("S", [1, 63, 65, 130, 1030])
def test_symbol_counts(me, orc, S):
    L = 128
    base = np.array([10_000 + 1_000 * s for s in range(S)], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = qm.QuoteModel(ob, S)
    with me.Engine(S, L, base, max_batch=2 * S + 8, max_resting=8 * S + 64, seq_ring=1 << 20) as eng:
        eng.quotes_enable(4 * S)
        _same(eng.quotes_drain(), model.expect(0), "enable on empty books")
        rows = Rows(me)
        # every symbol changes
        for s in range(S):
            rows.limit(s, BUY, int(base[s]) + 10, 5 + s % 7)
            rows.limit(s, SELL, int(base[s]) + 20, 3)
        b = rows.batch()
        eng.submit_batch(b)
        ob.submit(b)
        ev = eng.quotes_drain()
        assert len(ev) == S and ev["symbol"].tolist() == list(range(S))
        _same(ev, model.expect(1), "every symbol")
        # nothing changes: orders behind the best levels, and a cancel of nothing
        for s in (0, S // 2, S - 1):
            rows.limit(s, BUY, int(base[s]) + 5, 9)
            rows.limit(s, SELL, int(base[s]) + 30, 9)
        rows.cancel(0, 1 << 40)
        b = rows.batch()
        eng.submit_batch(b)
        ob.submit(b)
        before = _no_deferral(eng)
        ev = eng.quotes_drain()
        assert len(ev) == 0 and len(model.expect(2)) == 0
        st = _no_deferral(eng, groups=3)
        assert st["events"] == before["events"] == S
        # only the last symbol changes
        rows.limit(S - 1, BUY, int(base[S - 1]) + 11, 2)
        b = rows.batch()
        eng.submit_batch(b)
        ob.submit(b)
        ev = eng.quotes_drain()
        assert len(ev) == 1 and ev[0]["symbol"] == S - 1 and ev[0]["bid_price_q4"] == int(base[S - 1]) + 11
        _same(ev, model.expect(3), "last symbol")
        _no_deferral(eng, groups=4)


# ---- far best --------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [128, 1024])
def test_far_levels_are_the_best_of_an_empty_window_side(me, orc, L):
    S = 3
    base = np.array([1_000_000, 2_000_000, 3_000_000], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = qm.QuoteModel(ob, S)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20) as eng:
        eng.quotes_enable(64)
        model.expect(0)
        mid = int(base[1]) + L // 2
        far_bid, far_bid2, far_ask = int(base[1]) - 3 * L, int(base[1]) - 5 * L, int(base[1]) + 6 * L
        steps = []
        rows = Rows(me)
        # an ask inside the window, bids far below it: the bid quote is the better far price
        rows.limit(1, SELL, mid + 5, 10)
        rows.limit(1, BUY, far_bid2, 4)
        rows.limit(1, BUY, far_bid, 7)
        rows.limit(1, BUY, far_bid, 2)
        steps.append((rows.batch(), (far_bid, 9, mid + 5, 10, 3)))
        # a far ask behind the window's; a MARKET sweeps the window's asks: the ask side is far-only
        rows.limit(1, SELL, far_ask, 6)
        rows.market(1, BUY, 10)
        steps.append((rows.batch(), (far_bid, 9, far_ask, 6, 3)))
        # the far ask goes too: the ask side is absent; the best far bid is cancelled: the next one shows
        rows.market(1, BUY, 6)
        rows.cancel(1, 3)
        rows.cancel(1, 4)
        steps.append((rows.batch(), (far_bid2, 4, 0, 0, 1)))
        for k, (b, (bp, bq, ap, aq, fl)) in enumerate(steps):
            eng.submit_batch(b)
            ob.submit(b)
            ev = eng.quotes_drain()
            _same(ev, model.expect(k + 1), f"L={L} step {k}")
            assert len(ev) == 1 and ev[0]["symbol"] == 1
            e = ev[0]
            assert (e["bid_price_q4"], e["bid_qty"], e["ask_price_q4"], e["ask_qty"], e["flags"]) == (bp, bq, ap, aq, fl)
        _no_deferral(eng, groups=4)


# ---- values ----------------------------------------------------------------------------------------
def test_values_int64_totals_zero_and_negative_prices_emptied_books(me, orc):
    S, L = 4, 128
    base = np.array([-64, -1_000, 5_000, 9_000], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = qm.QuoteModel(ob, S)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20) as eng:
        eng.quotes_enable(64)
        model.expect(0)
        rows = Rows(me)
        rows.limit(0, BUY, 0, 5)            # price 0 is a price
        rows.limit(1, SELL, -990, 6)        # so is a negative one
        a = rows.limit(2, BUY, 5_010, BIG)  # a level total above 2^31
        b_ = rows.limit(2, BUY, 5_010, BIG)
        c = rows.limit(3, SELL, 9_050, 1)
        b = rows.batch()
        eng.submit_batch(b)
        ob.submit(b)
        ev = eng.quotes_drain()
        _same(ev, model.expect(1), "values")
        assert ev["symbol"].tolist() == [0, 1, 2, 3]
        assert ev[0]["flags"] == 1 and ev[0]["bid_price_q4"] == 0 and ev[0]["bid_qty"] == 5
        assert ev[1]["flags"] == 2 and ev[1]["ask_price_q4"] == -990
        assert ev[2]["bid_qty"] == 2 * BIG == 4_294_967_294
        # emptied by cancels: flags 0, prices and quantities 0
        rows.cancel(2, a)
        rows.cancel(2, b_)
        rows.cancel(3, c)
        b = rows.batch()
        eng.submit_batch(b)
        ob.submit(b)
        ev = eng.quotes_drain()
        _same(ev, model.expect(2), "emptied")
        assert ev["symbol"].tolist() == [2, 3] and not ev["flags"].any()
        assert not ev["bid_price_q4"].any() and not ev["bid_qty"].any() and not ev["ask_price_q4"].any()
        _no_deferral(eng, groups=3)


def test_symbol_ids_name_the_events(me, orc):
    S, L = 70, 128
    ids = np.arange(S, dtype=np.uint32) * 3 + 1000
    base = np.full(S, 50_000, dtype=np.int64)
    ob = orc.OracleBook(S)
    model = qm.QuoteModel(ob, S, symbol_ids=ids)
    with me.Engine(S, L, base, max_batch=256, max_resting=1024, seq_ring=1 << 20, symbol_ids=ids) as eng:
        eng.quotes_enable(1)  # raised to num_symbols
        model.expect(0)
        rows = Rows(me)
        for s in range(S):
            rows.limit(s, SELL, 50_070 + s % 3, 2)
        b = rows.batch()
        eng.submit_batch(b)
        ob.submit(b)
        ev = eng.quotes_drain()
        _same(ev, model.expect(1), "symbol ids")
        assert ev["symbol"].tolist() == ids.tolist()
        _no_deferral(eng, groups=2)


# ---- the host pipeline -----------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 4])
def test_host_pipeline_events_are_there_after_collect(me, orc, group):
    """submit_host with two tickets in flight. After collect(t) a read that launches and waits for nothing
    holds every event stamped <= t + 1 (t's ordinal): the events read so far replay to the books' tops after
    some X >= t + 1 batches, and for every stamp X seen, the events up to it replay to the tops after X."""
    S, L, nb, batch = 12, 128, 13, 200
    base, batches = _c5_stream(me, S, L, nb, batch)
    ob = orc.OracleBook(S)
    after = [qm.tops(ob, S)]
    for b in batches:
        ob.submit(b)
        after.append(qm.tops(ob, S))
    with feed_engine(me, "reg", S, base, batch, nb * batch + 1024, batches_per_launch=group) as eng:
        eng.quotes_enable(64 * S * nb)
        got = np.zeros(0, dtype=qm.QUOTE_DTYPE)
        tickets = []

        def collected(t, submitted):
            nonlocal got
            eng.collect(t)
            ev, left = eng.quotes_read(64 * S * nb)
            assert left == 0
            got = np.concatenate([got, ev])
            table = qm.replay(qm.tops(qm._Empty(), S), got)
            assert any(qm.same_quotes(table, after[x]) for x in range(t + 1, submitted + 1)), f"after collect({t})"

        for k, b in enumerate(batches):
            tickets.append(eng.submit_host(b))
            if len(tickets) > 2:
                collected(tickets.pop(0), k + 1)
        for t in tickets:
            collected(t, nb)
        assert np.all(np.diff(got["batches"].astype(np.int64)) >= 0)
        for x in np.unique(got["batches"]):
            table = qm.replay(qm.tops(qm._Empty(), S), got[got["batches"] <= x])
            assert qm.same_quotes(table, after[int(x)]), f"events up to stamp {x}"
        eng.sync()
        assert len(eng.quotes_drain()) == 0
        _no_deferral(eng)


# ---- the bounded log -------------------------------------------------------------------------------
def test_log_full_defers_and_catches_up(me, orc):
    S, L = 130, 128
    base = np.full(S, 20_000, dtype=np.int64)
    ob = orc.OracleBook(S)
    with me.Engine(S, L, base, max_batch=2 * S, max_resting=8 * S, seq_ring=1 << 20) as eng:
        eng.quotes_enable(S)
        rows = Rows(me)
        for step in range(2):  # two all-change jobs, nothing read in between
            for s in range(S):
                rows.limit(s, BUY, 20_010 + step, 1 + s)
            b = rows.batch()
            eng.submit_batch(b)
            ob.submit(b)
        st = eng.quotes_stats()
        assert st == {"groups": 3, "events": S, "deferred": 1}, st
        first, left = eng.quotes_read(S - 1)  # the log is not read empty yet: no catch-up
        assert len(first) == S - 1 and left == 1 and eng.quotes_stats()["groups"] == 3
        rest = eng.quotes_drain()
        got = np.concatenate([first, rest])
        assert len(got) == 2 * S and (got[:S]["batches"] == 1).all() and (got[S:]["batches"] == 2).all()
        assert (got[:S]["bid_price_q4"] == 20_010).all() and (got[S:]["bid_price_q4"] == 20_011).all()
        st = eng.quotes_stats()
        assert st == {"groups": 4, "events": 2 * S, "deferred": 1}, st
        assert qm.same_quotes(qm.replay(qm.tops(qm._Empty(), S), got), qm.tops(ob, S))
        # a deferred change that a later job carries: fill the log again, then free it before the next job
        def step(records):
            for s, side, px in records:
                rows.limit(s, side, px, 1)
            b = rows.batch()
            eng.submit_batch(b)
            ob.submit(b)

        step([(s, BUY, 20_012) for s in range(S)])   # fits the empty log and fills it
        step([(s, BUY, 20_013) for s in range(10)])  # ten changes, no room: deferred
        assert eng.quotes_stats() == {"groups": 6, "events": 3 * S, "deferred": 2}
        ev, left = eng.quotes_read(S - 1)            # one event stays: no catch-up
        assert len(ev) == S - 1 and left == 1
        got = np.concatenate([got, ev])
        step([(0, SELL, 20_100)])                    # the next job carries the ten, conflated with its own
        assert eng.quotes_stats() == {"groups": 7, "events": 3 * S + 10, "deferred": 2}
        ev = eng.quotes_drain()
        assert len(ev) == 11 and ev[1:]["symbol"].tolist() == list(range(10)) and (ev[1:]["batches"] == 5).all()
        assert ev[1]["flags"] == 3 and ev[1]["bid_price_q4"] == 20_013 and ev[1]["ask_price_q4"] == 20_100
        got = np.concatenate([got, ev])
        assert qm.same_quotes(qm.replay(qm.tops(qm._Empty(), S), got), qm.tops(ob, S))


# ---- enabling mid-stream, the feed off -------------------------------------------------------------
@pytest.mark.parametrize("path", ["reg", "deep"])
def test_enable_mid_stream(me, orc, path):
    S, L = 65, PATHS[path][0]
    base, batches = _c5_stream(me, S, L, 3, 300)
    ob = orc.OracleBook(S)
    with feed_engine(me, path, S, base, 300, 2048) as eng:
        for b in batches[:2]:
            eng.submit_batch(b)
            ob.submit(b)
        eng.quotes_enable(4 * S)
        model = qm.QuoteModel(ob, S)
        exp = model.expect(2)
        assert 0 < len(exp) <= S and exp["flags"].all()  # exactly the non-empty symbols
        _same(eng.quotes_drain(), exp, "first read after enabling")
        eng.submit_batch(batches[2])
        ob.submit(batches[2])
        _same(eng.quotes_drain(), model.expect(3), "the batch after")
        _no_deferral(eng, groups=2)
        # enabling again starts afresh; 0 turns the feed off
        eng.quotes_enable(4 * S)
        _same(eng.quotes_drain(), qm.QuoteModel(ob, S).expect(3), "re-enabled")
        eng.quotes_enable(0)
        with pytest.raises(me.EngineError) as ei:
            eng.quotes_read()
        assert ei.value.code == me.ME_E_INVALID


def test_feed_off_is_invalid(me):
    with me.Engine(4, 128, [1000] * 4, 64, 1024, 1 << 20) as eng:
        with pytest.raises(me.EngineError) as ei:
            eng.quotes_read()
        assert ei.value.code == me.ME_E_INVALID
        with pytest.raises(me.EngineError) as ei:
            eng.quotes_stats()
        assert ei.value.code == me.ME_E_INVALID
