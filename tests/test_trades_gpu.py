"""The trade feed (me_trades_*, DESIGN.md §2 "Trade feed") on every matching path against the model
(tests/trade_model.py fed the CPU oracle's tapes): exact array equality of every job's events. Needs an MI355X.

Every test but the log-full one sizes the log so that no job defers, and asserts it: a deferral must not be able to
hide a missing event.
"""
import functools

import numpy as np
import pytest

from tests import price_edges as pe
from tests import trade_model as tm
from tests.feed_common import BIG, BUY, SELL, Rows, _c5_stream, _same
from tests.gpu_harness import FEED_PATHS as PATHS, SMALL, env, feed_engine

pytestmark = pytest.mark.gpu

TIF_FOK, TIF_POST_ONLY = 2, 3


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle

    return oracle


def _no_deferral(eng, groups=None):
    st = eng.trades_stats()
    assert st["deferred"] == 0, st
    if groups is not None:
        assert st["groups"] == groups, st
    return st


def _trade(rows, s, px, q=1):
    """One fill of symbol s at px: a resting sell and the buy that takes it."""
    rows.limit(s, SELL, px, q)
    rows.limit(s, BUY, px, q)


# ---- every path and group size -----------------------------------------------------------------------
S_PATHS = 128
# group -> (batches, records per batch) on the small paths; the deep paths run SHAPE_DEEP, one batch per job
SHAPE = {1: (5, 400), 8: (12, 200), 32: (36, 100)}
SHAPE_DEEP = (4, 1500)


@functools.lru_cache(maxsize=None)
def _path_stream(me, orc, L, nb, batch, group):
    """(base, batches, events per job of the model, the tapes, half-the-symbols and two-batches guards): computed
    once per shape from the oracle alone and shared."""
    base, batches = _c5_stream(me, S_PATHS, L, nb, batch)
    ob = orc.OracleBook(S_PATHS)
    model = tm.TradeModel(S_PATHS)
    bounds = list(range(group, nb, group)) + [nb]
    exp, tapes, done, two = [], [], 0, False
    for x in bounds:
        for b in batches[done:x]:
            tapes.append(ob.submit(b)[1])
            model.feed(tapes[-1])
        done = x
        exp.append(model.expect(x))
        two = two or any(v >= 2 for v in model.spans.values())
    traded = len(np.unique(np.concatenate(exp)["symbol"]))
    return base, batches, bounds, exp, tapes, traded, two


@pytest.mark.parametrize("path,group", [(p, g) for p in SMALL for g in (1, 8, 32)] +
                         [(p, 1) for p in PATHS if p not in SMALL])
def test_events_of_every_group_on_every_path(me, orc, path, group):
    """A config-5-style stream (cancels, MARKET sweeps, 3 % far prices: symbols go through the continuation).
    Bucketed paths: device batches in groups of G, all enqueued before one sync, a partial group last; deep
    paths: one synchronous batch per job. The events of every job equal the model's."""
    L, grouped = PATHS[path][0], PATHS[path][3]
    nb, batch = SHAPE[group] if grouped else SHAPE_DEEP
    base, batches, bounds, exp, tapes, traded, two = _path_stream(me, orc, L, nb, batch, group if grouped else 1)
    # a silent feed cannot pass: on the oracle's side alone, half the symbols trade and (groups of several
    # batches) some event covers fills of two batches of one group
    assert traded >= S_PATHS // 2, traded
    assert two or group == 1
    total = nb * batch
    kw = {"batches_per_launch": group} if grouped else {}
    with feed_engine(me, path, S_PATHS, base, batch, 2 * total + 1024, **kw) as eng:
        eng.trades_enable(S_PATHS * (len(bounds) + 1))
        assert eng.trades_stats() == {"groups": 1, "events": 0, "deferred": 0}
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
            ev = eng.trades_drain()
            for x in bounds:  # the jobs by their stamps
                got.append(ev[ev["batches"] == x])
            assert sum(len(g) for g in got) == len(ev)
        else:
            for b in batches:
                eng.submit_batch(b)
                got.append(eng.trades_drain())
        for k, x in enumerate(bounds):
            _same(got[k], exp[k], f"{path} G={group} job {k}")
        _no_deferral(eng, groups=1 + len(bounds))
        if path == "reg":  # (continuation fills are folded)
            assert eng.stats()["handoffs"] > 0
        if path in ("hot_agg", "hot"):
            assert eng.stats()["hot_handoffs"] > 0
        tm.replay(np.concatenate(got), tapes, S_PATHS)


# ---- symbol counts: the mask words' edges ------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 63, 65, 130, 1030])
def test_symbol_counts(me, orc, S):
    L = 128
    base = np.array([10_000 + 1_000 * s for s in range(S)], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = tm.TradeModel(S)
    with me.Engine(S, L, base, max_batch=2 * S + 8, max_resting=8 * S + 64, seq_ring=1 << 20) as eng:
        eng.trades_enable(4 * S)
        assert len(eng.trades_drain()) == 0
        rows = Rows(me)

        def step(n):
            b = rows.batch()
            eng.submit_batch(b)
            model.feed(ob.submit(b)[1])
            ev = eng.trades_drain()
            _same(ev, model.expect(n), f"S={S} batch {n}")
            return ev

        for s in range(S):  # every symbol trades
            _trade(rows, s, int(base[s]) + 10 + s % 5, 1 + s % 7)
        ev = step(1)
        assert len(ev) == S and ev["symbol"].tolist() == list(range(S)) and (ev["trades"] == 1).all()
        for s in (0, S // 2, S - 1):  # nothing trades
            rows.limit(s, BUY, int(base[s]) + 5, 9)
            rows.limit(s, SELL, int(base[s]) + 30, 9)
        assert len(step(2)) == 0
        _trade(rows, S - 1, int(base[S - 1]) + 20, 3)  # only the last symbol
        ev = step(3)
        assert len(ev) == 1 and ev[0]["symbol"] == S - 1 and ev[0]["cum_trades"] == 2
        _no_deferral(eng, groups=4)


# ---- scripted: the fold's branches -------------------------------------------------------------------
@pytest.mark.parametrize("syms", [(1,), (0, 2)], ids=["one_symbol", "two_alternate"])
def test_one_and_two_symbols_fill_whole_waves(me, orc, syms):
    """256 records with one fill each: all of one symbol (every lane of a wave holds it: the reduced form), or of
    two symbols alternating (the mixed-wave form)."""
    S, L, n = 3, 128, 256
    base = np.array([10_000, 20_000, 30_000], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = tm.TradeModel(S)
    with me.Engine(S, L, base, max_batch=n, max_resting=4 * n, seq_ring=1 << 20) as eng:
        eng.trades_enable(16)
        rows = Rows(me)
        for i in range(n):
            s = syms[i % len(syms)]
            rows.limit(s, SELL, int(base[s]) + 10 + (i // 2) % 7, 1 + i % 3)
        b = rows.batch()
        eng.submit_batch(b)
        model.feed(ob.submit(b)[1])
        assert len(model.peek()) == 0
        for i in range(n):
            s = syms[i % len(syms)]
            rows.limit(s, BUY, int(base[s]) + 20, 1 + i % 3)
        b = rows.batch()
        eng.submit_batch(b)
        f = ob.submit(b)[1]
        assert len(f) >= n
        model.feed(f)
        ev = eng.trades_drain()
        exp = model.expect(2)
        assert len(exp) == len(syms) and sum(int(t) for t in exp["trades"]) == len(f)
        _same(ev, exp, f"{syms}")
        _no_deferral(eng, groups=3)


@pytest.mark.parametrize("form", ["0", "1", "2"])
def test_the_folds_other_forms_give_the_same_events(me, orc, form):
    """ME_TRADE_FOLD (read at enable time; tools/trades_probe.py measures the forms against each other): 0 every
    lane its own atomics to HBM, 1 a one-symbol wave reduces first, 2 the LDS table without that reduction; the
    shipped form is 3. 1,030 symbols (slots shared by two symbols of one workgroup), one symbol with whole
    waves of its own, a 70-fill run."""

    S, L = 1030, 128
    base = np.array([10_000 + 1_000 * s for s in range(S)], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = tm.TradeModel(S)
    with me.Engine(S, L, base, max_batch=2 * S + 512, max_resting=8 * S + 1024, seq_ring=1 << 20) as eng:
        with env({"ME_TRADE_FOLD": form}):
            eng.trades_enable(4 * S)
        rows = Rows(me)
        for k in range(2):
            for s in range(S):
                _trade(rows, s, int(base[s]) + 10 + (s + k) % 5, 1 + s % 7)
            for i in range(70):
                rows.limit(5, SELL, int(base[5]) + 40 + i % 3, 1)
            for i in range(130):
                _trade(rows, 7, int(base[7]) + 50 + i % 4, 2)
            rows.market(5, BUY, 70)
            b = rows.batch()
            eng.submit_batch(b)
            res, f = ob.submit(b)
            assert res[-1]["fill_count"] == 70
            model.feed(f)
            _same(eng.trades_drain(), model.expect(k + 1), f"form {form} batch {k}")
        _no_deferral(eng, groups=3)


@pytest.mark.parametrize("path", ["reg", "deep"])
def test_long_runs_are_read_by_the_wave(me, orc, path):
    """One taker's run of 1, 63, 64, 65 and 200 fills against 200 one-lot makers on five price levels."""
    S, L = 4, PATHS[path][0]
    base = np.array([10_000, 20_000, 30_000, 40_000], dtype=np.int64)
    ob = orc.OracleBook(S)
    model = tm.TradeModel(S)
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with feed_engine(me, path, S, base, 256, 4096, **kw) as eng:
        eng.trades_enable(64)
        rows = Rows(me)
        nbat = 0
        for run in (1, 63, 64, 65, 200):
            for i in range(200):
                rows.limit(2, SELL, 30_050 + i // 40, 1)
            rows.limit(1, SELL, 20_010, 2)  # (another symbol's record beside the long run)
            rows.limit(1, BUY, 20_010, 2)
            rows.market(2, BUY, run)
            b = rows.batch()
            eng.submit_batch(b)
            res, f = ob.submit(b)
            assert res[-1]["fill_count"] == run
            model.feed(f)
            nbat += 1
            ev = eng.trades_drain()
            _same(ev, model.expect(nbat), f"{path} run {run}")
            assert ev["symbol"].tolist() == [1, 2] and ev[1]["trades"] == run == ev[1]["volume"]
            rows.market(2, BUY, 200 - run)  # clear the rest
            b = rows.batch()
            eng.submit_batch(b)
            model.feed(ob.submit(b)[1])
            nbat += 1
            _same(eng.trades_drain(), model.expect(nbat), f"{path} rest of {run}")
        _no_deferral(eng, groups=1 + nbat)


# ---- values ------------------------------------------------------------------------------------------
def test_volume_past_2_32_and_orders_that_fill_nothing(me):
    from tests.reduce_model import ReduceBook  # (the model that knows FOK and POST_ONLY)

    S, L = 4, 128
    base = np.array([-64, -1_000, 5_000, 9_000], dtype=np.int64)
    ob = ReduceBook(S)
    model = tm.TradeModel(S)
    with me.Engine(S, L, base, max_batch=64, max_resting=1024, seq_ring=1 << 20) as eng:
        eng.trades_enable(64)
        rows = Rows(me)
        for _ in range(3):  # three fills of INT32_MAX in one event
            rows.limit(2, SELL, 5_010, BIG)
        for _ in range(3):
            rows.limit(2, BUY, 5_010, BIG)
        _trade(rows, 0, 0, 5)        # price 0 is a price
        _trade(rows, 1, -990, 6)     # so is a negative one
        # a FOK that is killed and a POST_ONLY that is rejected contribute nothing
        rows.limit(3, SELL, 9_050, 5)
        rows.r.append((rows.seq, 9_050, 10, 3, me.kind(BUY, 0, 0, TIF_FOK)))
        rows.seq += 1
        rows.r.append((rows.seq, 9_050, 1, 3, me.kind(BUY, 0, 0, TIF_POST_ONLY)))
        rows.seq += 1
        b = rows.batch()
        eng.submit_batch(b)
        res, f = ob.submit(b)
        assert res[-2]["status"] == 3 and res[-1]["status"] == 4 and not (f["symbol"] == 3).any()
        model.feed(f)
        ev = eng.trades_drain()
        _same(ev, model.expect(1), "values")
        assert ev["symbol"].tolist() == [0, 1, 2]
        assert ev[2]["volume"] == 3 * BIG > 1 << 32 and ev[2]["trades"] == 3 and ev[2]["last_qty"] == BIG
        assert (ev[0]["last_price_q4"], ev[0]["open_price_q4"], ev[0]["high_price_q4"], ev[0]["low_price_q4"]) == (0,) * 4
        assert (ev[1]["last_price_q4"], ev[1]["high_price_q4"], ev[1]["low_price_q4"]) == (-990,) * 3
        _no_deferral(eng, groups=2)


@pytest.mark.parametrize("path", ["reg", "deep"])
def test_prices_at_the_ends_of_int64(me, path):
    """price_edges.clamps: an order rests at INT64_MAX and at INT64_MIN and is taken, then a MARKET sweeps from one
    end of int64 to the other: INT64_MIN, INT64_MAX as open, last, high and low, one job per batch and one job for
    all four batches' worth (re-run with the events merged by the model)."""
    L = PATHS[path][0]
    from tests.reduce_model import ReduceBook  # (the script's noise records are IOCs)

    case = pe.clamps(L, pe.I64_MIN)
    ob = ReduceBook(case.S)
    model = tm.TradeModel(case.S)
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    seen = {"open": set(), "last": set(), "high": set(), "low": set()}
    with feed_engine(me, path, case.S, case.base, max(len(a) for a in case.batches), 4096, far_levels=8, **kw) as eng:
        eng.trades_enable(64)
        for k, a in enumerate(case.batches):
            b = me.Batch(a.seq, a.price_q4, a.qty, a.symbol, a.kind)
            eng.submit_batch(b)
            f = ob.submit(a)[1]
            assert [(int(x["taker_seq"]), int(x["maker_seq"]), int(x["price_q4"]), int(x["qty"])) for x in f] == \
                case.want[k]
            model.feed(f)
            ev = eng.trades_drain()
            _same(ev, model.expect(k + 1), f"{path} clamps batch {k}")
            for e in ev:
                seen["open"].add(int(e["open_price_q4"]))
                seen["last"].add(int(e["last_price_q4"]))
                seen["high"].add(int(e["high_price_q4"]))
                seen["low"].add(int(e["low_price_q4"]))
        _no_deferral(eng, groups=1 + len(case.batches))
    assert pe.I64_MAX in seen["open"] and pe.I64_MIN in seen["open"]
    assert pe.I64_MAX in seen["high"] and pe.I64_MIN in seen["low"]
    assert pe.I64_MIN in seen["last"] and pe.I64_MAX in seen["last"]
    assert any(p < 0 for p in seen["high"]) and any(p > 0 for p in seen["low"])


def test_symbol_ids_name_the_events(me, orc):
    S, L = 70, 128
    ids = np.arange(S, dtype=np.uint32) * 3 + 1000
    base = np.full(S, 50_000, dtype=np.int64)
    ob = orc.OracleBook(S, symbol_ids=ids)
    model = tm.TradeModel(S, symbol_ids=ids)
    with me.Engine(S, L, base, max_batch=256, max_resting=1024, seq_ring=1 << 20, symbol_ids=ids) as eng:
        eng.trades_enable(1)  # raised to num_symbols
        rows = Rows(me)
        for s in range(S):
            _trade(rows, s, 50_070 + s % 3, 2)
        b = rows.batch()
        eng.submit_batch(b)
        model.feed(ob.submit(b)[1])
        ev = eng.trades_drain()
        _same(ev, model.expect(1), "symbol ids")
        assert ev["symbol"].tolist() == ids.tolist()
        _no_deferral(eng, groups=2)


# ---- the host pipeline -------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 4])
def test_host_pipeline_events_are_there_after_collect(me, orc, group):
    """submit_host with two tickets in flight. After collect(t) a read that launches and waits for nothing holds
    every event stamped <= t + 1 (t's ordinal): the events read so far satisfy the feed's invariant against the
    tapes of the first X batches for some X >= t + 1, and, for every stamp X seen, so do the events up to it."""
    S, L, nb, batch = 12, 128, 13, 200
    base, batches = _c5_stream(me, S, L, nb, batch)
    ob = orc.OracleBook(S)
    tapes = [ob.submit(b)[1] for b in batches]

    def holds(ev, x):
        try:
            tm.replay(ev, tapes[:x], S)
        except AssertionError:
            return False
        return True

    with feed_engine(me, "reg", S, base, batch, nb * batch + 1024, batches_per_launch=group) as eng:
        eng.trades_enable(64 * S * nb)
        got = np.zeros(0, dtype=tm.TRADE_DTYPE)
        tickets = []

        def collected(t, submitted):
            nonlocal got
            eng.collect(t)
            ev, left = eng.trades_read(64 * S * nb)
            assert left == 0
            got = np.concatenate([got, ev])
            assert any(holds(got, x) for x in range(t + 1, submitted + 1)), f"after collect({t})"

        for k, b in enumerate(batches):
            tickets.append(eng.submit_host(b))
            if len(tickets) > 2:
                collected(tickets.pop(0), k + 1)
        for t in tickets:
            collected(t, nb)
        assert np.all(np.diff(got["batches"].astype(np.int64)) >= 0)
        for x in np.unique(got["batches"]):
            assert holds(got[got["batches"] <= x], int(x)), f"events up to stamp {x}"
        eng.sync()
        assert len(eng.trades_drain()) == 0
        assert holds(got, nb)
        _no_deferral(eng)


# ---- the bounded log ---------------------------------------------------------------------------------
def test_log_full_defers_and_catches_up(me, orc):
    S, L = 130, 128
    base = np.full(S, 20_000, dtype=np.int64)
    ob = orc.OracleBook(S)
    model = tm.TradeModel(S)
    tapes = []
    with me.Engine(S, L, base, max_batch=2 * S, max_resting=8 * S, seq_ring=1 << 20) as eng:
        eng.trades_enable(S)  # the minimum: one job in which every symbol trades
        rows = Rows(me)

        def step(trades):
            for s, px, q in trades:
                _trade(rows, s, px, q)
            b = rows.batch()
            eng.submit_batch(b)
            tapes.append(ob.submit(b)[1])
            model.feed(tapes[-1])

        step([(s, 20_010, 1 + s % 3) for s in range(S)])  # fits the empty log and fills it
        first = model.expect(1)
        step([(s, 20_020 + s, 2) for s in range(10)])     # ten symbols, no room: deferred
        assert eng.trades_stats() == {"groups": 3, "events": S, "deferred": 1}
        ev, left = eng.trades_read(S - 1)                 # one event stays: no catch-up
        assert len(ev) == S - 1 and left == 1 and eng.trades_stats()["groups"] == 3
        got = ev
        step([(0, 20_050, 7), (11, 20_051, 1)])           # the next job carries the ten, merged with its own
        assert eng.trades_stats() == {"groups": 4, "events": S + 11, "deferred": 1}
        ev = eng.trades_drain()
        got = np.concatenate([got, ev])
        _same(got, np.concatenate([first, model.expect(3)]), "a later job carries the deferred fills")
        e0 = ev[1]  # symbol 0: open from the deferred job's fill, last from the latest
        assert (e0["symbol"], e0["open_price_q4"], e0["last_price_q4"], e0["trades"], e0["volume"]) == (0, 20_020, 20_050, 2, 9)
        assert (e0["high_price_q4"], e0["low_price_q4"], e0["batches"], e0["last_qty"]) == (20_050, 20_020, 3, 7)
        assert eng.trades_stats()["groups"] == 4  # (nothing was outstanding: the drain ran no catch-up)
        # the catch-up of an empty read: fill the log, defer two jobs, read nothing in between
        step([(s, 20_060, 1) for s in range(S)])
        full = model.expect(4)
        step([(s, 20_070 + s, 3) for s in range(5)])
        step([(s, 20_080 - s, 4) for s in range(3, 8)])
        assert eng.trades_stats() == {"groups": 7, "events": 2 * S + 11, "deferred": 3}
        ev = eng.trades_drain()  # drains the log, finds it empty with a deferral outstanding: one catch-up job
        st = eng.trades_stats()
        assert st == {"groups": 8, "events": 2 * S + 11 + 8, "deferred": 3}, st
        _same(ev, np.concatenate([full, model.expect(6)]), "catch-up")
        m = ev[S + 3]  # symbol 3 traded in both deferred jobs
        assert (m["symbol"], m["open_price_q4"], m["last_price_q4"], m["trades"], m["volume"]) == (3, 20_073, 20_077, 2, 7)
        assert (m["high_price_q4"], m["low_price_q4"]) == (20_077, 20_073)
        got = np.concatenate([got, ev])
        tm.replay(got, tapes, S)


# ---- enabling mid-stream, the feed off ---------------------------------------------------------------
@pytest.mark.parametrize("path", ["reg", "deep"])
def test_enable_mid_stream(me, orc, path):
    S, L = 65, PATHS[path][0]
    base, batches = _c5_stream(me, S, L, 4, 300)
    ob = orc.OracleBook(S)
    with feed_engine(me, path, S, base, 300, 4096) as eng:
        for b in batches[:2]:
            eng.submit_batch(b)
            assert len(ob.submit(b)[1]) > 0  # fills before the feed is on: not counted
        eng.trades_enable(4 * S)
        model = tm.TradeModel(S)
        assert len(eng.trades_drain()) == 0
        assert eng.trades_stats() == {"groups": 1, "events": 0, "deferred": 0}
        eng.submit_batch(batches[2])
        f2 = ob.submit(batches[2])[1]
        model.feed(f2)
        ev = eng.trades_drain()
        assert len(ev) > 0
        _same(ev, model.expect(3), "the batch after enabling")
        tm.replay(ev, [f2], S)
        _no_deferral(eng, groups=2)
        # enabling again starts afresh (the counts too); 0 turns the feed off
        eng.trades_enable(4 * S)
        model = tm.TradeModel(S)
        eng.submit_batch(batches[3])
        model.feed(ob.submit(batches[3])[1])
        _same(eng.trades_drain(), model.expect(4), "re-enabled")
        eng.trades_enable(0)
        with pytest.raises(me.EngineError) as ei:
            eng.trades_read()
        assert ei.value.code == me.ME_E_INVALID


def test_feed_off_is_invalid(me):
    with me.Engine(4, 128, [1000] * 4, 64, 1024, 1 << 20) as eng:
        with pytest.raises(me.EngineError) as ei:
            eng.trades_read()
        assert ei.value.code == me.ME_E_INVALID
        with pytest.raises(me.EngineError) as ei:
            eng.trades_stats()
        assert ei.value.code == me.ME_E_INVALID


# ---- independence ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["gwalk", "deep"])
def test_the_other_feeds_and_the_outputs_do_not_depend_on_it(me, path):
    """The same stream with the quote and depth feeds on, once without and once with the trade feed: results,
    tapes, book dumps, quote events and depth events are equal."""
    S, L, grouped = 24, PATHS[path][0], PATHS[path][3]
    nb, batch = 6, 300
    base, batches = _c5_stream(me, S, L, nb, batch)

    def run(trades):
        kw = {"batches_per_launch": 4} if grouped else {}
        with feed_engine(me, path, S, base, batch, 2 * nb * batch + 1024, **kw) as eng:
            eng.quotes_enable(64 * S)
            eng.depth_enable(4, 64 * 16 * S)
            if trades:
                eng.trades_enable(64 * S)
            outs = []
            if grouped:
                ts = [eng.submit_host(b) for b in batches]
                outs = [eng.collect(t) for t in ts]
            else:
                outs = [eng.submit_batch(b) for b in batches]
            eng.sync()
            q, d = eng.quotes_drain(), eng.depth_drain()
            n = len(eng.trades_drain()) if trades else 0
            dumps = [eng.dump(s) for s in range(S)]
            return outs, q, d, dumps, n

    a, b = run(False), run(True)
    assert b[4] > 0 and len(a[1]) > 0 and len(a[2]) > 0
    for (ra, fa), (rb, fb) in zip(a[0], b[0]):
        assert np.array_equal(ra, rb) and np.array_equal(fa, fb)
    _same(b[1], a[1], f"{path}: quote events")
    _same(b[2], a[2], f"{path}: depth events")
    for da, db in zip(a[3], b[3]):
        assert np.array_equal(da, db)
