"""The test model of the trigger book (tests/stops_model.py) against a brute-force re-evaluation, fill by fill,
over the CPU oracle's tapes: which stops trigger, at what price, in what order; the int64 extremes. Runs on CPU."""
import numpy as np
import pytest

from tests import stops_model as sm
from tests.feed_common import _c5_stream

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
FILL_DTYPE = np.dtype([("taker_seq", "<u8"), ("maker_seq", "<u8"), ("price_q4", "<i8"), ("qty", "<i4"), ("symbol", "<u4")])


def _fills(rows):
    f = np.zeros(len(rows), dtype=FILL_DTYPE)
    for k, (s, p) in enumerate(rows):
        f[k]["symbol"], f[k]["price_q4"], f[k]["qty"] = s, p, 1
    return f


@pytest.mark.parametrize("group", [1, 3])
def test_model_equals_brute_force_over_the_oracles_tapes(built, group):
    import matching_engine_amd as me
    from oracle import oracle

    S, nb, batch = 24, 9, 250
    _, batches = _c5_stream(me, S, 128, nb, batch)
    ob = oracle.OracleBook(S)
    tapes = [ob.submit(b)[1] for b in batches]
    allf = np.concatenate(tapes)
    assert len(np.unique(allf["symbol"])) >= S // 2
    # stops scattered around every traded symbol's price range, both sides, ids ascending across symbols
    rng = np.random.default_rng(5)
    rows, nid = [], 1
    for rep in range(4):
        for s in np.unique(allf["symbol"]):
            px = allf["price_q4"][allf["symbol"] == s]
            for side in (sm.BUY, sm.SELL):
                rows.append((nid, int(rng.integers(px.min() - 3, px.max() + 4)), int(px.min()) - rep, 1 + rep, int(s),
                             me.kind(side, rep & 1)))
                nid += int(rng.integers(1, 5))
    model = sm.StopModel(S)
    model.add(sm.stops(rows))
    total = 0
    for j0 in range(0, nb, group):
        launch = tapes[j0:j0 + group]
        live = model.dump()
        for t in launch:
            model.feed(t)
        ev = model.job(j0 + len(launch))
        want = sm.brute(live, launch)
        assert ev["id"].tolist() == [int(live[k]["id"]) for k, _ in want]
        assert ev["trigger_px_q4"].tolist() == [p for _, p in want]
        assert (ev["batches"] == j0 + len(launch)).all()
        assert ev["id"].tolist() == sorted(ev["id"].tolist())  # table order = ascending id, across symbols
        for name in ("stop_px_q4", "limit_px_q4", "qty", "symbol", "kind"):
            assert ev[name].tolist() == [int(live[k][name]) for k, _ in want]
        gone = set(ev["id"].tolist())
        assert model.dump()["id"].tolist() == [int(i) for i in live["id"] if int(i) not in gone]
        total += len(ev)
    assert 0 < total < len(rows)  # some trigger, some never do


def test_event_order_is_table_order_not_symbol_order():
    m = sm.StopModel(4)
    k = 1  # BUY LIMIT
    m.add(sm.stops([(10, 100, 0, 1, 3, k), (11, 100, 0, 1, 0, k), (12, 100, 0, 1, 3, k), (13, 500, 0, 1, 0, k)]))
    m.feed(_fills([(0, 100), (3, 101)]))
    ev = m.job(1)
    assert ev["id"].tolist() == [10, 11, 12] and ev["symbol"].tolist() == [3, 0, 3]
    assert ev["trigger_px_q4"].tolist() == [101, 100, 101]
    assert m.dump()["id"].tolist() == [13]
    assert len(m.job(2)) == 0  # the launch's extremes are forgotten: nothing fed, nothing triggers


def test_int64_extremes_and_the_symbol_that_does_not_trade():
    m = sm.StopModel(3)
    buy, sell = 1, 2
    m.add(sm.stops([(1, I64_MIN, 0, 1, 0, buy), (2, I64_MAX, 0, 1, 0, sell), (3, I64_MAX, 0, 1, 1, buy),
                    (4, I64_MIN, 0, 1, 1, sell), (5, 0, 0, 1, 2, buy), (6, -1, 0, 1, 2, sell),
                    (7, I64_MIN, I64_MIN, 1, 1, buy), (8, I64_MAX, I64_MAX, 1, 1, sell)]))
    # symbol 0 does not trade: its stops, satisfied by any price at all, stay
    m.feed(_fills([(2, -1)]))
    ev = m.job(1)
    assert ev["id"].tolist() == [6] and ev[0]["trigger_px_q4"] == -1  # (BUY at 0 needs >= 0)
    m.feed(_fills([(0, -7)]))
    ev = m.job(2)
    assert ev["id"].tolist() == [1, 2] and ev["trigger_px_q4"].tolist() == [-7, -7]
    # symbol 1: a BUY at INT64_MAX and a SELL at INT64_MIN trigger only on those very prices
    m.feed(_fills([(1, I64_MAX - 1), (1, I64_MIN + 1)]))
    ev = m.job(3)
    assert ev["id"].tolist() == [7, 8] and ev["trigger_px_q4"].tolist() == [I64_MAX - 1, I64_MIN + 1]
    m.feed(_fills([(1, I64_MAX), (1, I64_MIN), (2, 0)]))
    ev = m.job(4)
    assert ev["id"].tolist() == [3, 4, 5] and ev["trigger_px_q4"].tolist() == [I64_MAX, I64_MIN, 0]
    assert len(m.dump()) == 0
    assert m.cancel([1]).tolist() == [0]
