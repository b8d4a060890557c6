"""me_service_mass_cancel on the HIP engine: two clients on two symbols, one symbol purged — the owners' CANCELED
updates, the untouched symbol, the persisted rows and a restart, OrderStatus, and the freed book handed to a
new symbol. Needs an MI355X."""
import sqlite3

import numpy as np
import pytest

from tests.service_common import FeedMatcher

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
ST_NEW, ST_PARTIAL, ST_CANCELED = 0, 1, 3
NOT_RESTING, RESTING = 0, 2
MID = 1_000_000


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _engine(me):
    return me.Engine(2, 128, np.full(2, MID - 64, dtype=np.int64), max_batch=4096, max_resting=1 << 14)


def _limit(svc, client, sym, side, px, q):
    r = svc.submit_order(client, sym, 0, side, px, 4, q)
    assert r["success"], r
    return r["order_id"]


def _rows(db):
    con = sqlite3.connect(db)
    try:
        return {oid: (st, rem) for oid, st, rem in con.execute("SELECT order_id, status, remaining_quantity FROM orders")}
    finally:
        con.close()


def test_one_symbol_purged(me, tmp_path):
    db = str(tmp_path / "purge.sqlite")
    eng = _engine(me)
    svc = me.MatchingEngineService(eng, ["A", "B"], db_path=db)
    try:
        a = {}  # order id -> (client, quantity left)
        for j in range(20):  # two bid levels of ten orders, six ask levels, both clients on both sides
            a[_limit(svc, "alice" if j % 3 else "bob", "A", BUY, MID - 1 - j % 2, 10 + j)] = ("alice" if j % 3 else "bob", 10 + j)
        for j in range(6):
            a[_limit(svc, "bob" if j % 2 else "alice", "A", SELL, MID + 2 + j, 5 + j)] = ("bob" if j % 2 else "alice", 5 + j)
        b = [_limit(svc, "alice", "B", BUY, MID - 2, 7), _limit(svc, "bob", "B", SELL, MID + 2, 9)]
        svc.flush(outputs=False)
        # a taker fills the oldest bid of A in part: its update must carry what is left
        first = next(iter(a))
        _limit(svc, "carol", "A", SELL, MID - 1, 4)
        svc.flush(outputs=False)
        a[first] = (a[first][0], a[first][1] - 4)
        svc.order_updates()
        # one order still in the open slice when the call comes: it is flushed first, then purged
        late = _limit(svc, "alice", "A", BUY, MID - 5, 3)
        a[late] = ("alice", 3)
        with pytest.raises(me.ServiceError) as ei:
            svc.mass_cancel(["A", "nope"])
        assert ei.value.code == me.ME_E_INVALID
        with pytest.raises(me.ServiceError) as ei:
            svc.mass_cancel(["A", "A"])
        assert ei.value.code == me.ME_E_INVALID
        with pytest.raises(me.ServiceError) as ei:
            svc.mass_cancel(["A"], sides=0)
        assert ei.value.code == me.ME_E_INVALID
        assert len(svc.order_book("A")[0]) == 20  # nothing changed (the late order is not matched yet)
        n = svc.mass_cancel(["A"])
        assert n == len(a) == 27
        ups = svc.order_updates()
        new = [u for u in ups if u["status"] == ST_NEW]
        assert [(u["order_id"], u["client_id"]) for u in new] == [(late, "alice")]
        got = {u["order_id"]: u for u in ups if u["status"] == ST_CANCELED}
        assert len(ups) == 1 + len(a) and set(got) == set(a)
        for oid, (client, left) in a.items():
            u = got[oid]
            assert (u["client_id"], u["symbol"], u["remaining_quantity"], u["fill_quantity"]) == (client, "A", left, 0), u
        # the book is empty, the other symbol untouched
        assert svc.order_book("A") == ([], [])
        bb, ba = svc.order_book("B")
        assert [x["order_id"] for x in bb] == [b[0]] and [x["order_id"] for x in ba] == [b[1]]
        assert eng.resting_count() == 2
        for client in ("alice", "bob"):
            mine = [oid for oid, (c, _) in a.items() if c == client]
            assert {r["state"] for r in svc.order_status(client, mine)} == {NOT_RESTING}
        assert svc.order_status("alice", [b[0]])[0]["state"] == RESTING
        # the rows
        rows = _rows(db)
        for oid, (_, left) in a.items():
            assert rows[oid] == (ST_CANCELED, left), (oid, rows[oid])
        assert rows[b[0]] == (ST_NEW, 7) and rows[b[1]] == (ST_NEW, 9)
        # nothing rests on A: again is a no-op; sides one at a time on B
        assert svc.mass_cancel(["A"]) == 0 and svc.order_updates() == []
        assert svc.mass_cancel(["B"], sides=SELL) == 1
        assert [(u["order_id"], u["client_id"], u["status"]) for u in svc.order_updates()] == [(b[1], "bob", ST_CANCELED)]
        # A's book is idle: a new symbol takes it over
        r0 = svc.stats()["reclaimed_books"]
        c1 = _limit(svc, "carol", "C", BUY, MID - 3, 5)
        svc.flush(outputs=False)
        assert svc.stats()["reclaimed_books"] == r0 + 1
        assert [x["order_id"] for x in svc.order_book("C")[0]] == [c1]
    finally:
        svc.close()
        eng.close()
    # a restart brings back what rests (B's bid, C's bid), not the purged orders
    eng = _engine(me)
    svc = me.MatchingEngineService(eng, ["A", "B"], db_path=db)
    try:
        svc.flush(outputs=False)
        assert svc.stats()["recovered_orders"] == 2
        assert eng.resting_count() == 2
        assert [x["order_id"] for x in svc.order_book("B")[0]] == [b[0]] and svc.order_book("B")[1] == []
        assert [x["order_id"] for x in svc.order_book("C")[0]] == [c1]
    finally:
        svc.close()
        eng.close()


def test_every_symbol_and_no_db(me):
    eng = _engine(me)
    svc = me.MatchingEngineService(eng, ["A", "B"])
    try:
        ids = [_limit(svc, "alice", "A", BUY, MID - 1, 10), _limit(svc, "bob", "B", SELL, MID + 1, 20),
               _limit(svc, "bob", "B", BUY, MID - 4, 30)]
        assert svc.mass_cancel(None, sides=BUY) == 2  # (flushes the open slice itself)
        ups = [u for u in svc.order_updates() if u["status"] == ST_CANCELED]
        assert sorted((u["order_id"], u["client_id"], u["remaining_quantity"]) for u in ups) == \
            sorted([(ids[0], "alice", 10), (ids[2], "bob", 30)])
        assert eng.resting_count() == 1
        assert svc.mass_cancel(None) == 1 and eng.resting_count() == 0
        assert svc.mass_cancel([]) == 0
    finally:
        svc.close()
        eng.close()


def test_a_matcher_has_no_mass_cancel(me):
    svc = me.MatchingEngineService(None, ["A"], matcher=FeedMatcher(1))
    try:
        with pytest.raises(me.ServiceError) as ei:
            svc.mass_cancel(["A"])
        assert ei.value.code == me.ME_E_INVALID and "no mass cancel" in str(ei.value)
    finally:
        svc.close()
