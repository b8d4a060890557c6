"""me_service_order_status on the HIP engine: the states of a client's orders through submit, flush, reduce,
fill and cancel, and what the call keeps to itself. Needs an MI355X."""
import numpy as np
import pytest

from tests.service_common import FeedMatcher

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
NOT_RESTING, PENDING, RESTING = 0, 1, 2
ZERO = {"side": 0, "quantity": 0, "price": 0, "qty_ahead": 0, "level_qty": 0, "qty_better": 0, "orders_ahead": 0,
        "levels_better": 0}


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _limit(svc, client, sym, side, px, q):
    r = svc.submit_order(client, sym, 0, side, px, 4, q)
    assert r["success"], r
    return r["order_id"]


def _place(r):
    return (r["state"], r["quantity"], r["qty_ahead"], r["orders_ahead"], r["level_qty"], r["levels_better"], r["qty_better"])


def test_states_of_a_clients_orders(me):
    assert (me.OS_NOT_RESTING, me.OS_PENDING, me.OS_RESTING) == (NOT_RESTING, PENDING, RESTING)
    mid = 1_000_000
    eng = me.Engine(2, 128, np.full(2, mid - 64, dtype=np.int64), max_batch=4096, max_resting=1 << 14)
    svc = me.MatchingEngineService(eng, ["A", "B"])
    try:
        a1 = _limit(svc, "alice", "A", BUY, mid - 1, 10)
        b1 = _limit(svc, "bob", "A", BUY, mid - 1, 20)
        a2 = _limit(svc, "alice", "A", BUY, mid - 1, 30)
        a3 = _limit(svc, "alice", "A", BUY, mid - 3, 5)
        a4 = _limit(svc, "alice", "B", SELL, mid + 2, 7)
        ids = [a1, a2, a3, a4]
        # submitted, not flushed: the service knows them, the engine does not
        st = svc.order_status("alice", ids)
        assert [r["order_id"] for r in st] == ids
        assert [(r["state"], r["quantity"], r["scale"]) for r in st] == [(PENDING, 10, 4), (PENDING, 30, 4), (PENDING, 5, 4),
                                                                       (PENDING, 7, 4)]
        assert all(r["qty_ahead"] == r["level_qty"] == r["price"] == r["side"] == 0 for r in st)
        svc.flush(outputs=False)
        st = svc.order_status("alice", ids)
        assert [_place(r) for r in st] == [(RESTING, 10, 0, 0, 60, 0, 0), (RESTING, 30, 30, 2, 60, 0, 0),
                                           (RESTING, 5, 0, 0, 5, 1, 60), (RESTING, 7, 0, 0, 7, 0, 0)]
        assert [(r["side"], r["price"], r["scale"]) for r in st] == [(BUY, mid - 1, 4), (BUY, mid - 1, 4), (BUY, mid - 3, 4),
                                                                     (SELL, mid + 2, 4)]
        # the engine's own answers are what the service passed on
        q = eng.order_query([int(x[4:]) for x in ids])
        for r, e in zip(st, q):
            assert int(e["found"]) == 1
            assert (r["quantity"], r["price"], r["qty_ahead"], r["level_qty"], r["qty_better"], r["orders_ahead"],
                    r["levels_better"], r["side"]) == tuple(int(e[f]) for f in (
                        "qty", "price_q4", "qty_ahead", "level_qty", "qty_better", "orders_ahead", "levels_better", "side"))
        # another client's order, malformed ids, an id never given out: nothing is revealed
        other = svc.order_status("alice", [b1, "OID-0", "OID-", "oid-3", "OID-12x", "", "OID-999999", a1])
        assert [r["state"] for r in other] == [NOT_RESTING] * 7 + [RESTING]
        for r in other[:7]:
            assert {k: r[k] for k in ZERO} == ZERO
        assert other[0]["order_id"] == b1 and svc.order_status("bob", [b1])[0]["state"] == RESTING
        assert svc.order_status("", [a1])[0]["state"] == NOT_RESTING
        assert svc.order_status("alice", []) == []
        # bob reduces: alice's second order moves up by exactly that much and keeps its place
        assert svc.reduce_order("bob", "A", b1, 15)["success"]
        assert svc.reduce_order("alice", "A", a1, 4)["success"]
        svc.flush(outputs=False)
        st = svc.order_status("alice", [a1, a2])
        assert [_place(r) for r in st] == [(RESTING, 6, 0, 0, 41, 0, 0), (RESTING, 30, 11, 2, 41, 0, 0)]
        assert _place(svc.order_status("bob", [b1])[0]) == (RESTING, 5, 6, 1, 41, 0, 0)
        # a taker fills a1 and part of b1; a cancel removes a3; a reduce to nothing removes a4
        _limit(svc, "carol", "A", SELL, mid - 1, 8)
        assert svc.cancel_order("alice", "A", a3)["success"]
        assert svc.reduce_order("alice", "B", a4, 7)["success"]
        pend = svc.order_status("alice", ids)  # the closing records are queued: the orders still rest as they were
        assert [r["state"] for r in pend] == [RESTING] * 4
        svc.flush(outputs=False)
        st = svc.order_status("alice", ids)
        assert [r["state"] for r in st] == [NOT_RESTING, RESTING, NOT_RESTING, NOT_RESTING]
        assert _place(st[1]) == (RESTING, 30, 3, 1, 33, 0, 0)
        for r in (st[0], st[2], st[3]):
            assert {k: r[k] for k in ZERO} == ZERO
    finally:
        svc.close()
        eng.close()


def test_a_matcher_has_no_order_query(me):
    svc = me.MatchingEngineService(None, ["A"], matcher=FeedMatcher(1))
    try:
        r = svc.submit_order("alice", "A", 0, BUY, 1_000, 4, 5)
        assert r["success"]
        with pytest.raises(me.ServiceError) as ei:
            svc.order_status("alice", [r["order_id"]])
        assert ei.value.code == me.ME_E_INVALID and "no order query" in str(ei.value)
    finally:
        svc.close()
