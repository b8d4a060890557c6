"""StreamMarketData as a change stream (me_service_market_subscribe / me_service_market_stream) over a
Python oracle matcher with a quote feed (tests/quote_model.py OracleFeed), and the cluster's QUOTES
collective over two TCP ranks with oracle shards. Runs on CPU."""
import numpy as np
import pytest

from tests.service_common import BIG, BUY, SELL, FeedMatcher, _limit, _run_cluster


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def test_stream_equals_poll_after_every_flush(me):
    syms = [f"S{i}" for i in range(8)]
    svc = me.MatchingEngineService(None, syms, matcher=FeedMatcher(8))
    try:
        svc.market_subscribe()
        assert svc.market_stream() == []
        rng = np.random.default_rng(3)
        poll = {s: svc.market_data(s) for s in syms}
        live, seen = [], set()
        for _ in range(6):
            for _ in range(150):
                s = syms[int(rng.integers(6))]  # (S6 and S7 never trade: never streamed)
                if live and rng.random() < 0.2:
                    oid, os_ = live.pop(int(rng.integers(len(live))))
                    svc.cancel_order("C", os_, oid)
                    continue
                market = rng.random() < 0.2
                r = svc.submit_order("C", s, 1 if market else 0, int(rng.choice([1, 2])),
                                     0 if market else 1000 + int(rng.integers(-6, 7)), 4, int(rng.integers(1, 40)))
                if not market:
                    live.append((r["order_id"], s))
            svc.flush(outputs=False)
            ups = svc.market_stream()
            names = [u["symbol"] for u in ups]
            assert len(set(names)) == len(names)  # one pending update per symbol
            seen |= set(names)
            for u in ups:
                assert u == svc.market_data(u["symbol"])
                assert u != poll[u["symbol"]]  # an update is a change
            for s in syms:
                if s not in names:
                    assert svc.market_data(s) == poll[s], f"{s} changed without an update"
            poll = {s: svc.market_data(s) for s in syms}
        assert seen == set(syms[:6])
    finally:
        svc.close()


def test_conflation_keeps_first_change_order_and_per_symbol_drain(me):
    svc = me.MatchingEngineService(None, ["A", "B", "C"], matcher=FeedMatcher(3))
    try:
        svc.market_subscribe()
        _limit(svc, "C", BUY, 100, 1)
        _limit(svc, "A", BUY, 200, 2)
        svc.flush(outputs=False)  # events A, C (symbol order within a slice)
        _limit(svc, "B", SELL, 300, 3)
        _limit(svc, "A", BUY, 201, 4)
        svc.flush(outputs=False)  # events A, B: A keeps its place with the newer payload
        only_c = svc.market_stream("C")
        assert [u["symbol"] for u in only_c] == ["C"] and only_c[0]["best_bid"] == 100
        assert svc.market_stream("C") == []
        ups = svc.market_stream()
        assert [u["symbol"] for u in ups] == ["A", "B"]
        assert ups[0]["best_bid"] == 201 and ups[0]["bid_size"] == 4 and not ups[0]["has_ask"]
        assert ups[1]["has_ask"] and ups[1]["best_ask"] == 300 and not ups[1]["has_bid"]
        assert svc.market_stream() == []
    finally:
        svc.close()


def test_sizes_saturate_like_the_poll(me):
    m = FeedMatcher(1)
    svc = me.MatchingEngineService(None, ["A"], matcher=m)
    try:
        svc.market_subscribe()
        _limit(svc, "A", BUY, 7, BIG)
        _limit(svc, "A", BUY, 7, BIG)
        svc.flush(outputs=False)
        (u,) = svc.market_stream()
        assert u["has_bid"] and u["best_bid"] == 7 and u["bid_size"] == BIG and u == svc.market_data("A")
        assert m.ob.snapshot(0, 1)[0][0]["total_qty"] == 2 * BIG  # the feed's int64 quantity is exact
    finally:
        svc.close()


def test_a_reused_book_is_named_by_the_slice_of_the_event(me):
    """Two books. A's last order fills in slice k; B takes A's book in slice k + 1. The matcher's events arrive
    one slice late (lag), so A's final empty quote is read after the book changed hands: it must still be A's,
    and B's first quote B's."""
    svc = me.MatchingEngineService(None, ["A", "X"], matcher=FeedMatcher(2, lag=1))
    try:
        svc.market_subscribe()
        _limit(svc, "A", SELL, 100, 5)
        _limit(svc, "X", SELL, 900, 1)
        svc.flush(outputs=False)  # slice 1 (its events are held back)
        svc.submit_order("C", "A", 0, BUY, 100, 4, 5)
        svc.flush(outputs=False)  # slice 2 = k: A's book empties; slice 1's events arrive
        ups = svc.market_stream()
        assert [(u["symbol"], u["best_ask"]) for u in ups] == [("A", 100), ("X", 900)]
        _limit(svc, "B", BUY, 50, 3)  # every book is taken: B takes A's idle one
        assert svc.stats()["reclaimed_books"] == 1
        svc.flush(outputs=False)  # slice 3 = k + 1; slice 2's event (A empty) arrives now
        ups = svc.market_stream()
        assert [u["symbol"] for u in ups] == ["A"], ups
        assert not ups[0]["has_bid"] and not ups[0]["has_ask"]
        _limit(svc, "X", SELL, 901, 1)
        svc.flush(outputs=False)  # slice 4; slice 3's event (B's bid) arrives
        ups = svc.market_stream()
        assert [u["symbol"] for u in ups] == ["B"], ups
        assert ups[0]["has_bid"] and ups[0]["best_bid"] == 50 and ups[0]["bid_size"] == 3
        assert ups[0] == svc.market_data("B")
    finally:
        svc.close()


def test_subscribe_needs_a_feed(me):
    svc = me.MatchingEngineService(None, ["A"], matcher=FeedMatcher(1, feed=False))
    try:
        with pytest.raises(me.ServiceError) as ei:
            svc.market_subscribe()
        assert ei.value.code == me.ME_E_INVALID
        with pytest.raises(me.ServiceError) as ei:
            svc.market_stream()
        assert ei.value.code == me.ME_E_INVALID
    finally:
        svc.close()


def test_cluster_two_tcp_ranks_oracle_shards(built, tmp_path):
    r = _run_cluster("oracle", 2, tmp_path)
    assert r["ok"], r["msg"]
    assert r["events"] > 40
