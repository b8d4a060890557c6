"""StreamMarketData as a change stream on the HIP engine: the service's stream against its poll, the
stream after restart recovery, and the cluster's QUOTES collective over RCCL (world size 1). Needs an MI355X."""
import numpy as np
import pytest

from tests.service_common import BIG, BUY, SELL, _limit, _run_cluster

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _traffic(svc, rng, syms, n, live):
    for _ in range(n):
        s = syms[int(rng.integers(len(syms)))]
        if live and rng.random() < 0.2:
            oid, os_ = live.pop(int(rng.integers(len(live))))
            svc.cancel_order("C", os_, oid)
            continue
        market = rng.random() < 0.2
        far = 0 if rng.random() > 0.03 else int(rng.choice([-1, 1])) * int(rng.integers(200, 900))
        r = svc.submit_order("C", s, 1 if market else 0, int(rng.choice([1, 2])),
                             0 if market else 1_000_000 + far + int(rng.integers(-6, 7)), 4, int(rng.integers(1, 40)))
        if not market:
            live.append((r["order_id"], s))


def test_stream_equals_poll_after_every_flush_on_the_engine(me):
    syms = [f"S{i}" for i in range(8)]
    eng = me.Engine(8, 128, np.full(8, 1_000_000 - 64, dtype=np.int64), max_batch=4096, max_resting=1 << 14)
    svc = me.MatchingEngineService(eng, syms)
    try:
        svc.market_subscribe()
        assert svc.market_stream() == []
        rng = np.random.default_rng(5)
        poll = {s: svc.market_data(s) for s in syms}
        live, seen = [], set()
        for k in range(6):
            _traffic(svc, rng, syms[:6], 150, live)
            if k == 3:  # a level total above 2^31: the stream saturates it as the poll does
                _limit(svc, "S7", BUY, 999_990, BIG)
                _limit(svc, "S7", BUY, 999_990, BIG)
            svc.flush(outputs=False)
            ups = svc.market_stream()
            names = [u["symbol"] for u in ups]
            assert len(set(names)) == len(names)
            seen |= set(names)
            for u in ups:
                assert u == svc.market_data(u["symbol"])
                assert u != poll[u["symbol"]]
            for s in syms:
                if s not in names:
                    assert svc.market_data(s) == poll[s], f"{s} changed without an update"
            poll = {s: svc.market_data(s) for s in syms}
            if k == 3:
                assert poll["S7"]["bid_size"] == BIG and "S7" in names
                bids, _ = eng.snapshot(7, 1)
                assert bids[0]["total_qty"] == 2 * BIG
        assert seen == set(syms[:6]) | {"S7"}
        assert svc.last_error() == ""
    finally:
        svc.close()
        eng.close()


def test_subscribe_after_restart_recovery(me, tmp_path):
    """The first read after subscribing on recovered books is exactly the non-empty symbols' quotes."""
    syms = [f"R{i}" for i in range(6)]
    db = str(tmp_path / "md.sqlite")
    base = np.full(6, 1_000_000 - 64, dtype=np.int64)
    e1 = me.Engine(6, 128, base, max_batch=4096, max_resting=1 << 14)
    s1 = me.MatchingEngineService(e1, syms, db_path=db)
    _traffic(s1, np.random.default_rng(9), syms[:4], 400, [])
    _limit(s1, "R5", SELL, 1_000_500, 3)  # (a far level)
    s1.flush(outputs=False)
    before = {s: s1.market_data(s) for s in syms}
    s1.close()
    e1.close()
    e2 = me.Engine(6, 128, base, max_batch=4096, max_resting=1 << 14)
    s2 = me.MatchingEngineService(e2, syms, db_path=db)
    try:
        assert s2.stats()["recovered_orders"] > 20
        s2.market_subscribe()
        ups = s2.market_stream()
        full = [s for s in syms if before[s]["has_bid"] or before[s]["has_ask"]]
        assert sorted(u["symbol"] for u in ups) == sorted(full) and "R4" not in full and "R5" in full
        for u in ups:
            assert u == before[u["symbol"]] == s2.market_data(u["symbol"])
        _limit(s2, "R4", BUY, 999_999, 2)
        s2.flush(outputs=False)
        ups = s2.market_stream()
        assert [u["symbol"] for u in ups] == ["R4"] and ups[0] == s2.market_data("R4")
    finally:
        s2.close()
        e2.close()


def test_cluster_rccl_single_rank(built, tmp_path):
    r = _run_cluster("rccl", 1, tmp_path)
    assert r["ok"], r["msg"]
    assert r["events"] > 40
