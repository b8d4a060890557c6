"""The service's trade stream (me_service_trades_subscribe / me_service_trades_stream) on the HIP engine: the
updates of every symbol name against the fold of the fills the service matched and persisted. Needs an MI355X."""
import sqlite3

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
BIG = 2_147_483_647


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _fold(rows):
    """rows: (price, qty) of one symbol's fills in order -> the summary an update carries."""
    px = [p for p, _ in rows]
    return dict(last_price=px[-1], last_size=rows[-1][1], open_price=px[0], high_price=max(px), low_price=min(px),
                volume=sum(q for _, q in rows), trades=len(rows))


def _persisted(db):
    """{symbol name: [(price, qty)] in fill order} from the fills table (two rows per fill: both parties')."""
    con = sqlite3.connect(db)
    rows = con.execute("SELECT symbol, fill_price, fill_quantity FROM fills ORDER BY id").fetchall()
    con.close()
    assert len(rows) % 2 == 0
    out = {}
    for a, b in zip(rows[0::2], rows[1::2]):
        assert a == b, (a, b)
        out.setdefault(a[0], []).append((a[1], a[2]))
    return out


def _limit(svc, sym, side, px, q):
    r = svc.submit_order("C", sym, 0, side, px, 4, q)
    assert r["success"], r
    return r["order_id"]


def test_updates_equal_the_fold_of_the_persisted_fills(me, tmp_path):
    syms = ["A", "B", "C", "D"]
    db = str(tmp_path / "trades.sqlite")
    eng = me.Engine(4, 128, np.full(4, 1_000_000 - 64, dtype=np.int64), max_batch=4096, max_resting=1 << 14)
    svc = me.MatchingEngineService(eng, syms, db_path=db)
    per_slice, total = [], {}
    try:
        svc.trades_subscribe()
        assert svc.trades_stream() == []
        rng = np.random.default_rng(5)
        for k in range(6):
            for _ in range(60):
                s = syms[int(rng.integers(3 if k in (0, 3) else 2))]  # (C trades in two slices, D never)
                market = rng.random() < 0.2
                svc.submit_order("C", s, 1 if market else 0, int(rng.choice([BUY, SELL])),
                                 0 if market else 1_000_000 + int(rng.integers(-6, 7)), 4, int(rng.integers(1, 40)))
            _, _, fills = svc.flush()
            ups = svc.trades_stream()
            names = [u["symbol"] for u in ups]
            assert len(set(names)) == len(names)  # one pending update per symbol
            want = {}
            for f in fills:  # (no book changes hands here: book id = index of the name)
                want.setdefault(syms[int(f["symbol"])], []).append((int(f["price_q4"]), int(f["qty"])))
            assert sorted(names) == sorted(want), f"slice {k}"
            for u in ups:
                w = _fold(want[u["symbol"]])
                t = total.setdefault(u["symbol"], [0, 0])
                t[0] += w["volume"]
                t[1] += w["trades"]
                assert u == dict(symbol=u["symbol"], scale=4, cum_volume=t[0], cum_trades=t[1], **w), f"slice {k}"
            per_slice.append(ups)
        assert svc.trades_stream() == [] and svc.last_error() == ""
    finally:
        svc.close()
        eng.close()
    # and against what was persisted: every name's updates chain up to the fold of its fills in the database
    rows = _persisted(db)
    assert set(rows) == set(total) == {"A", "B", "C"}
    for s, r in rows.items():
        w = _fold(r)
        ups = [u for sl in per_slice for u in sl if u["symbol"] == s]
        assert sum(u["volume"] for u in ups) == ups[-1]["cum_volume"] == w["volume"]
        assert sum(u["trades"] for u in ups) == ups[-1]["cum_trades"] == w["trades"]
        assert (ups[-1]["last_price"], ups[-1]["last_size"]) == (w["last_price"], w["last_size"])
        assert ups[0]["open_price"] == w["open_price"]
        assert max(u["high_price"] for u in ups) == w["high_price"] and min(u["low_price"] for u in ups) == w["low_price"]


def test_two_slices_merge_into_one_pending_update(me):
    syms = ["A", "B", "C"]
    eng = me.Engine(3, 128, np.full(3, 1_000, dtype=np.int64), max_batch=256, max_resting=1 << 12)
    svc = me.MatchingEngineService(eng, syms)
    try:
        svc.trades_subscribe()
        _limit(svc, "C", SELL, 1_010, 1)
        _limit(svc, "C", BUY, 1_010, 1)
        _limit(svc, "A", SELL, 1_020, BIG)
        _limit(svc, "A", BUY, 1_020, BIG)
        svc.flush(outputs=False)  # A and C are queued
        _limit(svc, "B", SELL, 1_030, 3)
        _limit(svc, "B", BUY, 1_030, 3)
        _limit(svc, "A", SELL, 1_015, BIG)
        _limit(svc, "A", SELL, 1_025, 7)
        _limit(svc, "A", BUY, 1_025, BIG)
        _limit(svc, "A", BUY, 1_025, 7)
        svc.flush(outputs=False)  # B joins; A keeps its place and merges its second slice in
        only_c = svc.trades_stream("C")
        assert [u["symbol"] for u in only_c] == ["C"] and only_c[0]["last_price"] == 1_010
        assert svc.trades_stream("C") == []
        ups = svc.trades_stream()
        assert [u["symbol"] for u in ups] == ["A", "B"]
        a = ups[0]
        assert (a["open_price"], a["last_price"], a["last_size"]) == (1_020, 1_025, 7)
        assert (a["high_price"], a["low_price"]) == (1_025, 1_015)
        assert a["volume"] == a["cum_volume"] == 2 * BIG + 7 and a["trades"] == a["cum_trades"] == 3  # no saturation
        assert (ups[1]["volume"], ups[1]["trades"], ups[1]["last_price"]) == (3, 1, 1_030)
        assert svc.trades_stream() == []
        _limit(svc, "A", SELL, 1_022, 2)
        _limit(svc, "A", BUY, 1_022, 2)
        svc.flush(outputs=False)  # a drained symbol starts a fresh update; its totals go on
        (a,) = svc.trades_stream()
        assert (a["open_price"], a["high_price"], a["low_price"], a["volume"], a["trades"]) == (1_022, 1_022, 1_022, 2, 1)
        assert a["cum_volume"] == 2 * BIG + 9 and a["cum_trades"] == 4
    finally:
        svc.close()
        eng.close()


def test_a_reused_book_reports_each_names_own_totals(me):
    """One book. A trades and its last order is cancelled; B takes the idle book and trades. The device's
    cumulative counters span both names; the service's are per name."""
    eng = me.Engine(1, 128, np.array([1_000], dtype=np.int64), max_batch=256, max_resting=1 << 12)
    svc = me.MatchingEngineService(eng, ["A"])
    try:
        svc.trades_subscribe()
        _limit(svc, "A", SELL, 1_050, 5)
        _limit(svc, "A", BUY, 1_050, 3)
        svc.flush(outputs=False)
        (a,) = svc.trades_stream()
        assert (a["symbol"], a["volume"], a["cum_volume"], a["cum_trades"], a["last_price"]) == ("A", 3, 3, 1, 1_050)
        _limit(svc, "A", BUY, 1_050, 2)  # A's book empties (its second fill is not drained yet)
        svc.flush(outputs=False)
        r = svc.submit_order("C", "B", 0, SELL, 1_040, 4, 4)  # the only book is idle: B takes it
        assert r["success"], r
        assert svc.stats()["reclaimed_books"] == 1
        _limit(svc, "B", BUY, 1_040, 4)
        svc.flush(outputs=False)
        ups = svc.trades_stream()
        assert [u["symbol"] for u in ups] == ["A", "B"]
        a, b = ups
        assert (a["volume"], a["trades"], a["cum_volume"], a["cum_trades"], a["last_size"]) == (2, 1, 5, 2, 2)
        assert (b["volume"], b["trades"], b["cum_volume"], b["cum_trades"]) == (4, 1, 4, 1)
        assert (b["open_price"], b["last_price"], b["high_price"], b["low_price"]) == (1_040,) * 4
        assert svc.trades_stream() == []
    finally:
        svc.close()
        eng.close()


def test_streaming_needs_a_subscription_and_off_drops_the_queue(me):
    eng = me.Engine(1, 128, np.array([1_000], dtype=np.int64), max_batch=256, max_resting=1 << 12)
    svc = me.MatchingEngineService(eng, ["A"])
    try:
        with pytest.raises(me.ServiceError) as ei:
            svc.trades_stream()
        assert ei.value.code == me.ME_E_INVALID
        svc.trades_subscribe()
        _limit(svc, "A", SELL, 1_050, 5)
        _limit(svc, "A", BUY, 1_050, 5)
        svc.flush(outputs=False)
        svc.trades_subscribe(False)
        with pytest.raises(me.ServiceError) as ei:
            svc.trades_stream()
        assert ei.value.code == me.ME_E_INVALID
        svc.trades_subscribe()  # afresh: nothing queued, the totals start again
        assert svc.trades_stream() == []
        _limit(svc, "A", SELL, 1_051, 1)
        _limit(svc, "A", BUY, 1_051, 1)
        svc.flush(outputs=False)
        (a,) = svc.trades_stream()
        assert (a["cum_volume"], a["cum_trades"]) == (1, 1)
    finally:
        svc.close()
        eng.close()
