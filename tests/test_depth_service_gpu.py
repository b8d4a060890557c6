"""The service's depth stream (me_service_depth_subscribe / me_service_depth_stream) on the HIP engine: every
book handed out equals the CPU oracle's top-D snapshot of the same orders. Needs an MI355X."""
import numpy as np
import pytest

from tests.service_common import FeedMatcher

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
BIG = 2_147_483_647


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


class Mirror:
    """Feeds the service and, record by record, a CPU oracle with the same orders."""

    def __init__(self, me, svc, syms):
        from oracle.oracle import OracleBook

        self.me, self.svc, self.syms = me, svc, syms
        self.ob = OracleBook(len(syms))
        self.seq, self.seq_of = 0, {}

    def _orc(self, px, q, s, kind, seq=None):
        from tests.tif_model import Arrays

        if seq is None:
            self.seq += 1
            seq = self.seq
        self.ob.submit(Arrays([seq], [px], [q], [self.syms.index(s)], [kind]))
        return seq

    def order(self, s, side, px, q, market=False):
        r = self.svc.submit_order("C", s, 1 if market else 0, side, 0 if market else px, 4, q)
        assert market or r["success"], r
        self.seq_of[r["order_id"]] = self._orc(0 if market else px, q, s, self.me.kind(side, 1 if market else 0))
        return r["order_id"]

    def cancel(self, s, oid):
        self.svc.cancel_order("C", s, oid)
        self._orc(self.seq_of[oid], 0, s, self.me.kind(BUY, 0, 1), seq=self.seq)

    def book(self, s, D):
        """The oracle's top-D book as depth_stream hands it out (sizes saturated to int32)."""
        bids, asks = self.ob.snapshot(self.syms.index(s), D)
        sat = lambda lv: [(int(x["price_q4"]), min(int(x["total_qty"]), BIG)) for x in lv]  # noqa: E731
        return {"symbol": s, "scale": 4, "bids": sat(bids), "asks": sat(asks)}


def test_books_equal_the_oracle_after_every_flush(me):
    syms, D = ["A", "B", "C"], 3
    eng = me.Engine(3, 128, np.full(3, 1_000_000 - 64, dtype=np.int64), max_batch=4096, max_resting=1 << 14)
    svc = me.MatchingEngineService(eng, syms)
    try:
        svc.depth_subscribe(D)
        assert svc.depth_stream() == []
        m = Mirror(me, svc, syms)
        rng = np.random.default_rng(7)
        prev = {s: m.book(s, D) for s in syms}
        live, seen = [], set()
        for k in range(6):
            touched = set()
            for _ in range(40):
                s = syms[int(rng.integers(3 if k in (0, 3) else 2))]  # (C trades in slices 0 and 3 only)
                touched.add(s)
                if live and rng.random() < 0.25:
                    oid, os_ = live.pop(int(rng.integers(len(live))))
                    m.cancel(os_, oid)
                    touched.add(os_)
                    continue
                market = rng.random() < 0.15
                side = int(rng.choice([BUY, SELL]))
                oid = m.order(s, side, 1_000_000 + int(rng.integers(-8, 9)), int(rng.integers(1, 40)), market)
                if not market:
                    live.append((oid, s))
            svc.flush(outputs=False)
            books = svc.depth_stream()
            names = [b["symbol"] for b in books]
            assert len(set(names)) == len(names)  # one pending book per symbol
            seen |= set(names)
            for b in books:
                assert b == m.book(b["symbol"], D), f"slice {k}"
                assert len(b["bids"]) <= D and len(b["asks"]) <= D
            now = {s: m.book(s, D) for s in syms}
            for s in syms:  # a changed view is handed out; a symbol nobody touched is not
                assert s in names or now[s] == prev[s], f"slice {k}: {s} changed without a book"
                assert s in touched or s not in names, f"slice {k}: {s} handed out unchanged"
            prev = now
        assert seen == set(syms)
        assert svc.depth_stream() == []
        assert svc.last_error() == ""
    finally:
        svc.close()
        eng.close()


def test_conflation_keeps_first_change_order_and_per_symbol_drain(me):
    syms, D = ["A", "B", "C"], 3
    eng = me.Engine(3, 128, np.full(3, 1_000, dtype=np.int64), max_batch=256, max_resting=1 << 12)
    svc = me.MatchingEngineService(eng, syms)
    try:
        svc.depth_subscribe(D)
        m = Mirror(me, svc, syms)
        m.order("C", BUY, 1_010, 1)
        m.order("A", BUY, 1_020, 2)
        svc.flush(outputs=False)  # A and C are queued
        m.order("B", SELL, 1_030, 3)
        m.order("A", BUY, 1_021, BIG)
        m.order("A", BUY, 1_021, BIG)  # (a level total above 2^31: the size saturates)
        svc.flush(outputs=False)  # B joins; A keeps its place and shows its newest book
        only_c = svc.depth_stream("C")
        assert only_c == [m.book("C", D)] and only_c[0]["bids"] == [(1_010, 1)]
        assert svc.depth_stream("C") == []
        books = svc.depth_stream()
        assert [b["symbol"] for b in books] == ["A", "B"]
        assert books[0]["bids"] == [(1_021, BIG), (1_020, 2)] and books[0]["asks"] == []
        assert eng.snapshot(0, 1)[0][0]["total_qty"] == 2 * BIG
        assert books[1] == m.book("B", D) and books[1]["asks"] == [(1_030, 3)]
        assert svc.depth_stream() == []
    finally:
        svc.close()
        eng.close()


def test_a_reused_book_is_named_by_the_slice_of_the_event(me):
    """One book. A rests and is cancelled empty; B takes the book. A's emptied book comes out under A's name
    with both counts 0, B's levels under B's name."""
    eng = me.Engine(1, 128, np.array([1_000], dtype=np.int64), max_batch=256, max_resting=1 << 12)
    svc = me.MatchingEngineService(eng, ["A"])
    try:
        svc.depth_subscribe(3)
        r = svc.submit_order("C", "A", 0, SELL, 1_050, 4, 5)
        svc.flush(outputs=False)
        assert svc.depth_stream() == [{"symbol": "A", "scale": 4, "bids": [], "asks": [(1_050, 5)]}]
        svc.cancel_order("C", "A", r["order_id"])
        svc.flush(outputs=False)  # A's book is empty: not drained yet
        r = svc.submit_order("C", "B", 0, BUY, 1_040, 4, 3)  # the only book is idle: B takes it
        assert r["success"], r
        assert svc.stats()["reclaimed_books"] == 1
        svc.flush(outputs=False)
        assert svc.depth_stream() == [{"symbol": "A", "scale": 4, "bids": [], "asks": []},
                                      {"symbol": "B", "scale": 4, "bids": [(1_040, 3)], "asks": []}]
        assert svc.depth_stream() == []
    finally:
        svc.close()
        eng.close()


def test_a_matcher_has_no_depth_feed_and_streaming_needs_a_subscription(me):
    svc = me.MatchingEngineService(None, ["A"], matcher=FeedMatcher(1))
    try:
        with pytest.raises(me.ServiceError) as ei:
            svc.depth_subscribe(3)
        assert ei.value.code == me.ME_E_INVALID and "no depth feed" in str(ei.value)
        with pytest.raises(me.ServiceError) as ei:
            svc.depth_stream()
        assert ei.value.code == me.ME_E_INVALID
    finally:
        svc.close()
    eng = me.Engine(1, 128, np.array([1_000], dtype=np.int64), max_batch=256, max_resting=1 << 12)
    svc = me.MatchingEngineService(eng, ["A"])
    try:
        with pytest.raises(me.ServiceError) as ei:
            svc.depth_stream()
        assert ei.value.code == me.ME_E_INVALID
        svc.depth_subscribe(3)
        assert svc.depth_stream() == []
        svc.depth_subscribe(0)
        with pytest.raises(me.ServiceError) as ei:
            svc.depth_stream()
        assert ei.value.code == me.ME_E_INVALID
    finally:
        svc.close()
        eng.close()
