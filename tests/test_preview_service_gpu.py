"""me_service_preview_order on the HIP engine: the service's preview is the engine's, it leaves the service as it
was, the same request submitted next gets the previewed outcome, a name without a book is an empty book, invalid
requests carry SubmitOrder's messages. Needs an MI355X."""
import sqlite3

import numpy as np
import pytest

from tests import preview_model as pm
from tests.service_common import FeedMatcher

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
LIMIT, MARKET = 0, 1
GTC, IOC, FOK, POST_ONLY = 0, 1, 2, 3


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _rows(db):
    con = sqlite3.connect(db)
    try:
        return con.execute("SELECT COUNT(*) FROM orders").fetchone()[0], con.execute("SELECT COUNT(*) FROM fills").fetchone()[0]
    finally:
        con.close()


def _row(r):
    return tuple(int(r[f]) for f in pm.FIELDS) + (bytes(r["pad"]),)


def test_preview_through_the_service(me, tmp_path):
    mid = 1_000_000
    db = str(tmp_path / "preview.db")
    eng = me.Engine(3, 128, np.full(3, mid - 64, dtype=np.int64), max_batch=4096, max_resting=1 << 14)
    svc = me.MatchingEngineService(eng, ["A", "B"], db_path=db)
    try:
        for client, side, px, q in (("alice", SELL, mid + 1, 10), ("bob", SELL, mid + 1, 20), ("alice", SELL, mid + 3, 30),
                                    ("carol", BUY, mid - 2, 15), ("carol", BUY, mid - 3, 25)):
            assert svc.submit_order(client, "A", LIMIT, side, px, 4, q)["success"]
        svc.flush(outputs=False)
        svc.order_updates()
        state0 = (svc.next_oid, svc.pending, svc.unpersisted, _rows(db))
        requests = [(LIMIT, BUY, mid + 1, 25, GTC), (LIMIT, BUY, mid + 3, 100, GTC), (LIMIT, BUY, mid + 2, 31, IOC),
                    (LIMIT, BUY, mid + 3, 61, FOK), (LIMIT, BUY, mid + 3, 60, FOK), (MARKET, SELL, 0, 20, GTC),
                    (MARKET, SELL, 0, 41, FOK), (LIMIT, SELL, mid - 2, 5, POST_ONLY), (LIMIT, SELL, mid - 1, 5, POST_ONLY),
                    (LIMIT, BUY, mid, 7, GTC)]
        got = []
        for typ, side, px, q, tif in requests:
            r = svc.preview_order("dave", "A", typ, side, px, 4, q, tif)
            e = eng.order_preview(0, me.kind(side, typ, 0, tif), px, q)[0]  # symbol "A" is local id 0
            assert _row(r) == _row(e), (typ, side, px, q, tif)
            got.append(r.copy())
        # (spot values, so that two equal wrong answers do not pass)
        assert (int(got[0]["filled_qty"]), int(got[0]["fill_count"]), int(got[0]["status"]), int(got[0]["flags"])) == \
            (25, 2, me.ST_FILLED, pm.PV_HAS_OPP | pm.PV_CROSSES)
        assert (int(got[1]["filled_qty"]), int(got[1]["remaining_qty"]), int(got[1]["levels"]), me.preview_notional(got[1])) == \
            (60, 40, 2, 30 * (mid + 1) + 30 * (mid + 3))
        assert int(got[3]["status"]) == me.ST_CANCELED and int(got[3]["filled_qty"]) == 0 and int(got[4]["status"]) == me.ST_FILLED
        assert int(got[7]["reason"]) == me.RJ_WOULD_CROSS and int(got[8]["flags"]) == pm.PV_HAS_OPP | pm.PV_RESTS
        assert int(got[9]["status"]) == me.ST_NEW and int(got[9]["flags"]) == pm.PV_HAS_OPP | pm.PV_RESTS
        # nothing of the service moved
        assert (svc.next_oid, svc.pending, svc.unpersisted, _rows(db)) == state0
        assert svc.order_updates() == []
        # an order in an open slice is not in the book the preview sees; once flushed it is
        before = svc.preview_order("dave", "A", MARKET, BUY, 0, 5, 4, GTC)
        assert svc.submit_order("erin", "A", LIMIT, SELL, mid + 1, 4, 1000)["success"]
        assert _row(svc.preview_order("dave", "A", MARKET, BUY, 0, 5, 4, GTC)) == _row(before) and svc.pending == 1
        svc.flush(outputs=False)
        svc.order_updates()
        # the same request, submitted next, gets the previewed outcome
        for typ, side, px, q, tif in ((LIMIT, BUY, mid + 3, 45, GTC), (LIMIT, SELL, mid - 3, 50, IOC), (LIMIT, BUY, mid + 1, 5000, FOK),
                                      (LIMIT, BUY, mid - 1, 9, POST_ONLY)):
            pv = svc.preview_order("dave", "A", typ, side, px, 4, q, tif)
            assert svc.submit_order("dave", "A", typ, side, px, 4, q, tif)["success"]
            seq, res, fills = svc.flush()
            assert len(res) == 1
            pm.assert_matches_submit(pv, res[0], fills, f"service {(typ, side, px, q, tif)}")
        # a name without a book: an empty book, and no book is claimed for it
        oid0 = svc.next_oid
        for typ, tif, st, flags in ((LIMIT, GTC, me.ST_NEW, pm.PV_RESTS), (LIMIT, POST_ONLY, me.ST_NEW, pm.PV_RESTS),
                                    (LIMIT, IOC, me.ST_CANCELED, 0), (LIMIT, FOK, me.ST_CANCELED, 0), (MARKET, GTC, me.ST_CANCELED, 0)):
            r = svc.preview_order("dave", "NOBOOK", typ, BUY, mid, 4, 12, tif)
            want = np.zeros(1, dtype=me.PREVIEW_DTYPE)[0]
            want["remaining_qty"], want["status"], want["flags"] = 12, st, flags
            assert _row(r) == _row(want), (typ, tif)
        assert svc.next_oid == oid0
        # the engine's third book is still there for the next new name: "NOBOOK" did not take it (an interned name
        # with no order is never listed idle, so "C" would have been refused)
        assert svc.submit_order("dave", "C", LIMIT, BUY, mid, 4, 1)["success"]
        # invalid requests: ME_E_INVALID with SubmitOrder's message
        for args, tif, msg in ((("dave", "", LIMIT, BUY, mid, 4, 5), GTC, "symbol is required"),
                               (("dave", "A", LIMIT, BUY, mid, 4, 0), GTC, "quantity must be > 0"),
                               (("dave", "A", LIMIT, BUY, 0, 4, 5), GTC, "price must be > 0 for LIMIT"),
                               (("dave", "A", LIMIT, BUY, mid, 4, 5), 4, "invalid time in force"),
                               (("dave", "A", MARKET, BUY, 0, 4, 5), POST_ONLY, "invalid time in force"),
                               (("dave", "A", LIMIT, BUY, mid, 99, 5), GTC, "scale out of range"),
                               (("dave", "A", LIMIT, BUY, 1 << 62, 0, 5), GTC, "overflow"),
                               (("dave", "A", LIMIT, 0, mid, 4, 5), GTC, "DB insert failed")):
            oid = svc.next_oid
            with pytest.raises(me.ServiceError) as ei:
                svc.preview_order(*args, tif=tif)
            assert ei.value.code == me.ME_E_INVALID and msg in str(ei.value), (args, tif, str(ei.value))
            sub = svc.submit_order(*args, tif=tif)  # SubmitOrder refuses the same request in-band, with the same text
            assert not sub["success"] and sub["error_message"] == msg, (args, sub)
            assert svc.next_oid - oid in (0, 1)
    finally:
        svc.close()
        eng.close()


def test_a_matcher_has_no_preview(me):
    svc = me.MatchingEngineService(None, ["A"], matcher=FeedMatcher(1))
    try:
        with pytest.raises(me.ServiceError) as ei:
            svc.preview_order("alice", "A", LIMIT, BUY, 1_000, 4, 5)
        assert ei.value.code == me.ME_E_INVALID and "no order preview" in str(ei.value)
    finally:
        svc.close()
