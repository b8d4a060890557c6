"""Stop orders through the service (me_service_stops_enable / _submit_stop / _cancel_stop / _stop_updates / _stops /
_stop_stats, include/me_service.h) over a Python matcher with the four stop hooks (tests/stops_service_common.py
StopMatcher: an OracleBook and tests/stops_model.StopModel). Runs on CPU."""
import numpy as np
import pytest

from tests import stops_service_common as c
from tests.stops_service_common import (ARMED, BUY, CANCEL_REJECTED, CANCELED, LIMIT, MARKET, MID, QUEUED, SELL,
                                        TRIGGERED, StopMatcher, limit, stop)


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _svc(me, syms=("A", "B"), cap=8, db=None, matcher=None, books=None, max_batch=4096):
    m = matcher or StopMatcher(books or len(syms), max_batch=max_batch)
    svc = me.MatchingEngineService(None, list(syms), db_path=db, matcher=m)
    if cap:
        svc.stops_enable(cap)
    return svc, m


def _states(ups):
    return [(u["stop_id"], u["state"]) for u in ups]


def test_validation_string_by_string(me):
    svc, _ = _svc(me, cap=0)
    try:
        # before the enable every call answers "not enabled"
        r = svc.submit_stop("a", "A", MARKET, BUY, 0, MID, 4, 1)
        assert (r["success"], r["error_message"], r["order_id"]) == (False, "stop orders are not enabled", "")
        r = svc.cancel_stop("a", "SID-1")
        assert (r["success"], r["error_message"]) == (False, "stop orders are not enabled")
        assert svc.stops() == [] and svc.stop_updates() == []
        assert svc.stop_stats() == {"live": 0, "triggered": 0, "recovered": 0}
        svc.stops_enable(2)
        with pytest.raises(me.ServiceError) as ei:
            svc.stops_enable(2)
        assert ei.value.code == me.ME_E_STATE
        oid0 = svc.next_oid
        bad = [  # (request, message, grpc status), in the order of the checks
            (("a", "", MARKET, BUY, 0, MID, 4, 1, 0), "symbol is required", 0),
            (("a", "A", MARKET, BUY, 0, MID, 4, 0, 0), "quantity must be > 0", 0),
            (("a", "", MARKET, BUY, 0, MID, 4, 0, 9), "symbol is required", 0),  # the first failing check wins
            (("a", "A", LIMIT, BUY, 0, MID, 4, 1, 0), "price must be > 0 for LIMIT", 0),
            (("a", "A", LIMIT, BUY, 0, MID, 4, 1, 9), "price must be > 0 for LIMIT", 0),
            (("a", "A", LIMIT, BUY, 5, MID, 4, 1, 4), "invalid time in force", 0),
            (("a", "A", LIMIT, BUY, 5, MID, 4, 1, -1), "invalid time in force", 0),
            (("a", "A", MARKET, BUY, 0, MID, 4, 1, 3), "invalid time in force", 0),  # POST_ONLY on a MARKET
            (("a", "A", LIMIT, BUY, 5, MID, 99, 1, 0), "scale out of range", 2),
            (("a", "A", LIMIT, BUY, 2 ** 62, MID, 0, 1, 0), "overflow", 2),
            (("a", "A", MARKET, BUY, 2 ** 62, 2 ** 62, 0, 1, 0), "overflow", 2),  # the stop price (a MARKET's price is ignored)
            (("a", "A", MARKET, BUY, 0, -2 ** 62, 0, 1, 0), "underflow", 2),
            (("a", "A", MARKET, 0, 0, MID, 4, 1, 0), "DB insert failed", 0),
            (("a", "A", MARKET, 3, 0, MID, 4, 1, 0), "DB insert failed", 0),
        ]
        for req, msg, grpc in bad:
            r = svc.submit_stop(*req)
            assert (r["success"], r["error_message"], r["grpc_status"], r["order_id"]) == (False, msg, grpc, ""), (req, r)
        # the same texts as SubmitOrder gives
        assert svc.submit_order("a", "A", LIMIT, BUY, 5, 99, 1)["error_message"] == "scale out of range"
        assert svc.submit_order("a", "A", LIMIT, BUY, 5, 4, 1, 9)["error_message"] == "invalid time in force"
        oid0 += 1  # (SubmitOrder's failed normalisation consumed one; no stop request did)
        assert svc.next_oid == oid0
        # a MARKET's price is ignored: not normalised, not checked
        assert svc.submit_stop("a", "A", MARKET, BUY, 2 ** 62, MID, 0, 1)["order_id"] == "SID-1"  # no SID was consumed
        assert svc.submit_stop("a", "A", LIMIT, SELL, MID, MID, 4, 1, 1)["order_id"] == "SID-2"
        r = svc.submit_stop("a", "A", MARKET, BUY, 0, MID, 4, 1)
        assert (r["success"], r["error_message"], r["grpc_status"], r["order_id"]) == (False, "stop capacity exhausted", 8, "")
        assert svc.next_oid == oid0 and svc.pending == 0
        assert [(u["stop_id"], u["state"], u["limit_price"]) for u in svc.stops()] == [("SID-1", QUEUED, 0), ("SID-2", QUEUED, MID)]
        # cancel's checks
        for sid in ("", "SID-", "SID-0", "OID-1", "SID-1x", "SID--1", "SID-18446744073709551616", " SID-1"):
            r = svc.cancel_stop("a", sid)
            assert (r["success"], r["error_message"]) == (False, "stop_id is invalid"), sid
        r = svc.cancel_stop("b", "SID-1")
        assert (r["success"], r["error_message"]) == (False, "stop belongs to another client")
        r = svc.cancel_stop("a", "SID-1")
        assert (r["success"], r["order_id"], r["error_message"]) == (True, "SID-1", "")
        assert svc.next_oid == oid0
    finally:
        svc.close()


def test_a_matcher_without_the_hooks_has_no_stop_orders(me):
    svc = me.MatchingEngineService(None, ["A"], matcher=c.PlainMatcher(1))
    try:
        with pytest.raises(me.ServiceError) as ei:
            svc.stops_enable(4)
        assert ei.value.code == me.ME_E_INVALID
        assert svc.submit_stop("a", "A", MARKET, BUY, 0, MID, 4, 1)["error_message"] == "stop orders are not enabled"
        limit(svc, "a", "A", BUY, MID, 1)  # the service is what it was
        svc.flush(outputs=False)
    finally:
        svc.close()


def test_basic_trigger(me):
    svc, m = _svc(me)
    try:
        steps, (sa, sb) = c.script_basic(svc)
        rest, trade, market, idle = steps
        assert (sa, sb) == ("SID-1", "SID-2")
        assert rest["stop_updates"] == [] and rest["next_oid"] == 2
        # first flush: ARMED twice, the trade, TRIGGERED with a fresh OID, the order pending, B's stop still listed
        assert trade["flush"][0] == [2]
        assert _states(trade["stop_updates"]) == [(sa, ARMED), (sb, ARMED), (sa, TRIGGERED)]
        t = trade["stop_updates"][2]
        assert (t["order_id"], t["client_id"], t["symbol"], t["trigger_price"], t["stop_price"], t["quantity"]) == \
            ("OID-3", "alice", "A", MID, MID, 5)
        assert t["kind"] == c.kind_of(BUY, MARKET)
        assert trade["pending"] == 1 and trade["next_oid"] == 4
        assert _states(trade["stops"]) == [(sb, ARMED)]
        assert trade["stats"] == {"live": 1, "triggered": 1, "recovered": 0}
        # second flush: the MARKET's fills; its OrderUpdates go to the stop's client
        assert market["flush"][0] == [3]
        assert market["flush"][2] == [(3, 1, MID, 5, 0)]
        mine = [u for u in market["order_updates"] if u["order_id"] == "OID-3"]
        assert [(u["client_id"], u["status"], u["fill_quantity"]) for u in mine] == [("alice", c.ST_FILLED, 5)]
        assert market["pending"] == 0 and market["stop_updates"] == []
        assert idle["flush"] == ([], [], []) and _states(idle["stops"]) == [(sb, ARMED)]
        assert m.model.dump()["id"].tolist() == [2]
    finally:
        svc.close()


def test_stream_position(me):
    """A trade through the stop price submitted BEFORE the stop (no flush in between) does not trigger it; the
    same trade submitted after it does."""
    svc, _ = _svc(me)
    try:
        limit(svc, "maker", "A", SELL, MID, 10)
        svc.flush(outputs=False)
        limit(svc, "carol", "A", BUY, MID, 1)  # before
        s1 = stop(svc, "alice", "A", MARKET, BUY, 0, MID, 2)
        svc.flush(outputs=False)
        assert _states(svc.stop_updates()) == [(s1, ARMED)] and svc.pending == 0
        limit(svc, "carol", "A", BUY, MID, 1)  # after
        svc.flush(outputs=False)
        assert _states(svc.stop_updates()) == [(s1, TRIGGERED)] and svc.pending == 1
        svc.flush(outputs=False)
    finally:
        svc.close()


def test_cascade_one_step_per_flush(me):
    from oracle.oracle import OracleBook

    svc, m = _svc(me)
    try:
        steps, n = c.script_cascade(svc)
        assert n == 4
        trig = [_states([u for u in s["stop_updates"] if u["state"] == TRIGGERED]) for s in steps[1:]]
        assert trig == [[("SID-1", TRIGGERED)], [("SID-2", TRIGGERED)], [("SID-3", TRIGGERED)], []]
        assert [s["pending"] for s in steps[1:]] == [1, 1, 1, 0]
        # replay what the flushes reported: every OID's record is known from the script and the TRIGGERED updates
        recs = {k + 1: (MID - k, 2, c.kind_of(BUY)) for k in range(5)}
        recs[6] = (MID, 1, c.kind_of(SELL))
        for s in steps:
            for u in s["stop_updates"]:
                if u["state"] == TRIGGERED:
                    recs[int(u["order_id"][4:])] = (u["limit_price"], u["quantity"], u["kind"])
        ob = OracleBook(2)
        for s in steps:
            seq, res, fills = s["flush"]
            if not seq:
                continue
            b = me.Batch(np.array(seq, np.uint64), np.array([recs[q][0] for q in seq], np.int64),
                         np.array([recs[q][1] for q in seq], np.int32), np.zeros(len(seq), np.uint32),
                         np.array([recs[q][2] for q in seq], np.uint8))
            r, f = ob.submit(b)
            assert [tuple(int(x[k]) for k in ("filled_qty", "remaining_qty", "fill_count", "tape_offset", "status", "reason"))
                    for x in r] == res
            assert [tuple(int(x[k]) for k in ("taker_seq", "maker_seq", "price_q4", "qty", "symbol")) for x in f] == fills
        for sidx in range(2):
            assert np.array_equal(ob.dump(sidx), m.ob.dump(sidx))
        assert sorted(recs) == list(range(1, 10))  # OIDs stay gap-free
    finally:
        svc.close()


def test_cancel(me):
    svc, _ = _svc(me)
    try:
        steps, (s1, s2, s3) = c.script_cancel(svc)
        armed, canceled, reject, one, drain = steps
        assert _states(armed["stop_updates"]) == [(s1, ARMED), (s2, ARMED)]
        assert _states(canceled["stop_updates"]) == [(s2, CANCELED)] and _states(canceled["stops"]) == [(s1, ARMED)]
        got = reject["stop_updates"]
        assert _states(got) == [(s1, TRIGGERED), (s1, CANCEL_REJECTED)]
        assert got[1]["client_id"] == "alice" and got[1]["symbol"] == "A" and got[1]["order_id"] == ""
        assert _states(one["stop_updates"]) == [(s3, ARMED), (s3, CANCELED), (s3, CANCEL_REJECTED), ("SID-999", CANCEL_REJECTED)]
        assert one["stop_updates"][3]["symbol"] == "" and one["stop_updates"][3]["client_id"] == "bob"
        assert one["stops"] == [] and one["stats"]["live"] == 0
        assert drain["pending"] == 0
        assert svc.stop_updates("alice") == []
    finally:
        svc.close()


def test_stop_updates_drain_per_client(me):
    svc, _ = _svc(me)
    try:
        a = stop(svc, "alice", "A", MARKET, BUY, 0, MID, 1)
        b = stop(svc, "bob", "A", MARKET, BUY, 0, MID, 1)
        svc.flush(outputs=False)  # a boundary with no slice behind it is applied by the flush
        assert _states(svc.stop_updates("bob")) == [(b, ARMED)]
        assert _states(svc.stops("alice")) == [(a, ARMED)]
        assert _states(svc.stop_updates()) == [(a, ARMED)] and svc.stop_updates() == []
    finally:
        svc.close()


def test_capacity(me):
    svc, _ = _svc(me, cap=2)
    try:
        limit(svc, "maker", "A", SELL, MID, 10)
        s1 = stop(svc, "a", "A", MARKET, BUY, 0, MID, 1)
        stop(svc, "a", "A", MARKET, BUY, 0, MID + 100, 1)
        r = svc.submit_stop("a", "A", MARKET, BUY, 0, MID, 4, 1)
        assert (r["success"], r["error_message"], r["grpc_status"]) == (False, "stop capacity exhausted", 8)
        limit(svc, "carol", "A", BUY, MID, 1)
        svc.flush(outputs=False)  # s1 triggers and its event is processed
        assert (s1, TRIGGERED) in _states(svc.stop_updates())
        assert stop(svc, "a", "A", MARKET, BUY, 0, MID, 1) == "SID-3"
        assert not svc.submit_stop("a", "A", MARKET, BUY, 0, MID, 4, 1)["success"]
        svc.flush(outputs=False)
        svc.flush(outputs=False)
        assert svc.pending == 0
    finally:
        svc.close()


def test_a_book_with_an_armed_stop_is_not_idle(me):
    svc, _ = _svc(me, syms=(), books=1)
    try:
        s1 = stop(svc, "a", "A", MARKET, BUY, 0, MID, 1)
        svc.flush(outputs=False)
        r = svc.submit_order("b", "B", LIMIT, BUY, MID, 4, 1)
        assert (r["success"], r["error_message"], r["grpc_status"]) == (False, "symbol capacity exhausted", 8)
        r = svc.submit_stop("b", "B", MARKET, BUY, 0, MID, 4, 1)
        assert (r["success"], r["error_message"], r["grpc_status"], r["order_id"]) == (False, "symbol capacity exhausted", 8, "")
        assert svc.cancel_stop("a", s1)["success"]
        svc.flush(outputs=False)
        assert _states(svc.stop_updates()) == [(s1, ARMED), (s1, CANCELED)]
        limit(svc, "b", "B", BUY, MID, 1)  # the book is handed over
        assert svc.stats()["reclaimed_books"] == 1
        svc.flush(outputs=False)
    finally:
        svc.close()


def test_persistence_and_restart(me, tmp_path):
    db = str(tmp_path / "stops.sqlite")
    svc, _ = _svc(me, cap=0, db=db)
    try:
        limit(svc, "maker", "A", SELL, MID, 10)
        svc.flush(outputs=False)
        assert not c.has_stops_table(db)  # a database that never enables stops keeps its schema
        svc.stops_enable(8)
        assert c.has_stops_table(db) and c.stop_rows(db) == []
        s1 = stop(svc, "alice", "A", MARKET, BUY, 0, MID, 2)           # will trigger and be flushed
        s2 = stop(svc, "alice", "A", LIMIT, BUY, MID + 7, MID + 3, 3, 1)  # stays armed (IOC stop-limit)
        s3 = stop(svc, "bob", "B", MARKET, SELL, 0, MID, 4)            # will be cancelled
        s4 = stop(svc, "bob", "A", MARKET, BUY, 0, MID + 1, 5)         # triggers last, its order never flushed
        svc.flush(outputs=False)
        rows = c.stop_rows(db)
        assert [r[0] for r in rows] == [1, 2, 3, 4] and {r[9] for r in rows} == {ARMED}
        assert rows[1] == (2, "alice", "A", BUY, LIMIT, 1, MID + 3, MID + 7, 3, ARMED, "", 0)
        assert svc.cancel_stop("bob", s3)["success"]
        limit(svc, "carol", "A", BUY, MID, 1)
        svc.flush(outputs=False)  # s3 CANCELED, s1 triggered: its order is pending, the row still ARMED
        rows = c.stop_rows(db)
        assert [r[9] for r in rows] == [ARMED, ARMED, CANCELED, ARMED]
        svc.flush(outputs=False)  # the order's slice: TRIGGERED commits with its orders row
        rows = c.stop_rows(db)
        assert rows[0][9:] == (TRIGGERED, "OID-3", MID) and [r[9] for r in rows[1:]] == [ARMED, CANCELED, ARMED]
        assert "OID-3" in [r[0] for r in c.order_rows(db)]
        limit(svc, "maker", "A", SELL, MID + 1, 10)
        limit(svc, "carol", "A", BUY, MID + 1, 8)  # 7 @ MID, 1 @ MID + 1
        svc.flush(outputs=False)  # s4 triggers; its order (OID-6) is never flushed
        ups = svc.stop_updates()
        assert (s4, TRIGGERED) in _states(ups) and svc.pending == 1
        assert svc.stop_stats() == {"live": 1, "triggered": 2, "recovered": 0}
    finally:
        svc.close()
    rows = c.stop_rows(db)
    assert [r[9] for r in rows] == [TRIGGERED, ARMED, CANCELED, ARMED]
    assert "OID-6" not in [r[0] for r in c.order_rows(db)]
    # ---- restart over a fresh model
    svc, m = _svc(me, cap=0, db=db)
    try:
        svc.flush(outputs=False)
        with pytest.raises(me.ServiceError) as ei:
            svc.stops_enable(1)
        assert ei.value.code == me.ME_E_CAPACITY
        assert svc.submit_stop("a", "A", MARKET, BUY, 0, MID, 4, 1)["error_message"] == "stop orders are not enabled"
        svc.stops_enable(8)
        assert svc.stop_stats() == {"live": 2, "triggered": 0, "recovered": 2}
        assert _states(svc.stops()) == [(s2, ARMED), (s4, ARMED)]  # TRIGGERED and CANCELED do not come back
        assert m.model.dump()["id"].tolist() == [2, 4]
        assert stop(svc, "zed", "B", MARKET, BUY, 0, MID, 1) == "SID-5"  # SIDs continue
        oid = svc.next_oid
        assert oid == 6  # (OID-6 was never persisted: the counter resumes from the rows)
        limit(svc, "carol", "A", BUY, MID + 1, 1)  # the next qualifying fill: s4 triggers again
        svc.flush(outputs=False)
        ups = svc.stop_updates()
        assert _states(ups) == [("SID-5", ARMED), (s4, TRIGGERED)]
        assert ups[1]["order_id"] == f"OID-{oid + 1}" and ups[1]["client_id"] == "bob"
        svc.flush(outputs=False)
        rows = c.stop_rows(db)
        assert [r[9] for r in rows] == [TRIGGERED, ARMED, CANCELED, TRIGGERED, ARMED]
        assert rows[3][10] == f"OID-{oid + 1}"
    finally:
        svc.close()


def test_no_database_works_in_memory(me):
    svc, _ = _svc(me)
    try:
        steps, _ = c.script_two_in_flight(svc)
        assert sum(u["state"] == TRIGGERED for s in steps for u in s["stop_updates"]) == 6
    finally:
        svc.close()


def test_a_boundary_is_applied_by_the_background_flusher(me):
    import time

    svc, _ = _svc(me)
    try:
        svc.start(interval_us=200)
        s1 = stop(svc, "a", "A", MARKET, BUY, 0, MID, 1)
        deadline = time.monotonic() + 20
        ups = []
        while not ups and time.monotonic() < deadline:
            ups = svc.stop_updates()
        assert _states(ups) == [(s1, ARMED)]
        svc.stop()
    finally:
        svc.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_differential(me, seed):
    syms = ["A", "B", "C", "D"]
    slice_max = 16  # small: slices also close at the slice size, in the middle of a flush
    svc, m = _svc(me, syms=syms, cap=6, max_batch=slice_max)
    mod = c.ServiceModel(syms, 6, slice_max)
    rng = np.random.default_rng(seed)
    clients = ["alice", "bob", "carol"]
    sids = []
    try:
        nflush = 0
        for step in range(400):
            x = rng.random()
            sym = syms[int(rng.integers(4))]
            cl = clients[int(rng.integers(3))]
            side = int(rng.choice([BUY, SELL]))
            px = MID + int(rng.integers(-4, 5))
            q = int(rng.integers(1, 9))
            if x < 0.55:
                market = rng.random() < 0.15
                tif = int(rng.choice([0, 0, 0, 1, 2])) if not market else 0
                r = svc.submit_order(cl, sym, MARKET if market else LIMIT, side, 0 if market else px, 4, q, tif)
                assert r["success"] and r["order_id"] == mod.submit_order(cl, sym, MARKET if market else LIMIT, side,
                                                                          0 if market else px, q, tif)
            elif x < 0.75:
                otype = MARKET if rng.random() < 0.5 else LIMIT
                tif = int(rng.choice([0, 1])) if otype == LIMIT else 0
                spx = MID + int(rng.integers(-3, 4))
                r = svc.submit_stop(cl, sym, otype, side, px if otype == LIMIT else 0, spx, 4, q, tif)
                exp = mod.submit_stop(cl, sym, otype, side, px, spx, q, tif)
                if exp is None:
                    assert (r["success"], r["error_message"]) == (False, "stop capacity exhausted")
                else:
                    assert r["success"] and r["order_id"] == exp
                    sids.append(int(exp[4:]))
            elif x < 0.85 and sids:
                sid = int(rng.choice(sids)) if rng.random() < 0.9 else int(rng.integers(1, 400))
                r = svc.cancel_stop(cl, f"SID-{sid}")
                assert r["success"] == mod.cancel_stop(cl, sid), (sid, r)
            elif x >= 0.85:
                nflush += 1
                seq, res, fills = svc.flush()
                mseq, mres, mtapes = mod.flush()
                assert [int(v) for v in seq] == mseq
                assert np.array_equal(res[["filled_qty", "remaining_qty", "fill_count", "status", "reason"]],
                                      np.concatenate(mres)[["filled_qty", "remaining_qty", "fill_count", "status", "reason"]]
                                      if mres else res[:0][["filled_qty", "remaining_qty", "fill_count", "status", "reason"]])
                assert np.array_equal(fills, np.concatenate(mtapes) if mtapes else fills[:0])
                assert svc.stop_updates() == mod.stop_updates
                assert svc.order_updates() == mod.order_updates
                mod.stop_updates, mod.order_updates = [], []
                assert svc.pending == mod.pending and svc.next_oid == mod.next_oid
                assert _states(svc.stops()) == mod.listed()
        while svc.pending:
            svc.flush(outputs=False)
            mod.flush()
        assert svc.stop_updates() == mod.stop_updates and svc.order_updates() == mod.order_updates
        assert nflush > 20 and len(mod.triggered) > 10 and len(set(mod.triggered)) == len(mod.triggered)
        assert svc.stop_stats()["triggered"] == len(mod.pairs)
        for sidx in range(4):
            assert np.array_equal(m.ob.dump(sidx), mod.ob.dump(sidx)), sidx
        assert m.model.dump()["id"].tolist() == mod.tb.dump()["id"].tolist()
    finally:
        svc.close()


def test_restart_script_over_the_matcher(me, tmp_path):
    """The script tests/test_stops_service_gpu.py compares between the engine and the matcher, on the matcher."""
    def make(db):
        svc = me.MatchingEngineService(None, ["A", "B"], db_path=db, matcher=StopMatcher(2, max_batch=8))
        return svc, svc.close

    steps, ids = c.script_restart(make, str(tmp_path / "restart.sqlite"))
    by = {s["what"]: s for s in steps}
    assert ids == ("SID-1", "SID-2", "SID-3", "SID-4") and len(steps) == 10
    assert [r[9] for r in by["destroyed"]["stop_rows"]] == [TRIGGERED, ARMED, CANCELED, ARMED]
    assert "OID-6" not in [r[0] for r in by["destroyed"]["order_rows"]]
    assert by["re-armed"]["stats"] == {"live": 2, "triggered": 0, "recovered": 2}
    assert _states(by["s2 triggers again"]["stop_updates"]) == [("SID-5", ARMED), ("SID-2", TRIGGERED)]
    assert by["its order"]["flush"][2] == [(7, 2, MID + 1, 3, 0)]
    assert [r[9] for r in by["destroyed again"]["stop_rows"]] == [TRIGGERED, TRIGGERED, CANCELED, ARMED, ARMED]


def test_sids_are_not_issued_again_after_off_and_on(me, tmp_path):
    for db in (None, str(tmp_path / "offon.sqlite")):
        svc, _ = _svc(me, db=db)
        try:
            assert stop(svc, "a", "A", MARKET, BUY, 0, MID, 1) == "SID-1"
            svc.flush(outputs=False)  # SID-1 is ARMED (and in the table, with a database)
            assert stop(svc, "a", "A", MARKET, BUY, 0, MID, 1) == "SID-2"  # QUEUED: never applied, never a row
            svc.stops_enable(0)
            assert svc.stops() == [] and svc.stop_updates() == []
            svc.stops_enable(8)
            assert svc.stop_stats()["recovered"] == (1 if db else 0)
            assert stop(svc, "b", "A", MARKET, BUY, 0, MID, 1) == "SID-3"
            svc.flush(outputs=False)
            assert ("SID-3", ARMED) in _states(svc.stop_updates())
        finally:
            svc.close()
