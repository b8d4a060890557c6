"""Stop orders through the service on the HIP engine: the scripts of tests/stops_service_common.py run once over
an engine and once over the StopMatcher (an OracleBook and the StopModel), and everything the two services show —
stop updates, OrderUpdates, flush outputs, listed stops, database rows — must be identical; a restart; a cascade
under the background flusher. Needs an MI355X.

The engine judges the stops once per LAUNCH GROUP (me_engine.h): the engines here match one batch per launch
(batches_per_launch = 1), so a job judges one slice as the model's does. The service still keeps two slices in
flight, so a later slice's events can be readable before the earlier slice is collected."""
import time

import numpy as np
import pytest

from tests import stops_service_common as c
from tests.stops_service_common import ARMED, BUY, CANCELED, MARKET, MID, SELL, TRIGGERED, StopMatcher, limit, stop

pytestmark = pytest.mark.gpu

CAP = 8
MAX_BATCH = 8  # small: a flush of many records is many slices


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _engine(me):
    return me.Engine(2, 128, np.full(2, MID - 64, dtype=np.int64), max_batch=MAX_BATCH, max_resting=1 << 14,
                     batches_per_launch=1)


def _no_job_deferred(eng):
    st = eng.stops_stats()  # raises unless me_stops_stats answers ME_OK (a deferred job is ME_E_STATE)
    assert set(st) >= {"jobs", "events", "live"}
    return st


def _run_on_engine(me, script, db):
    eng = _engine(me)
    svc = me.MatchingEngineService(eng, ["A", "B"], db_path=db)
    try:
        svc.stops_enable(CAP)
        out = script(svc, db)
        _no_job_deferred(eng)
        return out
    finally:
        svc.close()
        eng.close()


def _run_on_matcher(me, script, db):
    svc = me.MatchingEngineService(None, ["A", "B"], db_path=db, matcher=StopMatcher(2, max_batch=MAX_BATCH))
    try:
        svc.stops_enable(CAP)
        return script(svc, db)
    finally:
        svc.close()


@pytest.mark.parametrize("script", [c.script_basic, c.script_cascade, c.script_cancel, c.script_two_in_flight],
                         ids=lambda f: f.__name__)
def test_engine_and_matcher_show_the_same(me, tmp_path, script):
    got, extra = _run_on_engine(me, script, str(tmp_path / "engine.sqlite"))
    exp, extra_m = _run_on_matcher(me, script, str(tmp_path / "matcher.sqlite"))
    assert extra == extra_m
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        for key in e:
            assert g[key] == e[key], (e["what"], key)
    assert any(u["state"] == TRIGGERED for s in got for u in s["stop_updates"])


def test_restart_engine_and_matcher_show_the_same(me, tmp_path):
    """The restart script (persist, destroy, re-create over a fresh backend, re-arm) once over engines and once
    over StopMatchers: every step's stop updates, OrderUpdates, flush outputs, listed stops, stats and database
    rows are identical. Each engine ends with me_stops_stats answering ME_OK."""
    made = []

    def make_engine(db):
        eng = _engine(me)
        svc = me.MatchingEngineService(eng, ["A", "B"], db_path=db)

        def finish():
            svc.close()  # (an engine's trigger book stays on when its service goes)
            try:
                made.append(_no_job_deferred(eng))
            finally:
                eng.close()

        return svc, finish

    def make_matcher(db):
        svc = me.MatchingEngineService(None, ["A", "B"], db_path=db, matcher=StopMatcher(2, max_batch=MAX_BATCH))
        return svc, svc.close

    got, ids = c.script_restart(make_engine, str(tmp_path / "engine.sqlite"), CAP)
    exp, ids_m = c.script_restart(make_matcher, str(tmp_path / "matcher.sqlite"), CAP)
    assert ids == ids_m == ("SID-1", "SID-2", "SID-3", "SID-4") and len(made) == 2
    assert [s["what"] for s in got] == [s["what"] for s in exp] and len(got) == 10
    for g, e in zip(got, exp):
        for key in e:
            assert g[key] == e[key], (e["what"], key)
    # and what the script is about, on the engine's own log
    by = {s["what"]: s for s in got}
    assert [r[9] for r in by["destroyed"]["stop_rows"]] == [TRIGGERED, ARMED, CANCELED, ARMED]
    assert "OID-6" not in [r[0] for r in by["destroyed"]["order_rows"]]  # s2's order was never flushed
    assert by["re-armed"]["stats"] == {"live": 2, "triggered": 0, "recovered": 2}
    assert [(u["stop_id"], u["state"]) for u in by["re-armed"]["stops"]] == [("SID-2", ARMED), ("SID-4", ARMED)]
    again = by["s2 triggers again"]["stop_updates"]
    assert [(u["stop_id"], u["state"], u["order_id"]) for u in again] == [("SID-5", ARMED, ""), ("SID-2", TRIGGERED, "OID-7")]
    assert by["its order"]["flush"][2] == [(7, 2, MID + 1, 3, 0)]
    rows = by["destroyed again"]["stop_rows"]
    assert [r[9] for r in rows] == [TRIGGERED, TRIGGERED, CANCELED, ARMED, ARMED] and rows[1][10:] == ("OID-7", MID + 1)



def test_a_cascade_completes_under_the_background_flusher(me, tmp_path):
    db = str(tmp_path / "bg.sqlite")
    eng = _engine(me)
    svc = me.MatchingEngineService(eng, ["A", "B"], db_path=db)
    try:
        svc.stops_enable(CAP)
        svc.start(interval_us=200)
        for k in range(5):
            limit(svc, "maker", "A", BUY, MID - k, 2)
        for k in range(3):
            stop(svc, f"c{k}", "A", MARKET, SELL, 0, MID - k, 2 + k)
        limit(svc, "x", "A", SELL, MID, 1)
        deadline = time.monotonic() + 30
        done = False
        while not done and time.monotonic() < deadline:  # nobody flushes: the flusher walks the cascade
            done = svc.stop_stats()["triggered"] == 3 and svc.pending == 0 and svc.unpersisted == 0
        assert done, (svc.stop_stats(), svc.pending, svc.unpersisted, svc.last_error())
        svc.stop()
        assert svc.pending == 0 and svc.unpersisted == 0
        assert [(u["stop_id"], u["state"]) for u in svc.stop_updates() if u["state"] == TRIGGERED] == \
            [("SID-1", TRIGGERED), ("SID-2", TRIGGERED), ("SID-3", TRIGGERED)]
        assert [r[9] for r in c.stop_rows(db)] == [TRIGGERED] * 3
        assert svc.order_book("A")[0] == []  # the three sells took the whole ladder (1 + 2 + 3 + 4 = 10)
        _no_job_deferred(eng)
    finally:
        svc.close()
        eng.close()
