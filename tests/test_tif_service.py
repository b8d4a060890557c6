"""me_service_submit_order_tif (include/me_service.h) on the GPU engine: OIDs and responses, the in-band
"invalid time in force" answer, the OrderUpdate sequence of a partly filled IOC, a killed FOK and a rejected
POST_ONLY, SQLite rows at their final state, and a restart that rebuilds the book with the resting POST_ONLY
order and no IOC remainder. Then two TCP ranks on the one GPU: merged results and tapes of a time-in-force
stream against the model. Needs an MI355X."""
import json
import os
import socket
import sqlite3
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT, MARKET, BUY, SELL = 0, 1, 1, 2
ST_NEW, ST_PARTIAL, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
MID = 1_000_000


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _upd(u):
    return (u["order_id"], u["status"], u["fill_price"], u["fill_quantity"], u["remaining_quantity"])


def test_service_time_in_force(me, tmp_path):
    db = str(tmp_path / "tif.sqlite")
    base = [MID - 64, MID - 64]
    with me.Engine(2, 128, base, max_batch=1024, max_resting=1024) as eng:
        svc = me.MatchingEngineService(eng, ["SYM", "ABC"], db_path=db)
        r = svc.submit_order("M", "SYM", LIMIT, SELL, MID + 10, 4, 10)
        assert r["order_id"] == "OID-1" and r["success"]
        # in-band refusals: no OID consumed; the reference's own checks come first
        for tif in (4, 7, -1):
            r = svc.submit_order("T", "SYM", LIMIT, BUY, MID + 10, 4, 15, tif=tif)
            assert r == {"order_id": "", "success": False, "error_message": "invalid time in force", "grpc_status": 0}
        r = svc.submit_order("T", "SYM", MARKET, BUY, 0, 4, 15, tif=me.TIF_POST_ONLY)
        assert r["error_message"] == "invalid time in force" and not r["order_id"] and not r["success"]
        assert svc.submit_order("T", "", LIMIT, BUY, MID, 4, 1, tif=9)["error_message"] == "symbol is required"
        assert svc.submit_order("T", "SYM", LIMIT, BUY, MID, 4, 0, tif=9)["error_message"] == "quantity must be > 0"
        assert svc.submit_order("T", "SYM", LIMIT, BUY, 0, 4, 1, tif=9)["error_message"] == "price must be > 0 for LIMIT"
        assert svc.next_oid == 2
        assert svc.submit_order("T", "SYM", LIMIT, BUY, MID + 10, 4, 15, tif=me.TIF_IOC)["order_id"] == "OID-2"
        assert svc.submit_order("T", "SYM", LIMIT, BUY, MID + 20, 4, 5, tif=me.TIF_FOK)["order_id"] == "OID-3"
        assert svc.submit_order("M", "SYM", LIMIT, SELL, MID + 30, 4, 10)["order_id"] == "OID-4"
        assert svc.submit_order("T", "SYM", LIMIT, BUY, MID + 30, 4, 5, tif=me.TIF_POST_ONLY)["order_id"] == "OID-5"
        r = svc.submit_order("T", "SYM", LIMIT, BUY, MID - 10, 4, 7, tif=me.TIF_POST_ONLY)
        assert r == {"order_id": "OID-6", "success": True, "error_message": "", "grpc_status": 0}
        assert svc.submit_order("T", "SYM", MARKET, SELL, 0, 4, 3, tif=me.TIF_FOK)["order_id"] == "OID-7"
        seq, res, fills = svc.flush()
        assert seq.tolist() == [1, 2, 3, 4, 5, 6, 7]
        assert res["status"].tolist() == [ST_NEW, ST_CANCELED, ST_CANCELED, ST_NEW, ST_REJECTED, ST_NEW, ST_FILLED]
        assert res["reason"].tolist() == [0, 0, 0, 0, me.RJ_WOULD_CROSS, 0, 0]
        assert res["filled_qty"].tolist() == [0, 10, 0, 0, 0, 0, 3]
        assert res["remaining_qty"].tolist() == [10, 5, 5, 10, 5, 7, 0]
        assert len(fills) == 2
        ups = [_upd(u) for u in svc.order_updates()]
        assert ups == [
            ("OID-1", ST_NEW, 0, 0, 10),
            ("OID-1", ST_FILLED, MID + 10, 10, 0),            # the maker, then the IOC taker
            ("OID-2", ST_PARTIAL, MID + 10, 10, 5),
            ("OID-2", ST_CANCELED, 0, 0, 5),                  # the IOC remainder
            ("OID-3", ST_CANCELED, 0, 0, 5),                  # the killed FOK
            ("OID-4", ST_NEW, 0, 0, 10),
            ("OID-5", ST_REJECTED, 0, 0, 5),                  # POST_ONLY that would cross
            ("OID-6", ST_NEW, 0, 0, 7),
            ("OID-6", ST_PARTIAL, MID - 10, 3, 4),            # the resting POST_ONLY is an ordinary maker
            ("OID-7", ST_FILLED, MID - 10, 3, 0),
        ]
        con = sqlite3.connect(db)
        rows = con.execute("SELECT order_id, status, remaining_quantity, quantity FROM orders ORDER BY order_id").fetchall()
        con.close()
        assert rows == [("OID-1", ST_FILLED, 0, 10), ("OID-2", ST_CANCELED, 5, 15), ("OID-3", ST_CANCELED, 5, 5),
                        ("OID-4", ST_NEW, 10, 10), ("OID-5", ST_REJECTED, 5, 5), ("OID-6", ST_PARTIAL, 4, 7),
                        ("OID-7", ST_FILLED, 0, 3)]
        # an IOC never rests: nothing to cancel
        assert svc.cancel_order("T", "SYM", "OID-2")["success"]
        svc.flush()
        assert [_upd(u) for u in svc.order_updates()] == [("OID-2", ST_REJECTED, 0, 0, 0)]
        svc.close()
    # restart on fresh books: the resting orders come back as plain LIMITs, the IOC remainder does not
    with me.Engine(2, 128, base, max_batch=1024, max_resting=1024) as eng:
        svc = me.MatchingEngineService(eng, ["SYM", "ABC"], db_path=db)
        assert svc.stats()["recovered_orders"] == 2 and svc.next_oid == 8
        svc.flush()
        bids, asks = svc.order_book("SYM")
        assert [(o["order_id"], o["client_id"], o["price"], o["quantity"]) for o in bids] == [("OID-6", "T", MID - 10, 4)]
        assert [(o["order_id"], o["client_id"], o["price"], o["quantity"]) for o in asks] == [("OID-4", "M", MID + 30, 10)]
        assert eng.resting_count() == 2
        assert svc.cancel_order("T", "SYM", "OID-6")["success"]
        svc.flush()
        assert ("OID-6", ST_CANCELED, 0, 0, 4) in [_upd(u) for u in svc.order_updates()]
        svc.close()


def test_cluster_two_tcp_ranks_match_the_model(built, tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "tif_cluster.json")
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        # child processes (never exec over a GPU-initialised interpreter)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "tif_cluster_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors="replace")[-3000:])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    r = json.load(open(out))
    assert r["ok"], r["msg"]
    assert r["records"] >= 6000 and r["fills"] > 1000
