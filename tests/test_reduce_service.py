"""me_service_reduce_order (include/me_service.h): the owner check and the in-band errors with no OID consumed,
the OrderUpdate of a partial reduce (of a never-filled and of a partly filled order), of a covering reduce and
of a reduce of an unknown order, the SQLite rows for a target in the same slice and in an earlier one, and a
restart that rebuilds the book with the reduced order in its place. The scenarios run on the HIP engine
(needs an MI355X) and, for the service's own code, over the model behind me_service_create_matcher (no GPU).
Then two TCP ranks on the one GPU: merged results, tapes and books of a stream with reduces against the model.
"""
import json
import os
import socket
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT, MARKET, BUY, SELL = 0, 1, 1, 2
ST_NEW, ST_PARTIAL, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
MID = 1_000_000
BASE = [MID - 64, MID - 64]
BACKENDS = [pytest.param("engine", marks=pytest.mark.gpu), "model"]


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


class ModelBackend:
    """me_matcher over ONE ReduceBook (tests/reduce_model.py) holding every symbol."""

    def __init__(self, n):
        from tests.reduce_model import ReduceBook

        self.book = ReduceBook(n)
        self.num_symbols, self.max_batch, self.max_resting = n, 1024, 1024

    def match(self, b):
        return self.book.submit(b)

    def book_orders(self, s, depth):
        from matching_engine_amd import LEVEL_DTYPE
        from tests._parity import side_levels

        depth = depth or (1 << 20)
        d = self.book.dump(s)
        sides = [side_levels(d, 1, depth), side_levels(d, 2, depth)]
        levels = []
        for x in sides:
            prices = list(dict.fromkeys(x["price_q4"].tolist()))
            levels.append(np.array([(p, int(x["qty"][x["price_q4"] == p].sum()), int((x["price_q4"] == p).sum()), 0)
                                    for p in prices], dtype=LEVEL_DTYPE))
        return sides[0], sides[1], levels[0], levels[1]

    def c_matcher(self):
        from matching_engine_amd.cluster import python_matcher

        return python_matcher(self)

    def close(self):
        pass


class _Svc:
    """A service over a fresh backend of the given kind on `db`."""

    def __init__(self, me, backend, db):
        self.eng = me.Engine(2, 128, BASE, max_batch=1024, max_resting=1024) if backend == "engine" else None
        self.mb = ModelBackend(2) if self.eng is None else None
        self.svc = me.MatchingEngineService(self.eng, ["SYM", "ABC"], db_path=db, matcher=self.mb)

    def __enter__(self):
        return self.svc

    def __exit__(self, *a):
        self.svc.close()
        if self.eng is not None:
            self.eng.close()


def _upd(u):
    return (u["order_id"], u["client_id"], u["status"], u["fill_price"], u["fill_quantity"], u["remaining_quantity"])


def _rows(db):
    con = sqlite3.connect(db)
    rows = con.execute("SELECT order_id, status, remaining_quantity, quantity FROM orders "
                       "ORDER BY CAST(SUBSTR(order_id, 5) AS INTEGER)").fetchall()
    con.close()
    return rows


def _flush(svc):
    seq, res, fills = svc.flush()
    return seq.tolist(), res["status"].tolist(), res["remaining_qty"].tolist(), len(fills)


@pytest.mark.parametrize("backend", BACKENDS)
def test_service_reduce_order(me, tmp_path, backend):
    db = str(tmp_path / "reduce.sqlite")
    refused = lambda msg: {"order_id": "", "success": False, "error_message": msg, "grpc_status": 0}  # noqa: E731
    with _Svc(me, backend, db) as svc:
        assert svc.submit_order("M", "SYM", LIMIT, SELL, MID + 10, 4, 10)["order_id"] == "OID-1"
        assert svc.submit_order("M", "SYM", LIMIT, SELL, MID + 10, 4, 10)["order_id"] == "OID-2"
        # in-band refusals, first failing check first; none consumes an OID or queues a record
        assert svc.reduce_order("M", "", "OID-1", 3) == refused("symbol is required")
        assert svc.reduce_order("M", "SYM", "OID-1", 0) == refused("quantity must be > 0")
        assert svc.reduce_order("M", "SYM", "bogus", -5) == refused("quantity must be > 0")
        assert svc.reduce_order("M", "SYM", "bogus", 3) == refused("order_id is invalid")
        assert svc.reduce_order("M", "SYM", "OID-0", 3) == refused("order_id is invalid")
        assert svc.reduce_order("X", "SYM", "OID-1", 3) == refused("order belongs to another client")
        assert svc.next_oid == 3 and svc.pending == 2
        assert _flush(svc) == ([1, 2], [ST_NEW, ST_NEW], [10, 10], 0)
        assert svc.reduce_order("X", "SYM", "OID-1", 3) == refused("order belongs to another client")  # (resting now)
        svc.order_updates()
        # slice B: a target of the same slice, a target of an earlier slice (never filled), then a fill of it
        assert svc.submit_order("M", "SYM", LIMIT, BUY, MID - 10, 4, 20)["order_id"] == "OID-3"
        r = svc.reduce_order("M", "SYM", "OID-3", 5)
        assert r == {"order_id": "OID-3", "success": True, "error_message": "", "grpc_status": 0}
        assert svc.reduce_order("M", "SYM", "OID-1", 4)["success"]
        assert svc.next_oid == 4  # a reduce takes no OID
        assert svc.submit_order("T", "SYM", LIMIT, BUY, MID + 10, 4, 2)["order_id"] == "OID-4"
        assert _flush(svc) == ([3, 3, 3, 4], [ST_NEW, ST_NEW, ST_NEW, ST_FILLED], [20, 15, 6, 0], 1)
        assert [_upd(u) for u in svc.order_updates()] == [
            ("OID-3", "M", ST_NEW, 0, 0, 20),
            ("OID-3", "M", ST_NEW, 0, 0, 15),                # reduced in its own slice: still NEW
            ("OID-1", "M", ST_NEW, 0, 0, 6),                 # never filled: NEW with the smaller remainder
            ("OID-1", "M", ST_PARTIAL, MID + 10, 2, 4),      # it kept its place ahead of OID-2
            ("OID-4", "T", ST_FILLED, MID + 10, 2, 0),
        ]
        assert _rows(db) == [("OID-1", ST_PARTIAL, 4, 10), ("OID-2", ST_NEW, 10, 10), ("OID-3", ST_NEW, 15, 20),
                             ("OID-4", ST_FILLED, 0, 2)]
        # slice C: a partly filled target, a covering reduce, unknown targets (another requester hears of those)
        assert svc.reduce_order("M", "SYM", "OID-1", 1)["success"]
        assert svc.reduce_order("M", "SYM", "OID-2", 50)["success"]
        assert svc.reduce_order("Z", "SYM", "OID-999", 1)["success"]
        assert svc.reduce_order("M", "NOPE", "OID-3", 1)["order_id"] == "OID-3"  # a symbol with no book
        assert svc.reduce_order("T", "SYM", "OID-4", 1)["success"]               # filled: not resting
        assert _flush(svc) == ([4] * 5, [ST_NEW, ST_CANCELED, ST_REJECTED, ST_REJECTED, ST_REJECTED], [3, 10, 0, 0, 0], 0)
        assert [_upd(u) for u in svc.order_updates()] == [
            ("OID-1", "M", ST_PARTIAL, 0, 0, 3),             # the target's own status
            ("OID-2", "M", ST_CANCELED, 0, 0, 10),           # exactly a cancel's update
            ("OID-999", "Z", ST_REJECTED, 0, 0, 0),
            ("OID-3", "M", ST_REJECTED, 0, 0, 0),            # (OID-3 rests on SYM, untouched)
            ("OID-4", "T", ST_REJECTED, 0, 0, 0),
        ]
        assert _rows(db) == [("OID-1", ST_PARTIAL, 3, 10), ("OID-2", ST_CANCELED, 10, 10), ("OID-3", ST_NEW, 15, 20),
                             ("OID-4", ST_FILLED, 0, 2)]
        # slices D, E: an earlier slice's order reduced and then filled completely in one slice ends FILLED, 0
        assert svc.submit_order("M", "ABC", LIMIT, SELL, MID + 20, 4, 10)["order_id"] == "OID-5"
        _flush(svc)
        assert svc.reduce_order("M", "ABC", "OID-5", 4)["success"]
        assert svc.submit_order("T", "ABC", LIMIT, BUY, MID + 20, 4, 6)["order_id"] == "OID-6"
        assert _flush(svc) == ([5, 6], [ST_NEW, ST_FILLED], [6, 0], 1)
        assert _rows(db)[4:] == [("OID-5", ST_FILLED, 0, 10), ("OID-6", ST_FILLED, 0, 6)]
        # a later order at OID-1's price, then the restart
        assert svc.submit_order("N", "SYM", LIMIT, SELL, MID + 10, 4, 5)["order_id"] == "OID-7"
        _flush(svc)
        svc.order_updates()
    with _Svc(me, backend, db) as svc:
        assert svc.stats()["recovered_orders"] == 3 and svc.next_oid == 8
        svc.flush()
        bids, asks = svc.order_book("SYM")
        assert [(o["order_id"], o["client_id"], o["price"], o["quantity"]) for o in asks] == \
            [("OID-1", "M", MID + 10, 3), ("OID-7", "N", MID + 10, 5)]  # reduced, and still ahead
        assert [(o["order_id"], o["quantity"]) for o in bids] == [("OID-3", 15)]
        lb, la = svc.get_order_book("SYM")
        assert [(int(x["price_q4"]), int(x["total_qty"])) for x in la] == [(MID + 10, 8)]
        svc.order_updates()
        # recovery filled in what a reduce's update needs: OID-1 had traded, OID-3 had not
        assert svc.reduce_order("M", "SYM", "OID-1", 1)["success"]
        assert svc.reduce_order("M", "SYM", "OID-3", 1)["success"]
        assert svc.submit_order("T", "SYM", LIMIT, BUY, MID + 10, 4, 4)["order_id"] == "OID-8"
        seq, st, rem, nf = _flush(svc)
        assert (st, rem, nf) == ([ST_NEW, ST_NEW, ST_FILLED], [2, 14, 0], 2)
        assert [_upd(u) for u in svc.order_updates()] == [
            ("OID-1", "M", ST_PARTIAL, 0, 0, 2),
            ("OID-3", "M", ST_NEW, 0, 0, 14),
            ("OID-1", "M", ST_FILLED, MID + 10, 2, 0),       # the taker fills the reduced order first
            ("OID-8", "T", ST_PARTIAL, MID + 10, 2, 2),
            ("OID-7", "N", ST_PARTIAL, MID + 10, 2, 3),
            ("OID-8", "T", ST_FILLED, MID + 10, 2, 0),
        ]
        rows = dict((r[0], r[1:]) for r in _rows(db))
        assert rows["OID-1"] == (ST_FILLED, 0, 10) and rows["OID-3"] == (ST_NEW, 14, 20)
        assert rows["OID-7"] == (ST_PARTIAL, 3, 5)


@pytest.mark.gpu
def test_cluster_two_tcp_ranks_match_the_model(built, tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "reduce_cluster.json")
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        # child processes (never exec over a GPU-initialised interpreter)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "reduce_cluster_worker.py"), out], env=env,
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
    assert r["records"] >= 5900 and r["fills"] > 1000 and r["reduces"] > 600
