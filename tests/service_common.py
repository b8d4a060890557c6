"""What the service tests share: the me_matcher contract over an oracle book (FeedMatcher), a LIMIT through the
service, and the launcher of the QUOTES cluster workers (tests/quotes_cluster_worker.py)."""
import json
import os
import socket
import subprocess
import sys

from tests import quote_model as qm

HERE = os.path.dirname(os.path.abspath(__file__))
BUY, SELL = 1, 2
BIG = 2_147_483_647


class FeedMatcher:
    """The me_matcher contract over one OracleBook, with (feed=True) the quotes() hook."""

    def __init__(self, n, feed=True, lag=0):
        from oracle.oracle import OracleBook

        self.ob = OracleBook(n)
        self.num_symbols, self.max_batch, self.max_resting = n, 4096, 1 << 16
        if feed:
            self.feed = qm.OracleFeed(self.ob, n, lag=lag)
            self.quotes = self.feed.quotes

    def match(self, b):
        out = self.ob.submit(b)
        if hasattr(self, "feed"):
            self.feed.matched()
        return out

    def book_orders(self, s, depth):
        from tests._parity import side_levels

        d = self.ob.dump(s)
        lb, la = self.ob.snapshot(s, depth)
        return side_levels(d, 1, depth), side_levels(d, 2, depth), lb, la

    def c_matcher(self):
        from matching_engine_amd.cluster import python_matcher

        return python_matcher(self)


def _limit(svc, sym, side, px, q):
    r = svc.submit_order("C", sym, 0, side, px, 4, q)
    assert r["success"], r
    return r["order_id"]


def _run_cluster(kind, world, tmp_path, timeout=180):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / f"quotes_cluster_{kind}.json")
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        # child processes (never exec over a GPU-initialised interpreter)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "quotes_cluster_worker.py"), kind, out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors="replace")[-3000:])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return json.load(open(out))
