"""One rank of the quote-feed cluster check (launched through tests/service_common.py by tests/test_quotes_service.py and
tests/test_quotes_service_gpu.py). Rank 0 turns every shard's feed on (me_cluster_quotes_enable), sends a
config-5-style stream through me_cluster_submit / collect and, after each collected slice, replays what
me_cluster_quotes hands out into a table of quotes: it must equal the tops of ONE oracle book holding every
global symbol. The other ranks serve.

env: RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT; argv: KIND OUT_JSON
  oracle: oracle shards with an oracle-backed feed (me_shard_ops.quotes), TCP transport
  rccl:   a HIP engine shard over RCCL, world size 1
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    kind, out_path = sys.argv[1], sys.argv[2]
    import matching_engine_amd as me
    from matching_engine_amd.cluster import Cluster, ShardOps, shard_symbols
    from oracle.oracle import OracleBook
    from tests import quote_model as qm
    from tests.cluster_worker import OracleShard

    class FeedShard(OracleShard):
        def __init__(self, ids):
            super().__init__(ids)
            self.feed = qm.OracleFeed(self.ob, len(self.ids))

        def match(self, b):
            out = super().match(b)
            self.feed.matched()
            return out

        def quotes(self, cap):
            return self.feed.quotes(cap)

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    S, L, MB = 40, 128, 2048
    sc = me.preset(5, num_symbols=S, levels=L, batch=600, cancel_pct=30, market_pct=15, market_qty_mult=4, far_pct=3)
    st = me.Stream(sc)
    base = st.base_prices()
    ops = ShardOps(FeedShard(shard_symbols(S, world, rank)), 1 << 16) if kind == "oracle" else None
    cl = Cluster(rank, world, S, MB, transport="rccl" if kind == "rccl" else "tcp",
                 port=int(os.environ["MASTER_PORT"]), device=0, levels=L, base_prices=base, max_resting=1 << 16,
                 shard_ops=ops, timeout_ms=120000)
    if rank != 0:
        cl.serve()
        cl.close()
        return
    ok, msg, nev = True, "", 0
    ref = OracleBook(S)
    table = qm.tops(qm._Empty(), S)
    cl.quotes_enable(4 * S)
    batches = [st.next(sc.batch) for _ in range(6)]
    if len(cl.quotes_drain()):
        ok, msg = False, "events on empty books"
    pend = []
    for k, b in enumerate(batches):
        pend.append((cl.submit(b), k))
        if len(pend) == 2 or k == len(batches) - 1:
            while pend:
                t, j = pend.pop(0)
                cl.collect(t, len(batches[j]))
                ref.submit(batches[j])
                if pend:
                    continue  # (a later slice is applied already: compare once the books agree)
                ev = cl.quotes_drain()
                nev += len(ev)
                qm.replay(table, ev)
                if ok and not qm.same_quotes(table, qm.tops(ref, S)):
                    ok, msg = False, f"after slice {j}: the replayed quotes differ from one book's tops"
                if ok and len(ev) and int(ev["symbol"].max()) >= S:
                    ok, msg = False, "an event carries a symbol id outside the global ids"
    cl.quotes_enable(0)
    cl.stop()
    cl.close()
    json.dump({"ok": ok, "msg": msg, "events": nev}, open(out_path, "w"))


if __name__ == "__main__":
    main()
