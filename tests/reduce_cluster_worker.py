"""One rank of the REDUCE cluster check (launched by tests/test_reduce_service.py): two ranks, each with its
own HIP engine on the box's GPU, the protocol over TCP. Rank 0 sends a seeded stream with reduces (records
are routed by symbol; a REDUCE is not counted as a record that may rest) through me_cluster_submit / collect
(two slices in flight) and compares every slice's merged results and tape, then every symbol's book, with
the model (tests/reduce_model.py) holding all symbols; rank 1 serves.

env: RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT; argv: OUT_JSON
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_path = sys.argv[1]
    import matching_engine_amd as me
    from matching_engine_amd.cluster import Cluster
    from tests import reduce_model as rm

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    S, L, N = 16, 128, 1500
    base, arrays = rm.reduce_stream(78, S, L, 4, N, far_pct=2, drift=3)
    cl = Cluster(rank, world, S, 2048, transport="tcp", port=int(os.environ["MASTER_PORT"]), device=0, levels=L,
                 base_prices=base, max_resting=1 << 15, timeout_ms=120000)
    if rank != 0:
        cl.serve()
        cl.close()
        return
    tb = rm.ReduceBook(S)
    ok, msg, nfills = True, "", 0
    batches = [me.Batch(a.seq, a.price_q4, a.qty, a.symbol, a.kind) for a in arrays]
    pend = []
    for k, b in enumerate(batches):
        pend.append((cl.submit(b), k))
        if len(pend) == 2 or k == len(batches) - 1:
            while pend:
                t, j = pend.pop(0)
                res, tape = cl.collect(t, len(batches[j]))
                ro, fo = tb.submit(arrays[j])
                nfills += len(fo)
                if ok and not (len(tape) == len(fo) and np.array_equal(tape, fo)):
                    ok, msg = False, f"slice {j}: tape differs ({len(tape)} vs {len(fo)})"
                for x in ("filled_qty", "remaining_qty", "fill_count", "tape_offset", "status", "reason"):
                    if ok and not np.array_equal(res[x], ro[x]):
                        i = int(np.nonzero(res[x] != ro[x])[0][0])
                        ok, msg = False, f"slice {j}: results.{x} differs at {i}: {res[i]} vs {ro[i]} kind {arrays[j].kind[i]}"
    for s in range(S):
        bids, asks, _, _ = cl.book_orders(s, 0)
        got = [(int(o["seq"]), int(o["price_q4"]), int(o["qty"])) for o in list(bids) + list(asks)]
        exp = [(int(o["seq"]), int(o["price_q4"]), int(o["qty"])) for o in tb.dump(s)]
        if ok and got != exp:
            ok, msg = False, f"book of symbol {s} differs"
    cl.stop()
    cl.close()
    nred = sum(int(rm.is_reduce(a.kind).sum()) for a in arrays)
    json.dump({"ok": ok, "msg": msg, "records": sum(len(b) for b in batches), "fills": nfills, "reduces": nred},
              open(out_path, "w"))


if __name__ == "__main__":
    main()
