"""What a per-slice depth drain costs the cluster: bench.py's world-1 RCCL cluster leg (config 3's global slice
shape: 16 slices of 2^20 orders over 100,000 symbols, two in flight) run with the depth feed off and with
me_cluster_depth_enable(depth) plus a full me_cluster_depth drain after every collected slice, alternating.

python tools/cluster_depth_cost.py --depth 10 --reps 3 --out profiles/cluster_parity/depth_cost.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import matching_engine_amd as me  # noqa: E402
from matching_engine_amd.cluster import Cluster  # noqa: E402


def leg(depth, slices, sc, base, port):
    cl = Cluster(0, 1, len(base), sc.batch, transport="rccl", port=port, device=0, levels=sc.levels, base_prices=base,
                 max_resting=sc.batch * (len(slices) + 1), timeout_ms=120000, seq_ring=1 << 28, batches_per_launch=2)
    if depth:
        cl.depth_enable(depth, 8 * depth * len(base))
    ev = 0

    def drain():
        k = 0
        while True:
            e, left = cl.depth(1 << 20)
            k += len(e)
            if not left:
                return k

    t0 = time.perf_counter()
    pend, n = [], 0
    for b in slices:
        pend.append((cl.submit(b), len(b)))
        n += len(b)
        if len(pend) == 2:
            t, k = pend.pop(0)
            cl.collect(t, k, copy=False)
            if depth:
                ev += drain()
    for t, k in pend:
        cl.collect(t, k, copy=False)
        if depth:
            ev += drain()
    dt = time.perf_counter() - t0
    cl.stop()
    cl.close()
    return {"depth": depth, "orders_per_s": n / dt, "ms_per_slice": dt / len(slices) * 1e3, "depth_events": ev}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--port", type=int, default=29811)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    csc = me.preset(3, num_symbols=100_000, batch=1 << 20)
    cst = me.Stream(csc)
    base = cst.base_prices()
    whole = [cst.next(csc.batch) for _ in range(args.slices)]
    out = {"build": me._abi.load().me_build_info().decode(), "slices": args.slices, "slice_orders": csc.batch,
           "symbols": len(base), "runs": []}
    port = args.port
    for _ in range(args.reps):
        for depth in (0, args.depth):
            port += 1
            r = leg(depth, whole, csc, base, port)
            print(json.dumps(r), flush=True)
            out["runs"].append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
