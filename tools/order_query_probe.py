#!/usr/bin/env python3
"""Cost of me_order_query beside the only route there was before it, me_book_dump of the orders' symbols.

On bench.py's config 2 shape (1,024 symbols of 128 levels, the resting books a few launch groups leave) and
on config 4's deep window (100,000 symbols of 32,768 levels, the most popular books seeded to --per-side
levels a side), one GPU. The books are built, the live seqs are collected by dumping the books (all of them on
c2, the seeded ones on c4), and for n = 1, 1,024 and 65,536 random live seqs (drawn with replacement) the
probe times

    query   Engine.order_query(seqs): one launch, one copy each way (`query_repeat_ms`: the same call again at
            once, same seqs);
    dump    Engine.dump(s) for every distinct symbol among those orders, the host search not included.

Wall time around the call, the engine idle before it; `--reps` repetitions with fresh random seqs each, the
median and the minimum reported. `longest_queue` is the largest orders_ahead + 1 any answer held: that order's
walk went through at least ceil(longest_queue / 16) chunks, one dependent HBM round trip each.

    python tools/order_query_probe.py [--workload c2|c4] [--groups 3] [--reps 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import matching_engine_amd as me  # noqa: E402

SHAPES = {
    "c2": dict(preset=2, num_symbols=1024, batch=65536, group=20),
    "c4": dict(preset=4, num_symbols=100_000, batch=65536, group=1, seeded=1000),
}
COUNTS = (1, 1024, 65536)


def probe(args):
    w = SHAPES[args.workload]
    sc = me.preset(w["preset"], num_symbols=w["num_symbols"], batch=w["batch"])
    st = me.Stream(sc)
    base = st.base_prices()
    seeds = []
    if w.get("seeded") and args.per_side:
        sb = st.seed_books(range(w["seeded"]), args.per_side)
        seeds = [sb.take(slice(i, i + (1 << 20))) for i in range(0, len(sb), 1 << 20)]
    group = w["group"]
    nb = args.groups * group
    batches = [st.next(sc.batch) for _ in range(nb)]
    n_seed = sum(len(b) for b in seeds)
    grouped = sc.levels <= 128
    rng = np.random.default_rng(args.seed)
    with me.Engine(sc.num_symbols, sc.levels, base, max_batch=max([sc.batch] + [len(b) for b in seeds]) + 1,
                   max_resting=nb * sc.batch + n_seed + 65536, seq_ring=1 << 28,
                   batches_per_launch=group if grouped else 0) as eng:
        for b in seeds:
            eng.submit_batch(b, want_fills=False)
        dbs = [eng.upload(b) for b in batches]
        for db in dbs:
            eng.submit_device(db)
        eng.sync()
        for db in dbs:
            db.free()
        # the live seqs and their symbols, from the books themselves
        scan = range(w.get("seeded", sc.num_symbols))
        seqs, syms = [], []
        for s in scan:
            d = eng.dump(s)
            seqs.append(d["seq"])
            syms.append(np.full(len(d), s, dtype=np.uint32))
        seqs, syms = np.concatenate(seqs), np.concatenate(syms)
        assert len(seqs), "no resting order to ask about"
        out = {"workload": args.workload, "symbols": sc.num_symbols, "levels": sc.levels, "groups": args.groups,
               "batches": nb, "seed_orders": n_seed, "resting_total": eng.resting_count(),
               "live_seqs_scanned": int(len(seqs)), "symbols_scanned": len(scan), "reps": args.reps, "n": {}}
        longest = 0
        eng.order_query(seqs[:1])  # (the first call allocates the device buffers)
        for n in COUNTS:
            tq, tr, td, nsym = [], [], [], []
            for _ in range(args.reps):
                pick = rng.integers(0, len(seqs), n)
                q = np.ascontiguousarray(seqs[pick])
                eng.sync()
                t0 = time.perf_counter()
                ans = eng.order_query(q)
                tq.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                eng.order_query(q)  # the same seqs again, at once
                tr.append(time.perf_counter() - t0)
                assert int(ans["found"].sum()) == n and np.array_equal(ans["symbol"], syms[pick])
                longest = max(longest, int(ans["orders_ahead"].max()) + 1)
                distinct = np.unique(syms[pick])
                nsym.append(len(distinct))
                t0 = time.perf_counter()
                for s in distinct:
                    eng.dump(int(s))
                td.append(time.perf_counter() - t0)
            out["n"][str(n)] = {
                "query_ms_median": round(1e3 * statistics.median(tq), 4), "query_ms_min": round(1e3 * min(tq), 4),
                "dump_ms_median": round(1e3 * statistics.median(td), 4), "dump_ms_min": round(1e3 * min(td), 4),
                "dump_symbols_median": int(statistics.median(nsym)),
                "query_ms": [round(1e3 * t, 4) for t in tq], "dump_ms": [round(1e3 * t, 4) for t in td],
                "query_repeat_ms": [round(1e3 * t, 4) for t in tr],  # (all three in run order)
            }
        out["longest_queue"] = longest
        out["longest_queue_chunks_at_least"] = (longest + 15) // 16
    out["build"] = me.load().me_build_info().decode()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=sorted(SHAPES))
    ap.add_argument("--groups", type=int, default=3, help="launch groups matched before the probe (c4: batches)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--per-side", type=int, default=10_000, help="c4: levels a side of the seeded books (0: none)")
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    args = ap.parse_args()
    res = probe(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
