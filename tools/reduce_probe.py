#!/usr/bin/env python3
"""What REDUCE records cost on a config-5-shaped stream (for the record).

1,024 symbols, 65,536-record device batches, launch groups of 20: config 5's stream (LIMITs, MARKETs and
cancels) with a share of its CANCEL records turned into REDUCE records of quantity 1 — a partial reduce
whenever the target still holds more than one lot, else a covering one —
    plain       none,
    reduce1     1 % of the cancels,
    reduce10    10 % of the cancels.
Every fast path hands a symbol to the continuation launch at its first REDUCE, so the cost is the hand-offs.
Each leg: fresh engine, every batch resident in HBM, WARM untimed groups, then the timed groups between two
device syncs. Prints one JSON object and writes it to --out: orders/s, reduces, hand-offs (total and per
group) and the paths that were on at the end (the grouped path's hand-off policy may have switched it off,
me_engine.cpp).

    python tools/reduce_probe.py [--groups 6] [--warm 2] [--out profiles/reduce/probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import matching_engine_amd as me  # noqa: E402

S, BATCH, GROUP = 1024, 65536, 20


def leg(name, share, groups, warm):
    sc = me.preset(5, num_symbols=S, batch=BATCH)
    st = me.Stream(sc)
    base = st.base_prices()
    rng = np.random.default_rng(11)
    nb = (groups + warm) * GROUP
    total = nb * BATCH
    ncx = nred = 0
    with me.Engine(S, sc.levels, base, max_batch=BATCH, max_resting=total + (1 << 20), seq_ring=1 << 28,
                   batches_per_launch=GROUP) as eng:
        dbs = []
        for k in range(nb):
            b = st.next(BATCH)
            cx = (b.kind & 0x08) != 0
            red = cx & (rng.random(BATCH) < share)
            b.kind = np.where(red, me.KIND_REDUCE, b.kind).astype(np.uint8)
            b.qty = np.where(red, 1, b.qty).astype(np.int32)
            if k >= warm * GROUP:
                ncx += int(cx.sum())
                nred += int(red.sum())
            dbs.append(eng.upload(b))
        for db in dbs[: warm * GROUP]:
            eng.submit_device(db)
        eng.sync()
        h0 = eng.stats()["handoffs"]
        t0 = time.perf_counter()
        for db in dbs[warm * GROUP:]:
            eng.submit_device(db)
        eng.sync()
        dt = time.perf_counter() - t0
        h = eng.stats()["handoffs"] - h0
        out = {"leg": name, "share_of_cancels": share, "orders": groups * GROUP * BATCH, "cancel_records": ncx,
               "reduces": nred, "orders_per_s": groups * GROUP * BATCH / dt, "handoffs": h,
               "handoffs_per_group": h / groups, "handoffs_warm": h0, "paths": eng.paths(),
               "resting": eng.resting_count()}
        for db in dbs:
            db.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=6)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"shape": {"symbols": S, "batch": BATCH, "group": GROUP, "groups": a.groups, "warm": a.warm, "config": 5},
           "build": me._abi.load().me_build_info().decode(),
           "legs": [leg("plain", 0.0, a.groups, a.warm), leg("reduce1", 0.01, a.groups, a.warm),
                    leg("reduce10", 0.10, a.groups, a.warm)]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
