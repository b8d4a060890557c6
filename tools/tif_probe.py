#!/usr/bin/env python3
"""What the time-in-force instructions cost on a config-2-shaped stream (for the record).

1,024 symbols, 65,536-record device batches, launch groups of 20: config 2's stream (80 % LIMIT +-32 ticks,
20 % MARKET) with the time-in-force bits set on a share of its LIMIT records —
    plain       none,
    ioc30       30 % of the records IOC (native on the fast walks),
    fokpo30     15 % FOK + 15 % POST_ONLY (they hand their symbol to the continuation launch).
Each leg: fresh engine, every batch resident in HBM, WARM untimed groups, then the timed groups between two
device syncs. Prints one JSON object and writes it to --out: orders/s, hand-offs and the paths that were on
at the end (the grouped path's hand-off policy may have switched it off, me_engine.cpp).

    python tools/tif_probe.py [--groups 6] [--warm 2] [--out profiles/tif/probe.json]
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


def leg(name, ioc, fok, po, groups, warm):
    sc = me.preset(2, num_symbols=S, batch=BATCH)
    st = me.Stream(sc)
    base = st.base_prices()
    rng = np.random.default_rng(11)
    nb = (groups + warm) * GROUP
    total = nb * BATCH
    with me.Engine(S, sc.levels, base, max_batch=BATCH, max_resting=total + (1 << 20), seq_ring=1 << 28,
                   batches_per_launch=GROUP) as eng:
        dbs = []
        for _ in range(nb):
            b = st.next(BATCH)
            u = rng.random(BATCH)
            limit = (b.kind & 0x0C) == 0
            tif = np.where(u < ioc, me.TIF_IOC, np.where(u < ioc + fok, me.TIF_FOK,
                                                         np.where(u < ioc + fok + po, me.TIF_POST_ONLY, 0)))
            b.kind = (b.kind | np.where(limit, tif << 4, 0)).astype(np.uint8)
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
        out = {"leg": name, "ioc": ioc, "fok": fok, "post_only": po, "orders": groups * GROUP * BATCH,
               "orders_per_s": groups * GROUP * BATCH / dt, "handoffs": eng.stats()["handoffs"] - h0,
               "handoffs_warm": h0, "paths": eng.paths(), "resting": eng.resting_count()}
        for db in dbs:
            db.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=6)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"shape": {"symbols": S, "batch": BATCH, "group": GROUP, "groups": a.groups, "warm": a.warm},
           "build": me._abi.load().me_build_info().decode(),
           "legs": [leg("plain", 0.0, 0.0, 0.0, a.groups, a.warm), leg("ioc30", 0.30, 0.0, 0.0, a.groups, a.warm),
                    leg("fokpo30", 0.0, 0.15, 0.15, a.groups, a.warm)]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
