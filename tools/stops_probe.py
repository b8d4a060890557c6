#!/usr/bin/env python3
"""Cost of the trigger book's job (me_stops_*) at bench.py's plain-run shapes, one GPU.

Each round runs the same seeded stream on fresh engines, once per leg (the order of the legs reversed every
round): device-resident batches, `--warmup` untimed, `--steps` timed from the first submit to the end of
me_sync, exactly bench.py's timed region. The legs are

    off      the trigger book never enabled
    s0       enabled, no stop added: the host knows that nothing is live and enqueues no job
    s1k      1,000 stops pending through the whole timed region
    s100k    100,000 stops pending

The pending stops are spread over the symbols round-robin, BUY and SELL alternating, at INT64_MAX and INT64_MIN
with one tick taken off: no fill of the stream reaches them, so the table keeps its size and every job pays the
fold, a scan of every entry and an emit that finds nothing. They are added after the warmup (outside the timed
region). Prints one JSON line: orders/s of every leg, the medians, their ratios to `off`, the jobs run and the
cost per job worked out from the medians ((time of the leg - time of `off`) / jobs).

    python tools/stops_probe.py [--workload c2|c4] [--steps 320] [--warmup 32] [--rounds 3]
    rocprofv3 --kernel-trace --stats -- python tools/stops_probe.py --only s100k --rounds 1

c2 (1,024 symbols) runs groups of --batches-per-launch batches per job (default 20); c4 (100,000 symbols of
32,768 levels, the 1,000 most popular books seeded to --per-side levels a side) runs one batch per job.
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
    "c2": dict(preset=2, num_symbols=1024, batch=65536),
    "c4": dict(preset=4, num_symbols=100_000, batch=65536, seeded=1000),
}
LEGS = ("off", "s0", "s1k", "s100k")
PENDING = {"s0": 0, "s1k": 1_000, "s100k": 100_000}
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1


def never_triggering(n: int, num_symbols: int) -> np.ndarray:
    a = np.zeros(n, dtype=me.STOP_DTYPE)
    i = np.arange(n)
    a["id"] = 1 + i
    a["symbol"] = i % num_symbols
    a["qty"] = 1
    a["kind"] = np.where(i % 2 == 0, me.kind(me.SIDE_BUY, me.TYPE_MARKET), me.kind(me.SIDE_SELL, me.TYPE_MARKET))
    a["stop_px_q4"] = np.where(i % 2 == 0, I64_MAX - 1, I64_MIN + 1)
    return a


def leg(args, mode: str):
    w = SHAPES[args.workload]
    sc = me.preset(w["preset"], num_symbols=w["num_symbols"], batch=w["batch"])
    st = me.Stream(sc)
    base = st.base_prices()
    seeds = []
    if w.get("seeded") and args.per_side:
        sb = st.seed_books(range(w["seeded"]), args.per_side)
        seeds = [sb.take(slice(i, i + (1 << 20))) for i in range(0, len(sb), 1 << 20)]
    nb = args.warmup + args.steps
    batches = [st.next(sc.batch) for _ in range(nb)]
    total = nb * sc.batch
    n_seed = sum(len(b) for b in seeds)
    grouped = sc.levels <= 128
    group = (args.batches_per_launch or 20) if grouped else 1
    with me.Engine(sc.num_symbols, sc.levels, base, max_batch=max([sc.batch] + [len(b) for b in seeds]) + 1,
                   max_resting=min(total, 42 << 20) + n_seed + 65536, seq_ring=1 << 28,
                   batches_per_launch=group if grouped else 0) as eng:
        for b in seeds:
            eng.submit_batch(b, want_fills=False)
        dbs = [eng.upload(b) for b in batches]
        for db in dbs[: args.warmup]:
            eng.submit_device(db)
        eng.sync()
        if mode != "off":
            eng.stops_enable(max(PENDING[mode], 16))
            if PENDING[mode]:
                eng.stops_add(never_triggering(PENDING[mode], sc.num_symbols))
        t0 = time.perf_counter()
        for db in dbs[args.warmup:]:
            eng.submit_device(db)
        eng.sync()
        dt = time.perf_counter() - t0
        out = {"orders_per_s": args.steps * sc.batch / dt, "seconds": dt}
        if mode != "off":
            stt = eng.stops_stats()  # (raises had a job been deferred)
            assert stt["events"] == 0 and stt["live"] == PENDING[mode], stt
            out.update(batches_per_job=group, jobs=stt["jobs"], pending=PENDING[mode])
        for db in dbs:
            db.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=sorted(SHAPES))
    ap.add_argument("--steps", type=int, default=320)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches-per-launch", type=int, default=0)
    ap.add_argument("--per-side", type=int, default=10_000, help="c4: levels a side of the seeded books (0: none)")
    ap.add_argument("--only", choices=LEGS, default=None)
    args = ap.parse_args()
    legs = {k: [] for k in LEGS}
    secs = {k: [] for k in LEGS}
    stats = {}
    for r in range(args.rounds):
        for mode in (LEGS if r % 2 == 0 else LEGS[::-1]):
            if args.only and mode != args.only:
                continue
            o = leg(args, mode)
            legs[mode].append(o["orders_per_s"])
            secs[mode].append(o["seconds"])
            if mode != "off":
                stats[mode] = {k: v for k, v in o.items() if k not in ("orders_per_s", "seconds")}
    res = {"workload": args.workload, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "orders_per_s": {k: [round(x) for x in v] for k, v in legs.items()}, "stops": stats,
           "build": me.load().me_build_info().decode()}
    for k in LEGS:
        if legs[k]:
            res[f"median_{k}"] = round(statistics.median(legs[k]))
    for k in LEGS[1:]:
        if legs[k] and legs["off"]:
            res[f"{k}_over_off"] = round(res[f"median_{k}"] / res["median_off"], 4)
            if stats[k]["jobs"]:
                d = statistics.median(secs[k]) - statistics.median(secs["off"])
                res[f"{k}_us_per_job"] = round(1e6 * d / stats[k]["jobs"], 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
