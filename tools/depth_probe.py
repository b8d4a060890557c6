#!/usr/bin/env python3
"""Cost of the depth feed (me_depth_*) at bench.py's plain-run shapes, one GPU.

Each round runs the same seeded stream twice on fresh engines, feed off then feed on (order swapped
every round): device-resident batches, `--warmup` untimed, `--steps` timed from the first submit to the
end of me_sync, exactly bench.py's timed region. The feed-on leg enables the feed after the warmup
(so the enabling job is outside the timed region), sizes the log so that nothing defers and reads it
after the timed region. Prints one JSON line: orders/s of every leg, the medians, their ratio, and the
feed's counters (jobs, events, events per job, deferred).

The time of the three launches of a job (k_depth_scan, k_depth_offsets, k_depth_emit) comes from a kernel
trace of the feed-on leg alone:

    python tools/depth_probe.py [--workload c2|c3|c4] [--depth 10] [--steps 640] [--warmup 32] [--rounds 3]
    rocprofv3 --kernel-trace --stats -- python tools/depth_probe.py --only on --rounds 1

c2 and c3 run groups of --batches-per-launch batches per job (default 20); c4 (100,000 symbols of 32,768
levels, the 1,000 most popular books seeded to --per-side levels a side) runs one batch per job.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import matching_engine_amd as me  # noqa: E402

SHAPES = {
    "c2": dict(preset=2, num_symbols=1024, batch=65536),
    "c3": dict(preset=3, num_symbols=12500, batch=131072),
    "c4": dict(preset=4, num_symbols=100_000, batch=65536, seeded=1000),
}


def leg(args, feed: bool):
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
        if feed:
            jobs = (args.steps + group - 1) // group
            eng.depth_enable(args.depth, min(4 * args.depth * sc.num_symbols * (jobs + 2), 1 << 26))
            n0 = len(eng.depth_drain())
        t0 = time.perf_counter()
        for db in dbs[args.warmup:]:
            eng.submit_device(db)
        eng.sync()
        dt = time.perf_counter() - t0
        out = {"orders_per_s": args.steps * sc.batch / dt}
        if feed:
            stt = eng.depth_stats()
            ev = stt["events"] - n0  # (the enabling job's events were read before the timed region)
            assert len(eng.depth_drain()) == ev or stt["deferred"]
            out.update(depth=args.depth, batches_per_job=group, jobs=stt["groups"] - 1, enable_events=n0, events=ev,
                       deferred=stt["deferred"], events_per_job=round(ev / max(stt["groups"] - 1, 1), 1))
        for db in dbs:
            db.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=sorted(SHAPES))
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--steps", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches-per-launch", type=int, default=0)
    ap.add_argument("--per-side", type=int, default=10_000, help="c4: levels a side of the seeded books (0: none)")
    ap.add_argument("--only", choices=["off", "on"], default=None)
    args = ap.parse_args()
    legs = {"off": [], "on": []}
    feed_stats = None
    for r in range(args.rounds):
        order = ("off", "on") if r % 2 == 0 else ("on", "off")
        for mode in order:
            if args.only and mode != args.only:
                continue
            o = leg(args, mode == "on")
            legs[mode].append(o["orders_per_s"])
            if mode == "on":
                feed_stats = {k: v for k, v in o.items() if k != "orders_per_s"}
    res = {"workload": args.workload, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "orders_per_s": {k: [round(x) for x in v] for k, v in legs.items()}, "feed": feed_stats,
           "build": me.load().me_build_info().decode()}
    if legs["off"] and legs["on"]:
        res["median_off"] = round(statistics.median(legs["off"]))
        res["median_on"] = round(statistics.median(legs["on"]))
        res["on_over_off"] = round(res["median_on"] / res["median_off"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
