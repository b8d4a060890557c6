#!/usr/bin/env python3
"""Cost of the trade feed (me_trades_*) at bench.py's plain-run shapes, one GPU.

Each round runs the same seeded stream on fresh engines, once per leg (the order of the legs reversed every
round): device-resident batches, `--warmup` untimed, `--steps` timed from the first submit to the end of
me_sync, exactly bench.py's timed region. The legs are

    off    the feed never enabled
    table  the feed on, the fold as shipped: updates go through the workgroup's LDS table, a wave whose active
           lanes all hold one symbol reduces first (ME_TRADE_FOLD=3, the default)
    wave   the feed on, no table: a one-symbol wave reduces first and one lane issues the atomics to HBM,
           every other lane issues its own (ME_TRADE_FOLD=1)
    lane   the feed on, every lane issues its own atomics to HBM (ME_TRADE_FOLD=0)

A feed-on leg enables the feed after the warmup (the enabling job is outside the timed region), sizes the log
so that nothing defers and reads it after the timed region. Prints one JSON line: orders/s of every leg, the
medians, their ratios to `off`, and the feed's counters (jobs, events, events per job, deferred).

The time of the three launches of a job (k_trade_fold, k_trade_scan, k_trade_emit) comes from a kernel trace of
one feed-on leg alone:

    python tools/trades_probe.py [--workload c1|c2|c4] [--steps 320] [--warmup 32] [--rounds 3]
    rocprofv3 --kernel-trace --stats -- python tools/trades_probe.py --only table --rounds 1

c1 (one symbol: every fold atomic of a launch goes to one 64-B line) and c2 (1,024 symbols, spread) run groups
of --batches-per-launch batches per job (default 20); c4 (100,000 symbols of 32,768 levels, the 1,000 most
popular books seeded to --per-side levels a side, Zipf popularity: a hot symbol) runs one batch per job.
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
    "c1": dict(preset=1, num_symbols=1, batch=62500),
    "c2": dict(preset=2, num_symbols=1024, batch=65536),
    "c4": dict(preset=4, num_symbols=100_000, batch=65536, seeded=1000),
}
LEGS = ("off", "table", "wave", "lane")
FOLD = {"table": "3", "wave": "1", "lane": "0"}


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
            jobs = (args.steps + group - 1) // group
            os.environ["ME_TRADE_FOLD"] = FOLD[mode]  # (read by me_trades_enable)
            try:
                eng.trades_enable(min(sc.num_symbols * (jobs + 2), max(64 * sc.num_symbols, 1 << 24)))
            finally:
                del os.environ["ME_TRADE_FOLD"]
        t0 = time.perf_counter()
        for db in dbs[args.warmup:]:
            eng.submit_device(db)
        eng.sync()
        dt = time.perf_counter() - t0
        out = {"orders_per_s": args.steps * sc.batch / dt}
        if mode != "off":
            stt = eng.trades_stats()
            ev = eng.trades_drain()
            assert len(ev) == stt["events"] or stt["deferred"]
            out.update(batches_per_job=group, jobs=stt["groups"] - 1, events=stt["events"], deferred=stt["deferred"],
                       events_per_job=round(stt["events"] / max(stt["groups"] - 1, 1), 1),
                       fills=int(ev["trades"].sum()), fills_per_order=round(int(ev["trades"].sum()) / (args.steps * sc.batch), 3))
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
    feed_stats = {}
    for r in range(args.rounds):
        for mode in (LEGS if r % 2 == 0 else LEGS[::-1]):
            if args.only and mode != args.only:
                continue
            o = leg(args, mode)
            legs[mode].append(o["orders_per_s"])
            if mode != "off":
                feed_stats[mode] = {k: v for k, v in o.items() if k != "orders_per_s"}
    res = {"workload": args.workload, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "orders_per_s": {k: [round(x) for x in v] for k, v in legs.items()}, "feed": feed_stats,
           "build": me.load().me_build_info().decode()}
    for k in LEGS:
        if legs[k]:
            res[f"median_{k}"] = round(statistics.median(legs[k]))
    for k in LEGS[1:]:
        if legs[k] and legs["off"]:
            res[f"{k}_over_off"] = round(res[f"median_{k}"] / res["median_off"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
