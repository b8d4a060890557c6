#!/usr/bin/env python3
"""Cost of me_mass_cancel over every symbol of a shard beside the only route there was before it.

A config-3-shaped shard (12,500 symbols of 128 levels, one eighth of config 3's 100,000), its books loaded by
--batches device batches of config 3's stream. Two engines are built from the same batches, so both routes
start from the same books, on the same library:

    purge   Engine.mass_cancel(every symbol): the count launch, one copy of the counts, the remove launch, one
            copy of the removed orders (`purge_empty_ms`: the same call again on the emptied books — the count
            launch alone);
    old     Engine.dump(s) for every symbol (`dump_ms`), one CANCEL record per dumped order in batches of
            --batch records, each repeating the stream's last seq (`build_ms`: the arrays; `upload_ms`: their
            H2D copies), me_submit_batch_device of each and a sync (`match_ms`).

Wall time around the calls, the engine idle before them. Both engines must end empty and the purge must have
returned exactly the orders the dumps listed, in the same order.

    python tools/mass_cancel_probe.py [--symbols 12500] [--batches 4] [--batch 131072] [--reps 3] [--out FILE]
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


def _loaded(sc, base, batches, group):
    eng = me.Engine(sc.num_symbols, sc.levels, base, max_batch=sc.batch, max_resting=len(batches) * sc.batch + 65536,
                    seq_ring=1 << 26, batches_per_launch=group)
    dbs = [eng.upload(b) for b in batches]
    for db in dbs:
        eng.submit_device(db)
    eng.sync()
    for db in dbs:
        db.free()
    return eng


def one_rep(sc, base, batches, group, last_seq):
    S = sc.num_symbols
    out = {}
    everything = np.arange(S, dtype=np.uint32)
    # ---- the purge
    with _loaded(sc, base, batches, group) as eng:
        resting = eng.resting_count()
        eng.sync()
        t0 = time.perf_counter()
        ent, counts = eng.mass_cancel(everything)
        out["purge_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        e2, _ = eng.mass_cancel(everything)
        out["purge_empty_ms"] = 1e3 * (time.perf_counter() - t0)
        assert len(ent) == resting == int(counts.sum()) and len(e2) == 0 and eng.resting_count() == 0
    # ---- the route without it
    with _loaded(sc, base, batches, group) as eng:
        assert eng.resting_count() == resting
        eng.sync()
        t0 = time.perf_counter()
        dumps = [eng.dump(s) for s in range(S)]
        out["dump_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        d = np.concatenate(dumps)
        sym = np.repeat(everything, [len(x) for x in dumps])
        n = len(d)
        cx = me.Batch(np.full(n, last_seq, dtype=np.uint64), d["seq"].astype(np.int64), np.zeros(n, dtype=np.int32), sym,
                      np.full(n, me.kind(me.SIDE_BUY, op=me.OP_CANCEL), dtype=np.uint8))
        parts = [cx.take(slice(i, i + sc.batch)) for i in range(0, n, sc.batch)]
        out["build_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        dbs = [eng.upload(p) for p in parts]
        out["upload_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        for db in dbs:
            eng.submit_device(db)
        eng.sync()
        out["match_ms"] = 1e3 * (time.perf_counter() - t0)
        for db in dbs:
            db.free()
        assert eng.resting_count() == 0
        assert np.array_equal(d, ent), "the purge returned other orders than the dumps listed"
    out["old_ms"] = out["dump_ms"] + out["build_ms"] + out["upload_ms"] + out["match_ms"]
    out["resting"] = resting
    out["cancel_batches"] = len(parts)
    out["occupied_sides"] = int((counts > 0).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=12_500)
    ap.add_argument("--batches", type=int, default=4, help="device batches that load the books")
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    args = ap.parse_args()
    sc = me.preset(3, num_symbols=args.symbols, batch=args.batch)
    st = me.Stream(sc)
    base = st.base_prices()
    batches = [st.next(sc.batch) for _ in range(args.batches)]
    last_seq = int(batches[-1].seq.max())
    reps = [one_rep(sc, base, batches, min(args.batches, 32), last_seq) for _ in range(args.reps)]
    res = {"symbols": sc.num_symbols, "levels": sc.levels, "load_batches": args.batches, "batch": sc.batch,
           "resting": reps[0]["resting"], "occupied_sides": reps[0]["occupied_sides"],
           "cancel_batches": reps[0]["cancel_batches"], "reps": args.reps}
    for k in ("purge_ms", "purge_empty_ms", "dump_ms", "build_ms", "upload_ms", "match_ms", "old_ms"):
        v = [round(r[k], 3) for r in reps]
        res[k] = {"median": round(statistics.median(v), 3), "min": min(v), "runs": v}
    res["old_over_purge"] = round(res["old_ms"]["median"] / res["purge_ms"]["median"], 1)
    res["build"] = me.load().me_build_info().decode()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
