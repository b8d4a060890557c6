#!/usr/bin/env python3
"""Cost of me_order_preview beside the only route there was before it: me_book_orders of the queried symbols,
walked on the host.

Two books, one GPU:

    c2     bench.py's config 2 shape (1,024 symbols of 128 levels), the resting books a few launch groups leave;
    level  64 symbols of 128 levels; symbol 0 holds ONE bid level of --level-orders orders (10,000: 625 chunks),
           the others one order a side. Every query is a SELL against symbol 0, from one lot to the whole level,
           so a query's fill_count walk runs through up to every chunk of the level.

For n = 1, 1,024 and 65,536 random queries (symbols with replacement; BUY and SELL; MARKET, IOC and FOK LIMITs
within a few ticks of the best opposite price; quantities from one lot to a few levels) the probe times

    preview  Engine.order_preview(...): one copy in, one launch, one copy out (`preview_repeat_ms`: the same
             call again at once);
    host     one me_book_orders call per DISTINCT symbol among the queries (the whole book, into a buffer
             allocated before the clock starts), then the walk on the host: a cumulative sum per side and, per
             query, two binary searches (numpy). The walk restates only what the probe compares: filled_qty and
             fill_count; both must equal the device's.

Wall time around the calls, the engine idle before them; `--reps` repetitions with fresh random queries each,
the median and the minimum reported.

    python tools/preview_probe.py [--workload c2|level] [--groups 3] [--reps 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import matching_engine_amd as me  # noqa: E402
from matching_engine_amd._abi import BOOK_ENTRY_DTYPE, ptr  # noqa: E402

COUNTS = (1, 1024, 65536)
BUY, SELL = 1, 2
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def build_c2(args):
    sc = me.preset(2, num_symbols=1024, batch=65536)
    st = me.Stream(sc)
    group = 20
    batches = [st.next(sc.batch) for _ in range(args.groups * group)]
    eng = me.Engine(sc.num_symbols, sc.levels, st.base_prices(), max_batch=sc.batch + 1,
                    max_resting=len(batches) * sc.batch + 65536, seq_ring=1 << 28, batches_per_launch=group)
    dbs = [eng.upload(b) for b in batches]
    for db in dbs:
        eng.submit_device(db)
    eng.sync()
    for db in dbs:
        db.free()
    return eng, np.arange(sc.num_symbols, dtype=np.uint32), {"symbols": sc.num_symbols, "levels": sc.levels,
                                                             "batches": len(batches)}


def build_level(args):
    S, L, n = 64, 128, args.level_orders
    base = np.array([1_000_000 + 1_000 * s for s in range(S)], dtype=np.int64)
    seq = np.arange(1, n + 2 * S, dtype=np.uint64)
    px = np.concatenate([np.full(n, base[0] + 60), np.repeat(base[1:] + 60, 2) + np.tile([0, 4], S - 1), [base[0] + 70]])
    qty = np.concatenate([np.full(n, 10), np.full(2 * S - 1, 5)]).astype(np.int32)
    sym = np.concatenate([np.zeros(n), np.repeat(np.arange(1, S), 2), [0]]).astype(np.uint32)
    side = np.concatenate([np.full(n, BUY), np.tile([BUY, SELL], S - 1), [SELL]])
    kind = np.array([me.kind(int(x)) for x in side], dtype=np.uint8)
    eng = me.Engine(S, L, base, max_batch=len(seq), max_resting=len(seq) + 1024)
    eng.submit_batch(me.Batch(seq, px, qty, sym, kind), want_fills=False)
    return eng, np.zeros(1, dtype=np.uint32), {"symbols": S, "levels": L, "level_orders": n}


def fetch_book(eng, s, bids, asks):
    """ONE me_book_orders call: the whole book of symbol s into the two buffers."""
    nb, na = C.c_size_t(0), C.c_size_t(0)
    rc = eng.lib.me_book_orders(eng.h, int(s), 0xFFFFFFFF, ptr(bids), len(bids), C.byref(nb), ptr(asks), len(asks),
                                C.byref(na), None, None, None, None)
    assert rc == 0 and nb.value <= len(bids) and na.value <= len(asks), (rc, nb.value, na.value)
    return bids[: nb.value], asks[: na.value]


def host_walk(book, side, market, px, qty):
    """(filled_qty, fill_count) of a taker against `book` = (bids, asks), each in priority order."""
    opp = book[1] if side == BUY else book[0]
    if not len(opp):
        return 0, 0
    p = opp["price_q4"]
    k = len(p) if market else int(np.searchsorted(p, px, "right") if side == BUY else np.searchsorted(-p, -px, "right"))
    if not k:
        return 0, 0
    cum = np.cumsum(opp["qty"][:k].astype(np.int64))
    filled = min(int(qty), int(cum[-1]))
    return filled, int(np.searchsorted(cum, filled, "left")) + 1


def queries(rng, pool, n, args):
    sym = pool[rng.integers(0, len(pool), n)].astype(np.uint32)
    if args.workload == "level":
        total = 10 * args.level_orders
        side = np.full(n, SELL)
        qty = rng.integers(1, total + 1, n).astype(np.int32)
        tif = rng.integers(0, 3, n)
        market = rng.random(n) < 0.5
        px = np.full(n, 1_000_000 + 60 - 2, dtype=np.int64)
    else:
        side = rng.integers(1, 3, n)
        qty = rng.integers(1, 400, n).astype(np.int32)
        tif = rng.integers(0, 3, n)
        market = rng.random(n) < 0.3
        px = None
    return sym, side, market, tif, px, qty


def probe(args):
    eng, pool, info = (build_c2 if args.workload == "c2" else build_level)(args)
    rng = np.random.default_rng(args.seed)
    with eng:
        out = dict({"workload": args.workload, "resting_total": eng.resting_count(), "reps": args.reps, "n": {}}, **info)
        cap = max(int(eng.resting_count()), 1)
        bids, asks = np.zeros(cap, dtype=BOOK_ENTRY_DTYPE), np.zeros(cap, dtype=BOOK_ENTRY_DTYPE)
        mids = None
        if args.workload == "c2":  # LIMITs within a few ticks of each symbol's best opposite price
            lv, cnt = eng.levels_all(1)
            mids = np.where(cnt[:, 1] > 0, lv[:, 1, 0]["price_q4"], lv[:, 0, 0]["price_q4"])
        eng.order_preview(0, me.kind(BUY, 1), 0, 1)  # (the first call allocates the device buffers)
        most = 0
        for n in COUNTS:
            tp, tr, th, tf, nsym = [], [], [], [], []
            for _ in range(args.reps):
                sym, side, market, tif, px, qty = queries(rng, pool, n, args)
                if px is None:
                    px = mids[sym] + rng.integers(-3, 4, n)
                kd = np.array([me.kind(int(s), int(m), 0, int(t)) for s, m, t in zip(side, market, tif)], dtype=np.uint8)
                eng.sync()
                t0 = time.perf_counter()
                ans = eng.order_preview(sym, kd, px, qty)
                tp.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                eng.order_preview(sym, kd, px, qty)  # the same queries again, at once
                tr.append(time.perf_counter() - t0)
                most = max(most, int(ans["fill_count"].max()))
                distinct = np.unique(sym)
                nsym.append(len(distinct))
                t0 = time.perf_counter()
                books = {}
                for s in distinct:
                    b, a = fetch_book(eng, s, bids, asks)
                    books[int(s)] = (b.copy(), a.copy())
                t1 = time.perf_counter()
                walked = [host_walk(books[int(sym[i])], int(side[i]), bool(market[i]), int(px[i]), int(qty[i])) for i in range(n)]
                th.append(time.perf_counter() - t0)
                tf.append(t1 - t0)
                # the host's answer before the FOK rule: a killed FOK fills nothing
                for i, (f, c) in enumerate(walked):
                    if int(tif[i]) == 2 and f < int(qty[i]):
                        f, c = 0, 0
                    assert (f, c) == (int(ans["filled_qty"][i]), int(ans["fill_count"][i])), (i, f, c, ans[i])
            ms = lambda t: round(1e3 * t, 4)  # noqa: E731
            out["n"][str(n)] = {
                "preview_ms_median": ms(statistics.median(tp)), "preview_ms_min": ms(min(tp)),
                "host_ms_median": ms(statistics.median(th)), "host_ms_min": ms(min(th)),
                "host_fetch_ms_median": ms(statistics.median(tf)), "host_symbols_median": int(statistics.median(nsym)),
                "preview_ms": [ms(t) for t in tp], "preview_repeat_ms": [ms(t) for t in tr], "host_ms": [ms(t) for t in th],
            }
        out["most_fills_of_a_query"] = most
        out["most_chunks_walked_at_least"] = (most + 15) // 16
    out["build"] = me.load().me_build_info().decode()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=("c2", "level"))
    ap.add_argument("--groups", type=int, default=3, help="c2: launch groups matched before the probe")
    ap.add_argument("--level-orders", type=int, default=10_000, help="level: orders on symbol 0's one bid level")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    args = ap.parse_args()
    res = probe(args)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
