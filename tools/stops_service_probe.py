#!/usr/bin/env python3
"""Cost of stop orders on the service path: bench.py's C1 service leg (c1_paths' build_submitorder_batched — one
million SubmitOrders on 'SYM' through the background flusher, the GPU and one SQLite transaction per slice; the
clock stops when every order is matched and committed) with stop orders never enabled and with a handful armed.

    off      me_service_stops_enable never called: the service launches and persists what it always did
    armed    enabled (cap_stops 64) with --stops stops armed before the clock starts, BUY and SELL alternating at
             prices no fill of the stream reaches: the stops job runs behind every launch, the service reads the
             event ring after every collected slice, nothing triggers

Each round runs both legs on fresh engines and databases (order reversed every round). Prints one JSON line per
leg and round, then one with the medians and the build digest.

    python tools/stops_service_probe.py [--rounds 3] [--stops 8] [--only off|armed]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (c1_requests: the stream bench.py times)
import matching_engine_amd as me  # noqa: E402
from matching_engine_amd._abi import MeOrderRequest, MeOrderResponse  # noqa: E402

N = 1_000_000
I64_MAX = 2 ** 63 - 1


def leg(name, stream, n_stops, tmp, tag):
    otype, side, price, scale, qty, _, base = stream
    reqs = (MeOrderRequest * N)()
    a = np.frombuffer(reqs, dtype=np.dtype([("client", "<u8"), ("symbol", "<u8"), ("otype", "<i4"), ("side", "<i4"),
                                            ("price", "<i8"), ("scale", "<i4"), ("qty", "<i4")]))
    cs, ss = C.create_string_buffer(b"C1"), C.create_string_buffer(b"SYM")
    a["client"], a["symbol"] = C.addressof(cs), C.addressof(ss)
    a["otype"], a["side"], a["price"], a["scale"], a["qty"] = otype, side, price, scale, qty
    resps = (MeOrderResponse * N)()
    lib = me.load()
    eng = me.Engine(1, 128, base, max_batch=65536, max_resting=N + 1024, seq_ring=1 << 22)
    svc = me.MatchingEngineService(eng, ["SYM"], db_path=os.path.join(tmp, f"{tag}.db"))
    try:
        if name == "armed":
            svc.stops_enable(64)
            for k in range(n_stops):  # no fill reaches them: BUY far above, SELL far below
                buy = k % 2 == 0
                r = svc.submit_stop("C1", "SYM", 1, 1 if buy else 2, 0, (I64_MAX - k) if buy else -(I64_MAX - k), 4, 1)
                assert r["success"], r
            svc.flush(outputs=False)  # the boundary is applied: ARMED before the clock starts
            assert len(svc.stop_updates()) == n_stops
        svc.start(interval_us=1000, slice_orders=65536)
        t = time.perf_counter()
        step = 65536
        for i in range(0, N, step):
            lib.me_service_submit_orders(
                svc.h, C.cast(C.addressof(reqs) + i * C.sizeof(MeOrderRequest), C.POINTER(MeOrderRequest)),
                min(step, N - i), C.cast(C.addressof(resps) + i * C.sizeof(MeOrderResponse), C.POINTER(MeOrderResponse)))
        while svc.pending or svc.unpersisted:
            time.sleep(0.0005)
        dt = time.perf_counter() - t
        svc.stop()
        out = {"leg": name, "orders_per_s": N / dt, "seconds": dt, "error": svc.last_error()}
        if name == "armed":
            out["stops"] = svc.stop_stats()
            out["stop_jobs"] = eng.stops_stats()
        return out
    finally:
        svc.close()
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stops", type=int, default=8)
    ap.add_argument("--only", choices=["off", "armed"], default=None)
    args = ap.parse_args()
    stream = bench.c1_requests(N)
    legs = [args.only] if args.only else ["off", "armed"]
    got = {k: [] for k in legs}
    tmp = tempfile.mkdtemp(prefix="me_stops_service_")
    for r in range(args.rounds):
        for name in (legs if r % 2 == 0 else legs[::-1]):
            out = leg(name, stream, args.stops, tmp, f"{name}{r}")
            out["round"] = r
            got[name].append(out["orders_per_s"])
            print(json.dumps(out), flush=True)
    print(json.dumps({"median_orders_per_s": {k: statistics.median(v) for k, v in got.items()},
                      "min_max": {k: [min(v), max(v)] for k, v in got.items()},
                      "build": me.load().me_build_info().decode()}), flush=True)


if __name__ == "__main__":
    main()
