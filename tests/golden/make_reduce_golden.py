"""Regenerate tests/golden/match_reduce.npz: a seeded stream of tests/reduce_model.py (the time-in-force mix
of tests/tif_model.py with most of its cancels turned into REDUCE records, fresh reduces of resting orders,
a few far prices, drifting mids and bad records; half of the records on symbol 0) together with the model's
per-batch results and tapes and its final books, in the layout of match_c*.npz. The CPU suite replays it
through the model, the GPU suite through the engine.

usage: python tests/golden/make_reduce_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.reduce_model import ReduceBook, is_reduce, reduce_stream  # noqa: E402

S, L, NB, N = 12, 128, 4, 1000


def main():
    base, batches = reduce_stream(20261020, S, L, NB, N, far_pct=2, drift=3, skew=True)
    rb = ReduceBook(S)
    out = {"base": base, "levels": np.array([L]), "num_symbols": np.array([S]), "nbatches": np.array([NB])}
    nred = 0
    for k, b in enumerate(batches):
        res, fills = rb.submit(b)
        nred += int(is_reduce(b.kind).sum())
        for f in ("seq", "price_q4", "qty", "symbol", "kind"):
            out[f"b{k}_{f}"] = getattr(b, f)
        out[f"b{k}_res"] = res.view(np.uint8).reshape(len(res), 20)
        out[f"b{k}_fills"] = fills.view(np.uint8).reshape(len(fills), 32)
    dumps = [rb.dump(s) for s in range(S)]
    out["book_counts"] = np.array([len(d) for d in dumps], dtype=np.int64)
    out["book"] = np.concatenate(dumps).view(np.uint8).reshape(-1, 24)
    path = os.path.join(HERE, "match_reduce.npz")
    np.savez_compressed(path, **out)
    print(f"match_reduce.npz: {NB * N} records, {nred} reduces, "
          f"{sum(len(out[f'b{k}_fills']) for k in range(NB))} fills, {int(out['book_counts'].sum())} resting, "
          f"{os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
