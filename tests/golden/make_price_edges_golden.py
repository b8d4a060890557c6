"""Regenerate tests/golden/price_edges.npz: one draw of tests/price_edges.py's edge_stream (windows at the ends of
int64 and across 0, +-2^31 and 2^32; alias and extreme prices; jumps; REDUCEs) together with the model's per-batch
results and tapes and its final books, in the layout of match_tif.npz. The CPU suite replays it through the
model, the GPU suite through the engine.

usage: python tests/golden/make_price_edges_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.price_edges import edge_stream  # noqa: E402
from tests.reduce_model import ReduceBook  # noqa: E402

S, L, NB, N, SEED = 8, 128, 4, 600, 15


def records():
    return edge_stream(SEED, S, L, NB, N)


def main():
    base, batches = records()
    rb = ReduceBook(S)
    out = {"base": base, "levels": np.array([L]), "num_symbols": np.array([S]), "nbatches": np.array([NB])}
    for k, b in enumerate(batches):
        res, fills = rb.submit(b)
        for f in ("seq", "price_q4", "qty", "symbol", "kind"):
            out[f"b{k}_{f}"] = getattr(b, f)
        out[f"b{k}_res"] = res.view(np.uint8).reshape(len(res), 20)
        out[f"b{k}_fills"] = fills.view(np.uint8).reshape(len(fills), 32)
    dumps = [rb.dump(s) for s in range(S)]
    out["book_counts"] = np.array([len(d) for d in dumps], dtype=np.int64)
    out["book"] = np.concatenate(dumps).view(np.uint8).reshape(-1, 24)
    path = os.path.join(HERE, "price_edges.npz")
    np.savez_compressed(path, **out)
    print(f"price_edges.npz: {NB * N} records, {sum(len(out[f'b{k}_fills']) for k in range(NB))} fills, "
          f"{int(out['book_counts'].sum())} resting, {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
