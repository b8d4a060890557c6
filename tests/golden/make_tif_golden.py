"""Regenerate tests/golden/match_tif.npz: a seeded stream with the time-in-force mix of
tests/tif_model.py (GTC, IOC, FOK, POST_ONLY, MARKETs, cancels; a few far prices and bad records; half
of the records on symbol 0) together with the model's per-batch results and tapes and its final books,
in the layout of match_c*.npz. The CPU suite replays it through the model, the GPU suite through the
engine.

usage: python tests/golden/make_tif_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.tif_model import TifBook, tif_stream  # noqa: E402

S, L, NB, N = 12, 128, 4, 1000


def main():
    base, batches = tif_stream(20261019, S, L, NB, N, far_pct=2, skew=True)
    tb = TifBook(S)
    out = {"base": base, "levels": np.array([L]), "num_symbols": np.array([S]), "nbatches": np.array([NB])}
    for k, b in enumerate(batches):
        res, fills = tb.submit(b)
        for f in ("seq", "price_q4", "qty", "symbol", "kind"):
            out[f"b{k}_{f}"] = getattr(b, f)
        out[f"b{k}_res"] = res.view(np.uint8).reshape(len(res), 20)
        out[f"b{k}_fills"] = fills.view(np.uint8).reshape(len(fills), 32)
    dumps = [tb.dump(s) for s in range(S)]
    out["book_counts"] = np.array([len(d) for d in dumps], dtype=np.int64)
    out["book"] = np.concatenate(dumps).view(np.uint8).reshape(-1, 24)
    path = os.path.join(HERE, "match_tif.npz")
    np.savez_compressed(path, **out)
    print(f"match_tif.npz: {NB * N} records, {sum(len(out[f'b{k}_fills']) for k in range(NB))} fills, "
          f"{int(out['book_counts'].sum())} resting, {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
