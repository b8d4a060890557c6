"""What the CPU tests of the models share: field-by-field comparison of results, tapes and books, and the loader
of the committed model fixtures (tests/golden/match_tif.npz, match_reduce.npz, price_edges.npz)."""
import os

import numpy as np

from tests.tif_model import Arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS_RES = ("filled_qty", "remaining_qty", "fill_count", "tape_offset", "status", "reason")
FIELDS_FILL = ("taker_seq", "maker_seq", "price_q4", "qty", "symbol")
FIELDS_BOOK = ("seq", "price_q4", "qty", "side")


def same(a, b, fields, ctx):
    assert len(a) == len(b), f"{ctx}: {len(a)} vs {len(b)} entries"
    for f in fields:
        if not np.array_equal(np.asarray(a[f]), np.asarray(b[f])):
            i = int(np.nonzero(np.asarray(a[f]) != np.asarray(b[f]))[0][0])
            raise AssertionError(f"{ctx}: field {f} differs first at {i}: {a[i]} vs {b[i]}")


def load_model_fixture(name):
    """(meta, batches, results, fills, book) of tests/golden/`name`."""
    z = np.load(os.path.join(ROOT, "tests", "golden", name))
    from oracle.pybook import BOOK_DTYPE, FILL_DTYPE, RESULT_DTYPE

    batches, res, fills = [], [], []
    for k in range(int(z["nbatches"][0])):
        batches.append(Arrays(*[z[f"b{k}_{f}"] for f in ("seq", "price_q4", "qty", "symbol", "kind")]))
        res.append(np.ascontiguousarray(z[f"b{k}_res"]).view(RESULT_DTYPE).reshape(-1))
        fills.append(np.ascontiguousarray(z[f"b{k}_fills"]).view(FILL_DTYPE).reshape(-1))
    book = np.ascontiguousarray(z["book"]).view(BOOK_DTYPE).reshape(-1)
    meta = dict(num_symbols=int(z["num_symbols"][0]), levels=int(z["levels"][0]), base=z["base"],
                book_counts=z["book_counts"])
    return meta, batches, res, fills, book
