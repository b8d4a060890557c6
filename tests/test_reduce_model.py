"""The REDUCE model (tests/reduce_model.py) pinned with the unchanged native oracle (no GPU).

1. Hand cases, one per sentence of the semantics (include/me_engine.h ME_KIND_REDUCE).
2. Rewrite: the native oracle reads 0x0D as a plain cancel, so a stream with reduces becomes a stream it
   understands: a REDUCE with d >= r becomes a plain cancel; a strictly partial REDUCE is dropped and the
   target's SUBMITTED quantity is lowered by d instead (several reduces of one order summed). Before such a
   reduce the target had consumed q - r < q - d, as taker and as maker, so the smaller order behaves
   identically up to that point and holds the same quantity after it. Tapes and final books must be equal,
   and every result apart from the dropped records and the targets' own remaining_qty (which differs by the
   summed d). 60 seeded streams; every partial reduce of every stream takes part.
3. The committed fixture tests/golden/match_reduce.npz replays through the model.
4. ME_KIND_REDUCE is 0x0D in the header and in Python.
"""
import os
import re

import numpy as np
import pytest

from tests import reduce_model as rm
from tests.model_common import FIELDS_BOOK, FIELDS_FILL, FIELDS_RES, load_model_fixture, same
from tests.reduce_model import INT32_MAX, KIND_REDUCE, ReduceBook
from tests.tif_model import TIF_FOK, TIF_IOC, Arrays, TifBook, kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUY, SELL = 1, 2
ST_NEW, ST_PARTIAL, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
RJ_NONE, RJ_BAD_QTY, RJ_BAD_SYMBOL, RJ_UNKNOWN = 0, 1, 4, 5
CX = kind(BUY, 0, 1)
RD = KIND_REDUCE


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle

    return oracle


# ---- hand cases ----------------------------------------------------------------------------------

def _run(records, S=1, book=None):
    """records: (seq, price / target, qty, kind[, symbol]) -> results, tape, model."""
    rb = book or ReduceBook(S)
    a = Arrays([r[0] for r in records], [r[1] for r in records], [r[2] for r in records],
               [r[4] if len(r) > 4 else 0 for r in records], [r[3] for r in records])
    res, fills = rb.submit(a)
    return res, fills, rb


def _st(r):
    return (int(r["status"]), int(r["reason"]), int(r["filled_qty"]), int(r["remaining_qty"]), int(r["fill_count"]))


def _book(rb, s=0):
    return [(int(e["seq"]), int(e["qty"])) for e in rb.dump(s)]


def test_partial_reduce_keeps_the_place_in_the_queue():
    rest = [(1, 100, 10, kind(BUY)), (2, 100, 10, kind(BUY)), (3, 100, 10, kind(BUY))]
    res, fills, rb = _run(rest + [(3, 1, 4, RD), (4, 100, 8, kind(SELL))])
    assert _st(res[3]) == (ST_NEW, RJ_NONE, 0, 6, 0)
    assert [(int(f["maker_seq"]), int(f["qty"])) for f in fills] == [(1, 6), (2, 2)]
    assert _book(rb) == [(2, 8), (3, 10)]
    assert rb.resting() == 2


def test_level_total_and_resting_count_after_a_partial_reduce():
    res, _, rb = _run([(1, 100, 10, kind(SELL)), (2, 100, 7, kind(SELL)), (2, 2, 3, RD)])
    assert _st(res[2]) == (ST_NEW, RJ_NONE, 0, 4, 0)
    assert rb.resting() == 2 and _book(rb) == [(1, 10), (2, 4)]
    assert rb._liquidity(rb.side[0][1], BUY, True, 0, 1000) == 14


def test_covering_reduce_is_a_cancel():
    for d in (10, 11, INT32_MAX):
        res, _, rb = _run([(1, 100, 10, kind(BUY)), (2, 99, 5, kind(BUY)), (2, 1, d, RD)])
        assert _st(res[2]) == (ST_CANCELED, RJ_NONE, 0, 10, 0), d
        assert _book(rb) == [(2, 5)] and rb.resting() == 1
        assert rb.side[0][0].best() == 99  # the level is gone
    res, _, rb = _run([(1, 100, 10, kind(BUY)), (1, 1, 9, RD), (1, 1, 1, RD), (1, 1, 1, RD)])
    assert [_st(r) for r in res[1:]] == [(ST_NEW, RJ_NONE, 0, 1, 0), (ST_CANCELED, RJ_NONE, 0, 1, 0),
                                         (ST_REJECTED, RJ_UNKNOWN, 0, 0, 0)]


def test_reject_order():
    rest = [(1, 100, 10, kind(BUY))]
    res, _, rb = _run(rest + [(1, 1, 0, RD), (1, 1, -1, RD), (1, 77, 0, RD), (1, 77, 5, RD),
                              (1, 1, 0, RD, 9), (1, 1, 5, RD, 9)], S=2)
    assert _st(res[1]) == (ST_REJECTED, RJ_BAD_QTY, 0, 0, 0)      # d = 0 on a live target
    assert _st(res[2]) == (ST_REJECTED, RJ_BAD_QTY, 0, 0, 0)      # d < 0
    assert _st(res[3]) == (ST_REJECTED, RJ_BAD_QTY, 0, 0, 0)      # BAD_QTY before UNKNOWN_ORDER
    assert _st(res[4]) == (ST_REJECTED, RJ_UNKNOWN, 0, 0, 0)
    assert _st(res[5]) == (ST_REJECTED, RJ_BAD_SYMBOL, 0, 0, 0)   # BAD_SYMBOL before BAD_QTY
    assert _st(res[6]) == (ST_REJECTED, RJ_BAD_SYMBOL, 0, 0, 0)
    assert _book(rb) == [(1, 10)]
    # the target of another symbol, a filled one, a cancelled one, a taker that never rested
    res, _, rb = _run([(1, 100, 10, kind(BUY), 0), (2, 100, 10, kind(SELL), 1), (2, 1, 3, RD, 1),
                       (3, 100, 10, kind(BUY), 1), (3, 2, 3, RD, 1), (3, 3, 3, RD, 1),
                       (3, 1, 0, CX, 0), (3, 1, 3, RD, 0)], S=2)
    for i in (2, 4, 5, 7):
        assert _st(res[i]) == (ST_REJECTED, RJ_UNKNOWN, 0, 0, 0), i


def test_side_and_tif_bits_are_ignored_and_a_plain_cancel_ignores_qty():
    for k in (0x0C, 0x0D, 0x0E, 0x0F, 0x1D, 0x3E, 0xFD):
        res, _, rb = _run([(1, 100, 10, kind(SELL)), (1, 1, 4, k)])
        assert _st(res[1]) == (ST_NEW, RJ_NONE, 0, 6, 0), hex(k)
    for q in (0, -1, 4, 10, 99):
        res, _, rb = _run([(1, 100, 10, kind(SELL)), (1, 1, q, CX)])
        assert _st(res[1]) == (ST_CANCELED, RJ_NONE, 0, 10, 0), q
        assert rb.resting() == 0


def test_tape_offset_follows_the_general_rule_and_a_reduce_never_rests():
    res, fills, rb = _run([(1, 100, 10, kind(SELL)), (2, 100, 4, kind(BUY)), (2, 1, 2, RD), (3, 100, 1, kind(BUY)),
                           (3, 1, 0, RD), (3, 1, 50, RD)])
    assert [int(r["tape_offset"]) for r in res] == [0, 0, 1, 1, 2, 2]
    assert _st(res[2]) == (ST_NEW, RJ_NONE, 0, 4, 0)   # 10 - 4 filled = 6, less 2
    assert _st(res[5]) == (ST_CANCELED, RJ_NONE, 0, 3, 0)
    assert rb.resting() == 0 and len(fills) == 2


def test_reduced_quantity_is_what_fok_and_takers_see():
    rest = [(1, 100, 10, kind(SELL)), (2, 101, 10, kind(SELL)), (2, 1, 5, RD)]
    res, _, rb = _run(rest + [(3, 101, 16, kind(BUY, 0, 0, TIF_FOK)), (4, 101, 15, kind(BUY, 0, 0, TIF_FOK))])
    assert _st(res[3]) == (ST_CANCELED, RJ_NONE, 0, 16, 0)
    assert _st(res[4]) == (ST_FILLED, RJ_NONE, 15, 0, 2)
    res, _, rb = _run(rest + [(3, 100, 7, kind(BUY, 0, 0, TIF_IOC))])
    assert _st(res[3]) == (ST_CANCELED, RJ_NONE, 5, 2, 1)


def test_reduce_of_a_partly_filled_order_and_across_batches():
    rb = ReduceBook(1)
    _run([(1, 100, 10, kind(SELL)), (2, 100, 3, kind(BUY))], book=rb)
    res, _, _ = _run([(2, 1, 6, RD)], book=rb)
    assert _st(res[0]) == (ST_NEW, RJ_NONE, 0, 1, 0) and _book(rb) == [(1, 1)]
    res, _, _ = _run([(2, 1, 1, RD)], book=rb)
    assert _st(res[0]) == (ST_CANCELED, RJ_NONE, 0, 1, 0) and rb.resting() == 0


def test_without_reduces_the_model_is_the_tif_model():
    from tests.tif_model import tif_stream

    _, batches = tif_stream(5, 8, 128, 2, 800, far_pct=2)
    a, b = TifBook(8), ReduceBook(8)
    for k, x in enumerate(batches):
        ra, fa = a.submit(x)
        rb_, fb = b.submit(x)
        same(ra, rb_, FIELDS_RES, f"batch {k}")
        same(fa, fb, FIELDS_FILL, f"batch {k}")
        assert a.verdicts == b.verdicts


# ---- the pin to the native oracle ------------------------------------------------------------------

N_STREAMS = 60
PLAIN = dict(mix=(62, 0, 0, 0, 14, 24), market_tifs=(0,), max_qty=40)


def _rewrite_and_compare(orc, seed):
    """Returns (partial reduces of the stream, those the comparison covered, covering reduces)."""
    S = 5
    far = 4 if seed % 3 == 0 else 0
    _, batches = rm.reduce_stream(seed, S, 128, 3, 500, far_pct=far, drift=(seed % 4) * 5, convert_pct=70,
                                  fresh_pct=10, skew=bool(seed % 2), **PLAIN)
    rb = ReduceBook(S)
    outs, notes = [], []
    lowered = {}  # target seq -> summed d of its strictly partial reduces
    n_part = n_cover = 0
    for b in batches:
        outs.append(rb.submit(b))
        notes.append({i: (tgt, d, had) for i, tgt, d, had in rb.reduces})
        for i, tgt, d, had in rb.reduces:
            if had is not None and d < had:
                lowered[tgt] = lowered.get(tgt, 0) + d
                n_part += 1
            elif had is not None:
                n_cover += 1
    ob = orc.OracleBook(S)
    checked = 0
    fills_m, fills_o = [], []
    seen_targets = set()
    for k, b in enumerate(batches):
        rm_, fm = outs[k]
        keep, qty, kd = [], b.qty.copy(), (b.kind & 0x0F).copy()
        for i in range(len(b)):
            note = notes[k].get(i)
            if note is None:
                if not (int(b.kind[i]) & 8) and int(b.seq[i]) in lowered:
                    qty[i] -= lowered[int(b.seq[i])]
                    assert qty[i] > 0
                keep.append(i)
                continue
            tgt, d, had = note
            if d <= 0:
                assert _st(rm_[i])[:2] == (ST_REJECTED, RJ_BAD_QTY)
            elif had is not None and d < had:
                assert _st(rm_[i]) == (ST_NEW, RJ_NONE, 0, had - d, 0)
                checked += 1
            else:  # covering, or an unknown target: a plain cancel
                kd[i] = CX
                keep.append(i)
        keep = np.array(keep, dtype=np.int64)
        ro, fo = ob.submit(Arrays(b.seq[keep], b.price_q4[keep], qty[keep], b.symbol[keep], kd[keep]))
        fills_m.append(fm)
        fills_o.append(fo)
        got = rm_[keep]
        for f in FIELDS_RES:
            bad = np.nonzero(got[f] != ro[f])[0]
            for j in bad:
                i = int(keep[j])
                sq = int(b.seq[i])
                own = f == "remaining_qty" and not (int(b.kind[i]) & 8) and sq in lowered
                assert own and int(got[f][j]) - int(ro[f][j]) == lowered[sq], \
                    f"seed {seed} batch {k} record {i}: {f} {got[j]} vs {ro[j]}"
                seen_targets.add(sq)
    same(np.concatenate(fills_m), np.concatenate(fills_o), FIELDS_FILL, f"seed {seed} tape")
    for s in range(S):
        same(rb.dump(s), ob.dump(s), FIELDS_BOOK, f"seed {seed} book {s}")
    assert seen_targets == set(lowered), "every lowered target's own result differs, and only by the summed d"
    return n_part, checked, n_cover


@pytest.fixture(scope="module")
def pinned(orc):
    return [_rewrite_and_compare(orc, seed) for seed in range(100, 100 + N_STREAMS)]


def test_rewrite_pins_the_model_to_the_native_oracle(pinned):
    assert len(pinned) >= 50
    total = covered = 0
    for n_part, checked, n_cover in pinned:
        assert n_part > 0 and checked == n_part, "a stream whose partial reduces were not all compared"
        assert n_cover > 0
        total += n_part
        covered += checked
    assert covered == total and total > 50 * 20


# ---- the committed fixture ---------------------------------------------------------------------------

def test_fixture_replays_through_the_model():
    meta, batches, res, fills, book = load_model_fixture("match_reduce.npz")
    rb = ReduceBook(meta["num_symbols"])
    outcomes = set()
    for k, b in enumerate(batches):
        r, f = rb.submit(b)
        same(r, res[k], FIELDS_RES, f"batch {k} results")
        same(f, fills[k], FIELDS_FILL, f"batch {k} tape")
        red = rm.is_reduce(b.kind)
        outcomes |= set(zip(r["status"][red].tolist(), r["reason"][red].tolist()))
    dumps = np.concatenate([rb.dump(s) for s in range(meta["num_symbols"])])
    same(dumps, book, FIELDS_BOOK, "final book")
    assert {(ST_NEW, RJ_NONE), (ST_CANCELED, RJ_NONE), (ST_REJECTED, RJ_UNKNOWN), (ST_REJECTED, RJ_BAD_QTY)} <= outcomes


def test_fixture_generator_reproduces_the_committed_file():
    from tests.golden import make_reduce_golden as g

    base, batches = rm.reduce_stream(20261020, g.S, g.L, g.NB, g.N, far_pct=2, drift=3, skew=True)
    meta, fb, _, _, _ = load_model_fixture("match_reduce.npz")
    assert np.array_equal(base, meta["base"])
    for a, b in zip(batches, fb):
        for f in ("seq", "price_q4", "qty", "symbol", "kind"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f


# ---- the code point ----------------------------------------------------------------------------------

def test_kind_reduce_is_0x0d_in_header_and_python(built):
    import matching_engine_amd as me
    from matching_engine_amd import _abi

    eh = open(os.path.join(ROOT, "include", "me_engine.h")).read()
    m = re.search(r"#define\s+ME_KIND_REDUCE\s+\(\(uint8_t\)(0x[0-9A-Fa-f]+)\)", eh)
    assert m and int(m.group(1), 16) == 0x0D
    assert _abi.KIND_REDUCE == 0x0D == KIND_REDUCE == me.KIND_REDUCE
    assert _abi.KIND_REDUCE == _abi.kind(1, 1, 1)  # bits 3 and 2 (and a side the engine ignores)
    assert _abi.KIND_REDUCE & 0x0C == 0x0C
    sh = open(os.path.join(ROOT, "include", "me_service.h")).read()
    assert re.search(r"\bint\s+me_service_reduce_order\s*\(", sh)
    assert "me_service_reduce_order" in _abi.PROTOTYPES
