"""Every reader of the resting book over ONE book (tests/book_readers.py), each against the model its own tests
use. Needs an MI355X. Everything is exact.

The readers share one window walk and one far reader (matching_engine_amd/csrc/me_bookread.hpp); here they all
see the same hard cases — levels on both sides of 64-level and 4,096-level boundaries, both window edges, more
than 64 far levels, dead levels between live ones — at L = 128 (every total of a block is loaded), 1024 (16
occupancy words) and 8192 (128 occupancy words: two loads of 64). Behind every batch:

  snapshot with orders   book_orders at depths 16 and "all" against the oracle's dump and snapshot
  depth feed, D = 32     every job's events against tests/depth_model.py
  order query            every seq the scenario used against tests/order_query_model.py
  preview                sweeps from both sides of every symbol against tests/preview_model.py
and at the end the mass cancel of every symbol (count pass, then the removal list) against
tests/mass_cancel_model.py. tests/test_book_readers_model.py shows that the book is the one meant.
"""
import numpy as np
import pytest

from tests import book_audit
from tests import book_readers as br
from tests import depth_model as dm
from tests import mass_cancel_model as mc
from tests import order_query_model as oq
from tests import preview_cases as pc
from tests import preview_model as pm
from tests._parity import assert_books_equal, assert_fills_equal, assert_results_equal, side_levels
from tests.feed_common import _same
from tests.gpu_harness import FEED_PATHS, as_batch, engine_on
from tests.reduce_model import ReduceBook

pytestmark = pytest.mark.gpu

BUY, SELL = br.BUY, br.SELL
D = 32
ALL_LEVELS = 100_000


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _engine(me, sn):
    """The "reg" row at L = 128, the "deep" one above, at the scenario's own window size."""
    return engine_on(me, "reg" if sn.L <= 128 else "deep", sn.S, sn.base, sn.batches, table=FEED_PATHS, levels=sn.L, group=1)


def _sweeps(model, S):
    """tests/preview_cases.around for every symbol (the 18 best and the two worst levels of each side, the whole
    side, one more) and, per side, a MARKET for the quantity up to and including EVERY level."""
    q = []
    for s in range(S):
        q += pc.around(model, s, 20)
        lv = pm.levels_of(model, s)
        for side in (BUY, SELL):
            run = 0
            for _, fifo in lv[SELL if side == BUY else BUY]:
                run += sum(x for _, x in fifo)
                q.append((s, pc.kd(side, True), 0, run))
    return q


@pytest.mark.parametrize("L", br.LS)
def test_every_reader_over_one_book(me, L):
    from oracle.oracle import OracleBook

    sn = br.scenario(L)
    S = sn.S
    ob, rb = OracleBook(S), ReduceBook(S)
    depth = dm.DepthModel(ob, S, D)
    with _engine(me, sn) as eng:
        eng.depth_enable(D, 8 * D * S)
        _same(eng.depth_drain(), depth.expect(0), f"L={L} enable")
        for k, a in enumerate(sn.batches):
            ctx = f"L={L} batch {k}"
            r, f = eng.submit_batch(as_batch(me, a))
            ro, fo = ob.submit(a)
            rb.submit(a)
            assert_results_equal(r, ro, ctx)
            assert_fills_equal(f, fo, ctx)
            assert np.array_equal(eng.debug_export(("sym",))["sym"]["base"], sn.base), f"{ctx}: a window moved"
            # ---- depth feed
            _same(eng.depth_drain(), depth.expect(k + 1), f"{ctx} depth")
            assert eng.depth_stats()["deferred"] == 0
            # ---- snapshot with orders
            for s in range(S):
                dump = ob.dump(s)
                for n in (16, ALL_LEVELS):
                    bids, asks, lb, la = eng.book_orders(s, n)
                    assert np.array_equal(bids, side_levels(dump, BUY, n)), f"{ctx} symbol {s} depth {n}: bids"
                    assert np.array_equal(asks, side_levels(dump, SELL, n)), f"{ctx} symbol {s} depth {n}: asks"
                    sb, sa = ob.snapshot(s, n)
                    assert np.array_equal(lb, sb) and np.array_equal(la, sa), f"{ctx} symbol {s} depth {n}: levels"
            # ---- order query: every order of the scenario, resting or cancelled
            seqs = np.array(sn.seqs, dtype=np.uint64)
            want = oq.expected(rb, S, seqs)
            oq.assert_answers_equal(eng.order_query(seqs), want, f"{ctx} query")
            assert int(want["found"].sum()) == rb.resting() > 0
            # ---- preview
            queries = _sweeps(rb, S)
            got = eng.order_preview(np.array([q[0] for q in queries], dtype=np.uint32), np.array([q[1] for q in queries], dtype=np.uint8),
                                    np.array([q[2] for q in queries], dtype=np.int64), np.array([q[3] for q in queries], dtype=np.int32))
            pm.assert_answers_equal(got, pm.expected(rb, S, queries), f"{ctx} preview", queries)
            assert int(got["levels"].max()) == len(sn.window[(0, SELL)]) + br.NFAR  # (a sweep of a whole side)
        # (the readers read: the books are as the batches left them)
        assert_books_equal(eng, ob, range(S), f"L={L}")
        # ---- mass cancel: the count pass, then the removal list
        last = max(sn.seqs)
        want = mc.apply(ob, [2, 0, 3, 1], [SELL, 3, 3, 3], last)
        mc.assert_removed_equal(eng.mass_cancel([2, 0, 3, 1], [SELL, 3, 3, 3]), want, f"L={L} purge")
        assert want[1].tolist()[0][1] > 0 and want[1].tolist()[2] == [0, 0]
        _same(eng.depth_drain(), depth.expect(len(sn.batches)), f"L={L}: the purged sides leave the views")
        want = mc.apply(ob, [2], BUY, last)
        mc.assert_removed_equal(eng.mass_cancel([2], BUY), want, f"L={L} purge of the last side")
        assert int(want[1][0][0]) >= 68
        assert_books_equal(eng, ob, range(S), f"L={L} purged")
        assert eng.resting_count() == ob.resting() == 0
        v, _ = book_audit.audit(eng.debug_export(), last_seq=last)
        assert not v, f"L={L}: {v[:3]}"
        _same(eng.depth_drain(), depth.expect(len(sn.batches)), f"L={L}: the last views are deleted")
