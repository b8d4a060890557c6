"""me_order_preview (k_order_preview) on every matching path against the model
(tests/preview_model.py). Needs an MI355X. Everything is exact.

After every batch of a case of tests/preview_cases.py the whole query set is previewed and every field of every
answer compared with the model's; then one of the previewed records is submitted for real, as the next record
of the stream, through engine and model, and the engine's own me_order_result and the fold of its fills must
equal the preview taken just before: the preview kernel is a second observer of the TIF rules of whichever
matching path wrote the book. tests/test_preview_model.py asserts what kinds of answers the query sets hold.
"""
import ctypes as C

import numpy as np
import pytest

from tests import book_audit
from tests import preview_cases as pc
from tests import preview_model as pm
from tests._parity import assert_books_equal, assert_fills_equal, assert_results_equal
from tests.gpu_harness import PATHS, as_batch, engine_on
from tests.reduce_model import ReduceBook

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
ALL = tuple(PATHS)


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _preview(eng, queries):
    return eng.order_preview(np.array([q[0] for q in queries], dtype=np.uint32), np.array([q[1] for q in queries], dtype=np.uint8),
                             np.array([q[2] for q in queries], dtype=np.int64), np.array([q[3] for q in queries], dtype=np.int32))


def _submit(me, eng, a, device):
    """One batch, synchronously: a host batch, or a device batch of a launch group of its own."""
    if not device:
        return eng.submit_batch(as_batch(me, a))
    db = eng.upload(as_batch(me, a))
    try:
        eng.submit_device(db)
        eng.sync()
        return eng.fetch_group_outputs(eng.last_group_size() - 1, len(a))
    finally:
        db.free()


def _run(me, path, case, device=False, **kw):
    """The case through an engine of `path` and a ReduceBook beside it."""
    model = ReduceBook(case.S)
    total = sum(len(a) for a in case.batches) + len(case.batches)
    kw = dict({"max_resting": 2 * total + 1024}, **case.kw, **kw)
    with engine_on(me, path, case.S, case.base, case.batches, **kw) as eng:
        for k, a in enumerate(case.batches):
            ctx = f"{case.name} {path} batch {k}"
            if device:  # the batch waits in a partial launch group: the preview's me_sync launches it
                db = eng.upload(as_batch(me, a))
                eng.submit_device(db)
            else:
                r, f = eng.submit_batch(as_batch(me, a))
            ro, fo = model.submit(a)
            queries = case.queries(model, k)
            want = pm.expected(model, case.S, queries)
            got = _preview(eng, queries)
            if device:
                r, f = eng.fetch_group_outputs(eng.last_group_size() - 1, len(a))
                db.free()
            assert_results_equal(r, ro, ctx)
            assert_fills_equal(f, fo, ctx)
            pm.assert_answers_equal(got, want, ctx, queries)
            if k == 0 and case.window:  # the script's claim about the window, which the model test's tags lean on
                sym = eng.debug_export(("sym",))["sym"]
                for s, (b, _) in case.window.items():
                    assert int(sym["base"][s]) == b, f"{ctx}: the window of symbol {s} moved"
            i = case.real(k, want)
            rec = pc.one(case.free[k], queries[i])
            r1, f1 = _submit(me, eng, rec, device)
            ro1, fo1 = model.submit(rec)
            assert_results_equal(r1, ro1, f"{ctx} real record {i}")
            assert_fills_equal(f1, fo1, f"{ctx} real record {i}")
            pm.assert_matches_submit(got[i], r1[0], f1, f"{ctx} real record {i} {queries[i]}")
        assert_books_equal(eng, model, range(case.S), case.name)
        v, _ = book_audit.audit(eng.debug_export())
        assert not v, f"{case.name} {path}: {v[:3]}"


# ---- the directed cases: chunks, window walk order, far levels, quantities, every kind byte -------------------------

@pytest.mark.parametrize("path", ALL)
@pytest.mark.parametrize("script", ["chunks", "window_order", "far", "wide", "fok", "mixed"])
def test_scripts(me, path, script):
    _run(me, path, getattr(pc, script)(PATHS[path][0]))


@pytest.mark.parametrize("path", ALL)
@pytest.mark.parametrize("name", pc.EDGE_CASES)
def test_int64_edges(me, path, name):
    _run(me, path, pc.edges(PATHS[path][0], name))


# ---- seeded streams; device batches in a partial launch group where the path has groups ---------------------------------

@pytest.mark.parametrize("path", ALL)
def test_seeded(me, path):
    grouped = PATHS[path][3]
    _run(me, path, pc.seeded(PATHS[path][0]), device=grouped, **({"batches_per_launch": 8} if grouped else {}))


# ---- refusals, n == 0, empty books, a purged side ----------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["reg", "deep"])
def test_arguments_and_empty_books(me, path):
    case = pc.mixed(PATHS[path][0])
    S, mid = case.S, int(case.base[0]) + case.L // 2
    model = ReduceBook(S)
    with engine_on(me, path, S, case.base, case.batches) as eng:
        lib, h = eng.lib, eng.h
        empty = [(s, pc.kd(side, market, tif), mid, 5) for s in range(S) for side in (BUY, SELL) for market in (False, True)
                 for tif in range(4)]
        got = _preview(eng, empty)  # nothing was ever submitted
        pm.assert_answers_equal(got, pm.expected(model, S, empty), f"empty books {path}", empty)
        assert not (got["flags"] & pm.PV_HAS_OPP).any() and not got["fill_count"].any()
        assert len(eng.order_preview([], [], [], [])) == 0
        assert lib.me_order_preview(h, None, 0, None) == me.ME_OK
        eng.submit_batch(as_batch(me, case.batches[0]))
        model.submit(case.batches[0])
        sy, kd_, px, qt = (np.array([0], dtype=np.uint32), np.array([pc.kd(BUY)], dtype=np.uint8),
                           np.array([mid + 1], dtype=np.int64), np.array([3], dtype=np.int32))
        out = np.zeros(1, dtype=me.PREVIEW_DTYPE)

        def call(sy=sy, kd_=kd_, px=px, qt=qt, n=1, out=out, soa=True):
            at = lambda a: None if a is None else a.ctypes.data  # noqa: E731
            q = me._abi.MeOrderSoa(None, at(px), at(qt), at(sy), at(kd_)) if soa else None
            return lib.me_order_preview(h, C.byref(q) if soa else None, n, at(out))

        assert call() == me.ME_OK and int(out["filled_qty"][0]) == 3
        for bad in (dict(sy=None), dict(kd_=None), dict(px=None), dict(qt=None), dict(out=None), dict(soa=False),
                    dict(n=(1 << 24) + 1)):
            assert call(**bad) == me.ME_E_INVALID, bad
        # a CANCEL or a REDUCE among the queries: refused on the host, nothing answered
        for k8 in (me.kind(BUY, 0, 1), me.KIND_REDUCE, pc.kd(SELL, True, 2) | 8):
            out[:] = 0
            out["levels"] = 77
            kinds = np.array([pc.kd(BUY), k8], dtype=np.uint8)
            two = [np.array([0, 0], dtype=np.uint32), kinds, np.array([mid + 1, 4], dtype=np.int64), np.array([3, 1], dtype=np.int32)]
            o2 = np.zeros(2, dtype=me.PREVIEW_DTYPE)
            o2["levels"] = 77
            q = me._abi.MeOrderSoa(None, two[2].ctypes.data, two[3].ctypes.data, two[0].ctypes.data, two[1].ctypes.data)
            assert lib.me_order_preview(h, C.byref(q), 2, o2.ctypes.data) == me.ME_E_INVALID
            assert (o2["levels"] == 77).all() and not o2["status"].any(), "a refused call answered something"
        # none of that failed the engine
        full = case.queries(model, 0)
        pm.assert_answers_equal(_preview(eng, full), pm.expected(model, S, full), f"after the refusals {path}", full)
        # a side emptied by a mass cancel: HAS_OPP clear for the takers of that side
        removed, _ = eng.mass_cancel([0], SELL)
        assert len(removed) == 3
        for e in removed:
            model.submit(pc.one(0, (0, me.kind(BUY, 0, 1), int(e["seq"]), 0)))  # (the same orders, cancelled one by one)
        got = _preview(eng, full)
        pm.assert_answers_equal(got, pm.expected(model, S, full), f"after the mass cancel {path}", full)
        buys = np.array([q[0] == 0 and (q[1] & 3) == BUY and q[3] > 0 and not ((q[1] >> 4) & 3 == 3 and q[1] & 4) for q in full])
        assert buys.any() and not (got["flags"][buys] & pm.PV_HAS_OPP).any() and not got["fill_count"][buys].any()
        assert_books_equal(eng, model, range(S), f"arguments {path}")


# ---- the call reads and nothing else --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ALL)
def test_read_only(me, path):
    case = pc.seeded(PATHS[path][0], seed=1, per=512)
    S = case.S
    model = ReduceBook(S)
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with engine_on(me, path, S, case.base, case.batches, **kw) as eng:
        eng.quotes_enable(1 << 14)
        eng.depth_enable(5, 1 << 15)
        eng.trades_enable(1 << 14)
        for a in case.batches[:-1]:
            eng.submit_batch(as_batch(me, a))
            model.submit(a)
        assert model.resting() > 100
        feeds = ((eng.quotes_drain, eng.quotes_stats), (eng.depth_drain, eng.depth_stats), (eng.trades_drain, eng.trades_stats))
        for drain, _ in feeds:
            drain()
        stats0 = [st() for _, st in feeds]
        raw0 = eng.debug_export()
        resting0 = eng.resting_count()
        queries = [q for k in range(16) for q in case.queries(model, 100 + k)][:1000]
        assert len(queries) == 1000
        got = _preview(eng, queries)
        pm.assert_answers_equal(got, pm.expected(model, S, queries), f"read-only {path}", queries)
        assert int(got["fill_count"].sum()) > 500 and len(set(got["status"].tolist())) == 5
        raw1 = eng.debug_export()
        for name in me._abi.DBG_ARRAYS:
            assert raw0[name].tobytes() == raw1[name].tobytes(), f"{path}: the preview changed {name}"
        assert eng.resting_count() == resting0 == model.resting()
        v, _ = book_audit.audit(raw1)
        assert not v, v[:3]
        for (drain, st), s0 in zip(feeds, stats0):
            assert len(drain()) == 0 and st() == s0, f"{path}: a feed moved"
        # the next batch is stamped as if the preview had never been: it was no batch
        a = case.batches[-1]
        r, f = eng.submit_batch(as_batch(me, a))
        ro, fo = model.submit(a)
        assert_results_equal(r, ro, f"read-only {path} next batch")
        assert_fills_equal(f, fo, f"read-only {path} next batch")
        ev = eng.quotes_drain()
        assert len(ev) and set(ev["batches"].tolist()) == {len(case.batches)}
        assert_books_equal(eng, model, range(S), f"read-only {path}")
