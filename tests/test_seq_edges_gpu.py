"""Seq-repeating cancels at launch-group, batch and block starts (tests/seq_edges.py, DESIGN.md §6 "Stream-position
edges") on every matching path. Needs an MI355X. Everything is bit-exact.

The scripted cases carry their outcomes and final books written by hand (tests/test_seq_edges_model.py pins the
four models to them on the CPU); here every path must give them, launch group by launch group, together with
ReduceBook's full results and tapes, every book, the resting counters, the raw-array audit and the order query of
the boundary targets. The overlay streams run against ReduceBook. No stream here is invalid: the seq rule and
the ring-span rule hold for every one.
"""
import numpy as np
import pytest

from tests import order_query_model as oq
from tests import seq_edges as se
from tests._parity import assert_books_equal, assert_fills_equal, assert_results_equal
from tests.book_audit import audit, names
from tests.gpu_harness import PATHS, as_batch, engine_on, env
from tests.reduce_model import ReduceBook

pytestmark = pytest.mark.gpu

ALL = tuple(PATHS)
GROUPED = tuple(p for p in PATHS if PATHS[p][3])
ST_CANCELED = 3


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


class Run:
    """One engine against ReduceBook; `group` runs one launch group through both (pipelined host batches, one
    device group, or synchronous batches on the ungrouped paths) and checks everything the engine says and
    keeps."""

    def __init__(self, me, eng, S, path, mode, ctx):
        self.me, self.eng, self.S, self.ctx = me, eng, S, ctx
        self.grouped, self.mode = PATHS[path][3], mode
        self.model = ReduceBook(S)
        self.last_seq = 0

    def group(self, arrays, tag):
        eng, bs, ctx = self.eng, [as_batch(self.me, a) for a in arrays], f"{self.ctx} {tag}"
        if not self.grouped:
            outs = [eng.submit_batch(b) for b in bs]
        elif self.mode == "host":
            tickets = [eng.submit_host(b) for b in bs]
            outs = [eng.collect(t) for t in tickets]
        else:
            dbs = [eng.upload(b) for b in bs]
            try:
                for db in dbs:
                    eng.submit_device(db)
                eng.sync()
                outs = [eng.fetch_group_outputs(j, len(a)) for j, a in enumerate(arrays)]
            finally:
                for db in dbs:
                    db.free()
        if self.grouped:
            assert eng.last_group_size() == len(arrays), f"{ctx}: the batches were not one launch group"
        want = []
        for k, (a, (r, f)) in enumerate(zip(arrays, outs)):
            ro, fo = self.model.submit(a)
            assert_results_equal(r, ro, f"{ctx} batch {k}")
            assert_fills_equal(f, fo, f"{ctx} batch {k}")
            self.last_seq = max(self.last_seq, int(a.seq.max()))
            want.append(r)
        assert_books_equal(eng, self.model, range(self.S), ctx)
        assert eng.resting_count() == eng.admission()["resting"] == self.model.resting(), f"{ctx}: resting counters"
        raw = eng.debug_export()
        v, _ = audit(raw, last_seq=self.last_seq)
        assert not v, f"{ctx}: {len(v)} audit violations {names(v)}; first {v[:3]}"
        return want, raw


def _run_case(me, path, case, mode):
    grouped = PATHS[path][3]
    ctx = f"{case.name} [{path} {mode}]"
    with engine_on(me, path, case.S, case.base, case.batches, group=max(case.groups), ring=case.ring) as eng:
        run = Run(me, eng, case.S, path, mode, ctx)
        k = 0
        for gi, g in enumerate(case.groups):
            h0 = eng.stats()["handoffs"]
            res, raw = run.group(case.batches[k:k + g], f"group {gi}")
            for j, r in enumerate(res):  # the hand-written outcomes themselves
                assert se.outcomes(r) == [tuple(x) for x in case.expected[k + j]], f"{ctx} batch {k + j}"
            if gi == case.boundary:
                moved = eng.stats()["handoffs"] - h0
                if path == "gwalk_cx" and case.handoff is False:
                    assert moved == 0, f"{ctx}: {moved} hand-offs: the walk's own lookup did not answer"
                if path == "gwalk_cx" and case.handoff is True:
                    assert moved > 0, f"{ctx}: a REDUCE did not hand its symbol off"
                if case.family == "sweep_start":  # the sweep ran at this group: its first seq is the horizon
                    sq = raw["sq"][raw["info"]["sq_idx"]]
                    assert int(sq["horizon"]) == int(case.batches[k].seq[0]), f"{ctx}: horizon {sq}"
            asks = case.queries.get(gi, [])
            if asks:
                seqs = np.array([q for q, _ in asks], dtype=np.uint64)
                got = eng.order_query(seqs)
                oq.assert_answers_equal(got, oq.expected(run.model, case.S, seqs), ctx)
                for a, (q, w) in zip(got, asks):
                    if w is None:
                        assert not int(a["found"]), f"{ctx}: seq {q} still found"
                    else:
                        assert (int(a["found"]), int(a["qty"]), int(a["orders_ahead"])) == (1,) + w, f"{ctx}: seq {q}: {a}"
            k += g
        for s in range(case.S):
            assert se.book_rows(eng.dump(s)) == case.books[s], f"{ctx}: final book of symbol {s}"
    return grouped


MODES = [(p, "host") for p in ALL] + [(p, "device") for p in GROUPED]


@pytest.mark.parametrize("family", se.FAMILIES)
@pytest.mark.parametrize("path,mode", MODES)
def test_scripted(me, path, mode, family):
    """Every scripted case of the family, every form, on the path: pipelined host batches at the case's group
    size or one device group per launch group (L = 128 paths), one synchronous batch per launch elsewhere."""
    cases = [c for c in se.scripted(PATHS[path][0]) if c.family == family]
    assert cases
    for case in cases:
        _run_case(me, path, case, mode)


# ---- the seeded overlay ---------------------------------------------------------------------------------------------

OS, ONB, ON, OVERLAY_KW = se.OS, se.ONB, se.ON, se.OVERLAY_KW
SEEDS = (0, 1)
HIGH = se.OVERLAY_HIGH
_overlay = se.overlay_stream  # (base, batches, labels); their floors: tests/test_seq_edges_model.py


def _run_overlay(me, path, seed, group, ring, plain=False, high=False):
    L = PATHS[path][0]
    base, arrays, labels = _overlay(L, seed, plain, high)
    for k in range(0, len(arrays), group):  # a launch group has to span fewer seqs than the ring
        assert int(arrays[min(k + group, len(arrays)) - 1].seq[-1]) - int(arrays[k].seq[0]) < ring
    cancelled = 0
    with engine_on(me, path, OS, base, arrays, group=group, ring=ring) as eng:
        run = Run(me, eng, OS, path, "host", f"overlay {path} #{seed} G={group} ring={ring} plain={plain}")
        for k in range(0, len(arrays), group):
            res, raw = run.group(arrays[k:k + group], f"batches {k}..")
            cancelled += sum(int((r["status"] == ST_CANCELED).sum()) for r in res)
        sq = raw["sq"][raw["info"]["sq_idx"]]
        st = eng.stats()
    print(f"overlay {path} #{seed} G={group} ring={ring} plain={plain}: {st}, {cancelled} cancelled, "
          f"{se.boundary_successes(arrays, labels, group, OS)} own-seq successes at group starts, epoch {int(sq['epoch'])}")
    assert cancelled > 100
    return sq, st


GROUPS = [(p, g) for p in ALL for g in ((1, 4) if PATHS[p][3] else (1,))]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("path,group", GROUPS)
def test_overlay(me, path, group, seed):
    """boundary_stream against ReduceBook after every launch group: results, tapes, books, counters, audit."""
    _run_overlay(me, path, seed, group, 1 << 20)


@pytest.mark.parametrize("path,group", [(p, g) for p, g in GROUPS if PATHS[p][3]])
def test_overlay_plain(me, path, group):
    """The overlay without REDUCEs and time-in-force bits, every boundary record a CANCEL: nothing hands a symbol
    off by kind, so on the cancel walk the walk's own lookups answer the boundary cancels."""
    _, st = _run_overlay(me, path, 0, group, 1 << 20, plain=True)
    if path == "gwalk_cx":  # at most the symbols whose bucket passes 128 records leave the walk
        _, arrays, _ = _overlay(PATHS[path][0], 0, True, False)
        over = sum(int((np.bincount(a.symbol[a.symbol < OS]) > 128).sum()) for a in arrays)
        assert st["handoffs"] <= over, (st, over)


@pytest.mark.parametrize("path", GROUPED)
def test_overlay_small_ring(me, path):
    """seq_ring = 1,024 under seqs above 2^40, one batch per launch group (its ~800 records span most of the
    ring): horizons move with nearly every group, older targets go through the old-order table."""
    sq, _ = _run_overlay(me, path, 0, 1, 1024, high=True)
    assert int(sq["epoch"]) > 4 and int(sq["horizon"]) > HIGH, f"the horizon never moved: {sq}"


# ---- the service ------------------------------------------------------------------------------------------------------

def test_service_cancel_of_the_last_order(me):
    """The service's stream position for a cancel is the last OID it gave out: a cancel of the most recently
    accepted order is its slice's first record and repeats its target's seq. The engine behind the service is
    created under the gwalk_cx environment, so the cancel walk answers (asserted through paths())."""
    LIMIT, BUY, SELL, MID = 0, 1, 2, 1_000_000
    L, row_env, expect, _ = PATHS["gwalk_cx"]
    with env(row_env):
        eng = me.Engine(2, L, [MID - L // 2, MID - L // 2], max_batch=1024, max_resting=1024, batches_per_launch=1)
    with eng:
        p = eng.paths()
        assert all(p[k] == v for k, v in expect.items()), p
        svc = me.MatchingEngineService(eng, ["SYM", "ABC"])
        try:
            def flush():
                seq, res, fills = svc.flush()
                return seq.tolist(), res["status"].tolist(), res["reason"].tolist(), res["remaining_qty"].tolist()

            def upd():
                return [(u["order_id"], u["client_id"], u["status"], u["remaining_quantity"]) for u in svc.order_updates()]

            # 1. rest, close the slice, cancel as the next slice's only request
            assert svc.submit_order("M", "SYM", LIMIT, BUY, MID - 10, 4, 7)["order_id"] == "OID-1"
            assert flush() == ([1], [0], [0], [7])
            upd()
            h0 = eng.stats()["handoffs"]
            assert svc.cancel_order("M", "SYM", "OID-1")["success"]
            assert flush() == ([1], [ST_CANCELED], [0], [7])
            assert upd() == [("OID-1", "M", ST_CANCELED, 7)]
            assert svc.order_book("SYM") == ([], [])
            assert eng.resting_count() == 0
            # 2. two clients' orders rest; one slice cancels the older one, then the most recent one
            assert svc.submit_order("M", "SYM", LIMIT, BUY, MID - 10, 4, 5)["order_id"] == "OID-2"
            assert svc.submit_order("N", "ABC", LIMIT, SELL, MID + 10, 4, 6)["order_id"] == "OID-3"
            assert flush() == ([2, 3], [0, 0], [0, 0], [5, 6])
            upd()
            assert svc.cancel_order("M", "SYM", "OID-2")["success"] and svc.cancel_order("N", "ABC", "OID-3")["success"]
            assert flush() == ([3, 3], [ST_CANCELED, ST_CANCELED], [0, 0], [5, 6])
            assert upd() == [("OID-2", "M", ST_CANCELED, 5), ("OID-3", "N", ST_CANCELED, 6)]
            assert svc.order_book("SYM") == ([], []) and svc.order_book("ABC") == ([], [])
            assert eng.resting_count() == 0
            assert eng.stats()["handoffs"] == h0, "a cancel slice left the walk"
        finally:
            svc.close()
