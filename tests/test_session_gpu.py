"""Composed sessions on every matching path (tests/session.py): all four device feeds on, stops
armed, triggered stops injected back into the stream, and stops_add / stops_cancel / mass_cancel / order_query /
order_preview between and in the middle of launches, on one stream of the full record vocabulary. The plan is
computed on the CPU from the models alone (its reach is asserted in tests/test_session_model.py); here the engine
replays it step by step and every output is compared: per-batch results and tapes, after every stretch the books,
the raw arrays' audit, every feed's events job by job, the feeds' counters and the trigger book's dump, and every
between-launch call's own answer. No comparison is left out of any variant. Needs an MI355X.
"""
import numpy as np
import pytest

from tests import depth_model as dm
from tests import mass_cancel_model as mc
from tests import order_query_model as oq
from tests import preview_model as pv
from tests import quote_model as qm
from tests import session as ss
from tests import trade_model as tm
from tests._parity import assert_fills_equal, assert_results_equal
from tests.audit_run import Run
from tests.feed_common import _same
from tests.gpu_harness import as_batch, check_books, engine_on, pipelined

pytestmark = pytest.mark.gpu

FIELDS = ("seq", "price_q4", "qty", "symbol", "kind")


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


class _Levels:
    """One levels_all call as the snapshot() the feed models read."""

    def __init__(self, eng, depth):
        self.lv, self.cnt = eng.levels_all(depth)

    def snapshot(self, s, depth):
        return self.lv[s, 0, : self.cnt[s, 0]], self.lv[s, 1, : self.cnt[s, 1]]


def _by_stamp(got, exp, ctx):
    """The drained events job by job (a job's events carry its launch's batch count), then as a whole."""
    for x in np.unique(np.concatenate([got["batches"], exp["batches"]])):
        _same(got[got["batches"] == x], exp[exp["batches"] == x], f"{ctx}, the jobs stamped {int(x)}")
    _same(got, exp, ctx)


class _Replay:
    def __init__(self, me, eng, plan):
        self.me, self.eng, self.p = me, eng, plan
        self.ctx = plan.case.id
        self.run = Run(me, eng, ss.S, plan.grouped, self.ctx)
        self.events = None  # the stop events the engine gave at the last checkpoint
        self.all = {"quotes": [], "depth": [], "trades": []}

    def step(self, st, k):
        getattr(self, st["op"])(st, f"{self.ctx} step {k} {st['op']}")

    def stops_add(self, st, ctx):
        if not st["refused"]:
            self.eng.stops_add(st["stops"])
            return
        with pytest.raises(self.me.EngineError) as ei:
            self.eng.stops_add(st["stops"])
        assert ei.value.code == self.me.ME_E_CAPACITY, ctx  # nothing was added: the next checkpoint's dump shows it

    def stops_cancel(self, st, ctx):
        found = self.eng.stops_cancel(st["ids"])
        assert np.array_equal(found, st["found"]), f"{ctx}: found {found.tolist()}, planned {st['found'].tolist()}"

    def mass_cancel(self, st, ctx):
        mc.assert_removed_equal(self.eng.mass_cancel(st["symbols"], st["sides"]), (st["entries"], st["counts"]), ctx)

    def order_query(self, st, ctx):
        oq.assert_answers_equal(self.eng.order_query(st["seqs"]), st["answers"], ctx)

    def order_preview(self, st, ctx):
        q = st["queries"]
        got = self.eng.order_preview(q[:, 0], q[:, 1], q[:, 2], q[:, 3])
        pv.assert_answers_equal(got, st["answers"], ctx, q)

    def stretch(self, st, ctx):
        me, eng = self.me, self.eng
        batches = [as_batch(me, a) for a in st["batches"]]
        if st["inject_seq0"] is not None:  # the engine's own events become the records
            inj = me.stop_records(self.events, st["inject_seq0"])
            for f in FIELDS:
                assert np.array_equal(getattr(inj, f), getattr(st["batches"][0], f)), f"{ctx}: injected {f}"
            batches[0] = inj
        if st["form"] == "device":
            dbs = [eng.upload(b) for b in batches]
            try:
                for db in dbs:
                    eng.submit_device(db)
                eng.sync()
                assert eng.last_group_size() == len(batches), ctx
                outs = [eng.fetch_group_outputs(k, len(b)) for k, b in enumerate(batches)]
            finally:
                for db in dbs:
                    db.free()
        else:
            def stage(k, b):
                if k == st["mid_at"]:  # in the middle of a launch group: the call cuts it
                    if st["mid"] is None:
                        eng.sync()
                    else:
                        self.step(st["mid"], f"mid-group of {ctx}")
                return b

            outs = pipelined(eng, batches, st["lag"], stage)
        for k, ((res, fills), (mres, mfills)) in enumerate(zip(outs, st["outs"])):
            assert_results_equal(res, mres, f"{ctx} batch {k}")
            assert_fills_equal(fills, mfills, f"{ctx} batch {k}")

    def checkpoint(self, cp, ctx):
        eng = self.eng
        eng.sync()
        for name, drain, stats in (("quotes", eng.quotes_drain, eng.quotes_stats), ("depth", eng.depth_drain, eng.depth_stats),
                                   ("trades", eng.trades_drain, eng.trades_stats)):
            got = drain()
            self.all[name].append(got)
            _by_stamp(got, cp[name], f"{ctx} {cp['tag']}: {name} events")
            s = stats()
            assert (s["deferred"], s["events"]) == (cp["deferred"][name], cp["logged"][name]), (ctx, cp["tag"], name, s)
        self.events = eng.stops_drain()
        _by_stamp(self.events, cp["stops"], f"{ctx} {cp['tag']}: stop events")
        s = eng.stops_stats()  # raises had a stop job ever found its ring full
        assert (s["events"], s["live"]) == (cp["stop_events"], cp["stop_live"]), (ctx, cp["tag"], s)
        _same(eng.stops_dump(), cp["stop_dump"], f"{ctx} {cp['tag']}: stops_dump")
        check_books(eng, cp["books"], f"{ctx} {cp['tag']}")
        # the raw arrays audited clean, and the books rebuilt from raw memory are the model's
        self.run.model, self.run.last_seq = cp["books"], cp["last_seq"]
        self.run.checkpoint(cp["tag"])
        self.run.done()

    def end(self):
        eng, p = self.eng, self.p
        quotes, depth, trades = (np.concatenate(self.all[n]) for n in ("quotes", "depth", "trades"))
        assert qm.same_quotes(qm.replay(qm.tops(qm._Empty(), ss.S), quotes), qm.tops(_Levels(eng, 1), ss.S)), \
            f"{self.ctx}: the quote events replayed are not levels_all(1)"
        assert dm.same_views(dm.replay(dm.empty_maps(ss.S), depth), dm.views(_Levels(eng, ss.D), ss.S, ss.D)), \
            f"{self.ctx}: the depth events replayed are not levels_all({ss.D})"
        tm.replay(trades, p.tapes, ss.S)
        st = eng.stats()
        if p.grouped:
            assert st["handoffs"] > 0, st
        if p.case.path in ("hot", "hot_agg"):
            assert st["hot_handoffs"] > 0, st


@pytest.mark.parametrize("case", ss.PARAMS, ids=[c.id for c in ss.PARAMS])
def test_session(me, case):
    """One session (tests/session.py `cases`): two seeds on each of the seven rows with G = 1 and 4 on the grouped
    ones; the device-group form at G = 8; the feeds' rings at their minimum capacities (gwalk_cx, reg, deep), where
    the plan predicts every deferral and catch-up; a collect lag below the group, whose cuts the plan predicts and
    the feeds' stamps show; a wrapping seq ring under seqs above 2^40. Every comparison runs in every variant."""
    p = ss.plan(case)
    kw = dict(p.engine_kw)
    ring = kw.pop("seq_ring")
    with engine_on(me, case.path, ss.S, p.base, p.stream, ring=ring, group=case.group, **kw) as eng:
        eng.quotes_enable(p.caps["quotes"])
        eng.depth_enable(ss.D, p.caps["depth"])
        eng.trades_enable(p.caps["trades"])
        eng.stops_enable(p.caps["stops"])
        eng.stops_add(p.first_stops)
        r = _Replay(me, eng, p)
        for k, st in enumerate(p.steps):
            r.step(st, k)
        r.end()
