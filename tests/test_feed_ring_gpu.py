"""Both feeds at once on the one event-ring implementation (FeedRing): small rings whose
capacities are neither powers of two nor multiples of a job's event count, so that jobs wrap, defer and
catch up all through a run, under three reading habits. The whole run is planned on the CPU first — the
books against the oracle, the rings against the protocol — and the engine must then reproduce every single
read: its events, its count and what it leaves. Needs an MI355X.
"""
import numpy as np
import pytest

from tests import depth_model as dm
from tests import quote_model as qm
from tests.feed_common import BUY, SELL, Rows, _c5_stream, _same
from tests.gpu_harness import FEED_PATHS as PATHS, feed_engine

pytestmark = pytest.mark.gpu

S, D = 5, 2
QCAP, DCAP = 7, 43  # requested = resolved: 7 >= S, 43 >= 4 * D * S = 40
LAUNCHES = 40
# how launch k is read: HABITS[k % 10]
HABITS = ("all", "three", "all", "three", "all", "all", "three", "skip", "skip", "all")
BASE = np.array([10_000 + 1_000 * s for s in range(S)], dtype=np.int64)


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle

    return oracle


class RingModel:
    """The ring protocol over a feed model (QuoteModel / DepthModel): a job that does not fit
    cap - (tail - consumed) logs nothing and leaves a deferral pending; a read that empties the ring with one
    pending runs one catch-up job, whose events follow in the same read as far as the room goes."""

    def __init__(self, cap, model, dtype):
        self.cap, self.model = cap, model
        self.logged = np.zeros(0, dtype=dtype)
        self.tail = self.consumed = self.jobs = self.deferred = 0
        self.pending = False

    def job(self, stamp):
        self.jobs += 1
        if len(self.model.peek()) <= self.cap - (self.tail - self.consumed):
            self.logged = np.concatenate([self.logged, self.model.expect(stamp)])
            self.tail = len(self.logged)
            self.pending = False
        else:
            self.deferred += 1
            self.pending = True

    def read(self, room, stamp):
        lo = self.consumed
        self.consumed += min(self.tail - self.consumed, room)
        if self.consumed == self.tail and self.pending:
            self.job(stamp)
            assert not self.pending  # (an empty log holds any one job)
            self.consumed += min(self.tail - self.consumed, room - (self.consumed - lo))
        return self.logged[lo:self.consumed], self.tail - self.consumed

    def stats(self):
        return {"groups": self.jobs, "events": self.tail, "deferred": self.deferred}


def _launch_rows(rows, held, k):
    """Launch k: four of the five symbols replace one of their two resting orders per side (the one placed two
    launches of theirs ago) by one at another price and quantity — both sides of most symbols change."""
    for s in range(S):
        if (k + s) % 5 == 0:
            continue
        slot = k % 2
        for side in (BUY, SELL):
            if held[s][side][slot] is not None:
                rows.cancel(s, held[s][side][slot])
        b = int(BASE[s])
        held[s][BUY][slot] = rows.limit(s, BUY, b + 40 + (3 * k + 2 * s) % 7, 1 + (k + s) % 4)
        held[s][SELL][slot] = rows.limit(s, SELL, b + 60 + (5 * k + s) % 7, 1 + (2 * k + s) % 3)


def plan(me, orc):
    """The run on the CPU: (batches, per launch the reads [(feed, room, events, left)], the two ring models).
    `room` None is a drain: reads of the default room until nothing is left."""
    ob = orc.OracleBook(S)
    rings = {"quotes": RingModel(QCAP, qm.QuoteModel(ob, S), qm.QUOTE_DTYPE),
             "depth": RingModel(DCAP, dm.DepthModel(ob, S, D), dm.DEPTH_DTYPE)}
    default_room = {"quotes": S, "depth": 4 * D * S}
    for r in rings.values():
        r.job(0)  # enabling: the empty books
    rows = Rows(me)
    held = [{BUY: [None, None], SELL: [None, None]} for _ in range(S)]
    batches, reads = [], []
    for k in range(1, LAUNCHES + 1):
        _launch_rows(rows, held, k)
        b = rows.batch()
        batches.append(b)
        ob.submit(b)
        habit = HABITS[k % len(HABITS)] if k < LAUNCHES else "all"  # (the run ends with a drain)
        now = []
        for name, r in rings.items():
            r.job(k)
            if habit == "three":
                now.append((name, 3) + r.read(3, k))
            elif habit == "all":
                while True:
                    ev, left = r.read(default_room[name], k)
                    now.append((name, None, ev, left))
                    if not left:
                        break
        reads.append(now)
    return batches, reads, rings


@pytest.fixture(scope="module")
def planned(me, orc):
    return plan(me, orc)


def test_plan_defers_and_wraps(planned):
    """The script's own figures, fixed before the engine runs. Each feed runs 41 jobs behind enable and the 40
    launches and 4 catch-up jobs; each ring defers 8 jobs (at least once, at most 10: most jobs log). The 148
    quote events wrap the ring of 7 21 times, the 620 depth events the ring of 43 14 times; all 12 reads into
    a 3-event buffer leave something unread."""
    _, reads, rings = planned
    q, d = rings["quotes"], rings["depth"]
    assert (q.deferred, q.jobs, q.tail, q.tail // QCAP) == (8, 45, 148, 21)
    assert (d.deferred, d.jobs, d.tail, d.tail // DCAP) == (8, 45, 620, 14)
    for r in rings.values():
        assert 1 <= r.deferred <= 10 and r.tail // r.cap >= 3 and r.consumed == r.tail and not r.pending
    for name in rings:
        assert any(n == name and room == 3 and left > 0 for now in reads for n, room, _, left in now)


@pytest.mark.parametrize("path", ["reg", "deep"])
def test_both_feeds_wrap_defer_and_catch_up(me, planned, path):
    """40 single-batch launches with both feeds on (quote ring 7, depth ring 43 = the floor of 40 and 3), read
    in turn whole, into a 3-event buffer, and not at all for two launches: 8 deferrals per feed, 21 wraps of
    the quote ring and 14 of the depth ring (test_plan_defers_and_wraps). Every read returns the planned
    events, count and `left`; so the concatenation of everything read is the model's events with the deferred
    launches conflated into their catch-up jobs; the counters agree with the plan."""
    batches, reads, rings = planned
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with feed_engine(me, path, S, BASE, max(len(b) for b in batches), 64 * S, **kw) as eng:
        eng.quotes_enable(QCAP)
        eng.depth_enable(D, DCAP)
        read = {"quotes": eng.quotes_read, "depth": eng.depth_read}
        stats = {"quotes": eng.quotes_stats, "depth": eng.depth_stats}
        got = {"quotes": [np.zeros(0, dtype=qm.QUOTE_DTYPE)], "depth": [np.zeros(0, dtype=dm.DEPTH_DTYPE)]}
        for k, (b, now) in enumerate(zip(batches, reads), 1):
            eng.submit_batch(b)
            for name, room, exp, exp_left in now:
                ev, left = read[name]() if room is None else read[name](room)
                _same(ev, exp, f"{path} launch {k} {name} read({room})")
                assert left == exp_left, f"{path} launch {k} {name} read({room}): left {left}, planned {exp_left}"
                got[name].append(ev)
        for name, r in rings.items():
            all_read = np.concatenate(got[name])
            _same(all_read, r.logged, f"{path} {name}: everything read")
            st = stats[name]()
            assert st["events"] == len(all_read), st
            assert 1 <= st["deferred"] <= 10, st
            assert st["events"] // r.cap >= 3, st
            assert st == r.stats(), (st, r.stats())
            assert len(read[name]()[0]) == 0  # drained
        assert qm.same_quotes(qm.replay(qm.tops(qm._Empty(), S), np.concatenate(got["quotes"])), qm.tops(eng, S))
        assert dm.same_views(dm.replay(dm.empty_maps(S), np.concatenate(got["depth"])), dm.views(eng, S, D))


@pytest.mark.parametrize("path", ["reg", "deep"])
def test_reenable_one_feed_beside_the_other(me, orc, path):
    """Each feed is disabled and re-enabled with another capacity mid-stream while the other stays on: the
    first read after re-enabling holds the whole current state, and the feed that stayed on goes on exactly
    where it was."""
    S, L, D = 65, PATHS[path][0], 3
    base, batches = _c5_stream(me, S, L, 5, 300)
    ob = orc.OracleBook(S)
    with feed_engine(me, path, S, base, 300, 4096) as eng:
        def step(k):
            eng.submit_batch(batches[k])
            ob.submit(batches[k])

        step(0)
        eng.quotes_enable(4 * S)
        eng.depth_enable(D, 8 * D * S)
        qmod, dmod = qm.QuoteModel(ob, S), dm.DepthModel(ob, S, D)
        _same(eng.quotes_drain(), qmod.expect(1), "quotes: first read")
        _same(eng.depth_drain(), dmod.expect(1), "depth: first read")
        step(1)
        dexp = [dmod.expect(2)]  # (the depth job behind this batch: read later, modelled now)
        # the quote feed goes off and comes back with another ring; the depth feed stays on
        eng.quotes_enable(0)
        with pytest.raises(me.EngineError) as ei:
            eng.quotes_read()
        assert ei.value.code == me.ME_E_INVALID
        step(2)
        dexp.append(dmod.expect(3))
        eng.quotes_enable(2 * S + 3)
        qmod = qm.QuoteModel(ob, S)
        exp = qmod.expect(3)
        assert 0 < len(exp) <= S and exp["flags"].all()  # exactly the non-empty symbols
        _same(eng.quotes_drain(), exp, "quotes: first read after re-enabling")
        assert eng.quotes_stats() == {"groups": 1, "events": len(exp), "deferred": 0}
        _same(eng.depth_drain(), np.concatenate(dexp), "depth: beside it")
        assert eng.depth_stats()["groups"] == 3 and eng.depth_stats()["deferred"] == 0
        step(3)
        # and the other way round, at another depth
        eng.depth_enable(0, 0)
        with pytest.raises(me.EngineError) as ei:
            eng.depth_read()
        assert ei.value.code == me.ME_E_INVALID
        eng.depth_enable(2, 4 * 2 * S + 5)
        dmod = dm.DepthModel(ob, S, 2)
        exp = dmod.expect(4)
        vw = dm.views(ob, S, 2)
        assert 0 < len(exp) == sum(len(v[0]) + len(v[1]) for v in vw) and (exp["qty"] > 0).all()
        _same(eng.depth_drain(), exp, "depth: first read after re-enabling")
        assert eng.depth_stats() == {"groups": 1, "events": len(exp), "deferred": 0}
        _same(eng.quotes_drain(), qmod.expect(4), "quotes: beside it")
        step(4)
        _same(eng.quotes_drain(), qmod.expect(5), "quotes: the batch after")
        _same(eng.depth_drain(), dmod.expect(5), "depth: the batch after")
        assert eng.quotes_stats()["deferred"] == 0 and eng.depth_stats()["deferred"] == 0
