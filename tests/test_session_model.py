"""The composed sessions' plans on the CPU (tests/session.py): no engine. The plans are the same
objects tests/test_session_gpu.py replays (session.PARAMS, session.plan is cached): what is asserted here about
their reach holds for the GPU run."""
import numpy as np
import pytest

from tests import session as ss
from tests import stops_model as sm
from tests.reduce_model import check_seq_rule
from tests.tif_model import kind

BUY, SELL = 1, 2
IDS = [c.id for c in ss.PARAMS]

# what is counted -> the floor per session
FLOORS = {"stop_events": 20, "stop_jobs": 4, "inj_fill": 10, "inj_rest": 3, "cascade": 1, "refused": 1,
          "cancelled_live": 3, "purges": 2, "purged_orders": 20, "fok_kill": 10, "post_reject": 10,
          "reduce_partial": 10, "reduce_cover": 10, "bad": 10, "all_three": 3}


def shortfalls(p):
    """The floors a plan misses, as (name, count, floor)."""
    cn, out = p.counts, []
    want = dict(FLOORS)
    if p.knobs["far_pct"] > 0:
        want["purged_far"] = 1
    if p.case.variant == "lagcut":
        want["cuts"] = 2
    for name, floor in want.items():
        if cn[name] < floor:
            out.append((name, cn[name], floor))
    if p.case.variant == "tight":
        last = [s for s in p.steps if s["op"] == "checkpoint"][-1]
        out += [(f"deferred {n}", v, 1) for n, v in last["deferred"].items() if v < 1]
    return out


@pytest.mark.parametrize("case", ss.PARAMS, ids=IDS)
def test_floors(case):
    """Counted from the models alone, for every case the GPU suite runs."""
    p = ss.plan(case)
    assert not shortfalls(p), (case.id, shortfalls(p), p.counts)
    last = [s for s in p.steps if s["op"] == "checkpoint"][-1]
    if case.variant != "tight":  # ample rings: nothing defers
        assert not any(last["deferred"].values()), last["deferred"]
    assert 8 <= p.counts["launches"]
    if p.grouped and case.group >= 2 and case.variant != "device":
        assert p.counts["mid_adds"] >= 1 and p.counts["mid_purges"] >= 1, p.counts
    cuts = [s for s in p.steps if s["op"] == "stretch" and any(len(g) < case.group for g in s["launches"][:-1])]
    if case.variant == "lagcut":
        assert len(cuts) >= 2  # the feeds' stamps show them: launches shorter than the group in mid-stretch


@pytest.mark.parametrize("case", ss.PARAMS, ids=IDS)
def test_plan_is_deterministic_and_its_stream_is_valid(case):
    p = ss.plan(case)
    if ss.PARAMS.index(case) % 4 == 0:  # (planned a second time: every fourth case, the others cost the same again)
        q = ss.plan.__wrapped__(case)
        assert q is not p and ss.diff(p, q) is None
        assert p.engine_kw == q.engine_kw and p.counts == q.counts
    check_seq_rule(p.stream)
    ring = p.engine_kw["seq_ring"]
    assert ring & (ring - 1) == 0 and all(2 * s <= ring for s in p.spans), (ring, max(p.spans))
    if p.knobs["small_ring"]:  # the smallest such ring (below four spans: eight or more launches wrap it twice over)
        assert ring < 4 * max(p.spans)
        seqs = np.concatenate([b.seq[b.seq != 0] for b in p.stream])
        assert (int(seqs.max()) - int(seqs.min())) // ring >= 2
    # every batch is in the plan once, the stretches' outputs are the models' and the tapes line up
    n = sum(len(s["batches"]) for s in p.steps if s["op"] == "stretch")
    assert n == len(p.stream) == len(p.tapes)
    k = 0
    for s in p.steps:
        if s["op"] == "stretch":
            assert sorted(x for g in s["launches"] for x in g) == list(range(len(s["batches"])))
            for b, (res, fills) in zip(s["batches"], s["outs"]):
                assert b is p.stream[k] and fills is p.tapes[k]
                k += 1


def test_an_injected_record_is_its_event():
    """me.stop_records against a hand case: kind / limit_px_q4 / qty / symbol of the event, seqs from seq0."""
    from matching_engine_amd import stop_records

    ev = np.zeros(3, dtype=sm.STOP_EVENT_DTYPE)
    rows = [(7, 1_000, 990, 1_004, 5, 2, kind(SELL)), (9, 2_000, 0, 2_000, 11, 0, kind(BUY, 1)),
            (12, -5, -(1 << 63), -5, 3, 15, kind(BUY, 0, 0, 1))]
    for e, r in zip(ev, rows):
        e["id"], e["stop_px_q4"], e["limit_px_q4"], e["trigger_px_q4"], e["qty"], e["symbol"], e["kind"] = r
    b = stop_records(ev, (1 << 40) + 5)
    assert b.seq.tolist() == [(1 << 40) + 5, (1 << 40) + 6, (1 << 40) + 7]
    assert b.price_q4.tolist() == [990, 0, -(1 << 63)] and b.qty.tolist() == [5, 11, 3]
    assert b.symbol.tolist() == [2, 0, 15] and b.kind.tolist() == [kind(SELL), kind(BUY, 1), kind(BUY, 0, 0, 1)]
    # and in a plan: every injected batch is stop_records of the events drained at the checkpoint before it
    p = ss.plan(ss.PARAMS[0])
    seen, prev = 0, None
    for s in p.steps:
        if s["op"] == "checkpoint":
            prev = s["stops"]
        elif s["op"] == "stretch" and s["inject_seq0"] is not None:
            want, got = stop_records(prev, s["inject_seq0"]), s["batches"][0]
            for f in ("seq", "price_q4", "qty", "symbol", "kind"):
                assert np.array_equal(getattr(got, f), getattr(want, f)), f
            seen += 1
    assert seen >= 2


# the cases the wrong compositions are run on: a grouped row at G = 4 (the mid-group add), groups of one, a deep row
WRONG_ON = [c for c in ss.PARAMS if c.id in ("gwalk_cx-G4-host-s0", "reg-G4-host-s1", "gwalk-G1-host-s0",
                                             "deep-G1-host-s1", "reg-G4-lagcut-s30")]
assert len(WRONG_ON) == 5


@pytest.mark.parametrize("case", WRONG_ON, ids=[c.id for c in WRONG_ON])
@pytest.mark.parametrize("wrong", ss.WRONG)
def test_a_wrong_composition_changes_the_expected_outputs(case, wrong):
    """Four deliberately wrong compositions; each changes what the plan expects, and where it does first is
    named: (a) stops judged against a whole stretch's extremes instead of each launch's; (b) a stop that sees the
    fills of batches submitted before its add (the mid-group add); (c) a purge that clears the purged symbols'
    stops; (d) an injected stop-limit priced at stop_px_q4 instead of limit_px_q4."""
    right = ss.plan(case)
    if wrong == "add_sees_earlier_fills" and not right.counts["mid_adds"]:
        assert not right.grouped or case.group < 2  # nothing it can affect: no launch is cut by an add
        assert ss.diff(right, ss.plan(case, wrong)) is None
        return
    what = ss.diff(right, ss.plan(case, wrong))
    assert what is not None, f"{case.id}: the plan does not tell {wrong} from the right composition"
    expect = {"stretch_extremes": ("checkpoint", ": stops"),
              "add_sees_earlier_fills": ("checkpoint", ": stops"),
              "purge_clears_stops": ("checkpoint", ": stop"),
              "inject_at_stop_px": ("batch 0 price_q4 (injected)",)}[wrong]
    assert all(x in what for x in expect), f"{case.id}: {wrong} first shows in {what}"
