"""The order-preview model (tests/preview_model.py) against the matching models themselves. No GPU.

preview_model.expected is computed from model.dump(s) alone, with the time-in-force rules restated from DESIGN.md
§2. Here every answer is checked against what a deep copy of the model gives the same record when it is submitted
as the next record of the stream: the five result fields, the fold of its fills, and RESTS against the dump
afterwards. The books and query sets are those of tests/preview_cases.py, which the GPU test runs through the
engine; the last test asserts that they hold at least one answer of every kind the GPU test relies on.
"""
import copy

import numpy as np
import pytest

from tests import preview_cases as pc
from tests import preview_model as pm
from tests.reduce_model import ReduceBook

SEEN = {}  # case name -> the tags its answers showed (filled by test_cases, read by test_coverage)


def _check_against_submit(model, S, queries, exp, seq, ctx):
    for i, q in enumerate(queries):
        m = copy.deepcopy(model)
        res, fills = m.submit(pc.one(seq, q))
        row, c = exp[i], f"{ctx} query {i} {tuple(int(x) for x in q)}"
        pm.assert_matches_submit(row, res[0], fills, c)
        rests = bool(int(row["flags"]) & pm.PV_RESTS)
        in_dump = int(q[0]) < S and seq in set(m.dump(int(q[0]))["seq"].tolist())
        assert rests == in_dump, f"{c}: RESTS {rests}, in the dump afterwards {in_dump}"
        if not int(row["fill_count"]):
            assert not any(int(row[f]) for f in ("filled_qty", "levels", "first_price_q4", "last_price_q4", "notional_hi",
                                                 "notional_lo")), f"{c}: no fill, execution fields {row}"
        else:
            assert int(row["first_price_q4"]) == int(row["opp_price_q4"]), c
        if int(row["status"]) == pm.ST_REJECTED and int(row["reason"]) != pm.RJ_WOULD_CROSS:
            assert not int(row["flags"]) and not int(row["opp_price_q4"]), c


def _run(case, stride=1):
    """The case through a ReduceBook; every stride-th query behind every batch is checked against the submit."""
    model = ReduceBook(case.S)
    seen = set()
    for k, a in enumerate(case.batches):
        model.submit(a)
        queries = case.queries(model, k)
        exp = pm.expected(model, case.S, queries)
        ctx = f"{case.name} batch {k}"
        _check_against_submit(model, case.S, queries[::stride], exp[::stride], case.free[k], ctx)
        lv = {}
        for q, row in zip(queries, exp):
            s = int(q[0])
            if s < case.S:
                if s not in lv:
                    lv[s] = pm.levels_of(model, s)
                seen |= pc.tags(lv[s], q, row, case.window if k == 0 else None)  # (a real record may move a window)
        model.submit(pc.one(case.free[k], queries[case.real(k, exp)]))
    SEEN[case.name] = seen
    return seen


CASES = {c.name: c for c in pc.scripted(128) + [pc.seeded(128)]}


@pytest.mark.parametrize("name", list(CASES))
def test_cases(name):
    _run(CASES[name])


@pytest.mark.parametrize("L", pc.LS[1:])
def test_cases_at_the_deeper_windows(L):
    """The same scripts at the other window depths (the prices move with L): a sample of the queries each."""
    for c in pc.scripted(L) + [pc.seeded(L)]:
        _run(c, stride=7)


def test_notional_halves():
    for v in (0, 1, -1, 1 << 94, -(1 << 94), (1 << 127) - 1, -(1 << 127), (1 << 64) - 1, -(1 << 64)):
        hi, lo = pm.split128(v)
        row = np.zeros(1, dtype=pm.PREVIEW_DTYPE)[0]
        row["notional_hi"], row["notional_lo"] = hi, lo
        assert pm.notional(row) == v


WANT = {
    "chunks": {"partial", "boundary", "fok_killed", "fok_filled", "would_cross", "post_rests", "between"},
    "order": {"partial", "boundary", "between", "fok_killed", "fok_filled"},
    "far": {"reaches_far", "far_only", "between", "partial", "boundary", "fok_killed", "fok_filled", "would_cross"},
    "wide": {"partial", "boundary", "fok_killed", "fok_filled"},
    "fok": {"fok_killed", "fok_filled", "partial"},
    "clamps_min": {"neg_notional", "big_notional", "fok_killed", "fok_filled", "would_cross", "post_rests"},
    "mixed": {"would_cross", "post_rests", "fok_killed", "fok_filled", "partial", "boundary"},
    "seeded": {"partial", "fok_killed", "would_cross", "post_rests"},
}


@pytest.mark.parametrize("L", pc.LS)
def test_coverage(L):
    """The GPU tests cannot pass vacuously: at every window depth the cases' answers hold every kind."""
    for c in pc.scripted(L) + [pc.seeded(L)]:
        if c.name not in SEEN:
            _run(c, stride=10 ** 9)
    for prefix, want in WANT.items():
        got = set().union(*[t for n, t in SEEN.items() if n.startswith(prefix) and n.endswith(str(L)) or
                            n.startswith(f"{prefix}{L}")])
        assert want <= got, f"{prefix} at L={L}: no answer of kind {sorted(want - got)}"
