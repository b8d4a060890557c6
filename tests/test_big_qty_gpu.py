"""Quantities up to INT32_MAX and book sums past 2^31 and 2^32 on every matching path ("quantity
widths") against the model (tests/reduce_model.py, arbitrary-precision ints). Needs an MI355X. Bit-exact.

Every case checks each batch's results and tape, all books, the resting counters, the snapshot's int64 level
totals and the auditor's invariants over the raw device arrays. The inputs are tests/big_qty.py's; that they
reach the widths they are meant to reach is asserted on the CPU (tests/test_big_qty_model.py).
"""
import numpy as np
import pytest

from tests import big_qty as bq
from tests import depth_model as dm
from tests import quote_model as qm
from tests._parity import assert_books_equal, assert_fills_equal, assert_results_equal
from tests.book_audit import audit, names
from tests.gpu_harness import PATHS, as_batch, engine_on, pipelined
from tests.reduce_model import ReduceBook

pytestmark = pytest.mark.gpu

SELL = 2
RING = 1 << 16  # above every seq of these tests: no slot is reused


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _check_all(eng, model, last_seq, ctx):
    """Books, counters, snapshot totals and the raw arrays' invariants."""
    S = eng.num_symbols
    assert_books_equal(eng, model, range(S), ctx)
    assert eng.resting_count() == eng.admission()["resting"] == model.resting(), f"{ctx}: resting counters"
    for s in range(S):
        for side, got, want in zip("ba", eng.snapshot(s, 10), bq.model_snapshot(model, s, 10)):
            assert got["total_qty"].dtype == np.int64
            for f in ("price_q4", "total_qty", "order_count"):
                assert np.array_equal(got[f], want[f]), f"{ctx}: snapshot {side} of symbol {s}: {f} {got[f]} != {want[f]}"
    v, _ = audit(eng.debug_export(), last_seq=last_seq)
    assert not v, f"{ctx}: {len(v)} violations {names(v)}; first {v[:4]}"


def _last_seq(arrays):
    return max(int(a.seq.max()) for a in arrays)


def _run_groups(me, eng, model, groups, ctx, grouped):
    """Launch group after launch group (host batches, collected before the next group starts); everything is
    checked after each. Yields the group's index after its checks."""
    last = 0
    for g, arrays in enumerate(groups):
        bs = [as_batch(me, a) for a in arrays]
        if grouped:
            tickets = [eng.submit_host(b) for b in bs]
            outs = [eng.collect(t) for t in tickets]
        else:
            outs = [eng.submit_batch(b) for b in bs]
        for k, (a, (r, f)) in enumerate(zip(arrays, outs)):
            ro, fo = model.submit(a)
            assert_results_equal(r, ro, f"{ctx} group {g} batch {k}")
            assert_fills_equal(f, fo, f"{ctx} group {g} batch {k}")
        last = max(last, _last_seq(arrays))
        _check_all(eng, model, last, f"{ctx} group {g}")
        yield g


def _run_case(me, path, case, ctx, group=1):
    """A directed case, one batch per launch group; returns the engine's stats."""
    grouped = PATHS[path][3]
    kw = {"batches_per_launch": group} if grouped else {}
    model = ReduceBook(case.S)
    with engine_on(me, path, case.S, case.base, case.batches, ring=RING, **kw) as eng:
        for _ in _run_groups(me, eng, model, [[a] for a in case.batches], ctx, grouped):
            pass
        return eng.stats()


# ---- 1. stream parity --------------------------------------------------------------------------------------------

STREAM_CASES = [(p, n, m) for p in PATHS for n in bq.PATH_STREAMS[p]
                for m in (("sync", "pipelined") if PATHS[p][3] else ("sync",))]


@pytest.mark.parametrize("path,name,mode", STREAM_CASES)
def test_stream_parity(me, path, name, mode):
    """big_stream on every path. Grouped paths: one batch per launch with every check after each launch, and
    pipelined host batches in full groups of four. Deep and hot paths: synchronous batches, every check after
    each. The walks must have handed symbols off (LW_CAP, and the records they do not cover)."""
    seed, S, L, nb, n, group, kw = bq.STREAMS[name]
    assert L == PATHS[path][0]
    base, arrays, exp, final = bq.stream(name)
    ctx = f"{name} {path} {mode}"
    grouped = PATHS[path][3]
    if mode == "pipelined":
        batches = [as_batch(me, a) for a in arrays]
        with engine_on(me, path, S, base, arrays, ring=RING, batches_per_launch=group) as eng:
            outs = pipelined(eng, batches, 2 * group + 1)
            for k, (ro, fo) in enumerate(exp):
                assert_results_equal(outs[k][0], ro, f"{ctx} batch {k}")
                assert_fills_equal(outs[k][1], fo, f"{ctx} batch {k}")
            _check_all(eng, final, _last_seq(arrays), ctx)
            stats = eng.stats()
    else:
        model = ReduceBook(S)
        ekw = {"batches_per_launch": 1} if grouped else {}
        with engine_on(me, path, S, base, arrays, ring=RING, **ekw) as eng:
            for _ in _run_groups(me, eng, model, [[a] for a in arrays], ctx, grouped):
                pass
            stats = eng.stats()
    if path in ("hot_agg", "hot"):
        assert stats["hot_handoffs"] > 0, stats
    if path in ("gwalk", "gwalk_cx"):
        assert stats["handoffs"] > 0, stats


def test_gwalk_handoffs_are_lw_caps(me):
    """The control: the stream's GTC LIMITs and MARKETs priced inside the window, no cancels — records the plain
    grouped walk covers whatever their order. With every quantity replaced by 1 + q % 60 no symbol is handed off;
    the same records with their quantities are: those hand-offs are LW_CAP's (`lok`, `adm`)."""
    seed, S, L, nb, n, group, kw = bq.STREAMS["grouped"]
    base, arrays, _, _ = bq.stream("grouped")
    runs = {"small": bq.plain_subset(arrays, map_qty=lambda q: 1 + q % 60, far_free=(base, L)),
            "large": bq.plain_subset(arrays, far_free=(base, L))}
    hand = {}
    for tag, sub in runs.items():
        model = ReduceBook(S)
        groups = [sub[i:i + group] for i in range(0, len(sub), group)]
        with engine_on(me, "gwalk", S, base, sub, ring=RING, batches_per_launch=group) as eng:
            for _ in _run_groups(me, eng, model, groups, f"control {tag}", True):
                pass
            hand[tag] = eng.stats()["handoffs"]
    assert hand["small"] == 0 and hand["large"] > 0, hand


# ---- 2. saturating chunk ranking ---------------------------------------------------------------------------------

@pytest.mark.parametrize("one_batch", [False, True], ids=["own_batches", "one_batch"])
@pytest.mark.parametrize("nmakers", [16, 33])
@pytest.mark.parametrize("where", ["reg", "hot", "far"])
def test_saturating_chunk_ranking(me, where, nmakers, one_batch):
    """scan16_sat (me_wave.hpp) with prefixes at 2^32 - 1: the chunk take of k_match_reg (me_match_reg.hip), of
    the hot kernel (me_kernels.hip) and of a far level (me_far.hpp) — `ex = inc - uq`,
    `f = min(max(rem - ex, 0), uq)` stay exact because rem <= 2^31 - 1 < 2^32 - 1 - uq. Every pattern of
    big_qty.PATTERNS; each taker's (maker, quantity) list and the books after every batch against the model
    (whose own lists tests/test_big_qty_model.py pins by hand)."""
    path = "hot" if where == "hot" else "reg"
    for pattern in bq.PATTERNS:
        case = bq.chunk_case(where, pattern, nmakers, one_batch)
        stats = _run_case(me, path, case, f"chunk {where} {pattern} n={nmakers}")
        if where == "hot":  # the FOK left the hot kernel; the other takers ran on it
            assert stats["hot_handoffs"] >= 1


# ---- 3. LW_CAP ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["gwalk", "gwalk_cx", "hot_agg"])
def test_lw_cap_edges(me, path):
    """`w.ub < LW_CAP` (me_agg.hip: lw_init, lw_admit, and `lw.ub += qsum; adm = lw.ub < LW_CAP` in
    k_agg_gwalk) at 2^31 - 1 and 2^31: at a group's start, in a batch's second block, in a group's third batch
    (the bound, not the true sum, decides), with quantities that do not count (gw_prepare's clamp of a negative
    qty; a cancel's ignored field, 0 on the cancel walk), and back on the walk once takers drained the book.
    The hand-offs each group must add are big_qty.lw_cases' — derived there from those comparisons, checked
    against the scripts' sums in tests/test_big_qty_model.py — not observed ones."""
    L, base, cases = bq.lw_cases(path)
    assert L == PATHS[path][0]
    counter = "hot_handoffs" if path == "hot_agg" else "handoffs"
    for name, (G, groups) in cases.items():
        arrays = [a for g in groups for a in g[0]]
        kw = {"batches_per_launch": G} if PATHS[path][3] else {}
        model = ReduceBook(1)
        with engine_on(me, path, 1, base, arrays, ring=RING, **kw) as eng:
            seen = 0
            for g in _run_groups(me, eng, model, [x[0] for x in groups], f"LW_CAP {path} {name}", PATHS[path][3]):
                now = eng.stats()[counter]
                assert now - seen == groups[g][1], f"{path} {name} group {g}: {now - seen} hand-offs; {groups[g][2]}"
                seen = now


# ---- 4. FOK across 2^31 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["reg", "deep", "hot"])
def test_fok_across_2_31(me, path):
    """fok_fillable's running sum (me_kernels.hip; k_match_reg's twin) over window levels and far levels of
    INT32_MAX each: exactly enough, one lot too little (killed: the book byte-identical), more than 2^32 within
    the limit, and MARKET FOKs that need the far levels. big_qty.fok_case lists the steps."""
    case = bq.fok_case(PATHS[path][0], hot=path == "hot")
    grouped = PATHS[path][3]
    kw = {"batches_per_launch": 1} if grouped else {}
    model = ReduceBook(case.S)
    with engine_on(me, path, case.S, case.base, case.batches, ring=RING, **kw) as eng:
        before = None
        for g in _run_groups(me, eng, model, [[a] for a in case.batches], f"FOK {path}", grouped):
            now = [eng.dump(s) for s in range(case.S)]
            if g - 1 in case.killed:
                pads = case.pad * 2
                assert all(len(a) == len(b) + (pads if s == 0 else 0) for s, (a, b) in enumerate(zip(now, before)))
                asks = [d[d["side"] == SELL] for d in (now[0], before[0])]
                assert asks[0].tobytes() == asks[1].tobytes(), f"FOK {path}: a killed FOK changed the asks (step {g - 1})"
                if not pads:
                    assert now[0].tobytes() == before[0].tobytes()
            before = now


# ---- 5. REDUCE at width ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["reg", "deep"])
def test_reduce_at_width(me, path):
    """A target of INT32_MAX reduced by INT32_MAX - 1 (one lot rests, its place kept), by INT32_MAX (a cancel), and
    one behind more than 2^33 of queue reduced by 2^31 - 2 (big_qty.reduce_case)."""
    case = bq.reduce_case(PATHS[path][0])
    _run_case(me, path, case, f"REDUCE {path}")


# ---- 6. the feeds ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", list(bq.FEEDS))
def test_feeds_at_width(me, path):
    """The quote feed and the depth feed (D = 8) beside a big_stream run in launches of 256 / 300 records, rings
    large enough that nothing defers: the replayed int64 quantities equal the model's best-level totals and top-8
    totals after every launch (which pass 2^32: tests/test_big_qty_model.py)."""
    name, step = bq.FEEDS[path]
    seed, S, L, nb, n, group, kw = bq.STREAMS[name]
    base = bq.stream(name)[0]
    arrays = bq.slices(bq.stream(name)[1], step)
    D = 8
    model = ReduceBook(S)
    view = bq.Snap(model)
    ekw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with engine_on(me, path, S, base, arrays, ring=RING, **ekw) as eng:
        eng.quotes_enable(4 * S * (len(arrays) + 2))
        eng.depth_enable(D, 8 * D * S * (len(arrays) + 2))
        table, maps = qm.tops(qm._Empty(), S), dm.empty_maps(S)
        big = 0
        for k, a in enumerate(arrays):
            r, f = eng.submit_batch(as_batch(me, a))
            ro, fo = model.submit(a)
            assert_results_equal(r, ro, f"feeds {path} batch {k}")
            assert_fills_equal(f, fo, f"feeds {path} batch {k}")
            eng.sync()
            qm.replay(table, eng.quotes_drain())
            dm.replay(maps, eng.depth_drain())
            want = qm.tops(view, S)
            assert qm.same_quotes(table, want), f"feeds {path}: quotes after batch {k}"
            assert dm.same_views(maps, dm.views(view, S, D)), f"feeds {path}: depth views after batch {k}"
            big += int((want["bid_qty"] > 1 << 32).sum() + (want["ask_qty"] > 1 << 32).sum())
        assert big > 0
        assert eng.quotes_stats()["deferred"] == 0 and eng.depth_stats()["deferred"] == 0
        _check_all(eng, model, _last_seq(arrays), f"feeds {path}")
