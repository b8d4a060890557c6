"""Cancels that name hostile targets, on every matching path (needs an MI355X).

The streams of tests/cancel_targets.py (another symbol's order, a second cancel, the seq of a MARKET / IOC / FOK /
rejected / filled record, a seq not issued yet, the cancel's own seq, seq-ring aliases, 0 and seqs above 2^63)
against the reference books tests/test_cancel_targets_model.py pins on the CPU: every batch's results and tape,
every book and the resting counters. The three target lookups (cancel_order in me_kernels.hip, its twin in
me_match_reg.hip, gw_pre_target and the CX_TAG route in me_agg.hip) must all give the reference's answer.

Then the hand-off limits of the grouped cancel walk (me_agg.hip), each from both sides.
"""
import numpy as np
import pytest

from tests import cancel_targets as ct
from tests import tif_model as tm
from tests._parity import assert_books_equal, assert_fills_equal, assert_results_equal
from tests.gpu_harness import FEED_PATHS as PATHS, SMALL, as_batch, engine_on, pipelined
from tests.tif_model import TifBook, kind

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
ST_NEW, ST_PARTIAL, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
S = ct.S_CX


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle

    return oracle


def _check(eng, model, outs, exp, ctx):
    for k, (ro, fo) in enumerate(exp):
        assert_results_equal(outs[k][0], ro, f"{ctx} batch {k}")
        assert_fills_equal(outs[k][1], fo, f"{ctx} batch {k}")
    assert_books_equal(eng, model, range(eng.num_symbols), ctx)
    assert eng.resting_count() == eng.admission()["resting"] == len(model.live), f"{ctx}: resting counters"


def _run_case(me, name, path, group, device=False):
    c = ct.CASES[name]
    assert PATHS[path][0] == c.levels
    base, arrays, _, _ = ct.stream(name)
    exp, _, model = ct.expected(name)
    batches = [as_batch(me, a) for a in arrays]
    ctx = f"{name} {path} G={group}{' device' if device else ''}"
    grouped = PATHS[path][3]
    kw = {"batches_per_launch": group} if grouped else {}
    if device:  # (every record of a device batch counts as one that may rest)
        kw["max_resting"] = 2 * sum(len(b) for b in batches) + 1024
    with engine_on(me, path, S, base, batches, table=PATHS, ring=c.ring, **kw) as eng:
        if device:
            dbs = [eng.upload(b) for b in batches]
            try:
                for db in dbs:
                    eng.submit_device(db)
                eng.sync()
                assert eng.last_group_size() == len(batches) == group
                outs = [eng.fetch_group_outputs(k, len(b)) for k, b in enumerate(batches)]
            finally:
                for db in dbs:
                    db.free()
        elif grouped:
            outs = pipelined(eng, batches, 2 * group + 1)
        else:
            outs = [eng.submit_batch(b) for b in batches]
        _check(eng, model, outs, exp, ctx)
        return eng.stats()


def _case_of(path, variant):
    return f"l{PATHS[path][0]}_{variant}"


# ---- every path, every class ------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["tif", "plain"])
@pytest.mark.parametrize("path,group", [(p, g) for p in SMALL for g in (1, 8, 32)] + [(p, 1) for p in PATHS if p not in SMALL])
def test_hostile_targets_on_every_path(me, path, group, variant):
    """Pipelined host batches in launch groups of G (L = 128) or synchronous batches (the deep and hot paths);
    2 % of the LIMITs are far, so some targets sit on far levels and move when a window re-centres."""
    _run_case(me, _case_of(path, variant), path, group)


@pytest.mark.parametrize("variant", ["tif", "plain"])
@pytest.mark.parametrize("path", SMALL)
def test_hostile_targets_in_one_device_group(me, path, variant):
    """All eight batches enqueued as device batches before one sync: one launch group, so the future targets
    that cross a batch boundary stay inside the group (the order named must rest untouched)."""
    _run_case(me, _case_of(path, variant), path, 8, device=True)


@pytest.mark.parametrize("variant", ["tif", "plain"])
@pytest.mark.parametrize("path", SMALL + ("deep",))
def test_hostile_targets_small_ring(me, path, variant):
    """A 1,024-entry seq ring that wraps more than five times under seqs above 2^40: the aliases T +- k * 1,024
    fall on the ring slot of a live order, and cancels of orders more than a ring old go through the
    old-order table. L = 128: groups of four 200-record batches (fewer than 1,024 seqs); deep: 800-record batches."""
    name = f"ring{PATHS[path][0]}_{variant}"
    assert ct.CASES[name].ring == 1024
    _run_case(me, name, path, 4 if PATHS[path][3] else 1)


@pytest.mark.parametrize("name,group,device", [("walk128_plain", 8, False), ("walk128_plain", 8, True),
                                               ("walkring128_plain", 4, False)])
@pytest.mark.parametrize("path", SMALL)
def test_hostile_targets_the_walk_keeps(me, path, name, group, device):
    """The streams above hand most symbols to the continuation somewhere in a group (a far LIMIT, a FOK or
    POST_ONLY, more than 128 records of the hot symbol). These two carry none of that, so on the cancel walk the
    walk's own lookups (the CX_TAG route for this group's orders, gw_pre_target for older ones) answer the
    hostile cancels: at most one symbol in four may leave the walk per launch. The other two paths run them too."""
    stats = _run_case(me, name, path, group, device=device)
    if path == "gwalk_cx":
        launches = -(-ct.CASES[name].nbatches // group)
        assert stats["handoffs"] * 4 <= launches * S, stats


# ---- scripted: an order whose ring slot another record took -----------------------------------------------

class Rows:
    """Records appended in stream order; a cancel repeats the last seq."""

    def __init__(self, seq0):
        self.next = seq0
        self.r = []

    def new(self, s, side, px, q, market=False):
        self.r.append((self.next, px, q, s, kind(side, 1 if market else 0)))
        self.next += 1
        return self.next - 1

    def cancel(self, s, target):
        self.r.append((self.next - 1, ct.to_i64(target), 0, s, kind(BUY, 0, 1)))
        return len(self.r) - 1

    def arrays(self, lo, hi):
        return tm.Arrays(*[[x[i] for x in self.r[lo:hi]] for i in range(5)])


@pytest.mark.parametrize("sub", ["resting_other_symbol", "filled_own_symbol", "market"])
@pytest.mark.parametrize("path", ["reg", "gwalk_cx", "deep"])
def test_ring_slot_taken_by_a_later_record(me, path, sub):
    """seq_ring = 1,024. Orders A and A + 1 of symbol 0 rest; 1,022 records of symbol 1 pass; the records at
    A + 1,024 and A + 1,025 (the ring slots of A and A + 1) are resting orders of symbol 1, orders of symbol 0
    that rest and are filled by the next record, or MARKETs. Then symbol 0 cancels A + 1,024 (unknown), A
    (through the old-order table: CANCELED), A again (unknown) and A + 2,048 (unknown) — once in the batch of the
    records at A + 1,024 / A + 1,025, and the same for A + 1 one batch later."""
    L = PATHS[path][0]
    base = tm.base_prices(2, L)
    m0, m1 = int(base[0]) + L // 2, int(base[1]) + L // 2
    R = 1024
    sc = Rows(ct.SEQ_HIGH)
    A = sc.new(0, BUY, m0 - 5, 7)
    A2 = sc.new(0, BUY, m0 - 6, 9)
    for j in range(R - 2):
        if j % 2 == 0:
            sc.new(1, SELL, m1 + (10 if j % 100 == 0 else 1), 1)
        else:
            sc.new(1, BUY, m1 + 1, 1)
    assert sc.next == A + R and len(sc.r) == R
    if sub == "resting_other_symbol":
        X, X2 = sc.new(1, SELL, m1 + 20, 3), sc.new(1, SELL, m1 + 20, 3)
    elif sub == "filled_own_symbol":
        X, X2 = sc.new(0, SELL, m0 + 3, 4), sc.new(0, SELL, m0 + 3, 4)
        sc.new(0, BUY, m0 + 3, 8)
    else:  # (they take 4 of A's 7)
        X, X2 = sc.new(0, SELL, 0, 2, market=True), sc.new(0, SELL, 0, 2, market=True)
    assert (X, X2) == (A + R, A2 + R)
    first = [sc.cancel(0, t) for t in (X, A, A, A + 2 * R)]
    cut = len(sc.r)
    sc.new(1, BUY, m1 - 30, 1)
    second = [sc.cancel(0, t) for t in (X2, A2, A2, A2 + 2 * R)]
    if sub == "resting_other_symbol":  # symbol 1's orders were not touched
        own = [sc.cancel(1, X), sc.cancel(1, X2)]
    arrays = [sc.arrays(k, k + 256) for k in range(0, R, 256)] + [sc.arrays(R, cut), sc.arrays(cut, len(sc.r))]
    assert max(int(a.seq.max()) - int(a.seq.min()) for a in arrays) < R
    tb = TifBook(2)
    exp = [tb.submit(a) for a in arrays]
    # the script does what it says (on the reference)
    for res, idx in ((exp[-2][0], [i - R for i in first]), (exp[-1][0], [i - cut for i in second])):
        assert res["status"][idx].tolist() == [ST_REJECTED, ST_CANCELED, ST_REJECTED, ST_REJECTED]
    assert exp[-2][0]["remaining_qty"][first[1] - R] == (3 if sub == "market" else 7)
    assert exp[-1][0]["remaining_qty"][second[1] - cut] == 9
    if sub == "resting_other_symbol":
        assert exp[-1][0]["status"][[i - cut for i in own]].tolist() == [ST_CANCELED, ST_CANCELED]
    batches = [as_batch(me, a) for a in arrays]
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with engine_on(me, path, 2, base, batches, table=PATHS, ring=R, **kw) as eng:
        outs = [eng.submit_batch(b) for b in batches]
        _check(eng, tb, outs, exp, f"ring slot {path} {sub}")


# ---- the grouped cancel walk's hand-off limits --------------------------------------------------------------
# One symbol, L = 128, ME_REG_AGG=1, ME_GW_CANCEL=1. Batch 1 builds the book (no hand-off); batch 2 is the group
# under test: oracle equality and the exact number of hand-offs (one per symbol and group that leaves the walk).

@pytest.fixture
def cx_env(monkeypatch):
    monkeypatch.setenv("ME_REG_AGG", "1")
    monkeypatch.setenv("ME_GW_CANCEL", "1")


def _rows(me, rows, seq0):
    """rows: (side, type, op, price_q4 / cancel target, qty) of symbol 0"""
    n = len(rows)
    return me.Batch(np.arange(seq0, seq0 + n, dtype=np.uint64), [r[3] for r in rows], [r[4] for r in rows],
                    [0] * n, [me.kind(r[0], r[1], r[2]) for r in rows])


def _limit_case(me, orc, build, group, handoffs, ctx, built_handoffs=0):
    """build: the row lists of the batches before the group (at most 128 records each); group: the rows of
    the group under test. Every batch against the oracle, then the books and the counters."""
    ob = orc.OracleBook(1)
    total = sum(len(b) for b in build) + len(group)
    seq = 1
    with me.Engine(1, 128, [1000], max_batch=128, max_resting=total + 64, seq_ring=1 << 22) as eng:
        assert eng.paths()["grouped_cancels"]
        for k, rows in enumerate(build + [group]):
            if k == len(build):
                assert eng.stats()["handoffs"] == built_handoffs, f"{ctx}: hand-offs while building the book"
            b = _rows(me, rows, seq)
            seq += len(rows)
            r, f = eng.submit_batch(b)
            ro, fo = ob.submit(b)
            assert_results_equal(r, ro, f"{ctx} batch {k}")
            assert_fills_equal(f, fo, f"{ctx} batch {k}")
        assert_books_equal(eng, ob, [0], ctx)
        assert eng.resting_count() == eng.admission()["resting"] == ob.resting(), ctx
        assert eng.stats()["handoffs"] - built_handoffs == handoffs, f"{ctx}: {eng.stats()}"


def _asks(n, price, qty):
    return [(SELL, 0, 0, price(i) if callable(price) else price, qty(i) if callable(qty) else qty) for i in range(n)]


def _cx(t):
    return (BUY, 0, 1, t, 0)


@pytest.mark.parametrize("n,handoffs", [(64, 0), (65, 1)])
def test_limit_gw_cxp(me, orc, cx_env, n, handoffs):
    """GW_CXP = 64, gw_prepare_cx: a cancel of a pre-group order not yet in the symbol's list hands off when
    `np >= GW_CXP`, np the distinct pre-group orders the group cancelled so far. 64 distinct orders are kept; the
    65th hands off. (Ten cancels per level at the most: neither GW_CXL nor GW_CXN is near.)"""
    build = [_asks(70, lambda i: 1010 + i % 7, lambda i: 1 + i % 3)]
    group = [_cx(t) for t in range(1, n + 1)] + [(BUY, 1, 0, 0, 5)]
    _limit_case(me, orc, build, group, handoffs, f"GW_CXP n={n}")


@pytest.mark.parametrize("n,handoffs", [(63, 0), (64, 1)])
def test_limit_gw_cxn(me, orc, cx_env, n, handoffs):
    """GW_CXN = 64, lw_block_cx: a cancel that removes quantity hands off when `n + 1u >= GW_CXN`, n the cancels
    the level took in this group. 63 cancels at one level are kept; the 64th hands off. A MARKET first consumes
    three lots at the front; the targets (orders 7.., two lots each, cancelled front to back) lie behind it and
    the bounds decide each of them, so the level's list (GW_CXL = 20) is never read. 64 pre-group orders stay
    within GW_CXP (`np >= 64` is met only by a 65th)."""
    build = [_asks(72, 1010, 2)]
    group = [(BUY, 1, 0, 0, 3)] + [_cx(t) for t in range(7, 7 + n)] + [(BUY, 1, 0, 0, 2)]
    _limit_case(me, orc, build, group, handoffs, f"GW_CXN n={n}")


@pytest.mark.parametrize("chunk,slot,handoffs", [(64, 15, 0), (65, 0, 1)])
def test_limit_chunk_walk(me, orc, cx_env, chunk, slot, handoffs):
    """gw_pre_target walks the level's FIFO from its head to the target's chunk and hands off when
    `steps >= 64u` with the chunk not reached: a target in the chain's chunk 64 (counted from 0, the 65th) is
    the last one reached, one in chunk 65 the first not reached. 66 x 16 one-lot orders at one level, untouched,
    fill 66 chunks; the two targets are neighbours: the last slot of chunk 64 and the first of chunk 65."""
    C = me._abi.CHUNK_SLOTS
    assert C == 16
    orders = _asks(66 * C, 1010, 1)
    build = [orders[k:k + 128] for k in range(0, len(orders), 128)]
    target = chunk * C + slot + 1  # (seqs start at 1)
    group = [_cx(target), (BUY, 1, 0, 0, 5)]
    _limit_case(me, orc, build, group, handoffs, f"chunk walk chunk={chunk}")


@pytest.mark.parametrize("q,handoffs", [((1 << 24) - 1, 0), (1 << 24, 1)])
def test_limit_target_quantity(me, orc, cx_env, q, handoffs):
    """gw_pre_target: `q >= (1u << 24)` hands off (a pre-group target's descriptor keeps 24 bits of quantity).
    2^24 - 1 is kept, 2^24 hands off."""
    build = [[(SELL, 0, 0, 1010, 3), (SELL, 0, 0, 1010, q), (SELL, 0, 0, 1011, 2)]]
    group = [_cx(2), (BUY, 1, 0, 0, 4)]
    _limit_case(me, orc, build, group, handoffs, f"target quantity {q}")


@pytest.mark.parametrize("ahead,handoffs,before", [((1 << 31) - 2, 0, 0), ((1 << 31) - 1, 1, 1)])
def test_limit_quantity_ahead(me, orc, cx_env, ahead, handoffs, before):
    """gw_pre_target: `U >= (1ull << 31)` hands off, U the live quantity ahead of the target in its level. The
    walk runs only while the book's sum stays below LW_CAP = 2^31 (`w.ub < LW_CAP`, lw_init), and the sum
    includes U and the target itself, so U is at most 2^31 - 2 on the walk: neither U = 2^31 - 1 nor U = 2^31 can
    reach the comparison. Tested: U = 2^31 - 2 with a one-lot target (the sum is 2^31 - 1) is kept; with
    U = 2^31 - 1 the sum is 2^31 and LW_CAP, not this comparison, hands the symbol off — already in the batch
    that builds the book, and once more in the group. The group is the cancel alone: the quantities of a
    block's own records count towards LW_CAP too (`lw.ub += qsum`), so a take beside it would hand off as well."""
    build = [[(SELL, 0, 0, 1010, ahead), (SELL, 0, 0, 1010, 1)]]
    group = [_cx(2)]
    _limit_case(me, orc, build, group, handoffs, f"quantity ahead {ahead}", built_handoffs=before)
