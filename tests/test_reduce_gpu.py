"""REDUCE records (ME_KIND_REDUCE) on every matching path against the model
(tests/reduce_model.py): every batch's results and tape, the books of all symbols and the resting counters.
Needs an MI355X. Everything is bit-exact.

Two device loops execute a REDUCE: generic_record (me_kernels.hip: k_match, k_match_hot_cont) and
k_match_reg<true> (me_match_reg.hip); every fast path (k_match_reg<false>, the grouped walks, the hot walks)
hands the symbol off at the record, before anything changed.
"""
import functools

import numpy as np
import pytest

from tests import cancel_targets as ct
from tests import reduce_model as rm
from tests import tif_model as tm
from tests._parity import assert_fills_equal, assert_results_equal
from tests.big_qty import Script
from tests.gpu_harness import PATHS, as_batch, check_books, engine_on, pipelined
from tests.model_common import load_model_fixture
from tests.reduce_model import INT32_MAX, KIND_REDUCE, ReduceBook
from tests.tif_model import kind

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
ST_NEW, ST_PARTIAL, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
RJ_NONE, RJ_BAD_QTY, RJ_UNKNOWN = 0, 1, 5

DRAWS = range(10)


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _step(eng, model, a, ctx, me):
    """One synchronous batch through engine and model: results, tape and every book."""
    r, f = eng.submit_batch(as_batch(me, a))
    ro, fo = model.submit(a)
    assert_results_equal(r, ro, ctx)
    assert_fills_equal(f, fo, ctx)
    check_books(eng, model, ctx)
    return ro, fo


def _st(r):
    return (int(r["status"]), int(r["reason"]), int(r["filled_qty"]), int(r["remaining_qty"]), int(r["fill_count"]))


# ---- priority: what a cancel + new order cannot do ---------------------------------------------------------

@pytest.mark.parametrize("path", ["reg", "gwalk_cx", "deep256"])
def test_reduced_order_keeps_its_priority(me, path):
    """A(10), B(10), C(10) rest at one price; A is reduced by 4; a taker of 8 fills A 6, B 2 and leaves B 8,
    C 10. (An engine that reads 0x0D as a plain cancel removes A and fills B 8.)"""
    L = PATHS[path][0]
    base = tm.base_prices(1, L)
    p = int(base[0]) + L // 2
    sc = Script()
    A, B, C = (sc.new(0, BUY, p, 10) for _ in range(3))
    first = sc.take()
    sc.reduce(0, A, 4)
    sc.new(0, SELL, p, 8)
    second = sc.take()
    model = ReduceBook(1)
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with engine_on(me, path, 1, base, [first, second], **kw) as eng:
        eng.submit_batch(as_batch(me, first))
        model.submit(first)
        r, f = eng.submit_batch(as_batch(me, second))
        assert _st(r[0]) == (ST_NEW, RJ_NONE, 0, 6, 0)
        assert [(int(x["maker_seq"]), int(x["qty"])) for x in f] == [(A, 6), (B, 2)]
        assert [(int(e["seq"]), int(e["qty"])) for e in eng.dump(0)] == [(B, 8), (C, 10)]
        ro, fo = model.submit(second)
        assert_results_equal(r, ro, path)
        assert_fills_equal(f, fo, path)
        check_books(eng, model, path)


# ---- slots: chunks, blocks, quantities ------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["reg", "deep256"])
def test_slots_chunks_and_blocks(me, path):
    """Forty orders at one level (three chunks of 16 slots) and two at a worse one, symbol 0 of four; batches of
    at most 256 records, one per launch. Checked against the model after every batch."""
    L, S = PATHS[path][0], 4
    base = tm.base_prices(S, L)
    p = int(base[0]) + L // 2 - 3
    model = ReduceBook(S)
    sc = Script()
    o = [None] + [sc.new(0, BUY, p, 10) for _ in range(40)]  # o[1..40]; chunks 1-16, 17-32, 33-40
    low = [sc.new(0, BUY, p - 2, 7) for _ in range(2)]
    for s in (1, 2, 3):  # the other symbols hold a book too
        sc.new(s, SELL, int(base[s]) + L // 2 + 1, 5)
    script = [sc.take()]
    # partial reduces in the head, the middle and the tail chunk; a taker shows the order of the queue
    i_head, i_mid, i_tail = sc.reduce(0, o[3], 4), sc.reduce(0, o[20], 1), sc.reduce(0, o[38], 9)
    sc.new(0, SELL, p, 25)  # 1: 10, 2: 10, 3: 5 of its 6
    script.append(sc.take())
    # one 64-record block: several reduces of one order, a reduce of an order rested earlier in the block,
    # reduce then cancel, cancel then reduce, and the quantities around r
    i21 = [sc.reduce(0, o[21], d) for d in (1, 2, 3)]                  # 10 -> 9 -> 7 -> 4
    n43 = sc.new(0, BUY, p, 10)
    i43 = sc.reduce(0, n43, 5)
    i22 = sc.reduce(0, o[22], 3)
    sc.cancel(0, o[22])                                                # removes 7
    sc.cancel(0, o[23])
    i23 = sc.reduce(0, o[23], 3)                                       # UNKNOWN_ORDER
    i24 = [sc.reduce(0, o[24], d) for d in (0, -1, 1, 8)]              # BAD_QTY, BAD_QTY, 9 left, r - 1: 1 left
    i25, i26, i27 = sc.reduce(0, o[25], 10), sc.reduce(0, o[26], 11), sc.reduce(0, o[27], INT32_MAX)
    i_bits = sc.reduce(0, o[28], 2, kd=0xFE)                           # side, tif and reserved bits are ignored
    assert len(sc.r) <= 64
    script.append(sc.take())
    # covering reduces that empty the middle chunk, then the tail chunk, then the level
    left = {20: 9, 21: 4, 24: 1, 28: 8, 29: 10, 30: 10, 31: 10, 32: 10, 17: 10, 18: 10, 19: 10}
    for j, r in sorted(left.items()):
        sc.reduce(0, o[j], r if j % 2 else r + 5)
    script.append(sc.take())
    for j in range(33, 41):
        sc.reduce(0, o[j], INT32_MAX if j % 2 else (1 if j == 38 else 10))
    sc.reduce(0, n43, 5)
    script.append(sc.take())
    for j in range(3, 17):
        sc.reduce(0, o[j], 1 if j == 3 else 10)
    script.append(sc.take())
    sc.reduce(0, low[0], 6)  # the new best level
    sc.new(0, SELL, p - 2, 3)
    script.append(sc.take())
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with engine_on(me, path, S, base, script, **kw) as eng:
        outs = [_step(eng, model, a, f"slots {path} batch {k}", me) for k, a in enumerate(script)]
        # the script does what it says
        r = outs[1][0]
        assert [_st(r[i])[:4] for i in (i_head, i_mid, i_tail)] == [(ST_NEW, 0, 0, 6), (ST_NEW, 0, 0, 9), (ST_NEW, 0, 0, 1)]
        assert [(int(x["maker_seq"]), int(x["qty"])) for x in outs[1][1]] == [(o[1], 10), (o[2], 10), (o[3], 5)]
        r = outs[2][0]
        assert [int(r[i]["remaining_qty"]) for i in i21] == [9, 7, 4]
        assert _st(r[i43]) == (ST_NEW, RJ_NONE, 0, 5, 0) and _st(r[i22]) == (ST_NEW, RJ_NONE, 0, 7, 0)
        assert _st(r[i22 + 1]) == (ST_CANCELED, RJ_NONE, 0, 7, 0)
        assert _st(r[i23]) == (ST_REJECTED, RJ_UNKNOWN, 0, 0, 0)
        assert [_st(r[i])[:4] for i in i24] == [(ST_REJECTED, RJ_BAD_QTY, 0, 0), (ST_REJECTED, RJ_BAD_QTY, 0, 0),
                                                (ST_NEW, 0, 0, 9), (ST_NEW, 0, 0, 1)]
        assert [_st(r[i])[:4] for i in (i25, i26, i27)] == [(ST_CANCELED, 0, 0, 10)] * 3
        assert _st(r[i_bits]) == (ST_NEW, RJ_NONE, 0, 8, 0)
        assert set(outs[3][0]["status"].tolist()) == {ST_CANCELED} == set(outs[4][0]["status"].tolist())
        assert set(outs[5][0]["status"].tolist()) == {ST_CANCELED}
        bids, _ = eng.snapshot(0, 4)
        # the best price moved: low[0] held 1 after its reduce and the taker took it and 2 of low[1]'s 7
        assert [(int(b["price_q4"]), int(b["total_qty"]), int(b["order_count"])) for b in bids] == [(p - 2, 5, 1)]
        assert model.side[0][0].best() == p - 2


# ---- targets -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["reg", "gwalk", "deep256"])
def test_far_levels_on_each_side(me, path):
    """Orders far below and far above the window: partial reduces, a taker that reaches them, covering reduces."""
    L, S = PATHS[path][0], 2
    base = tm.base_prices(S, L)
    b0 = int(base[0])
    model = ReduceBook(S)
    sc = Script()
    fb = [sc.new(0, BUY, b0 - 3 * L, 20), sc.new(0, BUY, b0 - 3 * L, 30), sc.new(0, BUY, b0 - 5 * L, 10)]
    fa = [sc.new(0, SELL, b0 + 4 * L, 20), sc.new(0, SELL, b0 + 4 * L, 30), sc.new(0, SELL, b0 + 7 * L, 10)]
    sc.new(0, BUY, b0 + L // 2 - 1, 5)
    sc.new(0, SELL, b0 + L // 2 + 1, 5)
    sc.new(1, BUY, int(base[1]) + 3, 5)
    script = [sc.take()]
    sc.reduce(0, fb[0], 15)
    sc.reduce(0, fa[0], 19)
    sc.reduce(0, fb[2], 3)
    sc.reduce(0, fa[2], 3)
    script.append(sc.take())
    sc.new(0, SELL, b0 - 3 * L, 12)  # the window bid 5, then the far bids: 5 of fb[0], 2 of fb[1]
    sc.new(0, BUY, 0, 8, market=True)  # the window ask 5, fa[0] 1, fa[1] 2
    script.append(sc.take())
    sc.reduce(0, fb[1], 28)
    sc.reduce(0, fa[1], 1000)
    sc.reduce(0, fb[2], 7)
    sc.reduce(0, fa[2], INT32_MAX)
    sc.reduce(0, fa[2], 1)
    script.append(sc.take())
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with engine_on(me, path, S, base, script, **kw) as eng:
        outs = [_step(eng, model, a, f"far {path} batch {k}", me) for k, a in enumerate(script)]
        assert [_st(r)[:4] for r in outs[1][0]] == [(ST_NEW, 0, 0, 5), (ST_NEW, 0, 0, 1), (ST_NEW, 0, 0, 7), (ST_NEW, 0, 0, 7)]
        assert [int(x["qty"]) for x in outs[2][1]] == [5, 5, 2, 5, 1, 2]
        assert [_st(r)[:4] for r in outs[3][0]] == [(ST_CANCELED, 0, 0, 28), (ST_CANCELED, 0, 0, 28), (ST_CANCELED, 0, 0, 7),
                                                   (ST_CANCELED, 0, 0, 7), (ST_REJECTED, RJ_UNKNOWN, 0, 0)]
        if PATHS[path][3]:
            assert eng.stats()["handoffs"] > 0  # the fast launch executes no reduce


@pytest.mark.parametrize("path", ["reg", "gwalk_cx", "deep256"])
def test_target_older_than_the_ring_horizon(me, path):
    """seq_ring = 64: orders A and A2 rest, more than two rings of other records pass (16 per batch, so a launch
    group spans fewer than 64 seqs), then they are reduced in part and in full through the old-order table."""
    L, S, R = PATHS[path][0], 2, 64
    base = tm.base_prices(S, L)
    m0, m1 = int(base[0]) + L // 2, int(base[1]) + L // 2
    model = ReduceBook(S)
    sc = Script(ct.SEQ_HIGH)
    A, A2 = sc.new(0, BUY, m0 - 5, 9), sc.new(0, SELL, m0 + 5 * L, 12)  # (A2 on a far level)
    script = [sc.take()]
    for k in range(10):
        for j in range(16):
            sc.new(1 if j % 4 else 0, BUY if j % 2 else SELL, (m1 if j % 4 else m0) + (-2 if j % 2 else 2), 1 + j % 3)
        script.append(sc.take())
    assert sc.next - A > 2 * R
    i = [sc.reduce(0, A, 4), sc.reduce(0, A2, 11), sc.reduce(0, A + R, 1), sc.reduce(0, A, 4), sc.reduce(0, A, 1),
         sc.reduce(0, A2, 1), sc.reduce(0, A, 1)]
    script.append(sc.take())
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with engine_on(me, path, S, base, script, ring=R, **kw) as eng:
        outs = [_step(eng, model, a, f"old {path} batch {k}", me) for k, a in enumerate(script)]
        r = outs[-1][0]
        want = [(ST_NEW, 0, 0, 5), (ST_NEW, 0, 0, 1), None, (ST_NEW, 0, 0, 1), (ST_CANCELED, 0, 0, 1),
                (ST_CANCELED, 0, 0, 1), (ST_REJECTED, RJ_UNKNOWN, 0, 0)]
        for j, w in zip(i, want):
            if w is not None:
                assert _st(r[j])[:4] == w, (j, r[j])


@functools.lru_cache(maxsize=None)
def _hostile(name):
    """The hostile cancel targets of tests/cancel_targets.py with every cancel turned into a REDUCE (d drawn
    from a seeded list: mostly partial against quantities of 1..60, some covering) and the model's outputs."""
    base, batches, _, _ = ct.stream(name)
    rng = np.random.default_rng(ct.CASES[name].seed)
    arrays = []
    for b in batches:
        cx = (b.kind & 8) != 0
        qty, kd = b.qty.copy(), b.kind.copy()
        qty[cx] = rng.choice([1, 2, 3, 7, 20, 59, 60, 61, 1000, INT32_MAX, 0, -1], size=int(cx.sum()))
        kd[cx] |= 0x0C
        arrays.append(tm.Arrays(b.seq, b.price_q4, qty, b.symbol, kd))
    model = ReduceBook(ct.S_CX)
    exp = [model.submit(a) for a in arrays]
    st = np.concatenate([r["status"][rm.is_reduce(a.kind)] for a, (r, _) in zip(arrays, exp)])
    assert (st == ST_NEW).sum() > 100 and (st == ST_CANCELED).sum() > 50 and (st == ST_REJECTED).sum() > 100
    return base, arrays, exp, model


@pytest.mark.parametrize("name,path,group", [("l128_tif", "reg", 8), ("l128_tif", "gwalk_cx", 8), ("l128_plain", "gwalk", 1),
                                             ("l1024_tif", "deep", 1), ("ring128_tif", "reg", 4),
                                             ("ring1024_plain", "deep", 1)])
def test_hostile_targets_as_reduces(me, name, path, group):
    c = ct.CASES[name]
    assert PATHS[path][0] == c.levels
    base, arrays, exp, model = _hostile(name)
    batches = [as_batch(me, a) for a in arrays]
    kw = {"batches_per_launch": group} if PATHS[path][3] else {}
    with engine_on(me, path, ct.S_CX, base, arrays, ring=c.ring, **kw) as eng:
        outs = pipelined(eng, batches, 2 * group + 1) if PATHS[path][3] else [eng.submit_batch(b) for b in batches]
        for k, (ro, fo) in enumerate(exp):
            assert_results_equal(outs[k][0], ro, f"hostile {name} {path} batch {k}")
            assert_fills_equal(outs[k][1], fo, f"hostile {name} {path} batch {k}")
        check_books(eng, model, f"hostile {name} {path}")


# ---- every path: seeded model streams ----------------------------------------------------------------------------

SHAPES = {
    # name: (symbols, levels, batches, records per batch, stream keywords)
    "small": (12, 128, 8, 600, dict(far_pct=2, skew=True)),
    "grouped": (64, 128, 4, 2048, dict(far_pct=1)),
    "deep256": (12, 256, 4, 900, dict(far_pct=2, skew=True)),
    "hot2048": (6, 2048, 4, 900, dict(far_pct=1, skew=True)),
    "hot1024": (6, 1024, 4, 900, dict(far_pct=1, skew=True)),
}


@functools.lru_cache(maxsize=None)
def _draw(shape, draw):
    """(base, batches, [(results, fills)], model after the last batch, share of reduces). Shared between the
    tests: nobody changes the arrays or steps the model."""
    S, L, nb, n, kw = SHAPES[shape]
    base, arrays = rm.reduce_stream(9000 + 100 * len(shape) + draw, S, L, nb, n, convert_pct=60 + 5 * (draw % 5),
                                    fresh_pct=4 + 2 * (draw % 6), drift=(0, 2, 5)[draw % 3], **kw)
    model = ReduceBook(S)
    exp = [model.submit(a) for a in arrays]
    share = sum(int(rm.is_reduce(a.kind).sum()) for a in arrays) / sum(len(a) for a in arrays)
    assert 0.10 <= share <= 0.30, share
    part = sum(int(((r["status"] == ST_NEW) & rm.is_reduce(a.kind)).sum()) for a, (r, _) in zip(arrays, exp))
    assert part > 20, part
    return base, arrays, exp, model, share


def _run_draw(me, shape, draw, path, group=1, mode="pipelined", **kw):
    S = SHAPES[shape][0]
    assert SHAPES[shape][1] == PATHS[path][0]
    base, arrays, exp, model, _ = _draw(shape, draw)
    batches = [as_batch(me, a) for a in arrays]
    ctx = f"{shape}#{draw} {path} G={group} {mode}"
    if PATHS[path][3]:
        kw["batches_per_launch"] = group
    if mode == "device":  # (every record of a device batch counts as one that may rest)
        kw["max_resting"] = 2 * sum(len(a) for a in arrays) + 1024
    with engine_on(me, path, S, base, arrays, **kw) as eng:
        if mode == "device":
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
        elif mode == "pipelined":
            outs = pipelined(eng, batches, 2 * group + 1)
        else:
            outs = [eng.submit_batch(b) for b in batches]
        for k, (ro, fo) in enumerate(exp):
            assert_results_equal(outs[k][0], ro, f"{ctx} batch {k}")
            assert_fills_equal(outs[k][1], fo, f"{ctx} batch {k}")
        check_books(eng, model, ctx)
        return eng.stats()


@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("group", [1, 8])
def test_streams_on_k_match_reg(me, group, draw):
    stats = _run_draw(me, "small", draw, "reg", group)
    assert stats["handoffs"] > 0


@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("group", [1, 4])
@pytest.mark.parametrize("path", ["gwalk", "gwalk_cx"])
def test_streams_on_the_grouped_walk(me, path, group, draw):
    """ME_REG_AGG=1 pins the grouped aggregate path: the walk hands a symbol off at its first REDUCE and the
    continuation's results are exact from that record on."""
    stats = _run_draw(me, "grouped", draw, path, group)
    assert stats["handoffs"] > 0


@pytest.mark.parametrize("draw", DRAWS)
def test_streams_on_k_match(me, draw):
    _run_draw(me, "deep256", draw, "deep256", mode="sync")


@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("path,shape", [("hot", "hot2048"), ("hot_agg", "hot1024")])
def test_streams_on_the_hot_walks(me, path, shape, draw):
    """Half of the records are symbol 0's, well above ME_HOT_MIN = 64: its walk meets a REDUCE mid-batch and
    k_match_hot_cont finishes the batch."""
    stats = _run_draw(me, shape, draw, path, mode="sync")
    assert stats["hot_handoffs"] > 0


@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("mode", ["device", "sync"])
def test_streams_on_the_other_submit_paths(me, mode, draw):
    """Device batches in one launch group of eight, and synchronous host batches (the pipelined host path is
    what the tests above use)."""
    _run_draw(me, "small", draw, "reg", 8 if mode == "device" else 1, mode=mode)


def test_fixture_through_the_engine(me):
    meta, batches, res, fills, book = load_model_fixture("match_reduce.npz")
    S = meta["num_symbols"]
    with engine_on(me, "reg", S, meta["base"], batches) as eng:
        for k, a in enumerate(batches):
            r, f = eng.submit_batch(as_batch(me, a))
            assert_results_equal(r, res[k], f"fixture batch {k}")
            assert_fills_equal(f, fills[k], f"fixture batch {k}")
        dumps = np.concatenate([eng.dump(s) for s in range(S)])
        assert len(dumps) == len(book) and np.all(dumps == book)


# ---- the feeds follow ------------------------------------------------------------------------------------------------

def _replay_depth(state, ev):
    for e in ev:
        key = (int(e["symbol"]), int(e["side"]))
        if int(e["qty"]) == 0:
            state.setdefault(key, {}).pop(int(e["price_q4"]), None)
        else:
            state.setdefault(key, {})[int(e["price_q4"])] = int(e["qty"])


@pytest.mark.parametrize("path", ["reg", "deep256"])
def test_quote_and_depth_feeds_follow_a_reduce(me, path):
    L, S, D = PATHS[path][0], 2, 4
    base = tm.base_prices(S, L)
    m = int(base[0]) + L // 2
    model = ReduceBook(S)
    sc = Script()
    top = [sc.new(0, BUY, m - 1, 10), sc.new(0, BUY, m - 1, 10)]
    deep = [sc.new(0, BUY, m - 1 - j, 10) for j in range(1, 6)]  # m-2 .. m-6: m-6 lies below the top 4
    sc.new(0, SELL, m + 2, 5)
    sc.new(1, SELL, int(base[1]) + L // 2, 5)
    build = sc.take()
    sc.reduce(0, top[0], 4)
    at_top = sc.take()
    sc.reduce(0, deep[-1], 3)
    sc.reduce(0, deep[-2], 9)  # (m-5 is the fifth level: outside the view too)
    below = sc.take()
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with engine_on(me, path, S, base, [build, at_top, below], **kw) as eng:
        _step(eng, model, build, "feeds build", me)
        eng.quotes_enable(64)
        eng.depth_enable(D, 256)
        quotes = [eng.quotes_drain()]
        views = {}
        _replay_depth(views, eng.depth_drain())
        assert views[(0, BUY)] == {m - 1: 20, m - 2: 10, m - 3: 10, m - 4: 10}
        _step(eng, model, at_top, "feeds top", me)
        eng.sync()
        q, d = eng.quotes_drain(), eng.depth_drain()
        assert len(q) == 1 and int(q[0]["symbol"]) == 0 and int(q[0]["bid_price_q4"]) == m - 1 and int(q[0]["bid_qty"]) == 16
        assert int(q[0]["ask_price_q4"]) == m + 2 and int(q[0]["ask_qty"]) == 5
        assert [(int(e["symbol"]), int(e["side"]), int(e["price_q4"]), int(e["qty"])) for e in d] == [(0, BUY, m - 1, 16)]
        quotes.append(q)
        _replay_depth(views, d)
        _step(eng, model, below, "feeds below", me)
        eng.sync()
        q, d = eng.quotes_drain(), eng.depth_drain()
        assert len(q) == 0 and len(d) == 0  # a reduce below the top D is not an event
        # the replay equals the books
        lv, cnt = eng.levels_all(D)
        for s in range(S):
            for k, side in ((0, BUY), (1, SELL)):
                want = {int(x["price_q4"]): int(x["total_qty"]) for x in lv[s, k, : cnt[s, k]]}
                assert views.get((s, side), {}) == want, (s, side)
        last = {}
        for e in np.concatenate(quotes):
            last[int(e["symbol"])] = e
        lv1, cnt1 = eng.levels_all(1)
        for s in range(S):
            e = last[s]
            for k, (flag, pf, qf) in enumerate(((1, "bid_price_q4", "bid_qty"), (2, "ask_price_q4", "ask_qty"))):
                assert bool(int(e["flags"]) & flag) == bool(cnt1[s, k])
                if cnt1[s, k]:
                    assert (int(e[pf]), int(e[qf])) == (int(lv1[s, k, 0]["price_q4"]), int(lv1[s, k, 0]["total_qty"]))


# ---- admission ---------------------------------------------------------------------------------------------------------

def test_full_book_accepts_a_batch_of_reduces(me):
    """An engine whose books hold max_resting orders refuses a batch of GTC LIMITs and accepts a batch of only
    reduces (a REDUCE never rests: admission control does not count it)."""
    S, L, R = 4, 128, 512
    base = tm.base_prices(S, L)
    sc = Script()
    ids = []
    for i in range(R):
        s = i % S
        mid = int(base[s]) + L // 2
        ids.append((s, sc.new(s, BUY if i % 2 else SELL, mid + (-1 - i % 7 if i % 2 else 1 + i % 7), 10)))
    fill = sc.take()
    model = ReduceBook(S)
    with me.Engine(S, L, base, max_batch=1024, max_resting=R, seq_ring=1 << 20) as eng:
        _step(eng, model, fill, "fill", me)
        assert eng.admission()["resting"] == R
        g = Script(sc.next)
        for i in range(64):
            g.new(i % S, BUY, int(base[i % S]) + 10, 1)
        gtc = as_batch(me, g.take())
        with pytest.raises(me.EngineError) as ei:
            eng.submit_batch(gtc)
        assert ei.value.code == me.ME_E_CAPACITY
        for j, (s, t) in enumerate(ids):
            sc.reduce(s, t, (3, 10, 9, 11)[j % 4])
        red = sc.take()
        assert eng.admits(as_batch(me, red))
        ro, _ = _step(eng, model, red, "reduces on a full book", me)
        assert (ro["status"] == ST_NEW).sum() == R // 2 and (ro["status"] == ST_CANCELED).sum() == R // 2
        assert model.resting() == R // 2
