"""The price-edge streams and scripts of tests/price_edges.py on the CPU models alone (no GPU).

  * every stream the GPU tests run (price_edges.STREAMS, both draws) meets the floors: conditions on the inputs,
    counted from the model, so that a green GPU run has in fact traded at the ends of int64, jumped between
    them and rested orders at alias distances;
  * on the plain part of each stream ReduceBook and the native OracleBook agree: the two references agree at
    these prices before either judges a kernel;
  * two deliberately wrong models (prices compared modulo 2^32; INT64_MAX / INT64_MIN read as "side empty")
    differ from the right one on every draw and on the alias scripts: the inputs would catch those errors;
  * every directed script does on the model what price_edges wrote out by hand;
  * the helper models the GPU tests lean on (quote_model, depth_model, order_query_model, big_qty.model_snapshot,
    book_audit.audit) run over these prices without overflowing;
  * the committed fixture tests/golden/price_edges.npz replays through the model.

What each stream reaches, draw 0 / draw 1 (price_edges.coverage; test_floors prints it):

  stream      fills at    fills at   resting   books    jumps    alias      bad records  REDUCE       fills outside
              EXTREMES    MIN / MAX  at MIN /  >= 2^63           rests      at special   share        the initial
                                     MAX                                    prices                    windows
  l128        132 / 105   114 / 70   18 / 8    6 / 5    16 / 9   64 / 53    32 / 41      0.13 / 0.12  811 / 539
  l128_dev    211 / 711   157 / 612  8 / 12    6 / 6    26 / 38  147 / 153  100 / 82     0.12 / 0.13  2560 / 2518
  l256        62 / 76     49 / 62    6 / 7     5 / 5    13 / 15  53 / 64    24 / 36      0.13 / 0.12  704 / 860
  l1024       69 / 182    53 / 152   8 / 12    5 / 4    13 / 15  65 / 55    29 / 31      0.13 / 0.13  662 / 1019
  l1024_hot   86 / 166    66 / 137   10 / 14   5 / 8    21 / 18  75 / 66    32 / 27      0.12 / 0.12  1021 / 863
  l2048_hot   57 / 93     50 / 69    8 / 3     5 / 4    16 / 13  60 / 58    33 / 39      0.13 / 0.13  985 / 901
"""
import os

import numpy as np
import pytest

from tests import big_qty as bq
from tests import depth_model as dm
from tests import order_query_model as oq
from tests import price_edges as pe
from tests import quote_model as qm
from tests.book_audit import audit
from tests.model_common import FIELDS_BOOK, FIELDS_FILL, FIELDS_RES, load_model_fixture, same
from tests.price_edges import I64_MAX, I64_MIN
from tests.reduce_model import ReduceBook, check_seq_rule, is_reduce
from tests.tif_model import Arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_DRAWS = [(n, d) for n in pe.STREAMS for d in pe.DRAWS]
SCRIPT_LEVELS = (64, 128, 256, 1024, 2048, 32768)  # every window size a GPU script test runs at


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle

    return oracle


# ---- the streams -------------------------------------------------------------------------------------------------

def test_every_gpu_path_has_its_stream():
    assert set(pe.PATH_STREAM) == {"reg", "gwalk", "gwalk_cx", "deep256", "deep", "hot_agg", "hot"}
    assert len({pe.STREAMS[n][4][d] for n, d in ALL_DRAWS}) >= 10  # (mostly different seeds)


def test_bases_are_the_anchors():
    for L in (128, 32768):
        b = [int(x) for x in pe.bases(16, L)]
        assert b[:8] == [I64_MIN, I64_MAX - L + 1, I64_MAX, -L // 2, 2**32 - L // 2, -2**31 - L // 2, 1_000_000, 2**62]
        assert b[8:] == b[:8]


@pytest.mark.parametrize("name,d", ALL_DRAWS)
def test_floors(name, d):
    L, nb, n, skew, seeds = pe.STREAMS[name]
    base, arrays, exp, model, draw = pe.stream(name, d)
    assert len(arrays) == nb and all(len(a) == n for a in arrays)
    check_seq_rule(arrays)
    c = pe.coverage(base, arrays, L, draw)
    print(name, d, c)
    assert c["fills_extreme"] >= 50, c
    assert c["jumps"] >= 8, c
    assert c["span63"] >= 4, c
    assert c["alias_rest"] >= 20, c
    assert c["special_rejects"] >= 10, c
    assert 0.10 <= c["reduce_share"] <= 0.30, c
    # beyond the issue's floors: fills at INT64_MIN / INT64_MAX themselves, orders left there, executed partial
    # REDUCEs, fills at negative prices and outside the initial windows
    assert c["fills_exact"] >= 20 and c["rest_extreme"] >= 2 and c["reduces_partial"] >= 15, c
    assert c["neg_fills"] >= 100 and c["far_fills"] >= 100, c
    # the final books cannot lie around the initial windows: some window must have crossed 2^32 (the jumps do)
    forced = pe.forced_moves(base, L, model)
    assert forced and max(forced.values()) >= 1 << 32, forced
    px = np.concatenate([a.price_q4[(a.kind & 8) == 0] for a in arrays])
    for v in pe.EXTREMES:
        assert (px == v).any(), v
    if skew:
        assert all(int((a.symbol == 0).sum()) > 64 for a in arrays)


@pytest.mark.parametrize("name,d", ALL_DRAWS)
def test_references_agree_on_the_plain_part(orc, name, d):
    """GTC LIMITs, MARKETs and cancels (no TIF, no REDUCE) through ReduceBook and the native OracleBook."""
    base, arrays, _, _, _ = pe.stream(name, d)
    S = pe.S_EDGE
    sub = []
    for b in arrays:
        keep = ~is_reduce(b.kind) & (((b.kind & 8) != 0) | (((b.kind >> 4) & 3) == 0))
        sub.append(Arrays(b.seq[keep], b.price_q4[keep], b.qty[keep], b.symbol[keep], b.kind[keep] & 0x0F))
    check_seq_rule(sub)
    ob, pb = orc.OracleBook(S), ReduceBook(S)
    at_ends = 0
    for k, b in enumerate(sub):
        r1, f1 = ob.submit(b)
        r2, f2 = pb.submit(b)
        same(r2, r1, FIELDS_RES, f"{name}#{d} batch {k} results")
        same(f2, f1, FIELDS_FILL, f"{name}#{d} batch {k} tape")
        at_ends += int(np.isin(f1["price_q4"], (I64_MIN, I64_MAX)).sum())
        for s in range(S):
            same(pb.dump(s), ob.dump(s), FIELDS_BOOK, f"{name}#{d} batch {k} book {s}")
            for mine, theirs in zip(bq.model_snapshot(pb, s, 10), ob.snapshot(s, 10)):
                same(mine, theirs, ("price_q4", "total_qty", "order_count"), f"{name}#{d} batch {k} snapshot {s}")
    assert pb.resting() == ob.resting()
    assert at_ends > 0  # fills at the ends of int64 were compared


@pytest.mark.parametrize("name,d", ALL_DRAWS)
def test_wrong_models_differ_on_every_draw(name, d):
    base, arrays, exp, _, _ = pe.stream(name, d)
    assert pe.differs(pe.Mod32Book, pe.S_EDGE, arrays, exp)
    assert pe.differs(pe.SentinelBook, pe.S_EDGE, arrays, exp)
    assert not pe.differs(ReduceBook, pe.S_EDGE, arrays, exp)


def test_wrong_models_are_right_on_ordinary_prices():
    """The two wrong models are wrong only about what they are meant to be wrong about: on reduce_stream's
    prices (around 10^6) they are the right model."""
    from tests.reduce_model import reduce_stream

    base, arrays = reduce_stream(5, 6, 128, 3, 500, far_pct=3, skew=True)
    m = ReduceBook(6)
    exp = [m.submit(a) for a in arrays]
    assert not pe.differs(pe.Mod32Book, 6, arrays, exp) and not pe.differs(pe.SentinelBook, 6, arrays, exp)


# ---- the helper models at these prices ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["l128", "l1024_hot"])
def test_helper_models_carry_these_prices(name):
    """quote_model, depth_model, order_query_model and model_snapshot after every batch of a draw: every price
    they report is one the book holds (nothing wrapped), the extremes among them."""
    base, arrays, _, _, _ = pe.stream(name, 0)
    S, D = pe.S_EDGE, 4
    m = ReduceBook(S)
    view = bq.Snap(m)
    table, maps = qm.tops(qm._Empty(), S), dm.empty_maps(S)
    qmod, dmod = qm.QuoteModel(view, S), dm.DepthModel(view, S, D)
    seen, used = set(), set()
    for a in arrays:
        m.submit(a)
        used.update(int(x) for x in a.seq)
        qm.replay(table, qmod.expect(1))
        dm.replay(maps, dmod.expect(1))
        assert qm.same_quotes(table, qm.tops(view, S))
        assert dm.same_views(maps, dm.views(view, S, D))
        for s in range(S):
            d = m.dump(s)
            bids, asks = bq.model_snapshot(m, s, 1000)
            for side, lv in ((pe.BUY, bids), (pe.SELL, asks)):
                want = [int(x) for x in d["price_q4"][d["side"] == side]]
                assert [int(x) for x in lv["price_q4"]] == sorted(set(want), reverse=side == pe.BUY)
                assert int(lv["total_qty"].sum()) == int(d["qty"][d["side"] == side].astype(np.int64).sum())
            seen.update(int(x) for x in d["price_q4"])
        ans = oq.expected(m, S, sorted(used))
        live = {q: h for q, h in m.live.items()}
        assert int(ans["found"].sum()) == len(live)
        for r in ans[ans["found"] == 1]:
            assert int(r["price_q4"]) == live[int(r["seq"])][2]
    assert I64_MIN in seen and I64_MAX in seen


@pytest.mark.parametrize("L", [128, 1024])
def test_audit_with_the_base_at_both_clamps(L):
    """book_audit.audit over synthetic raw arrays (audit_images.build_image) of the clamps script's book
    — a bid at INT64_MIN, an ask at INT64_MAX — with the window at the bottom and at the top of int64."""
    from tests.audit_images import build_image

    for b0 in (I64_MIN, pe.top_base(L)):
        case = pe.clamps(L, b0)
        m = ReduceBook(2)
        for a in case.batches[:3]:
            m.submit(a)
        sc = bq.Script(int(case.batches[2].seq.max()) + 1)
        for j in range(20):  # a few more orders next to each end, so that the image has chunks to spare
            sc.new(0, pe.BUY, I64_MIN + j % 5, 2)
            sc.new(0, pe.SELL, I64_MAX - j % 5, 2)
        extra = sc.take()
        m.submit(extra)
        last = int(extra.seq.max())
        for base0 in (I64_MIN, pe.top_base(L)):
            raw = build_image(m, L, [base0, pe.OTHER], last)
            assert int(raw["sym"]["base"][0]) == base0
            v, books = audit(raw, last_seq=last)
            assert not v, v[:5]
            for s in range(2):
                want = m.dump(s)
                assert len(books[s]) == len(want) and np.all(books[s] == want), s
            assert raw["sym"]["nfar"][0].sum() > 0  # one end of the book lies 2^64 - L away, in a far level


# ---- the directed scripts ----------------------------------------------------------------------------------------

def _tape(f):
    return [(int(x["taker_seq"]), int(x["maker_seq"]), int(x["price_q4"]), int(x["qty"])) for x in f]


@pytest.mark.parametrize("L", SCRIPT_LEVELS)
def test_scripts_do_what_they_say(L):
    cases = pe.script_cases(L)
    assert tuple(cases) == pe.CASE_NAMES
    for name, build in cases.items():
        c = build()
        m = ReduceBook(c.S)
        assert len(c.batches) == len(c.want) == len(c.bases)
        for k, a in enumerate(c.batches):
            r, f = m.submit(a)
            assert _tape(f) == c.want[k], (name, k)
            assert int((a.symbol == 0).sum()) > 64, (name, k)  # above ME_HOT_MIN
            for (kb, i), w in c.status.items():
                if kb == k:
                    got = (int(r[i]["status"]), int(r[i]["reason"]), int(r[i]["filled_qty"]), int(r[i]["remaining_qty"]))
                    assert got == w, (name, k, i)
        got = [(int(e["seq"]), int(e["price_q4"]), int(e["qty"]), int(e["side"])) for e in m.dump(0)]
        assert got == c.rest, name


def test_scripts_reach_the_levels_and_prices_they_name():
    for L in SCRIPT_LEVELS:
        lv = pe.edge_levels(L)
        assert {0, 1, L - 2, L - 1} <= set(lv) and (L < 128 or {62, 63, 64, 65} <= set(lv))
    c = pe.window_edges(32768, I64_MAX)
    px = set(int(p) for a in c.batches for p in a.price_q4[a.symbol == 0])
    assert {I64_MAX, I64_MAX - 1, I64_MAX - 32767} <= px  # levels 32,767, 32,766 and 0 of the clamped window
    c = pe.clamps(128, I64_MIN)
    assert c.bases == [pe.top_base(128), I64_MIN, pe.top_base(128), I64_MIN]  # from one end to the other, four times
    c = pe.adjacent_far(128, -64)
    px = [int(p) for a in c.batches for p in a.price_q4[(a.symbol == 0) & ((a.kind & 8) == 0)]]
    assert -65 in px and 64 in px and all(b == -64 for b in c.bases)
    for up in (False, True):
        c = pe.recentres(128, -(1 << 31) - 64, up)
        assert c.bases[1] == -(1 << 31) - 64 + (64 if up else -65)


@pytest.mark.parametrize("L", [128, 32768])
def test_wrong_models_differ_on_the_alias_scripts(L):
    for name, build in pe.script_cases(L).items():
        if not name.startswith("aliases"):
            continue
        c = build()
        m = ReduceBook(c.S)
        exp = [m.submit(a) for a in c.batches]
        assert pe.differs(pe.Mod32Book, c.S, c.batches, exp), name
        assert pe.differs(pe.SentinelBook, c.S, c.batches, exp), name


# ---- the fixture ---------------------------------------------------------------------------------------------------

def test_fixture_replays_through_the_model():
    meta, batches, res, fills, book = load_model_fixture("price_edges.npz")
    S, L = meta["num_symbols"], meta["levels"]
    assert [int(b) for b in meta["base"]] == [int(b) for b in pe.bases(S, L)]
    m = ReduceBook(S)
    at_ends = 0
    for k, b in enumerate(batches):
        r, f = m.submit(b)
        same(r, res[k], FIELDS_RES, f"batch {k} results")
        same(f, fills[k], FIELDS_FILL, f"batch {k} tape")
        at_ends += int(np.isin(f["price_q4"], pe.EXTREMES).sum())
    dumps = np.concatenate([m.dump(s) for s in range(S)])
    same(dumps, book, FIELDS_BOOK, "final book")
    assert at_ends >= 50 and np.isin(book["price_q4"], (I64_MIN, I64_MAX)).sum() >= 2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "price_edges.npz")) < 128 * 1024
    # the file is what its generator makes today
    from tests.golden import make_price_edges_golden as gen

    base, arrays = gen.records()
    assert [int(x) for x in base] == [int(x) for x in meta["base"]] and len(arrays) == len(batches)
    for a, b in zip(arrays, batches):
        for fld in ("seq", "price_q4", "qty", "symbol", "kind"):
            assert np.array_equal(getattr(a, fld), getattr(b, fld)), fld
