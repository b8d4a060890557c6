"""The order-query model (tests/order_query_model.py) on hand-written books and on a randomized stream. No GPU.

1. The A(10), B(10), C(10) example of test_reduced_order_keeps_its_priority, before and after reducing A by 4,
   over the native oracle (before) and the REDUCE model (before and after).
2. Levels of both sides: *better* counts the levels and quantities listed before the order's own.
3. A randomized stream of a few thousand records (cancels, reduces, far prices, a drifting mid): after every
   batch the two ways of computing *ahead* agree, and the answers are consistent with the dump they came from.
"""
import numpy as np
import pytest

from tests import order_query_model as oq
from tests import reduce_model as rm
from tests import tif_model as tm
from tests.big_qty import Script
from tests.reduce_model import ReduceBook

BUY, SELL = 1, 2


def _row(a, seq):
    i = np.nonzero(a["seq"] == seq)[0]
    assert len(i) == 1
    return a[i[0]]


def _pos(r):
    return (int(r["found"]), int(r["qty"]), int(r["qty_ahead"]), int(r["orders_ahead"]), int(r["level_qty"]))


def test_abc_before_and_after_reducing_a(built):
    from oracle.oracle import OracleBook

    L = 128
    base = tm.base_prices(1, L)
    p = int(base[0]) + L // 2
    sc = Script()
    A, B, C = (sc.new(0, BUY, p, 10) for _ in range(3))
    first = sc.take()
    sc.reduce(0, A, 4)
    second = sc.take()
    seqs = [A, B, C, 0, C + 1]
    for book in (OracleBook(1), ReduceBook(1)):
        book.submit(first)
        e = oq.expected(book, 1, seqs)
        assert [_pos(_row(e, x)) for x in (A, B, C)] == [(1, 10, 0, 0, 30), (1, 10, 10, 1, 30), (1, 10, 20, 2, 30)]
        assert all(int(r["side"]) == BUY and int(r["price_q4"]) == p and int(r["symbol"]) == 0 for r in e[:3])
        assert not e["qty_better"][:3].any() and not e["levels_better"][:3].any()
        for r in e[3:]:
            assert int(r["found"]) == 0 and all(int(r[f]) == 0 for f in oq.FIELDS if f != "seq")
        assert [int(x) for x in e["seq"]] == seqs
    book = ReduceBook(1)
    book.submit(first)
    r, _ = book.submit(second)
    assert int(r[0]["status"]) == 0 and int(r[0]["remaining_qty"]) == 6
    e = oq.expected(book, 1, seqs)
    # A keeps its place and holds 6; the ones behind it lose exactly 4 of qty_ahead and keep orders_ahead
    assert [_pos(_row(e, x)) for x in (A, B, C)] == [(1, 6, 0, 0, 26), (1, 10, 6, 1, 26), (1, 10, 16, 2, 26)]


def test_better_levels_and_symbol_ids():
    L, S = 128, 2
    base = tm.base_prices(S, L)
    m = int(base[1]) + L // 2
    sc = Script()
    b1 = sc.new(1, BUY, m - 1, 5)
    b2 = sc.new(1, BUY, m - 3, 7)
    b2b = sc.new(1, BUY, m - 3, 1)
    b3 = sc.new(1, BUY, m - 50 * L, 9)  # far below
    a1 = sc.new(1, SELL, m + 2, 4)
    a2 = sc.new(1, SELL, m + 70 * L, 6)  # far above
    other = sc.new(0, SELL, int(base[0]) + 5, 3)
    book = ReduceBook(S)
    book.submit(sc.take())
    e = oq.expected(book, S, [b1, b2, b2b, b3, a1, a2, other], symbol_ids=[700, 900])
    got = [(int(r["side"]), int(r["levels_better"]), int(r["qty_better"]), int(r["level_qty"]), int(r["qty_ahead"]),
            int(r["symbol"])) for r in e]
    assert got == [(BUY, 0, 0, 5, 0, 900), (BUY, 1, 5, 8, 0, 900), (BUY, 1, 5, 8, 7, 900), (BUY, 2, 13, 9, 0, 900),
                   (SELL, 0, 0, 4, 0, 900), (SELL, 1, 4, 6, 0, 900), (SELL, 0, 0, 3, 0, 700)]


def test_int64_quantities():
    big = 2**31 - 1
    L = 128
    base = tm.base_prices(1, L)
    p = int(base[0]) + L // 2
    sc = Script()
    hi = [sc.new(0, BUY, p, big) for _ in range(3)]
    lo = [sc.new(0, BUY, p - 1, big) for _ in range(3)]
    book = ReduceBook(1)
    book.submit(sc.take())
    e = oq.expected(book, 1, hi + lo)
    assert int(e[2]["qty_ahead"]) == 4_294_967_294 == 2 * big
    assert int(e[5]["qty_better"]) == 3 * big and int(e[5]["qty_ahead"]) == 2 * big and int(e[5]["level_qty"]) == 3 * big


@pytest.mark.parametrize("seed", [1, 2])
def test_both_ways_of_computing_ahead_agree_on_a_random_stream(seed):
    S, L = 6, 128
    _, arrays = rm.reduce_stream(4100 + seed, S, L, 6, 600, far_pct=3, drift=3, skew=True)
    assert sum(len(a) for a in arrays) >= 3000
    book = ReduceBook(S)
    used = set()
    seen_partial = 0
    for k, a in enumerate(arrays):
        book.submit(a)
        used.update(int(x) for x in a.seq)
        q = sorted(used) + [max(used) + 1 + 7 * i for i in range(64)]
        e = oq.expected(book, S, q)
        by_seq = oq.ahead_by_seq(book, S)
        live = {int(s): hit for s, hit in book.live.items()}
        assert int(e["found"].sum()) == len(live) == len(by_seq), k
        for r in e:
            seq = int(r["seq"])
            if not int(r["found"]):
                assert seq not in live
                assert all(int(r[f]) == 0 for f in oq.FIELDS if f != "seq")
                continue
            s, side, price, entry = live[seq]
            assert (int(r["symbol"]), int(r["side"]), int(r["price_q4"]), int(r["qty"])) == (s, side, price, entry[1])
            assert (int(r["qty_ahead"]), int(r["orders_ahead"])) == by_seq[seq], (k, seq)
            assert int(r["level_qty"]) >= int(r["qty_ahead"]) + int(r["qty"]) > 0
        # per side: levels_better is the level's rank and qty_better the sum of the totals before it
        for s in range(S):
            for side in (BUY, SELL):
                rows = [r for r in e if int(r["found"]) and int(r["symbol"]) == s and int(r["side"]) == side]
                lv = {}
                for r in rows:
                    lv[int(r["price_q4"])] = (int(r["level_qty"]), int(r["levels_better"]), int(r["qty_better"]))
                prices = sorted(lv, reverse=side == BUY)
                run = 0
                for rank, px in enumerate(prices):
                    assert lv[px][1:] == (rank, run), (k, s, side, px)
                    run += lv[px][0]
        seen_partial += sum(1 for i, t, d, had in book.reduces if had is not None and d < had)
    assert seen_partial > 10
