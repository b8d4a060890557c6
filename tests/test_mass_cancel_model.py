"""The mass cancel's model (tests/mass_cancel_model.py) on the native oracle and on the REDUCE model. No GPU.

The helper's CANCEL batch leaves the asked sides empty, every cancel is CANCELED with remaining_qty = the
entry's quantity (apply() asserts it), a one-sided purge leaves the other side's dump unchanged, and a cancel
of a purged order is REJECTED / UNKNOWN_ORDER afterwards.
"""
import numpy as np
import pytest

from tests import mass_cancel_model as mc
from tests import tif_model as tm
from tests.big_qty import Script
from tests.reduce_model import ReduceBook

BUY, SELL = 1, 2
ST_REJECTED, RJ_UNKNOWN = 4, 5
S, L = 4, 128


def _books():
    from oracle.oracle import OracleBook

    return [OracleBook(S), ReduceBook(S)]


def _script():
    """Symbols 0..2 with bids and asks on several levels (two orders on some, far prices, a price <= 0);
    symbol 3 never used."""
    base = tm.base_prices(S, L)
    sc = Script()
    for s in range(3):
        m = int(base[s]) + L // 2
        for j in range(6):
            sc.new(s, BUY, m - 1 - j, 10 + j)
            sc.new(s, SELL, m + 1 + j, 20 + j)
            if j % 2:
                sc.new(s, BUY, m - 1 - j, 3)
                sc.new(s, SELL, m + 1 + j, 4)
        sc.new(s, BUY, m - 5 * L, 7)
        sc.new(s, SELL, m + 5 * L, 8)
    sc.new(2, BUY, 0, 9)
    sc.new(2, BUY, -17, 9)
    return sc


@pytest.mark.parametrize("which", [0, 1])
def test_the_cancel_batch_empties_the_asked_sides(built, which):
    book = _books()[which]
    sc = _script()
    book.submit(sc.take())
    last = sc.next - 1
    before = [book.dump(s) for s in range(S)]
    assert all(len(before[s]) > 10 for s in range(3)) and len(before[3]) == 0
    # one side of symbol 2, nothing of symbol 3 (never used): the other sides stay as they were
    ent, counts = mc.apply(book, [2, 3], [BUY, 3], last)
    assert counts.tolist() == [[int((before[2]["side"] == BUY).sum()), 0], [0, 0]]
    assert np.array_equal(ent, before[2][before[2]["side"] == BUY])
    assert np.array_equal(book.dump(2), before[2][before[2]["side"] == SELL])
    assert np.array_equal(book.dump(0), before[0]) and np.array_equal(book.dump(1), before[1])
    # several symbols, non-ascending, both sides
    ent, counts = mc.apply(book, [1, 0], 3, last)
    assert np.array_equal(ent, np.concatenate([before[1], before[0]]))
    assert counts.sum() == len(before[0]) + len(before[1])
    assert len(book.dump(0)) == 0 and len(book.dump(1)) == 0
    # again: nothing rests there, no batch
    a, ent, counts = mc.cancel_batch(book, [1, 0], 3, last)
    assert a is None and len(ent) == 0 and not counts.any()
    # a cancel of a purged order is unknown; the same symbol trades again
    sc.cancel(0, int(before[0]["seq"][0]))
    m = int(tm.base_prices(S, L)[0]) + L // 2
    x = sc.new(0, SELL, m + 1, 5)
    sc.new(0, BUY, m + 1, 5)
    r, f = book.submit(sc.take())
    assert (int(r[0]["status"]), int(r[0]["reason"])) == (ST_REJECTED, RJ_UNKNOWN)
    assert len(f) == 1 and int(f[0]["maker_seq"]) == x and int(f[0]["qty"]) == 5
    assert book.resting() == int((before[2]["side"] == SELL).sum())


def test_the_helper_refuses_what_the_engine_refuses(built):
    book = ReduceBook(S)
    with pytest.raises(AssertionError):
        mc.expected(book, [1, 1], 3)
    with pytest.raises(AssertionError):
        mc.expected(book, [1], 0)
    with pytest.raises(AssertionError):
        mc.expected(book, [1], 4)
