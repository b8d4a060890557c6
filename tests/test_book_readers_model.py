"""The book of tests/book_readers.py against the CPU oracle: its orders rest where the scenario says, so that
tests/test_book_readers_gpu.py walks the levels it means to walk. No GPU.
"""
import numpy as np
import pytest

from tests import book_readers as br

BUY, SELL = br.BUY, br.SELL


def _prices(dump, side):
    """The side's live prices in dump order (best first), each once."""
    out = []
    for p in dump[dump["side"] == side]["price_q4"].tolist():
        if not out or out[-1] != p:
            out.append(p)
    return out


@pytest.mark.parametrize("L", br.LS)
def test_orders_rest_where_the_scenario_says(built, L):
    from oracle.oracle import OracleBook

    sn = br.scenario(L)
    ob = OracleBook(sn.S)
    for k, a in enumerate(sn.batches):
        res, fills = ob.submit(a)
        assert len(fills) == 0, f"batch {k}: the scenario trades"
        assert not (res["status"] == 4).any(), f"batch {k}: a record was rejected"
    for s in range(sn.S):
        lo, hi = int(sn.base[s]), int(sn.base[s]) + L
        d = ob.dump(s)
        for side in (BUY, SELL):
            win, far = sn.window[(s, side)], sn.far[(s, side)]
            # window levels inside the window the engine is created with (nothing asks for a re-centre: every
            # bid of a symbol is below every ask, and both far sides lie outside), far prices outside it
            assert all(lo <= p < hi for p in win) and not any(lo <= p < hi for p in far)
            assert all(p < lo for p in far) if side == BUY else all(p >= hi for p in far)
            assert _prices(d, side) == win + far, f"symbol {s} side {side}"
    for s, side, px in sn.cancelled:
        d = ob.dump(s)
        assert not ((d["side"] == side) & (d["price_q4"] == px)).any(), f"cancelled level {px} of symbol {s} is live"
        live = sn.window[(s, side)] + sn.far[(s, side)]
        assert min(live) < px < max(live), "a cancelled level lies between live ones"
    assert len(sn.far[(0, SELL)]) == len(sn.far[(1, BUY)]) == br.NFAR == 70 and len(sn.far[(2, BUY)]) == 68
    assert len(sn.far[(2, SELL)]) == 5 and not sn.far[(0, BUY)] and not sn.far[(1, SELL)]
    assert len(ob.dump(3)) == 0
    # the hard window levels are there: both sides of every 64-level and 4,096-level boundary the window has
    asks0 = {p - int(sn.base[0]) for p in sn.window[(0, SELL)]}
    bids1 = {L - 1 - (p - int(sn.base[1])) for p in sn.window[(1, BUY)]}
    assert asks0 == bids1 == set(br.ask_levels(L))
    assert {63, 64, L - 65, L - 64, L - 3} <= asks0 and (L < 8192 or {4095, 4096} <= asks0)
    assert len(np.unique(np.concatenate([a.seq[(a.kind & 8) == 0] for a in sn.batches]))) == len(sn.seqs)
