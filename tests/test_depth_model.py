"""The depth feed's test model (tests/depth_model.py) over the CPU oracle, and the feed's C-ABI surface.
Runs on CPU."""
import ctypes as C

import numpy as np
import pytest

from tests import depth_model as dm
from tests import quote_model as qm

S, NB, BATCH = 6, 20, 200


@pytest.fixture(scope="module")
def stream(built):
    """A config-5-style stream: cancels, MARKET sweeps, 3 % far prices."""
    import matching_engine_amd as me

    sc = me.preset(5, num_symbols=S, levels=128, batch=BATCH, cancel_pct=30, market_pct=15, market_qty_mult=4,
                   far_pct=3, zipf_s=1.1, seed=11)
    st = me.Stream(sc)
    return [st.next(BATCH) for _ in range(NB)]


@pytest.mark.parametrize("D", [1, 5, 32])
def test_replaying_the_models_events_gives_the_snapshot(built, stream, D):
    from oracle import oracle

    ob = oracle.OracleBook(S)
    model = dm.DepthModel(ob, S, D)
    maps = dm.empty_maps(S)
    assert len(model.expect(0)) == 0
    total = 0
    for k, b in enumerate(stream):
        ob.submit(b)
        assert len(model.peek()) > 0
        ev = model.expect(k + 1)
        assert (ev["batches"] == k + 1).all() and not ev["pad"].any()
        # at most 2 D events per side, sides in order, priority order inside a side
        key = ev["symbol"].astype(np.int64) * 2 + (ev["side"] == dm.SELL)
        assert np.all(np.diff(key) >= 0)
        for x in np.unique(key):
            e = ev[key == x]
            assert len(e) <= 2 * D
            d = np.diff(e["price_q4"])
            assert np.all(d < 0) if x % 2 == 0 else np.all(d > 0)
        total += len(ev)
        dm.replay(maps, ev)
        assert dm.same_views(maps, dm.views(ob, S, D)), f"D={D} after batch {k + 1}"
        if D == 1:  # the depth-1 view is the quote
            t = qm.tops(ob, S)
            for s in range(S):
                bid = [(int(t[s]["bid_price_q4"]), int(t[s]["bid_qty"]))] if t[s]["flags"] & qm.HAS_BID else []
                ask = [(int(t[s]["ask_price_q4"]), int(t[s]["ask_qty"]))] if t[s]["flags"] & qm.HAS_ASK else []
                assert sorted(maps[s][0].items()) == bid and sorted(maps[s][1].items()) == ask
    assert total > NB
    assert len(model.peek()) == 0


def test_pushed_out_and_back_in_the_model(built):
    from matching_engine_amd import _abi
    from oracle import oracle
    from tests.tif_model import Arrays

    k = _abi.kind
    ob = oracle.OracleBook(1)
    m = dm.DepthModel(ob, 1, 2)
    ob.submit(Arrays([1, 2], [100, 99], [5, 6], [0, 0], [k(1), k(1)]))
    ev = m.expect(1)
    assert [(int(e["price_q4"]), int(e["qty"])) for e in ev] == [(100, 5), (99, 6)]
    ob.submit(Arrays([3], [101], [7], [0], [k(1)]))  # a better level pushes 99 out: SET 101, DELETE 99
    ev = m.expect(2)
    assert [(int(e["price_q4"]), int(e["qty"])) for e in ev] == [(101, 7), (99, 0)]
    ob.submit(Arrays([4], [0], [7], [0], [k(2, 1)]))  # a MARKET takes 101: DELETE 101, 99 is SET again
    ev = m.expect(3)
    assert [(int(e["price_q4"]), int(e["qty"])) for e in ev] == [(101, 0), (99, 6)]
    assert (ev["side"] == dm.BUY).all()


def test_the_abi_declares_and_exports_the_depth_feed(built):
    from matching_engine_amd import _abi

    assert _abi.DEPTH_DTYPE == dm.DEPTH_DTYPE and _abi.DEPTH_DTYPE.itemsize == 32 and _abi.DEPTH_MAX == 32
    lib = C.CDLL(_abi.LIB_PATH)
    for name in ("me_depth_enable", "me_depth_read", "me_depth_stats", "me_service_depth_subscribe",
                 "me_service_depth_stream"):
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
    # a null engine or service is refused, not dereferenced
    lib = _abi.load()
    assert lib.me_depth_enable(None, 5, 16) == _abi.ME_E_INVALID
    assert lib.me_depth_read(None, None, 0, None, None) == _abi.ME_E_INVALID
    assert lib.me_depth_stats(None, None, None, None) == _abi.ME_E_INVALID
    assert lib.me_service_depth_subscribe(None, 3) == _abi.ME_E_INVALID
    assert lib.me_service_depth_stream(None, None, None, 0, None) == _abi.ME_E_INVALID
