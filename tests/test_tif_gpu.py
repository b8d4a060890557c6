"""IOC, FOK and POST_ONLY on every matching path against the model (tests/tif_model.py):
every batch's results and tape, the books of all symbols and the resting counters. Needs an MI355X.

Paths: k_match_reg (L = 128, ME_REG_AGG=0), the grouped walk (ME_REG_AGG=1, ME_GW_CANCEL=0), the cancel
walk (ME_GW_CANCEL=1), the deep generic kernel (L = 1,024, ME_HOT_MIN=0), the aggregate hot walk (L = 1,024,
a symbol above ME_HOT_MIN) and k_match_hot (L = 2,048, ME_HOT_AGG=0). An IOC priced inside the window runs
natively on the fast walks; FOK and POST_ONLY hand their symbol to the generic loops.
"""
import numpy as np
import pytest

from tests import tif_model as tm
from tests._parity import assert_fills_equal, assert_results_equal
from tests.gpu_harness import FEED_PATHS as PATHS, SMALL, as_batch, check_books, engine_on, pipelined
from tests.model_common import load_model_fixture
from tests.tif_model import TIF_FOK, TIF_GTC, TIF_IOC, TIF_POST_ONLY, TifBook, kind

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
ST_NEW, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 2, 3, 4

@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _engine(me, path, S, base, batches, **kw):
    return engine_on(me, path, S, base, batches, table=PATHS, **kw)


def _check_outputs(tb, batches, outs, ctx):
    exp = []
    for k, b in enumerate(batches):
        ro, fo = tb.submit(b)
        assert_results_equal(outs[k][0], ro, f"{ctx} batch {k}")
        assert_fills_equal(outs[k][1], fo, f"{ctx} batch {k}")
        exp.append((ro, fo))
    return exp


def _run(me, path, S, base, arrays, group=1, ctx="", env_over=None):
    """The batches through one engine of `path` (pipelined host batches in groups for L <= 128) against a
    fresh model; returns (engine stats, model)."""
    batches = [as_batch(me, a) for a in arrays]
    tb = TifBook(S)
    kw = {"batches_per_launch": group} if PATHS[path][3] else {}
    with _engine(me, path, S, base, batches, env_over=env_over, **kw) as eng:
        if PATHS[path][3]:
            outs = pipelined(eng, batches, 2 * group + 1)
        else:
            outs = [eng.submit_batch(b) for b in batches]
        _check_outputs(tb, arrays, outs, ctx)
        check_books(eng, tb, ctx)
        return eng.stats(), tb


# ---- scripted records ------------------------------------------------------------------------------

class Script:
    """Records appended in stream order; seqs ascend."""

    def __init__(self, seq0=1):
        self.seq = seq0
        self.r = []

    def new(self, s, side, px, q, tif=TIF_GTC, market=False):
        self.r.append((self.seq, px, q, s, kind(side, 1 if market else 0, 0, tif)))
        self.seq += 1
        return self.seq - 1

    def arrays(self):
        return tm.Arrays(*[[x[i] for x in self.r] for i in range(5)])


def _block_edges(base, L):
    """Symbol 0: FOKs at positions 0, 63 and 64 of its run (the one at 64 is killed only because the one at
    63, in the block before, took the liquidity). Symbol 1: POST_ONLYs at 0, 63 and 64 (the one at 64 would
    cross only because the one at 63 rested). The two runs are interleaved; symbol 2 trades in between."""
    m0, m1, m2 = (int(base[s]) + L // 2 for s in range(3))
    a, b = [], []  # per-symbol records: (side, px, q, tif)
    a.append((BUY, m0 + 5, 10, TIF_FOK))                                   # 0: empty book, killed
    a += [(SELL, m0 + 1 + i % 5, 10, TIF_GTC) for i in range(40)]          # 1..40: 400 on the ask side
    a += [(BUY, m0 - 1 - i % 5, 10, TIF_GTC) for i in range(22)]           # 41..62
    a.append((BUY, m0 + 5, 395, TIF_FOK))                                  # 63: fillable, leaves 5
    a.append((BUY, m0 + 5, 6, TIF_FOK))                                    # 64: killed, one short
    a.append((BUY, m0 + 5, 5, TIF_FOK))                                    # 65: exactly the rest
    a += [(SELL, m0 - 3, 35, TIF_IOC), (SELL, m0 - 9, 1000, TIF_FOK), (SELL, m0 - 5, 190, TIF_FOK)]
    b.append((BUY, m1 - 1, 5, TIF_POST_ONLY))                              # 0: empty side, rests
    b += [(SELL, m1 + 2 + i % 4, 7, TIF_GTC) for i in range(31)]           # 1..31
    b += [(BUY, m1 - 2 - i % 4, 7, TIF_GTC) for i in range(31)]            # 32..62
    b.append((BUY, m1 + 1, 5, TIF_POST_ONLY))                              # 63: inside the spread, rests
    b.append((SELL, m1 + 1, 5, TIF_POST_ONLY))                             # 64: would cross 63's order
    b.append((SELL, m1 + 2, 5, TIF_POST_ONLY))                             # 65: rests
    b += [(SELL, m1 + 1, 3, TIF_IOC), (BUY, m1 + 2, 1000, TIF_IOC)]
    sc = Script()
    for i in range(max(len(a), len(b))):
        for s, run in ((0, a), (1, b)):
            if i < len(run):
                sc.new(s, *run[i][:3], tif=run[i][3])
        sc.new(2, BUY if i % 2 else SELL, m2, 3, tif=(TIF_GTC, TIF_IOC)[i % 3 == 0])
    sc.new(0, BUY, 0, 5, tif=TIF_POST_ONLY, market=True)  # BAD_TIF
    sc.new(1, SELL, 0, 50, tif=TIF_FOK, market=True)
    return sc.arrays()


def _far_script(base, L):
    """Far levels and re-centring, one case per symbol (prices relative to the window [base, base + L))."""
    sc = Script()
    inw, far1, far2 = L - 28, L + 72, 2 * L + 44
    p = lambda s, off: int(base[s]) + off  # noqa: E731
    # 3: an IOC priced outside the window sweeps the window level, then far levels up to its limit
    sc.new(3, SELL, p(3, inw), 10)
    sc.new(3, SELL, p(3, far1), 10)
    sc.new(3, SELL, p(3, far2), 10)
    sc.new(3, BUY, p(3, far1 + 50), 25, tif=TIF_IOC)
    # 4: a FOK whose liquidity is partly far: short by 1, then exactly enough
    sc.new(4, SELL, p(4, inw), 10)
    sc.new(4, SELL, p(4, far1), 10)
    sc.new(4, SELL, p(4, far2), 10)
    sc.new(4, BUY, p(4, far1), 21, tif=TIF_FOK)
    sc.new(4, BUY, p(4, far1), 20, tif=TIF_FOK)
    sc.new(4, BUY, 0, 11, tif=TIF_FOK, market=True)  # only far2's 10 are left
    sc.new(4, BUY, 0, 10, tif=TIF_FOK, market=True)
    # 5: POST_ONLY against a side whose only levels are far; one that rests outside the window (re-centre)
    sc.new(5, BUY, p(5, 40), 10)
    sc.new(5, SELL, p(5, far2), 10)
    sc.new(5, BUY, p(5, far2), 5, tif=TIF_POST_ONLY)      # would cross the far ask
    sc.new(5, SELL, p(5, far2 + 90), 5, tif=TIF_POST_ONLY)  # rests far
    sc.new(5, BUY, p(5, far2 - 1), 5, tif=TIF_POST_ONLY)  # rests above the window: re-centres
    sc.new(5, SELL, p(5, far2 - 1), 5, tif=TIF_POST_ONLY)  # would cross it
    sc.new(5, SELL, p(5, 40), 12, tif=TIF_IOC)             # sweeps down to the old bid, now far below
    # 6: the mirror image on the bid side
    sc.new(6, BUY, p(6, 28), 10)
    sc.new(6, BUY, p(6, -72), 10)
    sc.new(6, BUY, p(6, -L - 44), 10)
    sc.new(6, SELL, p(6, -72), 21, tif=TIF_FOK)
    sc.new(6, SELL, p(6, -100), 15, tif=TIF_IOC)
    sc.new(6, SELL, p(6, -L - 44), 16, tif=TIF_FOK)
    sc.new(6, SELL, p(6, -L - 44), 15, tif=TIF_FOK)
    return sc.arrays()


def _native_then_verdict(base, L, seq0):
    """Symbols 7 and 8: twenty resting orders, then fifty in-window GTC, IOC and MARKET records (what every
    fast walk covers), and only then the first FOK (symbol 7) or POST_ONLY (symbol 8), followed by a few more
    of each kind. Each run is longer than 64 records."""
    sc = Script(seq0)
    for s, first in ((7, TIF_FOK), (8, TIF_POST_ONLY)):
        m = int(base[s]) + L // 2
        for i in range(10):
            sc.new(s, SELL, m + 1 + i % 5, 10)
            sc.new(s, BUY, m - 1 - i % 5, 10)
        for i in range(50):
            k = i % 5
            if k == 0:
                sc.new(s, BUY, m + 2, 4, tif=TIF_IOC)
            elif k == 1:
                sc.new(s, SELL, m + 3, 6)
            elif k == 2:
                sc.new(s, SELL, 0, 2, market=True)
            elif k == 3:
                sc.new(s, BUY, m - 2, 5)
            else:
                sc.new(s, SELL, m - 1, 3, tif=TIF_IOC)
        if first == TIF_FOK:
            sc.new(s, BUY, m + 5, 20, tif=TIF_FOK)
            sc.new(s, BUY, m + 5, 100000, tif=TIF_FOK)
            sc.new(s, SELL, m + 9, 5, tif=TIF_POST_ONLY)
        else:
            sc.new(s, BUY, m - 6, 5, tif=TIF_POST_ONLY)
            sc.new(s, BUY, m + 5, 5, tif=TIF_POST_ONLY)
            sc.new(s, SELL, m - 5, 25, tif=TIF_FOK)
        sc.new(s, BUY, m + 1, 7, tif=TIF_IOC)
        sc.new(s, SELL, m + 2, 7)
        sc.new(s, BUY, 0, 3, tif=TIF_FOK, market=True)
    return sc.arrays()


S_MIX = 12


@pytest.mark.parametrize("path", list(PATHS))
def test_scripted_batches_on_every_path(me, path):
    L = PATHS[path][0]
    base = tm.base_prices(S_MIX, L)
    arrays = [_block_edges(base, L)]
    far = _far_script(base, L)
    far.seq += np.uint64(int(arrays[0].seq.max()) + 1)
    arrays.append(far)
    arrays.append(_native_then_verdict(base, L, int(far.seq.max()) + 1))
    # the hot paths: every run of 64 records or more is a hot symbol's (symbols 0, 1, 2 of the first batch, 7 and
    # 8 of the third)
    hot = path in ("hot_agg", "hot")
    stats, tb = _run(me, path, S_MIX, base, arrays, ctx=f"scripted {path}", env_over={"ME_HOT_MIN": "64"} if hot else None)
    assert tb.resting() > 0
    # symbols 0 and 1 leave the hot walk at their first record (a FOK, a POST_ONLY), 7 and 8 at their first FOK /
    # POST_ONLY after seventy native records, symbol 2 (GTC and IOC only) never
    assert stats["hot_handoffs"] == (4 if hot else 0)


@pytest.mark.parametrize("path,group", [(p, g) for p in SMALL for g in (1, 8)] + [(p, 1) for p in PATHS if p not in SMALL])
def test_random_stream_on_every_path(me, path, group):
    L = PATHS[path][0]
    base, arrays = tm.tif_stream(7 + len(path), S_MIX, L, 7, 1500, far_pct=2, skew=True)
    stats, tb = _run(me, path, S_MIX, base, arrays, group=group, ctx=f"random {path} G={group}")
    assert tb.resting() > 0
    assert (stats["hot_handoffs"] > 0) == (path in ("hot_agg", "hot"))  # (the hot symbol was picked, and left)


def test_fixture_through_the_engine(me):
    meta, batches, res, fills, book = load_model_fixture("match_tif.npz")
    S = meta["num_symbols"]
    with _engine(me, "reg", S, meta["base"], [as_batch(me, a) for a in batches]) as eng:
        for k, a in enumerate(batches):
            r, f = eng.submit_batch(as_batch(me, a))
            assert_results_equal(r, res[k], f"fixture batch {k}")
            assert_fills_equal(f, fills[k], f"fixture batch {k}")
        dumps = np.concatenate([eng.dump(s) for s in range(S)])
        assert len(dumps) == len(book) and np.all(dumps == book)


@pytest.mark.parametrize("path", ["reg", "gwalk", "deep"])
def test_killed_and_rejected_change_nothing(me, path):
    L = PATHS[path][0]
    S = 8
    base, arrays = tm.tif_stream(31, S, L, 2, 1000, far_pct=2, mix=(70, 10, 0, 0, 10, 10))
    tb = TifBook(S)
    seq = int(max(a.seq.max() for a in arrays)) + 1
    with _engine(me, path, S, base, [as_batch(me, a) for a in arrays]) as eng:
        for a in arrays:
            eng.submit_batch(as_batch(me, a))
            tb.submit(a)
        sc = Script(seq)
        for s in range(S):
            d = tb.dump(s)
            bids, asks = d[d["side"] == BUY], d[d["side"] == SELL]
            assert len(bids) and len(asks)
            sc.new(s, BUY, int(asks["price_q4"].max()), int(asks["qty"].sum()) + 1, tif=TIF_FOK)
            sc.new(s, SELL, int(bids["price_q4"].min()), int(bids["qty"].sum()) + 1, tif=TIF_FOK)
            sc.new(s, BUY, 0, int(asks["qty"].sum()) + 1, tif=TIF_FOK, market=True)
            sc.new(s, BUY, int(asks["price_q4"].min()), 5, tif=TIF_POST_ONLY)
            sc.new(s, SELL, int(bids["price_q4"].max()) - 3, 5, tif=TIF_POST_ONLY)
            sc.new(s, SELL, 0, 5, tif=TIF_POST_ONLY, market=True)
        before = [eng.dump(s) for s in range(S)]
        rest0, hw0 = eng.resting_count(), eng.chunk_stats()["high_water"]
        a = sc.arrays()
        r, f = eng.submit_batch(as_batch(me, a))
        ro, fo = tb.submit(a)
        assert_results_equal(r, ro, path)
        assert len(f) == 0 and len(fo) == 0
        assert set(r["status"].tolist()) == {ST_CANCELED, ST_REJECTED} and not r["filled_qty"].any()
        for s in range(S):
            assert np.array_equal(eng.dump(s), before[s]), f"book of symbol {s} changed"
        assert eng.resting_count() == rest0 == eng.admission()["resting"]
        assert eng.chunk_stats()["high_water"] == hw0


@pytest.mark.parametrize("path", SMALL)
def test_in_window_ioc_runs_natively(me, path):
    """LIMIT, IOC and MARKET records priced inside the window, no far levels, at most 128 records of a
    symbol per batch: the stream hands off nothing, with the bits and with them cleared."""
    S, L = 16, 128
    base, arrays = tm.tif_stream(5, S, L, 8, 1024, spread=20, bad_pct=0, mix=(50, 30, 0, 0, 20, 0),
                                 market_tifs=(0, 1))
    assert max(np.bincount(a.symbol).max() for a in arrays) <= 128
    assert sum(int((((a.kind >> 4) & 3) == TIF_IOC).sum()) for a in arrays) > 2000
    for a in arrays:
        a.kind &= 0x3F
    stats, _ = _run(me, path, S, base, arrays, group=4, ctx=f"native IOC {path}")
    assert stats["handoffs"] == 0
    plain = [tm.Arrays(a.seq, a.price_q4, a.qty, a.symbol, a.kind & 0x0F) for a in arrays]
    stats, _ = _run(me, path, S, base, plain, group=4, ctx=f"plain {path}")
    assert stats["handoffs"] == 0


@pytest.mark.parametrize("path", ["hot_agg", "hot"])
def test_hot_walks_take_ioc(me, path):
    """A hot symbol's LIMIT, IOC and MARKET records inside the window stay on the hot walk: nothing is handed
    to the generic loop (the random stream above shows the counter moving when a walk does hand off)."""
    S, L = 6, PATHS[path][0]
    base, arrays = tm.tif_stream(9, S, L, 4, 1500, spread=20, bad_pct=0, mix=(50, 30, 0, 0, 20, 0),
                                 market_tifs=(0, 1), skew=True)
    assert min(int(np.bincount(a.symbol)[0]) for a in arrays) >= 200  # symbol 0 is hot in every batch
    stats, _ = _run(me, path, S, base, arrays, ctx=f"hot IOC {path}")
    assert stats["hot_handoffs"] == 0


def test_full_book_accepts_ioc_and_fok(me):
    """An engine filled to max_resting matches a batch of IOCs and FOKs; a batch of GTC LIMITs is refused
    with ME_E_CAPACITY before and after, and the refusal is not sticky."""
    S, L, R = 4, 128, 512
    base = tm.base_prices(S, L)
    sc = Script()
    for i in range(R):
        s = i % S
        mid = int(base[s]) + L // 2
        sc.new(s, BUY if i % 2 else SELL, mid + (-1 - i % 7 if i % 2 else 1 + i % 7), 10)
    fill = sc.arrays()
    tb = TifBook(S)
    with me.Engine(S, L, base, max_batch=1024, max_resting=R, seq_ring=1 << 20) as eng:
        r, f = eng.submit_batch(as_batch(me, fill))
        tb.submit(fill)
        assert eng.admission()["resting"] == R

        def gtc(seq0):
            g = Script(seq0)
            for i in range(64):
                g.new(i % S, BUY, int(base[i % S]) + 10, 1)
            return g.arrays()

        with pytest.raises(me.EngineError) as ei:
            eng.submit_batch(as_batch(me, gtc(sc.seq)))
        assert ei.value.code == me.ME_E_CAPACITY
        t = Script(sc.seq)
        for i in range(400):
            s = i % S
            mid = int(base[s]) + L // 2
            side = SELL if i % 2 else BUY  # (the fill above left symbol s with the other side only)
            px = mid + (3 if side == BUY else -3)
            t.new(s, side, px, 1 + i % 25, tif=(TIF_IOC, TIF_FOK)[i % 3 == 0])
        a = t.arrays()
        r, f = eng.submit_batch(as_batch(me, a))
        ro, fo = tb.submit(a)
        assert_results_equal(r, ro, "IOC/FOK on a full book")
        assert_fills_equal(f, fo, "IOC/FOK on a full book")
        assert len(fo) > 100
        check_books(eng, tb, "full book")
        room = R - tb.resting()
        assert 0 < room < 512
        g = Script(t.seq)
        for i in range(room + 1):
            g.new(i % S, BUY, int(base[i % S]) + 10, 1)
        with pytest.raises(me.EngineError) as ei:
            eng.submit_batch(as_batch(me, g.arrays()))
        assert ei.value.code == me.ME_E_CAPACITY
        p = Script(t.seq)  # POST_ONLY may rest: it counts
        for i in range(room + 1):
            p.new(i % S, BUY, int(base[i % S]) + 10, 1, tif=TIF_POST_ONLY)
        with pytest.raises(me.EngineError) as ei:
            eng.submit_batch(as_batch(me, p.arrays()))
        assert ei.value.code == me.ME_E_CAPACITY
        check_books(eng, tb, "after the refusals")


@pytest.mark.parametrize("path", SMALL)
def test_device_batches_one_group(me, path):
    S, L = 12, 128
    base, arrays = tm.tif_stream(41, S, L, 8, 1200, far_pct=2, skew=True)
    batches = [as_batch(me, a) for a in arrays]
    tb = TifBook(S)
    total = sum(len(b) for b in batches)
    # every record of a device batch counts as one that may rest
    with _engine(me, path, S, base, batches, batches_per_launch=8, max_resting=2 * total + 1024) as eng:
        dbs = [eng.upload(b) for b in batches]
        try:
            for db in dbs:
                eng.submit_device(db)
            eng.sync()
            assert eng.last_group_size() == 8
            outs = [eng.fetch_group_outputs(k, len(b)) for k, b in enumerate(batches)]
        finally:
            for db in dbs:
                db.free()
        _check_outputs(tb, arrays, outs, f"device {path}")
        check_books(eng, tb, f"device {path}")
