"""The resident book's structural invariants on every matching path (tests/book_audit.py).
Needs an MI355X.

Every other GPU test checks what the engine says (results, tapes, the book k_book_snapshot dumps). Here the
engine runs `reduce_stream` against `ReduceBook` as those suites do and, after EVERY launch group, the raw
device arrays are exported (Engine.debug_export) and audited: no violation, and the book rebuilt from raw
memory == the model's dump == Engine.dump. Each scenario asserts that it exercised what it is for and prints
its figures. No test provokes a device error: every stream is one the parity suites consider valid.
"""
import functools

import numpy as np
import pytest

from tests import book_audit as ba
from tests import reduce_model as rm
from tests import tif_model as tm
from tests.audit_run import Run
from tests.book_audit import audit, names
from tests.gpu_harness import PATHS, engine_on
from tests.reduce_model import ReduceBook
from tests.tif_model import kind

pytestmark = pytest.mark.gpu

BUY, SELL = 1, 2
ST_CANCELED = 3
RING = 1 << 20


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


@functools.lru_cache(maxsize=None)
def _stream(seed, S, L, nb, n, **kw):
    """(base, batches): shared between the tests, nobody changes the arrays. More resting LIMITs than
    tif_stream's default mix, close to the mid, half of the records on symbol 0: books a few hundred orders deep
    whose busiest levels span several chunks."""
    kw.setdefault("far_pct", 2)
    kw.setdefault("mix", (60, 8, 4, 8, 5, 15))
    kw.setdefault("spread", 5)
    kw.setdefault("skew", True)
    return rm.reduce_stream(seed, S, L, nb, n, **kw)


def _peak(S, arrays):
    """max_resting at the stream's own need: the resting orders before each batch plus its records that may rest."""
    model, need = ReduceBook(S), 0
    for a in arrays:
        may = int(np.count_nonzero(((a.kind & 0x0C) == 0) & ((((a.kind >> 4) ^ (a.kind >> 5)) & 1) == 0)))
        need = max(need, model.resting() + may)
        model.submit(a)
    return need


def _engine(me, path, S, base, arrays, group=1, ring=RING, env=None, **kw):
    kw.setdefault("max_resting", _peak(S, arrays) + group * max(len(a) for a in arrays) + 1024)
    kw.setdefault("max_batch", max(4096, max(len(a) for a in arrays)))  # (room for the drain's cancels)
    return engine_on(me, path, S, base, arrays, ring=ring, env_over=env, group=group, **kw)


def _groups(arrays, g):
    return [arrays[i:i + g] for i in range(0, len(arrays), g)]


def _drain(run, mode, max_batch):
    """Empty every book through the engine: cancels of every live order (each must answer CANCELED), or one
    MARKET per side and symbol that takes the whole side. Then the image must be empty."""
    model = run.model
    assert model.resting() > 0
    if mode == "cancel":
        recs = [(run.last_seq, q, 0, hit[0], kind(BUY, 0, 1)) for q, hit in sorted(model.live.items())]
        for i in range(0, len(recs), max_batch):
            part = recs[i:i + max_batch]
            res, _ = run.group([tm.Arrays(*[[r[j] for r in part] for j in range(5)])], f"drain cancels {i}")
            assert (res[0]["status"] == ST_CANCELED).all(), f"{run.ctx}: a live order could not be cancelled"
    else:
        recs, q = [], run.last_seq + 1
        for s in range(run.S):
            d = model.dump(s)
            for side, have in ((SELL, BUY), (BUY, SELL)):  # a SELL takes the bids
                total = int(d["qty"][d["side"] == have].sum())
                if total:
                    recs.append((q, 0, total, s, kind(side, 1, 0)))
                    q += 1
        run.group([tm.Arrays(*[[r[j] for r in recs] for j in range(5)])], "drain markets")
    assert model.resting() == 0
    raw = run.eng.debug_export()
    left = ba.is_drained(raw)
    assert not left, f"{run.ctx}: after the drain ({mode}): {left}"
    assert audit.last["linked_chunks"] == 0 and audit.last["live_orders"] == 0


# ---- 1. every path ---------------------------------------------------------------------------------------------------

# levels: (symbols, batches, records per batch, stream keywords)
SHAPES = {
    128: (8, 64, 512, dict(drift=1)),
    256: (8, 8, 900, dict()),
    1024: (6, 8, 900, dict(far_pct=1)),
    2048: (6, 8, 900, dict(far_pct=1)),
}
EVERY = [("reg", 1), ("reg", 8), ("gwalk", 1), ("gwalk", 4), ("gwalk_cx", 1), ("gwalk_cx", 4), ("deep256", 1),
         ("deep", 1), ("hot_agg", 1), ("hot", 1)]


def _path_stream(path, group):
    L = PATHS[path][0]
    S, nb, n, kw = SHAPES[L]
    base, arrays = _stream(7100 + L, S, L, nb, n, **kw)
    if PATHS[path][3]:
        arrays = arrays[:max(8, 8 * group)]  # eight groups (G = 1: eight batches)
    return S, base, arrays


@pytest.mark.parametrize("drain", ["cancel", "market"])
@pytest.mark.parametrize("path,group", EVERY)
def test_every_path(me, path, group, drain):
    S, base, arrays = _path_stream(path, group)
    with _engine(me, path, S, base, arrays, group) as eng:
        run = Run(me, eng, S, PATHS[path][3], f"{path} G={group}")
        for k, g in enumerate(_groups(arrays, group)):
            run.group(g, f"group {k}")
        st = eng.stats()
        print(f"every_path {path} G={group}: {st} checkpoints {len(run.raws)} "
              f"live {[f['live_orders'] for f in run.raws]} chunks {[f['linked_chunks'] for f in run.raws]} "
              f"nfar {[f['nfar'] for f in run.raws]} multi {[f['multi'] for f in run.raws]}")
        assert len(run.raws) >= 8
        assert max(f["live_orders"] for f in run.raws) > 200 and max(f["nfar"] for f in run.raws) > 0
        assert max(f["multi"] for f in run.raws) > 0  # some level's FIFO spans chunks
        if PATHS[path][3]:
            assert st["handoffs"] > 0
        if path in ("hot", "hot_agg"):
            assert st["hot_handoffs"] > 0
        run.done()
        _drain(run, drain, eng.max_batch)
        run.done()


# ---- 2. path changes on one book -------------------------------------------------------------------------------------

def _plain(a):
    """The records no grouped walk hands off for: GTC / IOC LIMITs and MARKETs."""
    keep = ((a.kind & 8) == 0) & (((a.kind >> 4) & 2) == 0)
    return tm.Arrays(a.seq[keep], a.price_q4[keep], a.qty[keep], a.symbol[keep], a.kind[keep])


def test_automatic_flip_plain_walk_to_cancel_walk(me, monkeypatch):
    """L = 128, ME_REG_AGG and ME_GW_CANCEL unset, a configuration whose shape picks the grouped path: three
    groups without cancels, reduces, FOK or POST_ONLY run on the plain walk; the full stream then hands symbols
    off and the engine switches to the walk that covers cancels. Audited after each group."""
    monkeypatch.delenv("ME_REG_AGG", raising=False)
    monkeypatch.delenv("ME_GW_CANCEL", raising=False)
    S, G = 16, 4
    base, arrays = _stream(7301, S, 128, 12 * G, 1024, far_pct=0, skew=False)
    arrays = [_plain(a) if k < 3 * G else a for k, a in enumerate(arrays)]
    with me.Engine(S, 128, base, max_batch=8192, max_resting=_peak(S, arrays) + G * 1024 + 1024, seq_ring=RING,
                   batches_per_launch=G) as eng:
        run = Run(me, eng, S, True, "auto flip")
        seen = []
        for k, g in enumerate(_groups(arrays, G)):
            run.group(g, f"group {k}")
            seen.append(eng.paths())
        print("auto flip:", [(p["grouped_agg"], p["grouped_cancels"]) for p in seen], eng.stats())
        assert all(p["grouped_agg"] and not p["grouped_cancels"] for p in seen[:3]), seen[:3]
        assert any(p["grouped_agg"] and p["grouped_cancels"] for p in seen[3:]), seen
        assert eng.stats()["handoffs"] > 0
        run.done()


def test_handoffs_mid_group(me):
    """The grouped walk at G = 4 on a stream whose only hand-off cause is a far LIMIT (no cancel, reduce, FOK
    or POST_ONLY record): a symbol leaves the walk in the middle of a group and the continuation finishes it."""
    S, G = 8, 4
    base, arrays = _stream(7302, S, 128, 8 * G, 512, far_pct=6, mix=(60, 20, 0, 0, 20, 0), fresh_pct=0, bad_pct=0)
    assert not any(((a.kind & 8) != 0).any() for a in arrays)
    with _engine(me, "gwalk", S, base, arrays, G) as eng:
        run = Run(me, eng, S, True, "hand-offs mid-group")
        for k, g in enumerate(_groups(arrays, G)):
            run.group(g, f"group {k}")
        print("mid-group hand-offs:", eng.stats(), [f["nfar"] for f in run.raws])
        assert eng.stats()["handoffs"] > 0 and max(f["nfar"] for f in run.raws) > 0
        run.done()


def test_hot_then_generic_then_hot(me):
    """L = 1,024, ME_HOT_MIN = 64: in the even batches every symbol has more than 64 records (the hot aggregate
    walk), in the odd ones fewer (k_match): one book goes hot -> generic -> hot. The hot hand-off counter moves in
    every hot batch (its walk meets a cancel or a REDUCE) and stands still in every generic one."""
    S, nb = 4, 10
    base, arrays = _stream(7303, S, 1024, nb, 640, skew=False)
    arrays = [a if k % 2 == 0 else tm.Arrays(a.seq[:160], a.price_q4[:160], a.qty[:160], a.symbol[:160], a.kind[:160])
              for k, a in enumerate(arrays)]
    for k, a in enumerate(arrays):
        cnt = np.bincount(a.symbol[a.symbol < S], minlength=S)
        assert (cnt > 64).all() if k % 2 == 0 else (cnt < 64).all(), (k, cnt)
    with _engine(me, "hot_agg", S, base, arrays) as eng:
        run = Run(me, eng, S, False, "hot/generic")
        hh = [0]
        for k, a in enumerate(arrays):
            run.group([a], f"batch {k}")
            hh.append(eng.stats()["hot_handoffs"])
        d = np.diff(hh)
        print("hot/generic: hot hand-offs per batch", d.tolist())
        assert (d[0::2] > 0).all() and (d[1::2] == 0).all(), d
        run.done()


# ---- 3. re-centring -----------------------------------------------------------------------------------------------------

def _pull_far_level_in(run, s, up, L):
    """Two scripted batches on symbol s: a LIMIT that rests just outside the window (above it when `up`), then an
    opposite LIMIT beyond the window's edge and short of that price, large enough to take everything standing
    before it and rest 3: the rest would break Invariant I, so the window re-centres onto it and the far level
    three ticks further comes into the window."""
    base = int(run.raws[-1]["base"][s])
    d = run.model.dump(s)
    if up:
        p_far, p_in, far_side, in_side = base + L + 5, base + L + 2, SELL, BUY
        before = d[(d["side"] == SELL) & (d["price_q4"] <= p_in)]
    else:
        p_far, p_in, far_side, in_side = base - 6, base - 3, BUY, SELL
        before = d[(d["side"] == BUY) & (d["price_q4"] >= p_in)]
    q = run.last_seq + 1
    run.group([tm.Arrays([q], [p_far], [7], [s], [kind(far_side, 0, 0)])], f"symbol {s}: a far level placed")
    assert p_far in run.raws[-1]["far"][s], "the scripted level should rest outside the window"
    run.group([tm.Arrays([q + 1], [p_in], [int(before["qty"].sum()) + 3], [s], [kind(in_side, 0, 0)])],
              f"symbol {s}: re-centre onto the far level")
    assert {p_far, p_in} <= run.raws[-1]["win"][s], "the window should have re-centred over both prices"


@pytest.mark.parametrize("drain", ["cancel", "market"])
@pytest.mark.parametrize("path,group", [("reg", 1), ("gwalk_cx", 2), ("deep256", 1)])
def test_recentring(me, path, group, drain):
    """Prices drift by 2.5 windows over the run, upwards for even symbols and downwards for odd ones: every
    window re-centres again and again and levels leave it for the far regions. What stands in the market's way is
    traded through before the window arrives, so far levels re-entering the window are scripted at the end: one
    above symbol 0's window, one below symbol 1's."""
    L = PATHS[path][0]
    S, nb = 4, 10 * group
    step = (5 * L // 2) // nb + 1  # 2.5 windows over the run: a window trails the market by up to L / 2
    base, arrays = _stream(7400 + L, S, L, nb, 512, drift=step, far_pct=5)
    with _engine(me, path, S, base, arrays, group) as eng:
        run = Run(me, eng, S, PATHS[path][3], f"recentre {path}")
        for k, g in enumerate(_groups(arrays, group)):
            run.group(g, f"group {k}")
        bases = np.array([f["base"] for f in run.raws])
        _pull_far_level_in(run, 0, True, L)
        _pull_far_level_in(run, 1, False, L)
        nfar = np.array([f["nfar_sides"] for f in run.raws], dtype=np.int64)  # [checkpoint][symbol * 2 + side]
        moved = bases[-1] - np.asarray(base)
        # price levels that were in the window at one checkpoint and far at the next, and the other way round
        out = sum(len(a["win"][s] & b["far"][s]) for a, b in zip(run.raws, run.raws[1:]) for s in range(S))
        back = sum(len(a["far"][s] & b["win"][s]) for a, b in zip(run.raws, run.raws[1:]) for s in range(S))
        print(f"recentre {path}: window moves {moved.tolist()} base changes "
              f"{(np.diff(bases, axis=0) != 0).sum(axis=0).tolist()} levels window -> far {out}, far -> window {back}; "
              f"nfar per side {nfar.T.tolist()}")
        assert (moved[0::2] > L).all() and (moved[1::2] < -L).all(), moved
        assert ((np.diff(bases, axis=0) != 0).sum(axis=0) >= 2).all()
        assert out > 0 and back > 0, (out, back)
        assert (np.diff(nfar, axis=0) > 0).any() and (np.diff(nfar, axis=0) < 0).any(), nfar.T
        run.done()
        _drain(run, drain, eng.max_batch)
        run.done()


# ---- 4. far arena ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path,group", [("reg", 4), ("gwalk", 4), ("deep", 1)])
def test_far_arena_after_collections(me, path, group):
    """Eight inline far levels and a collection trigger of 64 arena entries, 20 % far LIMITs on a drifting
    market: sides outgrow their regions again and again and k_seq_sweep collects the arena between groups. The
    audit right after a collection sees disjoint regions in the active half and small sides back inline."""
    L = PATHS[path][0]
    S, nb = 4, 12 * group if group > 1 else 12
    base, arrays = _stream(7500 + L, S, L, nb, 512, drift=3, far_pct=20)
    with _engine(me, path, S, base, arrays, group, env={"ME_FAR_GC_AT": "64"}, far_levels=8) as eng:
        run = Run(me, eng, S, PATHS[path][3], f"far arena {path}")
        after_gc, prev = 0, 0
        for k, g in enumerate(_groups(arrays, group)):
            run.group(g, f"group {k}")
            c = eng.far_stats()["collections"]
            after_gc += c > prev  # the sweep ahead of this group collected: this audit is the first after it
            prev = c
        st = eng.far_stats()
        print(f"far arena {path}: {st} audits right after a collection {after_gc} moved sides "
              f"{[f['moved'] for f in run.raws]} nfar {[f['nfar'] for f in run.raws]}")
        assert st["moves"] > 4 and st["collections"] > 2, st
        assert after_gc > 2 and max(f["moved"] for f in run.raws) > 0
        run.done()


# ---- 5. chunk reclamation ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["reg", "gwalk", "deep"])
def test_chunk_partition_after_reclamation(me, path):
    """Liquidity migrates between symbols: symbol s rests R orders at R prices (a chunk each), a MARKET sweeps
    them, the next symbol does the same. max_resting is the stream's own peak and max_chunks the default, so the
    pool only lasts because k_seq_sweep reclaims the free chunks; the partition is audited after every batch."""
    L = PATHS[path][0]
    S, R = 4, 300
    base = tm.base_prices(S, L)
    arrays, q = [], 1
    for cyc in range(8):
        s = cyc % S
        p0 = int(base[s]) + L // 2
        arrays.append(tm.Arrays(np.arange(q, q + R), [p0 + k for k in range(R)], [1 + k % 3 for k in range(R)], [s] * R,
                                [kind(SELL, 0, 0)] * R))
        q += R
        arrays.append(tm.Arrays([q], [0], [10 * R], [s], [kind(BUY, 1, 0)]))
        q += 1
    need = _peak(S, arrays)
    with _engine(me, path, S, base, arrays, 4, max_resting=need, max_batch=1024) as eng:
        assert eng.chunk_stats()["pool"] == need + 32 * S + 64
        run = Run(me, eng, S, False, f"reclaim {path}")  # (synchronous batches: every batch is its own group)
        after, prev = 0, 0
        for k, a in enumerate(arrays):
            run.group([a], f"batch {k}")
            c = eng.chunk_stats()["reclaims"]
            after += c > prev
            prev = c
        cs = eng.chunk_stats()
        print(f"reclaim {path}: {cs} audits right after a reclamation {after}")
        assert cs["reclaims"] > 0 and after > 0 and cs["high_water"] <= cs["pool"]
        run.done()


# ---- 6. ring wrap ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("drain", ["cancel", "market"])
@pytest.mark.parametrize("path", ["reg", "gwalk_cx", "deep256"])
def test_ring_wrap(me, path, drain):
    """seq_ring = 1,024 and seqs above 2^40: the horizon moves every other batch and k_seq_sweep rebuilds the
    old-order table; live orders older than the horizon exist at the audit points and are found in it."""
    L = PATHS[path][0]
    S, nb = 4, 12
    base, arrays = _stream(7600 + L, S, L, nb, 480, seq_start=(1 << 40) + 7)
    with _engine(me, path, S, base, arrays, 1, ring=1024) as eng:
        run = Run(me, eng, S, PATHS[path][3], f"ring wrap {path}")
        for k, a in enumerate(arrays):
            run.group([a], f"batch {k}")
        hz = [f["horizon"] for f in run.raws]
        old = [f["old_orders"] for f in run.raws]
        print(f"ring wrap {path}: horizons {[h - (1 << 40) if h else 0 for h in hz]} old orders {old}")
        assert len(set(hz)) > 3 and max(old) > 0 and hz[-1] > 1 << 40
        run.done()
        _drain(run, drain, eng.max_batch)
        run.done()


# ---- 8. the auditor bites on real images ------------------------------------------------------------------------------

def test_auditor_reports_corruptions_of_a_real_image(me):
    """One real export of the register kernel's book; five single-field corruptions of the HOST copy (nothing
    is written back to the device) are each reported under their invariant's name."""
    from tests.audit_images import corrupt

    S, base, arrays = _path_stream("reg", 1)
    with _engine(me, "reg", S, base, arrays[:4], 1) as eng:
        run = Run(me, eng, S, True, "real image")
        for k, a in enumerate(arrays[:4]):
            _, raw = run.group([a], f"batch {k}")
        run.done()
        for name in ("total + 1", "a loc entry pointing at another slot", "a linked chunk also in an fcache row",
                     "occ bit of an occupied level cleared", "resting - 1"):
            bad, inv = corrupt(raw, name)
            v, _ = audit(bad, last_seq=run.last_seq)
            assert inv in names(v), (name, names(v))
        assert not audit(raw, last_seq=run.last_seq)[0]
        # the export's capacity check
        import ctypes as C

        nb = C.c_size_t(0)
        small = np.zeros(8, dtype=np.uint8)
        assert eng.lib.me_debug_export(eng.h, 0, small.ctypes.data, small.nbytes, C.byref(nb)) == me.ME_E_INVALID
        assert nb.value == S * 128 * 16 and not small.any()
        assert eng.lib.me_debug_export(eng.h, 99, None, 0, None) == me.ME_E_INVALID
