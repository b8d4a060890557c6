"""Prices at the ends of int64, windows across 0, +-2^31 and 2^32, alias distances and the window's own boundary
levels on every matching path ("price range") against the model (tests/reduce_model.py, Python
ints). Needs an MI355X. Bit-exact; no tolerances; every stream is valid input.

Every case checks each batch's results and tape and, after every launch group, all books (Engine.dump and the book
rebuilt from the raw device arrays), the resting counters and the auditor's invariants over the raw arrays
(tests/book_audit.py). The inputs are tests/price_edges.py's; that they reach the prices they are meant to reach
is asserted on the CPU (tests/test_price_edges_model.py), that the ENGINE's windows went where the inputs send
them is asserted here from the exported bases.
"""
import numpy as np
import pytest

from tests import big_qty as bq
from tests import depth_model as dm
from tests import order_query_model as oq
from tests import price_edges as pe
from tests import quote_model as qm
from tests._parity import assert_fills_equal, assert_results_equal, side_levels
from tests.audit_run import Run
from tests.gpu_harness import PATHS, SMALL, as_batch, engine_on, pipelined
from tests.model_common import load_model_fixture
from tests.price_edges import I64_MAX, I64_MIN
from tests.reduce_model import ReduceBook

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
S = pe.S_EDGE
DEEP = [p for p in PATHS if not PATHS[p][3]]


@pytest.fixture(scope="module")
def me(built):
    import matching_engine_amd

    return matching_engine_amd


def _bases(eng):
    return [int(b) for b in eng.debug_export(["sym"])["sym"]["base"]]


def _group(run, arrays, tag):
    """One launch group through engine and model (Run.group), then the device-wide resting counter; returns the
    ENGINE's (results, fills) per batch."""
    bs = [as_batch(run.me, a) for a in arrays]
    if run.grouped:
        tickets = [run.eng.submit_host(b) for b in bs]
        outs = [run.eng.collect(t) for t in tickets]
    else:
        outs = [run.eng.submit_batch(b) for b in bs]
    for k, (a, (r, f)) in enumerate(zip(arrays, outs)):
        ro, fo = run.model.submit(a)
        assert_results_equal(r, ro, f"{run.ctx} {tag} batch {k}")
        assert_fills_equal(f, fo, f"{run.ctx} {tag} batch {k}")
        if a.seq.max():
            run.last_seq = max(run.last_seq, int(a.seq.max()))
    run.checkpoint(tag)
    assert run.eng.resting_count() == run.eng.admission()["resting"] == run.model.resting(), f"{run.ctx} {tag}: resting"
    return outs


def _dead(last):
    return [0, last + 1, last + 64, last + 12345, 1 << 63, (1 << 63) + 5, U64_MAX - 1, U64_MAX]


def _final(eng, model, nsym, used, ctx, D=4):
    """levels_all, snapshot, book_orders and order_query of every seq ever used against the model."""
    lv, cnt = eng.levels_all(D)
    for s in range(nsym):
        want = bq.model_snapshot(model, s, 10)
        got = eng.snapshot(s, 10)
        d = model.dump(s)
        ob, oa, lb, la = eng.book_orders(s, 3)
        for k, side in enumerate("ba"):
            for f in ("price_q4", "total_qty", "order_count"):
                assert np.array_equal(got[k][f], want[k][f]), f"{ctx}: snapshot {side} of symbol {s}: {f}"
                assert np.array_equal(lv[s, k, :cnt[s, k]][f], want[k][:D][f]), f"{ctx}: levels_all {side} of {s}: {f}"
                assert np.array_equal((lb, la)[k][f], want[k][:3][f]), f"{ctx}: book_orders levels {side} of {s}: {f}"
            assert cnt[s, k] == min(D, len(want[k]))
            exp = side_levels(d, k + 1, 3)
            have = (ob, oa)[k]
            assert len(have) == len(exp) and np.all(have == exp), f"{ctx}: book_orders {side} of symbol {s}"
    q = np.array(sorted(used) + _dead(max(used)), dtype=np.uint64)
    oq.assert_answers_equal(eng.order_query(q), oq.expected(model, nsym, q), f"{ctx}: order_query")


def _window_coverage(base, L, seen, model, ctx):
    """From the engine's exported bases (`seen`: one list per checkpoint, the first taken before any record)."""
    top = pe.top_base(L)
    assert seen[0] == [min(int(b), top) for b in base], f"{ctx}: initial bases (INT64_MAX must start clamped)"
    assert int(base[2]) == I64_MAX and seen[0][2] == top
    assert any(I64_MIN in row for row in seen) and any(top in row for row in seen)
    assert all(I64_MIN <= b <= top for row in seen for b in row)
    forced = pe.forced_moves(base, L, model)
    assert forced and max(forced.values()) >= 1 << 32, f"{ctx}: the stream should force a window across 2^32"
    for s, dist in forced.items():
        assert abs(seen[-1][s] - seen[0][s]) >= dist, f"{ctx}: symbol {s}: base {seen[0][s]} -> {seen[-1][s]}"


# ---- 1. the streams on every path ------------------------------------------------------------------------------------

MODES = [(p, g, m) for p in SMALL for g in (1, 8) for m in ("host", "pipelined")] + [(p, 8, "device") for p in SMALL] + \
    [(p, 1, "sync") for p in DEEP]


@pytest.mark.parametrize("d", pe.DRAWS)
@pytest.mark.parametrize("path,group,mode", MODES)
def test_streams(me, path, group, mode, d):
    """edge_stream's draws: S = 8, 6 batches of 600 (the device group: 8 of 1,200). Grouped paths, launch groups of
    1 and 8: host batches collected group by group with every check after each group ("host"), the same batches
    kept 2 G + 1 in flight with the checks at the end ("pipelined"), and one group of eight device batches; deep
    and hot paths: synchronous batches. far_levels = 8, so that sides outgrow their inline far regions and the
    arena holds levels at these prices too."""
    name = "l128_dev" if mode == "device" else pe.PATH_STREAM[path]
    L = pe.STREAMS[name][0]
    assert L == PATHS[path][0]
    base, arrays, exp, final, _ = pe.stream(name, d)
    ctx = f"{name}#{d} {path} G={group} {mode}"
    grouped = PATHS[path][3]
    kw = {"batches_per_launch": group} if grouped else {}
    if mode == "device":  # (every record of a device batch counts as one that may rest)
        kw["max_resting"] = 2 * sum(len(a) for a in arrays) + 1024
    used = set(int(x) for a in arrays for x in a.seq)
    with engine_on(me, path, S, base, arrays, far_levels=8, **kw) as eng:
        run = Run(me, eng, S, grouped, ctx)
        seen = [_bases(eng)]
        if mode in ("device", "pipelined"):
            if mode == "pipelined":
                outs = pipelined(eng, [as_batch(me, a) for a in arrays], 2 * group + 1)
            else:
                dbs = [eng.upload(as_batch(me, a)) for a in arrays]
                try:
                    for db in dbs:
                        eng.submit_device(db)
                    eng.sync()
                    assert eng.last_group_size() == len(arrays) == group
                    outs = [eng.fetch_group_outputs(k, len(a)) for k, a in enumerate(arrays)]
                finally:
                    for db in dbs:
                        db.free()
            for k, (ro, fo) in enumerate(exp):
                assert_results_equal(outs[k][0], ro, f"{ctx} batch {k}")
                assert_fills_equal(outs[k][1], fo, f"{ctx} batch {k}")
            run.model, run.last_seq = final, max(used)  # (shared: only read from here on)
            run.checkpoint("the end")
            assert eng.resting_count() == eng.admission()["resting"] == final.resting()
            seen.append([int(b) for b in run.raws[-1]["base"]])
        else:
            for g in range(0, len(arrays), group):
                _group(run, arrays[g:g + group], f"group {g // group}")
                seen.append([int(b) for b in run.raws[-1]["base"]])
                _final(eng, run.model, S, used, f"{ctx} group {g // group}")  # (seqs still to come: not found)
        run.done()
        _final(eng, run.model, S, used, ctx)
        _window_coverage(base, L, seen, run.model, ctx)
        st, fs = eng.stats(), eng.far_stats()
        print(f"{ctx}: {st} {fs} nfar {[f['nfar'] for f in run.raws]} moved sides {[f['moved'] for f in run.raws]}")
        assert max(f["nfar"] for f in run.raws) > 0 and fs["moves"] > 0, fs
        if path in ("gwalk", "gwalk_cx"):
            assert st["handoffs"] > 0, st
        if path in ("hot_agg", "hot"):
            assert st["hot_handoffs"] > 0, st


# ---- 2. the directed scripts -----------------------------------------------------------------------------------------

# configuration: (path, window size); every path at its own size, k_match_reg at the smallest window and the hot
# aggregate walk at 32,768 levels (level 32,767 is the top of the ladder walks' level field)
CONFIGS = {p: (p, PATHS[p][0]) for p in PATHS}
CONFIGS["reg_l64"] = ("reg", 64)
CONFIGS["hot_agg_l32768"] = ("hot_agg", 32768)


def _tape(f):
    return [(int(x["taker_seq"]), int(x["maker_seq"]), int(x["price_q4"]), int(x["qty"])) for x in f]


@pytest.mark.parametrize("name", pe.CASE_NAMES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_scripts(me, config, name):
    """Every directed case of price_edges.script_cases, one batch per launch: besides equality with the model, the
    ENGINE's fills (who, at which price), the named records' outcomes, what rests at the end and — where the script
    pins it — the window base after each batch are compared with what the script wrote out by hand."""
    path, L = CONFIGS[config]
    case = pe.script_cases(L)[name]()
    ctx = f"{name} {config}"
    grouped = PATHS[path][3]
    kw = {"batches_per_launch": 1} if grouped else {}
    used = set(int(x) for a in case.batches for x in a.seq)
    with engine_on(me, path, case.S, case.base, case.batches, levels=L, **kw) as eng:
        assert eng.config()["levels"] == L
        run = Run(me, eng, case.S, grouped, ctx)
        assert _bases(eng)[0] == min(int(case.base[0]), pe.top_base(L))
        counter = "hot_handoffs" if path in ("hot_agg", "hot") else "handoffs"
        hand = [eng.stats()[counter]]
        for k, a in enumerate(case.batches):
            (r, f), = _group(run, [a], f"batch {k}")
            hand.append(eng.stats()[counter])
            assert _tape(f) == case.want[k], f"{ctx}: fills of batch {k}"
            for (kb, i), w in case.status.items():
                if kb == k:
                    got = (int(r[i]["status"]), int(r[i]["reason"]), int(r[i]["filled_qty"]), int(r[i]["remaining_qty"]))
                    assert got == w, f"{ctx}: batch {k} record {i}: {got}, scripted {w}"
            if case.bases[k] is not None:
                assert int(run.raws[-1]["base"][0]) == case.bases[k], f"{ctx}: base after batch {k}"
        run.done()
        got = [(int(e["seq"]), int(e["price_q4"]), int(e["qty"]), int(e["side"])) for e in eng.dump(0)]
        assert got == case.rest, f"{ctx}: what rests"
        _final(eng, run.model, case.S, used, ctx)
        if name.startswith("window_edges") and path in ("gwalk", "gwalk_cx", "hot_agg", "hot"):
            # batches 0, 1 and 3 hold in-window GTC / IOC LIMITs and MARKETs only, fewer than 128 of a symbol, and no
            # far level exists: the fast walk covers every record (a_classify), so it ran the edge and word-boundary
            # levels itself; batch 2's cancels are what the plain walk and the hot walks hand off
            d = np.diff(hand)
            assert d[0] == d[1] == d[3] == 0, f"{ctx}: hand-offs per batch {d.tolist()}"
            assert (d[2] > 0) == (path != "gwalk_cx"), f"{ctx}: hand-offs per batch {d.tolist()}"
        if path in ("hot_agg", "hot"):  # more than ME_HOT_MIN records of symbol 0 a batch: its hot walk started, and
            assert eng.stats()["hot_handoffs"] > 0  # met a record it hands off (a cancel, a far price, a FOK)
        if name.startswith(("adjacent_far", "clamps")):  # (an alias order rests and trades within one batch: its
            assert max(f["nfar"] for f in run.raws) > 0   # level is a far one because the pinned base never moves)


# ---- 3. the feeds ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["reg", "gwalk_cx", "deep", "hot_agg"])
def test_feeds(me, path):
    """The quote feed and the depth feed (D = 4), enabled before the stream: replaying every event gives exactly
    the model's tops and top-4 views at every drain point (after each launch) and at the end."""
    name = pe.PATH_STREAM[path]
    base, arrays, exp, _, _ = pe.stream(name, 0)
    D = 4
    model = ReduceBook(S)
    view = bq.Snap(model)
    kw = {"batches_per_launch": 1} if PATHS[path][3] else {}
    with engine_on(me, path, S, base, arrays, **kw) as eng:
        eng.quotes_enable(4 * S * (len(arrays) + 2))
        eng.depth_enable(D, 8 * D * S * (len(arrays) + 2))
        table, maps = qm.tops(qm._Empty(), S), dm.empty_maps(S)
        ends = 0
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
            ends += int((np.isin(want["bid_price_q4"], pe.EXTREMES) & (want["flags"] & 1 != 0)).sum() +
                        (np.isin(want["ask_price_q4"], pe.EXTREMES) & (want["flags"] & 2 != 0)).sum())
        assert ends > 0  # a top of book at the end of int64 was compared
        assert eng.quotes_stats()["deferred"] == 0 and eng.depth_stats()["deferred"] == 0


# ---- 4. the fixture ----------------------------------------------------------------------------------------------------

def test_fixture_through_the_engine(me):
    meta, batches, res, fills, book = load_model_fixture("price_edges.npz")
    n = meta["num_symbols"]
    with engine_on(me, "reg", n, meta["base"], batches) as eng:
        for k, a in enumerate(batches):
            r, f = eng.submit_batch(as_batch(me, a))
            assert_results_equal(r, res[k], f"fixture batch {k}")
            assert_fills_equal(f, fills[k], f"fixture batch {k}")
        dumps = np.concatenate([eng.dump(s) for s in range(n)])
        assert len(dumps) == len(book) and np.all(dumps == book)


# ---- 5. the service ------------------------------------------------------------------------------------------------------

def test_service_orders_at_the_top_price(me, tmp_path):
    """me_service_submit_order at the largest raw price that normalises to INT64_MAX Q4 (INT64_MAX at scale 4; one
    decimal fewer overflows and is refused in band): a SELL and a BUY there cross, and the rest of the SELL shows
    at that price in GetOrderBook and MarketData."""
    LIMIT, BUY, SELL = 0, 1, 2
    with me.Engine(1, 128, [1_000_000], max_batch=64, max_resting=64) as eng:
        svc = me.MatchingEngineService(eng, ["SYM"], db_path=str(tmp_path / "top.sqlite"))
        assert svc.submit_order("M", "SYM", LIMIT, SELL, I64_MAX, 4, 10)["order_id"] == "OID-1"
        assert svc.submit_order("T", "SYM", LIMIT, BUY, I64_MAX, 4, 4)["order_id"] == "OID-2"
        r = svc.submit_order("T", "SYM", LIMIT, BUY, I64_MAX, 3, 1)
        assert not r["success"] and not r["order_id"] and r["error_message"] == "overflow"
        seq, res, fills = svc.flush()
        assert seq.tolist() == [1, 2] and res["status"].tolist() == [0, 2] and res["filled_qty"].tolist() == [0, 4]
        assert [(int(x["taker_seq"]), int(x["maker_seq"]), int(x["price_q4"]), int(x["qty"])) for x in fills] == \
            [(2, 1, I64_MAX, 4)]
        bids, asks = svc.order_book("SYM")
        assert bids == [] and [(o["order_id"], o["price"], o["quantity"]) for o in asks] == [("OID-1", I64_MAX, 6)]
        lb, la = svc.get_order_book("SYM", 4)
        assert len(lb) == 0 and [(int(x["price_q4"]), int(x["total_qty"])) for x in la] == [(I64_MAX, 6)]
        md = svc.market_data("SYM")
        assert md["has_ask"] and not md["has_bid"] and md["best_ask"] == I64_MAX and md["ask_size"] == 6
        svc.close()
