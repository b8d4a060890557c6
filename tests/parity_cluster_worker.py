"""One rank of the cluster-parity checks (launched by tests/test_cluster_parity.py): the depth feed, the trade
feed, the order query and the order preview over the C++ cluster (include/me_cluster.h), and the service over
me_cluster_matcher using them. Every comparison is exact, against ONE oracle book holding every global symbol.

Rank 0 drives; the other ranks serve. Phases, on one cluster:
  A  direct calls, two slices in flight: depth at D = 5 and D = 1 (re-enabled on resting books, D = 33 refused),
     trades, order query (chunked: more seqs than max_batch), order preview (chunked; books untouched; a CANCEL
     kind refused without a command; after phase B: the promise kept by a submit)
  B  through me_cluster_matcher's hooks, all three feeds on: only the quotes drained for four slices, then
     depth and trades; then depth drained every slice and the quotes last. Every event's `batches` must be the
     number of the slice that produced it.
  C  a service over me_cluster_matcher next to a service over one book: depth_stream, trades_stream,
     order_status, preview_order.

env: RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT; argv: KIND OUT_JSON
  oracle:  oracle shards with model-backed hooks (me_shard_ops), TCP transport
  nohook:  oracle shards, the last rank's without `depth`: me_cluster_depth_enable is ME_E_INVALID, not sticky
  gpu:     HIP engine shards on device 0, TCP transport
  rccl:    a HIP engine shard over RCCL, world size 1
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import depth_model as dm  # noqa: E402
from tests import order_query_model as oqm  # noqa: E402
from tests import preview_model as pvm  # noqa: E402
from tests import quote_model as qm  # noqa: E402
from tests import trade_model as tm  # noqa: E402
from tests.cluster_worker import OracleShard  # noqa: E402

U64_MAX = 2**64 - 1
S, L, MB, MR = 40, 128, 1024, 1 << 16
E_INVALID = -1


def check(cond, msg):
    if not cond:
        raise AssertionError(msg)


class _Log:
    """A feed's unread events: read(cap) honours cap / left as quote_model.OracleFeed does."""

    def __init__(self, dtype):
        self.ev = np.zeros(0, dtype=dtype)

    def add(self, ev):
        self.ev = np.concatenate([self.ev, ev])

    def read(self, cap):
        k = min(int(cap), len(self.ev))
        out, self.ev = self.ev[:k], self.ev[k:]
        return out, len(self.ev)


class QueryHooks:
    """order_query / order_preview / trades / quotes over the shard's oracle book: local symbol ids, `batches`
    = the parts matched."""

    def _init_hooks(self):
        self.n, self.nb = max(len(self.ids), 1), 0
        self.row = {int(g): i for i, g in enumerate(self.ids)}
        self.depth_m = self.trade_m = None
        self.dlog, self.tlog = _Log(dm.DEPTH_DTYPE), _Log(tm.TRADE_DTYPE)
        self.qfeed = qm.OracleFeed(self.ob, self.n)

    def match(self, b):
        res, tape = super().match(b)
        self.nb += 1
        self.qfeed.matched()
        if self.depth_m is not None:
            self.dlog.add(self.depth_m.expect(self.nb))
        if self.trade_m is not None:
            self.trade_m.feed(tape)
            ev = self.trade_m.expect(self.nb)
            ev["symbol"] = [self.row[int(g)] for g in ev["symbol"]]  # the fills carry global ids
            self.tlog.add(ev)
        return res, tape

    def quotes(self, cap):
        return self.qfeed.quotes(cap)

    def trades_enable(self, cap):
        self.tlog = _Log(tm.TRADE_DTYPE)
        self.trade_m = tm.TradeModel(self.n, symbol_ids=self.ids if len(self.ids) else None) if cap else None

    def trades(self, cap):
        if self.trade_m is None:
            raise ValueError("trade feed off")
        return self.tlog.read(cap)

    def order_query(self, seqs):
        return oqm.expected(self.ob, self.n, seqs)

    def order_preview(self, symbol, kind, price_q4, qty):
        return pvm.expected(self.ob, self.n, list(zip(symbol.tolist(), kind.tolist(), price_q4.tolist(), qty.tolist())))


class DepthHooks:
    def depth_enable(self, depth, cap):
        if depth > 32:
            raise ValueError("depth above ME_DEPTH_MAX")
        self.dlog = _Log(dm.DEPTH_DTYPE)
        self.depth_m = None
        if depth and cap:
            self.depth_m = dm.DepthModel(self.ob, self.n, depth)
            self.dlog.add(self.depth_m.expect(self.nb))

    def depth(self, cap):
        if self.depth_m is None:
            raise ValueError("depth feed off")
        return self.dlog.read(cap)


class ParityShard(QueryHooks, DepthHooks, OracleShard):
    def __init__(self, ids):
        OracleShard.__init__(self, ids)
        self._init_hooks()


class NoDepthShard(QueryHooks, OracleShard):
    def __init__(self, ids):
        OracleShard.__init__(self, ids)
        self._init_hooks()


class FullBook(ParityShard):
    """One book holding every symbol, with every hook, as a me_matcher (cluster.python_matcher)."""

    def __init__(self):
        super().__init__(np.arange(S, dtype=np.uint32))
        self.num_symbols, self.max_batch, self.max_resting = S, MB, 4 * MR

    def c_matcher(self):
        from matching_engine_amd.cluster import python_matcher

        return python_matcher(self)


class Driver:
    """Rank 0: the cluster, the reference book, and every slice sent so far."""

    def __init__(self, me, cl, st, sc):
        from oracle.oracle import OracleBook

        self.me, self.cl, self.st, self.sc = me, cl, st, sc
        self.ref = OracleBook(S)
        self.sent = []      # every batch the cluster matched, in order (slice number = index + 1)
        self.tapes = []     # ... and its tape
        self.last_seq = 0

    def next_batch(self):
        b = self.st.next(self.sc.batch)
        self.last_seq = int(b.seq[-1])
        return b

    def apply(self, b, res, tape, ctx):
        ro, fo = self.ref.submit(b)
        check(len(tape) == len(fo) and np.array_equal(tape, fo), f"{ctx}: tape differs from one book's")
        for x in ("filled_qty", "remaining_qty", "fill_count", "tape_offset", "status", "reason"):
            check(np.array_equal(res[x], ro[x]), f"{ctx}: results.{x} differs from one book's")
        self.sent.append(b)
        self.tapes.append(fo)
        return ro, fo

    def run(self, batches, ctx):
        """Two in flight; returns after every slice is collected and applied to the reference."""
        pend = []
        for k, b in enumerate(batches):
            pend.append((self.cl.submit(b), b))
            if len(pend) == 2 or k == len(batches) - 1:
                while pend:
                    t, bb = pend.pop(0)
                    res, tape = self.cl.collect(t, len(bb))
                    self.apply(bb, res, tape, f"{ctx} slice {len(self.sent) + 1}")

    def one(self, b, ctx):
        res, tape = self.cl.match(b)
        return self.apply(b, res, tape, ctx)


def expect_code(fn, code, what):
    from matching_engine_amd.cluster import ClusterError

    try:
        fn()
    except ClusterError as e:
        check(e.code == code, f"{what}: code {e.code}, expected {code}")
        return
    raise AssertionError(f"{what}: no error")


def check_depth(d, maps, D, ctx):
    ev = d.cl.depth_drain()
    check(not len(ev) or int(ev["symbol"].max()) < S, f"{ctx}: a depth event's symbol is outside the global ids")
    dm.replay(maps, ev)
    check(dm.same_views(maps, dm.views(d.ref, S, D)), f"{ctx}: the replayed depth events differ from one book's top {D}")
    return len(ev)


def phase_a(d, counts):
    cl, me = d.cl, d.me
    D = 5
    cl.depth_enable(D, 64 * D * S)
    cl.trades_enable(64 * S)
    check(len(cl.depth_drain()) == 0, "depth events on empty books")
    check(len(cl.trades_drain()) == 0, "trade events on empty books")
    maps = dm.empty_maps(S)
    tev, t_from = [], len(d.tapes)

    def check_trades(ctx):
        ev = cl.trades_drain()
        check(not len(ev) or int(ev["symbol"].max()) < S, f"{ctx}: a trade event's symbol is outside the global ids")
        tev.append(ev)
        counts["trade_events"] += len(ev)
        tm.replay(np.concatenate(tev), d.tapes[t_from:], S)

    d.run([d.next_batch() for _ in range(2)], "A")
    counts["depth_events"] += check_depth(d, maps, D, "A after slice 2")
    check_trades("A after slice 2")
    # D = 33 is refused by every shard and the cluster stays usable; enabling again on resting books replays
    # to the same views
    expect_code(lambda: cl.depth_enable(33, 4096), E_INVALID, "depth_enable(33)")
    cl.depth_enable(D, 64 * D * S)
    maps = dm.empty_maps(S)
    counts["depth_events"] += check_depth(d, maps, D, "A re-enabled at D = 5 on resting books")
    d.run([d.next_batch() for _ in range(2)], "A")
    counts["depth_events"] += check_depth(d, maps, D, "A after slice 4")
    check_trades("A after slice 4")
    D = 1
    cl.depth_enable(D, 64 * S)
    maps = dm.empty_maps(S)
    counts["depth_events"] += check_depth(d, maps, D, "A re-enabled at D = 1")
    d.run([d.next_batch() for _ in range(2)], "A")
    counts["depth_events"] += check_depth(d, maps, D, "A after slice 6 (D = 1)")
    check_trades("A after slice 6")
    cl.depth_enable(0, 0)
    cl.trades_enable(0)
    expect_code(cl.depth_drain, E_INVALID, "depth read with the feed off")

    # ---- order query: the last two slices' seqs, hostile seqs, duplicates; n > max_batch (chunked) and n small
    last = d.last_seq
    seqs = [int(x) for b in d.sent[-2:] for x in b.seq]
    seqs += [0, last + 1, last + 64, last + 12345, 1 << 63, (1 << 63) + 5, U64_MAX - 1, U64_MAX]
    seqs += seqs[:50] + seqs[-8:]
    check(len(seqs) > MB, "the seq list must exceed max_batch")
    q = np.array(seqs, dtype=np.uint64)
    want = oqm.expected(d.ref, S, seqs)
    check(int(want["found"].sum()) > 20, "the query list holds too few resting orders to mean anything")
    oqm.assert_answers_equal(cl.order_query(q), want, "order query (chunked)")
    small = np.concatenate([q[:300], q[-70:]])
    oqm.assert_answers_equal(cl.order_query(small), oqm.expected(d.ref, S, small.tolist()), "order query (one chunk)")
    check(len(cl.order_query(np.zeros(0, np.uint64))) == 0, "order query n == 0")
    counts["found"] = int(want["found"].sum())

    # ---- order preview
    rng = np.random.default_rng(5)
    mid = d.st.base_prices() + L // 2
    queries = []
    for s in range(S):
        for side in (1, 2):
            for market in (0, 1):
                for tif in range(4):
                    px = int(mid[s]) + int(rng.integers(-30, 31))
                    queries.append((s, me.kind(side, market, 0, tif), px, int(rng.integers(1, 400))))
    queries += [(S, me.kind(1), int(mid[0]), 10), (S + 5, me.kind(2, 1), 0, 10), (0xFFFFFFFF, me.kind(1), 5, 1),
                (3, me.kind(1), int(mid[3]), 0), (4, me.kind(2), int(mid[4]), -5), (S, me.kind(1), 1, 0)]
    queries = queries + queries[::-1]  # duplicates are independent queries; more than max_batch: chunked
    check(len(queries) > MB, "the query list must exceed max_batch")
    cols = [np.array([x[i] for x in queries]) for i in range(4)]
    books = [[x.tobytes() for x in cl.book_orders(s, 0)] for s in range(S)]
    got = cl.order_preview(*cols)
    pvm.assert_answers_equal(got, pvm.expected(d.ref, S, queries), "order preview (chunked)", queries)
    one = [np.array(c[:200]) for c in cols]
    pvm.assert_answers_equal(cl.order_preview(*one), pvm.expected(d.ref, S, queries[:200]), "order preview (one chunk)")
    bad = [np.array(c[-3:]) for c in cols]  # only symbols no shard owns: rank 0 answers alone
    pvm.assert_answers_equal(cl.order_preview(*bad), pvm.expected(d.ref, S, queries[-3:]), "order preview (unknown symbols)")
    check([[x.tobytes() for x in cl.book_orders(s, 0)] for s in range(S)] == books, "a preview changed a book")
    st0 = cl.stats()
    for k8 in (me.kind(1, 0, 1), me.KIND_REDUCE):
        c2 = [np.array(c[:5]) for c in cols]
        c2[1] = c2[1].copy()
        c2[1][3] = k8
        expect_code(lambda: cl.order_preview(*c2), E_INVALID, "preview of a CANCEL / REDUCE kind")
    check(cl.stats() == st0, "a refused preview issued a command")
    counts["previews"] = len(queries)
    return queries


def promise(d, queries):
    """Submit the same record next and get what the preview said (after the stream's last slice: the records
    take the seqs that follow it)."""
    cl, me = d.cl, d.me
    kept = 0
    for i in (0, 4, 20, 40, 68, 100, 224, 332, 480, 612):  # GTC records: the reference book knows no other
        s, kd, px, qty = queries[i]
        check((kd >> 4) & 3 == 0, "the promise checks use GTC records")
        row = cl.order_preview([s], [kd], [px], [qty])[0]
        d.last_seq += 1
        b = me.Batch([d.last_seq], [px], [qty], [s], [kd])
        ro, fo = d.one(b, f"A promise {i}")
        pvm.assert_matches_submit(row, ro[0], fo, f"preview query {queries[i]}")
        kept += 1
    check(kept >= 6, "too few promise checks ran")


def _mread(m, fn, dtype):
    """Drain one of the matcher's feed hooks."""
    import ctypes as C

    parts = []
    while True:
        out = np.zeros(4096, dtype=dtype)
        n, left = C.c_size_t(0), C.c_size_t(0)
        rc = fn(m.ctx, out.ctypes.data, len(out), C.byref(n), C.byref(left))
        check(rc == 0, f"a matcher feed hook answered {rc}")
        parts.append(out[: n.value])
        if not left.value:
            return np.concatenate(parts)


def phase_b(d, counts):
    """Re-stamping through the matcher: slice by slice against the reference book. One slice at a time here, so a
    shard's feed job never covers two slices and "the events stamped k turn the books after slice k - 1 into
    those after slice k" is exact for engine shards too (phase A keeps two in flight)."""
    cl = d.cl
    m = cl.c_matcher()
    D = 5
    for role in ("quotes every slice", "depth every slice"):
        cl.quotes_enable(64 * S)
        check(m.depth_enable(m.ctx, D, 64 * D * S) == 0, "matcher depth_enable")
        check(m.trades_enable(m.ctx, 64 * S) == 0, "matcher trades_enable")
        first = len(d.sent)  # slices before this round: their number is <= first
        table, maps = qm.tops(qm._Empty(), S), dm.empty_maps(S)
        cumv = np.zeros(S, dtype=np.int64)
        for ev in (_mread(m, m.quotes, qm.QUOTE_DTYPE),):
            check(not len(ev) or int(ev["batches"].max()) <= first, "an initial quote is stamped with a later slice")
            qm.replay(table, ev)
        ev = _mread(m, m.depth, dm.DEPTH_DTYPE)
        check(not len(ev) or int(ev["batches"].max()) <= first, "an initial depth event is stamped with a later slice")
        dm.replay(maps, ev)
        check(len(_mread(m, m.trades, tm.TRADE_DTYPE)) == 0, "trade events right after enable")
        want = {}  # slice number -> (tops, views, cumulative volume per symbol since enable)
        vol = np.zeros(S, dtype=np.int64)

        def by_slice(ev, lo, hi, apply, same, what):
            """Events stamped k, for every k in (lo, hi], must turn the state after slice k - 1 into slice k's."""
            check(not len(ev) or (int(ev["batches"].min()) > lo and int(ev["batches"].max()) <= hi),
                  f"B ({role}): {what} stamps outside slices {lo + 1}..{hi}: {np.unique(ev['batches']).tolist()}")
            for k in range(lo + 1, hi + 1):
                apply(ev[ev["batches"] == k])
                check(same(k), f"B ({role}): {what} events stamped <= {k} do not give the books after slice {k}")

        def trades_apply(ev):
            for e in ev:
                cumv[int(e["symbol"])] = int(e["cum_volume"])

        checks = {
            "quotes": (m.quotes, qm.QUOTE_DTYPE, lambda ev: qm.replay(table, ev), lambda k: qm.same_quotes(table, want[k][0])),
            "depth": (m.depth, dm.DEPTH_DTYPE, lambda ev: dm.replay(maps, ev), lambda k: dm.same_views(maps, want[k][1])),
            "trades": (m.trades, tm.TRADE_DTYPE, trades_apply, lambda k: np.array_equal(cumv, want[k][2])),
        }
        often = "quotes" if role.startswith("quotes") else "depth"
        for _ in range(4):
            b = d.next_batch()
            _, fo = d.one(b, f"B ({role})")
            k = len(d.sent)
            np.add.at(vol, fo["symbol"], fo["qty"].astype(np.int64))
            want[k] = (qm.tops(d.ref, S), dm.views(d.ref, S, D), vol.copy())
            fn, dt, apply, same = checks[often]
            ev = _mread(m, fn, dt)
            counts["restamped"] += len(ev)
            by_slice(ev, k - 1, k, apply, same, often)
        for name in ("quotes", "depth", "trades"):
            if name == often:
                continue
            fn, dt, apply, same = checks[name]
            ev = _mread(m, fn, dt)
            counts["restamped"] += len(ev)
            check(len(np.unique(ev["batches"])) >= 3, f"B ({role}): late {name} events carry too few distinct stamps")
            by_slice(ev, first, len(d.sent), apply, same, name + " (drained last)")
        cl.quotes_enable(0)
        check(m.depth_enable(m.ctx, 0, 0) == 0 and m.trades_enable(m.ctx, 0) == 0, "matcher feeds off")


def phase_c(d, counts, tmp):
    """A service over me_cluster_matcher against a service over one book with the same hooks."""
    me, cl = d.me, d.cl
    full = FullBook()
    for b in d.sent:
        full.ob.submit(b)  # the same books as the cluster's
    syms = [f"S{i:02d}" for i in range(S)]
    mid = d.st.base_prices() + L // 2
    svcs = [me.MatchingEngineService(None, syms, matcher=cl), me.MatchingEngineService(None, syms, matcher=full)]
    try:
        for _ in range(d.last_seq):  # OIDs below the books' seqs: burnt by requests refused after allocation
            for v in svcs:
                v.submit_order("C", "S00", 0, 0, 100, 4, 1)
        for v in svcs:
            v.depth_subscribe(5)
            v.trades_subscribe(True)

        def by_symbol(rows):
            return sorted(rows, key=lambda r: r["symbol"])

        a, b = (by_symbol(v.depth_stream()) for v in svcs)
        check(a == b and len(a) > 0, "service: the initial depth books differ")
        rng = np.random.default_rng(23)
        owner, live = {}, []
        for rnd in range(3):
            for _ in range(300):
                if live and rng.random() < 0.2:
                    oid = live[int(rng.integers(len(live)))]
                    for v in svcs:
                        v.cancel_order(owner[oid][0], owner[oid][1], f"OID-{oid}")
                    continue
                si = int(rng.integers(S))
                otype = 1 if rng.random() < 0.2 else 0
                side = int(rng.choice([1, 2]))
                px = int(mid[si]) + int(rng.integers(-30, 31))
                client = f"C{int(rng.integers(3))}"
                qn = int(rng.integers(1, 200))
                r = [v.submit_order(client, syms[si], otype, side, 0 if otype else px, 4, qn) for v in svcs]
                check(r[0] == r[1] and r[0]["success"], f"service: SubmitOrder answers differ: {r}")
                oid = int(r[0]["order_id"][4:])
                owner[oid] = (client, syms[si])
                if otype == 0:
                    live.append(oid)
            outs = [v.flush() for v in svcs]
            for x, y, what in zip(outs[0], outs[1], ("seq", "results", "tape")):
                diff = [f for f in (x.dtype.names or ()) if len(x) == len(y) and not np.array_equal(x[f], y[f])]
                check(len(x) == len(y) and np.array_equal(x, y),
                      f"service round {rnd}: {what} differs ({len(x)} vs {len(y)} rows; fields {diff})")
            a, b = (by_symbol(v.depth_stream()) for v in svcs)
            check(a == b and len(a) > 0, f"service round {rnd}: depth_stream books differ")
            counts["svc_books"] += len(a)
            a, b = (by_symbol(v.trades_stream()) for v in svcs)
            check(a == b and len(a) > 0, f"service round {rnd}: trades_stream updates differ")
            counts["svc_trades"] += len(a)
        mine = [o for o in live if owner[o][0] == "C0"][:150]
        others = [o for o in live if owner[o][0] == "C1"][:20]
        ids = [f"OID-{o}" for o in mine + others] + ["OID-0", "bogus", f"OID-{d.last_seq + 10**6}"]
        a, b = (v.order_status("C0", ids) for v in svcs)
        check(a == b, "service: order_status differs")
        check(sum(r["state"] == me.OS_RESTING for r in a[: len(mine)]) > 5, "service: no resting order in the status check")
        check(all(r["state"] == me.OS_NOT_RESTING for r in a[len(mine):]), "service: another client's order is visible")
        for si in range(0, S, 3):
            for side in (1, 2):
                for otype, tif in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 2)):
                    args = ("C0", syms[si], otype, side, 0 if otype else int(mid[si]) + (7 if side == 1 else -7), 4, 150, tif)
                    a, b = (v.preview_order(*args) for v in svcs)
                    check(a.tobytes() == b.tobytes(), f"service: preview_order{args} differs: {a} vs {b}")
                    counts["svc_previews"] += 1
        a, b = (v.preview_order("C0", "NOSUCH", 0, 1, 100, 4, 5) for v in svcs)
        check(a.tobytes() == b.tobytes(), "service: preview of a name without a book differs")
        for v in svcs:
            v.depth_subscribe(0)
            v.trades_subscribe(False)
        errs = [v.last_error() for v in svcs]
        check(errs == ["", ""], f"service errors: {errs}")
    finally:
        for v in svcs:
            v.close()


def main():
    kind, out_path = sys.argv[1], sys.argv[2]
    import matching_engine_amd as me
    from matching_engine_amd.cluster import Cluster, ShardOps, shard_symbols

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    sc = me.preset(5, num_symbols=S, levels=L, batch=600, cancel_pct=30, market_pct=15, market_qty_mult=4, far_pct=3)
    st = me.Stream(sc)
    base = st.base_prices()
    engines = kind in ("gpu", "rccl")
    ops = None
    if not engines:
        ids = shard_symbols(S, world, rank)
        ops = ShardOps(NoDepthShard(ids) if kind == "nohook" and rank == world - 1 else ParityShard(ids), MR)
    cl = Cluster(rank, world, S, MB, transport="rccl" if kind == "rccl" else "tcp", port=int(os.environ["MASTER_PORT"]),
                 device=0, levels=L, base_prices=base, max_resting=MR, shard_ops=ops, timeout_ms=120000)
    if rank != 0:
        cl.serve()
        cl.close()
        return
    d = Driver(me, cl, st, sc)
    d.engines = engines
    counts = dict(depth_events=0, trade_events=0, restamped=0, svc_books=0, svc_trades=0, svc_previews=0)
    ok, msg = True, ""
    try:
        if kind == "nohook":
            d.run([d.next_batch()], "nohook")
            expect_code(lambda: cl.depth_enable(5, 4096), E_INVALID, "depth_enable with a shard that has no depth hook")
            cl.trades_enable(64 * S)  # the other hooks are there
            d.run([d.next_batch() for _ in range(2)], "nohook, after the refusal")
            tm.replay(cl.trades_drain(), d.tapes[1:], S)
        else:
            queries = phase_a(d, counts)
            phase_b(d, counts)
            promise(d, queries)
            with tempfile.TemporaryDirectory() as tmp:
                phase_c(d, counts, tmp)
    except Exception as e:  # the other ranks still have to be stopped
        import traceback

        ok, msg = False, f"{type(e).__name__}: {e}\n{traceback.format_exc()[-1500:]}"
    stats = cl.stats()
    cl.stop()
    cl.close()
    json.dump({"ok": ok, "msg": msg, "slices": stats["slices"], "world": world, **counts}, open(out_path, "w"))


if __name__ == "__main__":
    main()
