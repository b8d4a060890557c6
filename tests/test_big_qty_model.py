"""The big-quantity streams and scripts of tests/big_qty.py on the CPU models alone (no GPU).

  * every stream the GPU tests run (big_qty.STREAMS) meets the coverage floors: they are conditions on the
    inputs, counted from the model, so that a green GPU run has in fact crossed 2^31 and 2^32 where it claims to;
  * on the plain subset of each stream the Python model and the native oracle (int64 level totals) agree on
    results, tapes, books and snapshot totals: the two references agree at these widths before either judges a
    kernel;
  * every directed script does on the model what its docstring says.

What each stream reaches (big_qty.coverage; test_coverage_floors prints it; the floors are in the test):

  stream       up/down  mid_   group_ level_ sat_   fok_    fok_   big_   far_big walk_big   refused_later
               (min)    batch  over   over   chunk  filled  killed reduce _fill   plain/cx   plain/cx
  grouped_far   5 / 4    213     2     33     15     59      12     93     10     543/544     15/15
  grouped       5 / 5    236     6     44     16     70      11    124      -     238/277      6/7
  deep256_far  11 / 11   222     3     38     16     56       7     89      8    1003/1109    28/31
  deep256      11 / 11   218     6     38     24     68       9    103      -     837/930     23/24
  deep_far     11 / 11   220     3     43     15     51       6     83      7     627/676     18/18
  deep         10 / 10   217     4     35     11     61      14    102      -     571/627     18/19
  hot1024_far   5 / 5    204     8     36      9     61       9    104     10     601/646     11/11
  hot1024       4 / 4    192     4     34      9     54       7    101      -     713/818      6/9
  hot2048_far   5 / 5    216     4     24      8     49      10     98      7     864/930      9/11
  hot2048       6 / 6    218     4     38     11     55      13     90      -     788/826      9/9

Rejects are 0.8 to 1.1 % of the NEW records on every stream.
"""
import numpy as np
import pytest

from tests import big_qty as bq
from tests.big_qty import CAP31, CAP32, MAX, Q28
from tests.model_common import FIELDS_BOOK, FIELDS_FILL, FIELDS_RES, same
from tests.reduce_model import ReduceBook, check_seq_rule, is_reduce
from tests.tif_model import Arrays

BUY, SELL = 1, 2
ST_NEW, ST_FILLED, ST_CANCELED = 0, 2, 3


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle

    return oracle


def _fills(f):
    return [(int(x["maker_seq"]), int(x["qty"])) for x in f]


# ---- the streams -------------------------------------------------------------------------------------------------

def test_every_gpu_path_has_its_streams():
    assert set(bq.PATH_STREAMS) == {"reg", "gwalk", "gwalk_cx", "deep256", "deep", "hot_agg", "hot"}
    for names in bq.PATH_STREAMS.values():
        far = [bool(bq.STREAMS[n][6].get("far_pct")) for n in names]
        assert sorted(far) == [False, True]  # one seed with far prices, one without


@pytest.mark.parametrize("name", list(bq.STREAMS))
def test_coverage_floors(name):
    seed, S, L, nb, n, group, kw = bq.STREAMS[name]
    base, batches, exp, model = bq.stream(name)
    assert len(batches) == nb and all(len(b) == n for b in batches)
    check_seq_rule(batches)
    c = bq.coverage(batches, S, group, levels=L)
    print(name, {k: v for k, v in c.items() if k != "sum_end"})
    assert min(c["up"]) >= 3 and min(c["down"]) >= 3, c
    for k in ("mid_batch", "group_over", "level_over", "sat_chunk", "big_reduce", "fok_filled", "fok_killed"):
        assert c[k] >= 1, (k, c)
    if kw.get("far_pct"):
        assert c["far_big_fill"] >= 1, c
    # the fast walks do not only refuse: they run records of >= 2^20 themselves, and the bound stops them after
    # they ran part of a group
    assert min(c["walk_big"], c["walk_big_cx"]) >= 100 and min(c["refused_later"], c["refused_later_cx"]) >= 3, c
    assert c["rejects"] <= 0.02 * c["news"], c
    # the counters' book sums are the model's: the final ones equal the final books
    for s in range(S):
        assert c["sum_end"][s] == int(model.dump(s)["qty"].astype(np.int64).sum()), s
    # quantities: the whole int32 range, the constants included
    q = np.concatenate([b.qty[(b.kind & 8) == 0] for b in batches]).astype(np.int64)
    for v in bq.CONSTS:
        assert (q == v).any(), v
    assert ((q >= 1) & (q <= 60)).any() and ((q >= 1 << 20) & (q <= 1 << 26)).any() and (q >= Q28).sum() > len(q) // 20
    cq = np.concatenate([b.qty[(b.kind & 12) == 8] for b in batches])
    assert set(cq.tolist()) == {0, -1, MAX}  # a cancel's ignored field


def test_trace_is_the_sum_before_each_record():
    seed, S, L, nb, n, group, kw = bq.STREAMS["grouped"]
    base, batches, _, _ = bq.stream("grouped")
    tr = bq.trace(batches[:2], S)
    assert sum(len(t) for t in tr) == sum(int((b.symbol < S).sum()) for b in batches[:2])
    model = ReduceBook(S)
    # the sum before a symbol's first record of batch 1 is the model's book after batch 0
    model.submit(batches[0])
    for s in range(S):
        first = next(x for x in tr[s] if x[0] == 1)
        assert first[2] == int(model.dump(s)["qty"].astype(np.int64).sum()), s
        assert tr[s][0][2] == 0


def test_phases_do_not_follow_the_batches():
    """The records that cross 2^31 sit at every kind of place: in the first and the second half of a batch, in
    every batch of a launch group."""
    seed, S, L, nb, n, group, kw = bq.STREAMS["grouped"]
    base, batches, _, _ = bq.stream("grouped")
    tr = bq.trace(batches, S)
    halves, places = set(), set()
    for s in range(S):
        for (k0, i0, b0), (k1, i1, b1) in zip(tr[s], tr[s][1:]):
            if (b0 < CAP31) != (b1 < CAP31):
                halves.add(i0 >= n // 2)
                places.add(k0 % group)
    assert halves == {False, True} and places == set(range(group))


@pytest.mark.parametrize("name", list(bq.STREAMS))
def test_references_agree_on_the_plain_subset(orc, name):
    """GTC LIMITs, MARKETs and cancels (no TIF, no REDUCE) through ReduceBook and the native OracleBook."""
    seed, S, L, nb, n, group, kw = bq.STREAMS[name]
    base, batches, _, _ = bq.stream(name)
    sub = []
    for b in batches:
        keep = ~is_reduce(b.kind) & (((b.kind & 8) != 0) | (((b.kind >> 4) & 3) == 0))
        sub.append(Arrays(b.seq[keep], b.price_q4[keep], b.qty[keep], b.symbol[keep], b.kind[keep] & 0x0F))
    check_seq_rule(sub)
    ob, pb = orc.OracleBook(S), ReduceBook(S)
    over = 0
    for k, b in enumerate(sub):
        r1, f1 = ob.submit(b)
        r2, f2 = pb.submit(b)
        same(r2, r1, FIELDS_RES, f"{name} batch {k} results")
        same(f2, f1, FIELDS_FILL, f"{name} batch {k} tape")
        for s in range(S):
            same(pb.dump(s), ob.dump(s), FIELDS_BOOK, f"{name} batch {k} book {s}")
            for mine, theirs in zip(bq.model_snapshot(pb, s, 10), ob.snapshot(s, 10)):
                same(mine, theirs, ("price_q4", "total_qty", "order_count"), f"{name} batch {k} snapshot {s}")
                over += int((mine["total_qty"] > CAP32).sum())
    assert pb.resting() == ob.resting()
    assert over > 0  # level totals past 2^32 were compared


@pytest.mark.parametrize("path", list(bq.FEEDS))
def test_feed_runs_publish_totals_past_2_32(path):
    """At the launches of the feed tests a best level and a top-8 level hold more than 2^32, and several hold
    2^31 or more: the feeds' int64 quantities are compared beyond int32 and beyond uint32."""
    from tests import depth_model as dm
    from tests import quote_model as qm

    name, step = bq.FEEDS[path]
    S = bq.STREAMS[name][1]
    m = ReduceBook(S)
    view = bq.Snap(m)
    best, top = [], []
    for a in bq.slices(bq.stream(name)[1], step):
        m.submit(a)
        t = qm.tops(view, S)
        best += t["bid_qty"].tolist() + t["ask_qty"].tolist()
        top += [q for vw in dm.views(view, S, 8) for side in vw for _, q in side]
    for got in (best, top):
        assert sum(q >= CAP31 for q in got) >= 5 and sum(q > CAP32 for q in got) >= 1


def test_control_subset_is_small_and_plain():
    seed, S, L, nb, n, group, kw = bq.STREAMS["grouped"]
    base, batches, _, _ = bq.stream("grouped")
    big = bq.plain_subset(batches, far_free=(base, L))
    small = bq.plain_subset(batches, map_qty=lambda q: 1 + q % 60, far_free=(base, L))
    assert [len(a) for a in big] == [len(a) for a in small]
    for a, b in zip(big, small):
        assert np.array_equal(a.seq, b.seq) and np.array_equal(a.kind, b.kind) and np.array_equal(a.price_q4, b.price_q4)
        assert not (a.kind & 0xF8).any()
        pos = b.qty > 0
        assert b.qty[pos].max() <= 60 and np.array_equal(a.qty[~pos], b.qty[~pos])
    # the small run stays far below 2^31, the large one crosses it
    assert max(x[2] for t in bq.trace(small, S) for x in t) < 1 << 20
    assert max(x[2] for t in bq.trace(big, S) for x in t) >= CAP31


# ---- the directed scripts ----------------------------------------------------------------------------------------

def _run(case):
    m = ReduceBook(case.S)
    return m, [m.submit(b) for b in case.batches]


@pytest.mark.parametrize("where", ["reg", "hot", "far"])
@pytest.mark.parametrize("one_batch", [False, True])
def test_chunk_scripts_16(where, one_batch):
    """What the four takers get from one chunk of each pattern (m[j]: the j-th maker, from 1)."""
    want = {
        "max": ([[(1, MAX)], [(2, 1)], [(2, MAX - 1)], [(3, MAX)]], (4, MAX)),
        # MAX = 8 * 2^28 - 1: seven makers and all but one lot of the eighth; the LIMIT of MAX - 1 ends 7 short
        # of the 16th maker's 2^28 + 5, and the FOK finds 7 < MAX: killed
        "q28": ([[(j, Q28) for j in range(1, 8)] + [(8, Q28 - 1)], [(8, 1)],
                 [(j, Q28) for j in range(9, 16)] + [(16, Q28 - 2)], []], (16, 7)),
        "hole": ([[(1, MAX)], [(2, 1)], [(2, MAX - 1)], [(3, 1), (4, MAX - 1)]], (4, 1)),
        # the chunk holds 2^31 - 2^15 < MAX: the MARKET takes all of it, the IOC finds nothing, the LIMIT rests
        "pow2": ([[(j + 1, 1 << (15 + j)) for j in range(16)], [], [], []], None),
    }
    for pattern in bq.PATTERNS:
        c = bq.chunk_case(where, pattern, 16, one_batch)
        m = ReduceBook(c.S)
        m.submit(c.batches[0])
        got = {}
        for b in c.batches[1:c.named_end]:
            r, f = m.submit(b)
            for t in c.takers:
                got.setdefault(t, []).extend(_fills(f[f["taker_seq"] == t]))
        lists, head = want[pattern]
        for t, w in zip(c.takers[:4], lists):
            assert got[t] == [(c.makers[j - 1], q) for j, q in w], (pattern, t)
        asks = [e for e in m.dump(0) if e["side"] == SELL]
        if head is None:
            assert not asks
        else:
            assert (int(asks[0]["seq"]), int(asks[0]["qty"])) == (c.makers[head[0] - 1], head[1]), pattern
        for b in c.batches[c.named_end:]:
            m.submit(b)
        assert not [e for e in m.dump(0) if e["side"] == SELL]  # drained


@pytest.mark.parametrize("pattern", bq.PATTERNS)
def test_chunk_scripts_33(pattern):
    """33 makers: every maker is filled in order, for exactly its quantity, across the three chunks."""
    c = bq.chunk_case("reg", pattern, 33, False)
    m, outs = _run(c)
    f = np.concatenate([o[1] for o in outs])
    f = f[f["price_q4"] == c.price]
    per = {}
    order = []
    for x in f:
        k = int(x["maker_seq"])
        if k not in per:
            order.append(k)
        per[k] = per.get(k, 0) + int(x["qty"])
    assert order == c.makers and [per[k] for k in c.makers] == c.qs
    if pattern != "pow2":
        assert sum(c.qs[:16]) >= CAP32  # the first chunk's ranking saturates


@pytest.mark.parametrize("L", [128, 1024, 2048])
def test_fok_script(L):
    c = bq.fok_case(L, hot=L == 2048)
    m, outs = _run(c)
    for k, w in c.want.items():
        r, f = outs[k + 1]
        i = c.pad  # (the record between the pads)
        assert _fills(f) == w, k
        if k in c.killed:
            assert (int(r[i]["status"]), int(r[i]["filled_qty"]), int(r[i]["remaining_qty"])) == (ST_CANCELED, 0, MAX), k
        elif k not in (0, 4):
            assert (int(r[i]["status"]), int(r[i]["filled_qty"])) == (ST_FILLED, MAX), k
    asks = [(int(e["seq"]), int(e["qty"])) for e in m.dump(0) if e["side"] == SELL]
    assert asks == [(c.a[7], MAX - 1)]


def test_reduce_script():
    c = bq.reduce_case(128)
    m, outs = _run(c)
    r = outs[1][0]
    assert (int(r[0]["status"]), int(r[0]["remaining_qty"])) == (ST_NEW, 1)
    assert _fills(outs[1][1]) == [(c.A, 1), (c.B, 2)]
    r = outs[2][0]
    assert (int(r[0]["status"]), int(r[0]["remaining_qty"])) == (ST_CANCELED, MAX)
    r = outs[3][0]
    assert (int(r[0]["status"]), int(r[0]["remaining_qty"])) == (ST_NEW, 1)
    assert 5 * MAX > 1 << 33  # the queue ahead of X
    f = outs[4][1]
    assert _fills(f) == [(c.B, 3)] + [(q, MAX) for q in c.Q] + [(c.X, 1), (c.Y, 1)]
    assert len(m.dump(0)) == 0


@pytest.mark.parametrize("path", ["gwalk", "gwalk_cx", "hot_agg"])
def test_lw_cap_scripts_start_where_they_say(path):
    """The sums the hand-off counts are derived from: the book sum at each group's start, and the group's
    quantities as the helper wave counts them."""
    L, base, cases = bq.lw_cases(path)
    want_start = {"i_keep": [0, CAP31 - 1 - bq.LW_Q], "i_over": [0, CAP31 - 1 - bq.LW_Q, CAP31, 1 << 30],
                  "iii_keep": [0, 1 << 30, CAP31 - 1 - 2 * ((1 << 29) + (1 << 28))],
                  "iii_over": [0, 1 << 30, CAP31 - 2 * ((1 << 29) + (1 << 28))],
                  "iv_below": [0, CAP31 - 1], "iv_at": [0, CAP31, CAP31, 1 << 30],
                  "v": [0, CAP31 - 2] if path == "gwalk_cx" else [0, CAP31 - 2, CAP31 - 1]}
    want_start["ii_keep"], want_start["ii_over"] = want_start["i_keep"], want_start["i_over"]
    for name, (G, groups) in cases.items():
        m = ReduceBook(1)
        starts = []
        for arrs, delta, why in groups:
            starts.append(int(m.dump(0)["qty"].astype(np.int64).sum()))
            assert len(arrs) == G
            for a in arrs:
                if path == "hot_agg":
                    assert len(a) >= 64
                assert len(a) <= 128  # one bucket
                m.submit(a)
            # the rule of lw_cases' docstring, on the grouped walks
            if path != "hot_agg":
                cx = path == "gwalk_cx"
                ub = starts[-1]
                hand = ub >= CAP31
                for a in arrs:
                    for lo in range(0, len(a), 64):
                        kd, q = a.kind[lo:lo + 64], a.qty[lo:lo + 64].astype(np.int64)
                        ub += int(np.where((kd & 8) != 0 if cx else False, 0, np.maximum(q, 0)).sum())
                        hand |= ub >= CAP31 or bool(((kd & 8) != 0).any() and not cx)
                assert int(hand) == delta, (name, why)
        assert starts == want_start[name], (name, starts)
