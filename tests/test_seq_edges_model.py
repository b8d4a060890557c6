"""The inputs of tests/seq_edges.py, checked on the CPU (no GPU, seconds in all).

  * every scripted case: OracleBook, PyBook and TifBook (where the case stays inside their vocabulary) and
    ReduceBook give the outcomes and final books its author wrote down, and the fills of its taker;
  * the overlay at the GPU tests' shapes, ten seeds: the models agree where they share the vocabulary, every
    (boundary kind, target class) pair occurs at least 5 times per draw, and at least 30 boundary records per draw
    succeed with target == own seq == their launch group's first seq;
  * two deliberately wrong models differ from ReduceBook exactly on the families they are aimed at;
  * `k_seq_sweep`'s arithmetic, restated, says that the sweep is due at sweep_start's boundary group and that
    span_edge's group is the longest the ring accepts.

The floor of 30 is asserted for one batch per launch group. In groups of four, sixteen batches give three group
starts that can name an earlier order, each with a run of at most four records: twelve at the most, so there the
floor is two at every such group start (the batch before ends with a resting order of at least 2; the run names
it first, reducing it by 1, and once more).
"""
import numpy as np
import pytest

from oracle.oracle import OracleBook
from oracle.pybook import PyBook
from tests import seq_edges as se
from tests.reduce_model import ReduceBook, check_seq_rule, is_reduce
from tests.seq_edges import OVERLAY_KW, ON, ONB, OS, overlay_seed
from tests.tif_model import TifBook

LS = (128, 1024)
SEEDS = range(10)


def _vocabulary(case):
    """(has a REDUCE, has time-in-force bits on a NEW record)."""
    kd = np.concatenate([b.kind for b in case.batches])
    return bool(is_reduce(kd).any()), bool((((kd & 8) == 0) & ((kd >> 4) & 3 != 0)).any())


def _models(case):
    red, tif = _vocabulary(case)
    out = [ReduceBook]
    if not red:
        out.append(TifBook)
        if not tif:
            out += [PyBook, OracleBook]
    return out


def _ids(cases):
    return [c.name for c in cases]


CASES = se.scripted(128)


def test_the_families_are_all_there():
    fams = {c.family for c in CASES}
    assert fams == set(se.FAMILIES)
    for fam in se.FAMILIES:
        forms = {c.form for c in CASES if c.family == fam}
        assert set(se.FORMS) <= forms, (fam, forms)
    assert any(c.form == "mixed" for c in CASES)
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        check_seq_rule(c.batches)
        assert sum(c.groups) == len(c.batches) and 0 <= c.boundary < len(c.groups)
        assert all(len(b) == len(e) for b, e in zip(c.batches, c.expected))


@pytest.mark.parametrize("L", LS)
def test_models_give_the_hand_written_outcomes(L):
    n = 0
    for case in se.scripted(L):
        for M in _models(case):
            model = M(case.S)
            outs = se.run_model(model, case)
            for k, (r, f) in enumerate(outs):
                assert se.outcomes(r) == [tuple(x) for x in case.expected[k]], (case.name, M.__name__, k)
                if k in case.fills:
                    got = [(int(x["maker_seq"]), int(x["qty"])) for x in f]
                    assert got == case.fills[k], (case.name, M.__name__, k)
            for s in range(case.S):
                assert se.book_rows(model.dump(s)) == case.books[s], (case.name, M.__name__, s)
            n += 1
    assert n >= len(CASES) + 3 * 30  # (the CANCEL forms ran on four models)


def test_cancel_forms_run_on_all_four_models():
    plain = [c for c in CASES if c.form == "cancel" and "never ioc" not in c.name and "never fok" not in c.name]
    assert len(plain) > 30
    for c in plain:
        assert len(_models(c)) == 4, c.name


def test_boundary_records_sit_where_the_families_say():
    """From the arrays alone: the boundary record repeats its target's seq and sits at the position the family
    names."""
    for c in CASES:
        k0 = sum(c.groups[:c.boundary])
        b = c.batches[k0]
        if c.family in ("group_start", "group_start_run", "sweep_start", "span_edge"):
            assert int(b.kind[0]) & 8 and int(b.seq[0]) == int(c.batches[k0 - 1].seq[-1]), c.name
            run = [i for i in range(len(b)) if int(b.kind[i]) & 8 and int(b.seq[i]) == int(b.seq[0])]
            run = run[:next((j for j, i in enumerate(run) if i != j), len(run))]
            assert any((int(b.price_q4[i]) & (2**64 - 1)) == int(b.seq[0]) for i in run), c.name
        elif c.family == "group_start_limit":
            assert not int(b.kind[0]) & 8 and int(b.kind[1]) & 8 and int(b.seq[1]) == int(b.seq[0]), c.name
        elif c.family == "batch_start_in_group":
            g = c.groups[c.boundary]
            hits = [j for j in range(1, g) if int(c.batches[k0 + j].kind[0]) & 8
                    and int(c.batches[k0 + j].seq[0]) == int(c.batches[k0 + j - 1].seq[-1])]
            assert hits and g in (4, 8), c.name
        elif c.family == "block_start":
            sym0 = np.nonzero(b.symbol == 0)[0]
            at = [j for j, i in enumerate(sym0) if int(b.kind[i]) & 8]
            assert at and at[0] in (64, 63, 127), (c.name, at)
            i = sym0[at[0]]
            assert (int(b.price_q4[i]) & (2**64 - 1)) == int(b.seq[i]) == int(b.seq[sym0[at[0] - 1]]), c.name
            assert ("interleaved" in c.name) == (int(i) != at[0]), c.name
            assert len(sym0) <= 128


# ---- the two wrong models ---------------------------------------------------------------------------------------

def _differs(M, case):
    a = se.run_model(M(case.S), case)
    b = se.run_model(ReduceBook(case.S), case)
    return any(se.outcomes(x[0]) != se.outcomes(y[0]) for x, y in zip(a, b))


def test_group_first_seq_model_differs_where_it_should():
    """(a) differs wherever the boundary target is a live order from before its cancel's launch group (every
    group_start, span_edge and sweep_start case, group_start_run's runs, batch_start_in_group with b = -1) and
    the form can tell (a REDUCE by 0 is BAD_QTY whatever it names), and nowhere else."""
    hit = {f: 0 for f in se.FAMILIES}
    for c in CASES:
        want = c.pre and c.form != "d0"
        assert _differs(se.GroupFirstSeq, c) == want, c.name
        hit[c.family] += want
    assert hit["group_start"] and hit["group_start_run"] and hit["batch_start_in_group"]
    assert not hit["group_start_limit"] and not hit["block_start"]
    for c in CASES:
        if c.family in ("group_start", "span_edge", "sweep_start") or (c.family == "group_start_run"
                                                                       and "never" not in c.name):
            assert c.pre, c.name


def test_block_snapshot_model_differs_where_it_should():
    """(b) differs on every block_start case whose form can tell, and on no other scripted case."""
    n = 0
    for c in CASES:
        want = c.block and c.form != "d0"
        assert _differs(se.BlockSnapshot, c) == want, c.name
        n += want
    assert n == 3 * 2 * 3
    assert all(c.block == (c.family == "block_start") for c in CASES)


# ---- the sweep and the span ---------------------------------------------------------------------------------------

def test_sweep_is_due_at_the_boundary_group():
    for c in CASES:
        if c.family not in ("sweep_start", "span_edge"):
            continue
        gs = se.group_seqs(c)
        states = se.sweep_states(gs, c.ring)
        assert all(ok for _, ok, _ in states), c.name  # every group's span is accepted
        need, _, horizon = states[c.boundary]
        gmin, gmax = gs[c.boundary]
        first = c.batches[sum(c.groups[:c.boundary])]
        tgts = [int(first.price_q4[i]) & (2**64 - 1) for i in range(len(first)) if int(first.kind[i]) & 8]
        assert need and horizon == gmin and gmin in tgts, c.name
        if c.family == "span_edge":
            assert gmax - gmin == c.ring - 1
            assert not se.sweep_states([(gmin, gmax + 1)], c.ring)[0][1]  # one seq more is refused
        else:
            assert gmin >= 1 << 62, c.name
            assert not states[c.boundary - 1][0], c.name  # (the group before needed no sweep: this one moves it)
            if "old" in c.name:
                assert min(tgts) <= gmin - 3 * c.ring and min(tgts) < states[c.boundary - 1][2]


# ---- the overlay ----------------------------------------------------------------------------------------------------

def _agree(models, arrays, ctx):
    for k, b in enumerate(arrays):
        outs = [m.submit(b) for m in models]
        for m, (r, f) in zip(models[1:], outs[1:]):
            for fld in ("filled_qty", "remaining_qty", "fill_count", "tape_offset", "status", "reason"):
                assert np.array_equal(r[fld], outs[0][0][fld]), (ctx, type(m).__name__, k, fld)
            assert len(f) == len(outs[0][1]) and np.array_equal(f, outs[0][1]), (ctx, type(m).__name__, k)
    S = models[0].S
    for m in models[1:]:
        for s in range(S):
            assert se.book_rows(m.dump(s)) == se.book_rows(models[0].dump(s)), (ctx, type(m).__name__, s)


def _own_seq_floors(arrays, labels, plain=False):
    """At one batch per group at least 30 a draw; at both group sizes every group start after the first at least
    2 (the batch before ends with a resting order of at least 2, the run names it first, by 1, and again). The
    plain variant's runs are CANCELs: the first succeeds, so 1 per group start."""
    each = 1 if plain else 2
    assert se.boundary_successes(arrays, labels, 1, OS) >= (ONB - 1 if plain else 30)
    for group in (1, 4):
        per = se.boundary_successes(arrays, labels, group, OS, per_start=True)
        assert len(per) == len(range(group, ONB, group)) and min(per) >= each, (group, per)


def test_floors_of_the_other_streams_the_gpu_tests_run():
    """The plain variant at full length and the stream of the small-ring run (seqs above 2^40)."""
    base, arrays, labels = se.overlay_stream(128, 0, plain=True)
    assert len(arrays) == ONB
    _own_seq_floors(arrays, labels, plain=True)
    base, arrays, labels = se.overlay_stream(128, 0, high=True)
    assert len(arrays) == ONB and int(arrays[0].seq[0]) >= se.OVERLAY_HIGH
    _own_seq_floors(arrays, labels)
    lab = np.concatenate(labels)
    assert np.bincount(lab[lab >= 0], minlength=se.NLAB).min() >= 5
    assert max(int(a.seq[-1]) - int(a.seq[0]) for a in arrays) < 1024  # one batch per group fits the ring


@pytest.mark.parametrize("L,seed", [(128, s) for s in SEEDS] + [(L, s) for L in (256, 1024, 2048) for s in (0, 1)])
def test_overlay_floors(L, seed):
    base, arrays, labels = se.overlay_stream(L, seed)
    check_seq_rule(arrays)
    assert len(arrays) == ONB and all(len(a) == len(lb) for a, lb in zip(arrays, labels))
    lab = np.concatenate(labels)
    cnt = np.bincount(lab[lab >= 0], minlength=se.NLAB)
    for kd in se.KINDS:
        for tg in se.TARGETS:
            assert cnt[se.label(kd, tg)] >= 5, (kd, tg, cnt.tolist())
    _own_seq_floors(arrays, labels)
    # every inserted record repeats the seq of the record before it; at a block start it takes the position
    for k, (b, lb) in enumerate(zip(arrays, labels)):
        ins = np.nonzero(lb >= 0)[0]
        assert (b.kind[ins] & 8).all() and (ins.min() == 0 or k == 0)
        for i in ins[ins > 0]:
            assert int(b.seq[i]) == int(b.seq[i - 1])
        pos = np.zeros(len(b), dtype=np.int64)
        seen = {}
        for i in range(len(b)):
            s = int(b.symbol[i])
            pos[i] = seen.get(s, 0)
            seen[s] = pos[i] + 1
        blk = ins[(lb[ins] >= len(se.TARGETS)) & (pos[ins] % 64 == 0) & (pos[ins] > 0)]
        assert len(blk) > 0


@pytest.mark.parametrize("seed", SEEDS)
def test_overlay_plain_models_agree(seed):
    """The plain variant stays inside the vocabulary all four models share (eight batches of the GPU tests' shape)."""
    base, arrays, labels = se.boundary_stream(overlay_seed(128, seed), OS, 128, 8, ON, 1, plain=True, **OVERLAY_KW)
    kd = np.concatenate([b.kind for b in arrays])
    assert not is_reduce(kd).any() and not (kd >> 4).any()
    assert se.boundary_successes(arrays, labels, 1, OS) >= len(arrays) - 2
    _agree([ReduceBook(OS), TifBook(OS), PyBook(OS), OracleBook(OS)], arrays, f"plain #{seed}")


@pytest.mark.parametrize("seed", range(3))
def test_overlay_models_agree_without_the_reduces(seed):
    """The full overlay with its REDUCE records left out is a stream of TifBook's vocabulary: both give the same."""
    base, arrays, labels = se.boundary_stream(overlay_seed(128, seed), OS, 128, 4, ON, 1, **OVERLAY_KW)
    subs = []
    for b in arrays:
        keep = ~is_reduce(b.kind)
        subs.append(se.Arrays(b.seq[keep], b.price_q4[keep], b.qty[keep], b.symbol[keep], b.kind[keep]))
    _agree([ReduceBook(OS), TifBook(OS)], subs, f"no reduces #{seed}")
