"""The hostile-cancel streams (tests/cancel_targets.py) on the CPU: the references agree on them, the streams
reach what they are meant to reach, and they tell a wrong target lookup from a right one (no GPU).

1. Plain variant: OracleBook (C++), PyBook and TifBook agree on every batch's results and tape, on every book
   and on resting(). TIF variant: TifBook against its verdict rewrite run through OracleBook (the check of
   tests/test_tif_model.py::test_rewrite_into_plain_records).
2. Non-vacuity, for exactly the cases the GPU file runs: every class at least 20 times, at least 25 % of the
   cancels CANCELED, 10 successful own_seq cancels, 10 future targets issued later and resting at the end of
   their batch (some in the cancel's batch, some in a later one), books never empty; in the small-ring cases 20
   successful cancels of orders more than a ring old and 20 alias targets on the ring slot of a live order.
3. Five deliberately wrong books (no owner check; lookup by seq % R without confirming the seq; never-resting
   seqs cancellable; a second cancel succeeds; a cancel reaches a later record of its batch) each disagree
   with the reference on every case.
"""
import numpy as np
import pytest

from oracle.pybook import BUY, FILL_DTYPE, RESULT_DTYPE, RJ_UNKNOWN, ST_CANCELED, ST_REJECTED, PyBook
from tests import cancel_targets as ct
from tests import tif_model as tm
from tests.model_common import FIELDS_BOOK, FIELDS_FILL, FIELDS_RES, same
from tests.tif_model import Arrays, TifBook, kind

S = ct.S_CX


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle

    return oracle


def differ(a, b, fields):
    return len(a) != len(b) or any(not np.array_equal(np.asarray(a[f]), np.asarray(b[f])) for f in fields)


# ---- 1. the references agree ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n, c in ct.CASES.items() if not c.tif])
def test_plain_references_agree(orc, name):
    _, batches, _, _ = ct.stream(name)
    outs, resting, book = ct.expected(name)  # PyBook
    ob, tb = orc.OracleBook(S), TifBook(S)
    for k, b in enumerate(batches):
        ro, fo = ob.submit(b)
        rt, ft = tb.submit(b)
        same(outs[k][0], ro, FIELDS_RES, f"{name} batch {k} results (PyBook, oracle)")
        same(outs[k][1], fo, FIELDS_FILL, f"{name} batch {k} tape (PyBook, oracle)")
        same(rt, ro, FIELDS_RES, f"{name} batch {k} results (TifBook, oracle)")
        same(ft, fo, FIELDS_FILL, f"{name} batch {k} tape (TifBook, oracle)")
        assert resting[k] == ob.resting() == tb.resting(), f"{name} batch {k}: resting()"
    for s in range(S):
        same(book.dump(s), ob.dump(s), FIELDS_BOOK, f"{name} book {s} (PyBook, oracle)")
        same(tb.dump(s), ob.dump(s), FIELDS_BOOK, f"{name} book {s} (TifBook, oracle)")


@pytest.mark.parametrize("name", [n for n, c in ct.CASES.items() if c.tif])
def test_tif_rewrite_into_plain_records(orc, name):
    """An IOC / fillable FOK LIMIT becomes a LIMIT followed by a cancel of itself, a killed FOK and a rejected
    POST_ONLY are dropped, an accepted POST_ONLY becomes a LIMIT: the oracle on the rewritten stream gives the
    same fills, books and (for the records it keeps, the hostile cancels among them) the same results."""
    _, batches, _, _ = ct.stream(name)
    ob, tb = orc.OracleBook(S), TifBook(S)
    fills_t, fills_o = [], []
    n_ioc = n_cancel = 0
    for k, b in enumerate(batches):
        rt, ft = tb.submit(b)
        fills_t.append(ft)
        sq, px, qt, sy, kd, back = [], [], [], [], [], []  # back: (tif record, is the self-cancel)
        for i, v in enumerate(tb.verdicts):
            if v == tm.V_DROP:
                continue
            sq.append(b.seq[i]); px.append(b.price_q4[i]); qt.append(b.qty[i]); sy.append(b.symbol[i])
            kd.append(int(b.kind[i]) & 0x0F)
            back.append((i, False))
            if v == tm.V_IOC:
                sq.append(b.seq[i]); px.append(int(b.seq[i])); qt.append(0); sy.append(b.symbol[i])
                kd.append(kind(BUY, 0, 1))
                back.append((i, True))
        ro, fo = ob.submit(Arrays(sq, px, qt, sy, kd))
        fills_o.append(fo)
        for j, (i, selfcx) in enumerate(back):
            v = tb.verdicts[i]
            if v == tm.V_IOC and not selfcx:
                n_ioc += 1
                assert rt[i]["filled_qty"] == ro[j]["filled_qty"], f"{name} batch {k} record {i}: IOC filled"
                assert rt[i]["fill_count"] == ro[j]["fill_count"]
                cx = ro[j + 1]
                removed = 0 if (cx["status"] == ST_REJECTED and cx["reason"] == RJ_UNKNOWN) else int(cx["remaining_qty"])
                assert rt[i]["remaining_qty"] == removed, f"{name} batch {k} record {i}: IOC remainder"
            elif not selfcx and v in (tm.V_PLAIN, tm.V_POST, tm.V_MARKET):
                n_cancel += bool(int(b.kind[i]) & 8)
                for f in ("filled_qty", "remaining_qty", "fill_count", "status", "reason"):
                    assert rt[i][f] == ro[j][f], f"{name} batch {k} record {i} ({v}): {f}"
        assert tb.resting() == ob.resting()
    same(np.concatenate(fills_t), np.concatenate(fills_o), FIELDS_FILL, "fills")
    for s in range(S):
        same(tb.dump(s), ob.dump(s), FIELDS_BOOK, f"{name} book {s}")
    assert n_ioc > 300 and n_cancel > 2000
    outs, _, _ = ct.expected(name)  # (what the GPU tests compare with is this run)
    assert not differ(np.concatenate([o[1] for o in outs]), np.concatenate(fills_t), FIELDS_FILL)


# ---- 2. the streams reach what they are meant to reach ------------------------------------------------------

@pytest.mark.parametrize("name", list(ct.CASES))
def test_streams_are_not_vacuous(name):
    c = ct.CASES[name]
    _, batches, classes, info = ct.stream(name)
    outs, resting, _ = ct.expected(name)
    cls = np.concatenate(classes)
    status = np.concatenate([o[0]["status"] for o in outs])
    seq = np.concatenate([b.seq for b in batches])
    tgt = np.concatenate([b.price_q4 for b in batches]).view(np.uint64)
    sym = np.concatenate([b.symbol for b in batches])
    knd = np.concatenate([b.kind for b in batches])
    cancel = (knd & 8) != 0
    assert np.array_equal(cancel, cls >= 0)
    counts = {n: int((cls == i).sum()) for n, i in ct.CLS.items()}
    assert min(counts.values()) >= 20, counts
    ok = cancel & (status == ST_CANCELED)
    assert ok.sum() * 4 >= cancel.sum(), f"{ok.sum()} of {cancel.sum()} cancels end CANCELED"
    assert (ok & (cls == ct.CLS["own_seq"])).sum() >= 10
    assert min(resting) > 0, resting
    # the hostile classes are hostile: none of these may ever succeed
    for n in ("other_symbol", "repeat", "never_rests", "filled_later", "rejected", "zero", "huge"):
        assert not (ok & (cls == ct.CLS[n])).any(), n
    # future targets that were issued later as LIMITs of the same symbol and rest at the end of their batch
    # (replayed on a fresh book: the book of each batch's end)
    where = {}  # seq -> (batch, symbol) of the NEW records
    for k, b in enumerate(batches):
        for i in np.nonzero((b.kind & 8) == 0)[0]:
            where[int(b.seq[i])] = (k, int(b.symbol[i]))
    book = TifBook(S) if c.tif else PyBook(S)
    live_at_end = []
    for b in batches:
        book.submit(b)
        live_at_end.append(set(book.live))
    same_batch = later_batch = 0
    bidx = np.concatenate([np.full(len(b), k) for k, b in enumerate(batches)])
    for i in np.nonzero(cls == ct.CLS["future"])[0]:
        t = int(tgt[i])
        assert 1 <= t - int(seq[i]) <= 200
        assert status[i] == ST_REJECTED  # nothing above the cancel's own seq exists yet
        k, s = where.get(t, (-1, -1))
        if s == int(sym[i]) and t in live_at_end[k]:
            same_batch += k == bidx[i]
            later_batch += k > bidx[i]
    assert same_batch + later_batch >= 10 and same_batch >= 3 and later_batch >= 3, (same_batch, later_batch)
    if name in ct.RING_CASES:
        assert int(seq.max()) - int(seq.min()) >= 5 * c.ring  # the ring wraps at least five times
        old = ok & ((seq - tgt) > c.ring) & (tgt < seq)
        assert old.sum() >= 20, f"{old.sum()} successful cancels of orders more than a ring old"
        assert info["alias_on_live"] >= 20
    if name.startswith("walk"):  # what the grouped cancel walk keeps
        assert max(np.bincount(b.symbol).max() for b in batches) <= 128
        new_limit = (knd & 0x0C) == 0
        px = np.concatenate([b.price_q4 for b in batches])
        mid = (tm.base_prices(S, c.levels) + c.levels // 2)[sym]
        assert (np.abs(px - mid)[new_limit] <= 14).all()  # every LIMIT inside the window
    al = (cls == ct.CLS["alias_plus"]) | (cls == ct.CLS["alias_minus"])
    assert info["alias_on_live"] == al.sum()


# ---- 3. wrong books disagree -------------------------------------------------------------------------------

MUTANTS = ("no_owner", "ring_alias", "never_rests", "twice", "later")


def mutant(base_cls, what, ring):
    """A book of `base_cls` whose cancel lookup is wrong in one way. NEW records run through the base class one
    at a time; cancels through `_cancel` below."""

    class Wrong(base_cls):
        def __init__(self, num_symbols):
            super().__init__(num_symbols)
            self.slot, self.dropped, self.gone, self.doomed = {}, {}, {}, set()

        def _remove(self, t):
            s, side, price, entry = self.live.pop(t)
            got, entry[1] = entry[1], 0
            (self.side[s][0] if side == BUY else self.side[s][1]).drop_if_empty(price)
            return got

        def _cancel(self, s, t, i, index):
            """-> the quantity removed, or None (UNKNOWN_ORDER)."""
            if what == "ring_alias":  # the ring slot's order, its seq unconfirmed
                t = self.slot.get(t % ring, -1)
            hit = self.live.get(t)
            if hit is not None and (hit[0] == s or what == "no_owner"):
                got = self._remove(t)
                self.gone[t] = (s, got)
                return got
            if what == "never_rests" and self.dropped.get(t, (-1, 0))[0] == s:
                return self.dropped.pop(t)[1]
            if what == "twice" and self.gone.get(t, (-1, 0))[0] == s:
                return self.gone[t][1]
            if what == "later" and t in index and index[t][0] > i and index[t][1] == s:
                self.doomed.add(t)
                return index[t][2]
            return None

        def submit(self, b):
            n = len(b.seq)
            res = np.zeros(n, dtype=RESULT_DTYPE)
            tapes, nt = [], 0
            index = {int(b.seq[i]): (i, int(b.symbol[i]), int(b.qty[i])) for i in range(n)
                     if ct.may_rest(int(b.kind[i]), int(b.qty[i]))} if what == "later" else {}
            for i in range(n):
                s, kd, seq = int(b.symbol[i]), int(b.kind[i]), int(b.seq[i])
                if (kd & 8) and s < self.S:
                    got = self._cancel(s, int(b.price_q4[i]) & ((1 << 64) - 1), i, index)
                    res[i]["tape_offset"] = nt
                    if got is None:
                        res[i]["status"], res[i]["reason"] = ST_REJECTED, RJ_UNKNOWN
                    else:
                        res[i]["status"], res[i]["remaining_qty"] = ST_CANCELED, got
                    continue
                r, f = base_cls.submit(self, ct.one(b, i))
                res[i] = r[0]
                res[i]["tape_offset"] = nt
                tapes.append(f)
                nt += len(f)
                if seq in self.live:
                    self.slot[seq % ring] = seq
                    if seq in self.doomed:
                        self._remove(seq)
                elif r[0]["status"] != ST_REJECTED:
                    self.dropped[seq] = (s, int(r[0]["remaining_qty"]))
            fills = np.concatenate(tapes) if tapes else np.zeros(0, dtype=FILL_DTYPE)
            return res, fills

    return Wrong


@pytest.mark.parametrize("what", MUTANTS)
@pytest.mark.parametrize("name", list(ct.CASES))
def test_wrong_books_disagree(name, what):
    c = ct.CASES[name]
    _, batches, _, _ = ct.stream(name)
    outs, _, _ = ct.expected(name)
    wrong = mutant(TifBook if c.tif else PyBook, what, c.ring)(S)
    for k, b in enumerate(batches):
        r, f = wrong.submit(b)
        if differ(r, outs[k][0], FIELDS_RES) or differ(f, outs[k][1], FIELDS_FILL):
            return
    raise AssertionError(f"{name}: a book with the '{what}' fault passes the stream")


def test_the_unmutated_stepper_is_the_reference():
    """The record-by-record stepper the wrong books are built on, with no fault switched on, equals the
    reference: a disagreement above comes from the fault alone."""
    name = "l128_tif"
    _, batches, _, _ = ct.stream(name)
    outs, _, book = ct.expected(name)
    right = mutant(TifBook, "none", ct.CASES[name].ring)(S)
    for k, b in enumerate(batches[:3]):
        r, f = right.submit(b)
        same(r, outs[k][0], FIELDS_RES, f"batch {k} results")
        same(f, outs[k][1], FIELDS_FILL, f"batch {k} tape")
