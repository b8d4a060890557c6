"""Hostile cancel targets — TEST INFRASTRUCTURE ONLY.

`tif_model.tif_stream` names only polite targets (an issued LIMIT of the cancel's own symbol, or seq + 1000).
`overlay` rewrites the target of every cancel of such a stream: it steps a reference book (`TifBook`, or
`PyBook` for the plain variant) record by record, so at each cancel it knows what is live, draws one of the
classes below and writes the target into `price_q4`. All classes are judged at the cancel's position:

  live_own      a live order of the cancel's symbol (weighted up: the book churns but stays populated). Where
                the symbol has orders more than a ring old, seven in ten draws name one of them (the old-order
                table's route); of the rest 85 % name one of its eight youngest, so that some grow old
  other_symbol  a live order of another symbol
  repeat        one of the last four targets this symbol cancelled successfully
  never_rests   the seq of an earlier MARKET, IOC or FOK of this symbol (filled or killed), or of a GTC LIMIT
                that filled completely on entry
  filled_later  a LIMIT of this symbol that rested and was consumed since
  rejected      the seq of a record of this symbol rejected for BAD_QTY, BAD_SIDE, WOULD_CROSS or BAD_TIF
  future        a seq 1..200 above the cancel's own. Such a target is not live at its cancel whatever it is, so
                a second pass picks it after the books are known: where it can, a LIMIT of the same symbol
                issued later that rests at the end of its batch (the cancel's batch or, preferred, a later
                one): that order must rest untouched. Cancels near the end of a batch draw this class more often
  own_seq       the cancel's own seq (the previous NEW record's): succeeds exactly when that record is this
                symbol's and rested
  alias_plus / alias_minus   T +- k * R for a live T of this symbol, the engine's seq-ring size R, k in {1, 2}
  zero, huge    0; -1, INT64_MIN, INT64_MAX in the int64 field (u64 seqs at or above 2^63)

The module also holds the (seed, shape) list the CPU model tests and the GPU tests share (`CASES`), the cached
streams and the cached reference outputs.
"""
from __future__ import annotations

import functools
from collections import deque, namedtuple

import numpy as np

from oracle.pybook import RJ_BAD_QTY, RJ_BAD_SIDE, ST_CANCELED, ST_REJECTED, PyBook
from tests import tif_model as tm
from tests.tif_model import RJ_BAD_TIF, RJ_WOULD_CROSS, Arrays, TifBook

CLASSES = ("live_own", "other_symbol", "repeat", "never_rests", "filled_later", "rejected", "future", "own_seq",
           "alias_plus", "alias_minus", "zero", "huge")
CLS = {name: i for i, name in enumerate(CLASSES)}
# live_own is weighted so that at least a quarter of all cancels remove an order and the books stay populated
# (tuned on the CPU: tests/test_cancel_targets_model.py asserts the conditions for every case)
WEIGHTS = {name: 1.0 for name in CLASSES}
WEIGHTS["live_own"] = 5.0
OWN_SEQ_BOOST = 0.05  # a cancel right behind a resting order of its symbol names it this often
FUTURE_BOOST = 0.5  # a cancel in the last quarter of its batch's seqs (200 at the most) draws `future` this often, and then mostly with
                    # the look-ahead: targets in the next batch
HUGE = (-1, -(1 << 63), (1 << 63) - 1)
MIX = (30, 10, 5, 5, 10, 40)
MIX_RING = (35, 10, 5, 5, 5, 40)  # fewer MARKETs: thin books let them sweep the far levels, and no order grows old
REJECTS = (RJ_BAD_QTY, RJ_BAD_SIDE, RJ_WOULD_CROSS, RJ_BAD_TIF)


def to_i64(v):
    """A u64 seq (mod 2^64) as the int64 the price field carries."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def one(b, i, px=None):
    """Record i of a batch as a one-record batch."""
    return Arrays(b.seq[i:i + 1], b.price_q4[i:i + 1] if px is None else [px], b.qty[i:i + 1], b.symbol[i:i + 1],
                  b.kind[i:i + 1])


def may_rest(kd, qty):
    """A LIMIT record (GTC or POST_ONLY, valid side and quantity) — one that can leave a resting order."""
    return not (kd & 0x0C) and ((kd >> 4) & 3) in (tm.TIF_GTC, tm.TIF_POST_ONLY) and (kd & 3) in (1, 2) and qty > 0


def overlay(seed, num_symbols, batches, *, tif, ring, weights=None):
    """Rewrites the cancel targets of `batches` (their TIF bits kept for tif=True, cleared by the caller for
    the plain variant). Returns (batches, classes, info): new Arrays, per batch an int8 array with the class of
    each cancel (-1 elsewhere), and counters taken while stepping the reference book."""
    rng = np.random.default_rng(seed)
    S = num_symbols
    book = TifBook(S) if tif else PyBook(S)
    w = dict(WEIGHTS, **(weights or {}))
    p = np.array([w[c] for c in CLASSES], dtype=np.float64)
    p /= p.sum()
    ahead = {}  # seq -> (batch, symbol) of the LIMITs that may rest
    for k, b in enumerate(batches):
        for i in np.nonzero((b.kind & 8) == 0)[0]:
            if may_rest(int(b.kind[i]), int(b.qty[i])) and int(b.seq[i]):
                ahead[int(b.seq[i])] = (k, int(b.symbol[i]))
    live = [dict() for _ in range(S)]  # the symbol's live seqs, oldest first
    done = [deque(maxlen=4) for _ in range(S)]  # its last successful cancel targets
    never, never_rem, filled, rejected = ([[] for _ in range(S)] for _ in range(4))
    last_new = 0  # the seq of the last NEW record (what a cancel repeats)
    info = {"alias_on_live": 0, "future_ahead_same": 0, "future_ahead_later": 0}

    def pick(lst):
        return lst[int(rng.integers(len(lst)))]

    def target(c, s, k, own):
        """The class's target for a cancel of symbol s in batch k, or None when the class has no candidate."""
        if c == "live_own":
            if live[s]:
                keys = list(live[s])
                old = [t for t in keys if own - t > ring]
                if old and rng.random() < 0.7:
                    return pick(old)
                return pick(keys[-8:]) if rng.random() < 0.85 else pick(keys)
        elif c == "other_symbol":
            others = [t for t in range(S) if t != s and live[t]]
            if others:
                return pick(list(live[pick(others)]))
        elif c == "repeat":
            if done[s]:
                return pick(list(done[s]))
        elif c == "never_rests":
            if never_rem[s] and rng.random() < 0.5:  # (half of them: a remainder was discarded)
                return pick(never_rem[s])
            if never[s]:
                return pick(never[s])
        elif c == "filled_later":
            if filled[s]:
                return pick(filled[s])
        elif c == "rejected":
            if rejected[s]:
                return pick(rejected[s])
        elif c == "future":  # (never live at the cancel, so the choice changes no book: see the second pass)
            return own + int(rng.integers(1, 201))
        elif c == "own_seq":
            return own
        elif c in ("alias_plus", "alias_minus"):
            if live[s]:
                t = pick(list(live[s])) + (1 if c == "alias_plus" else -1) * int(rng.integers(1, 3)) * ring
                info["alias_on_live"] += 1
                return t
        elif c == "zero":
            return 0
        elif c == "huge":
            return pick(HUGE)
        return None

    pxs, classes, pending, live_end = [], [], [], []
    for k, b in enumerate(batches):
        px = b.price_q4.copy()
        cls = np.full(len(b), -1, dtype=np.int8)
        last_seq = int(b.seq.max())
        near = min(200, (last_seq - int(b.seq.min())) // 4)
        for i in range(len(b)):
            s, kd, seq = int(b.symbol[i]), int(b.kind[i]), int(b.seq[i])
            if s >= S:
                book.submit(one(b, i))
                continue
            if kd & 8:
                c = CLASSES[int(rng.choice(len(CLASSES), p=p))]
                if seq == last_new and seq in live[s] and rng.random() < OWN_SEQ_BOOST:
                    c = "own_seq"
                elif k + 1 < len(batches) and last_seq - seq < near and rng.random() < FUTURE_BOOST:
                    c = "future"
                t = target(c, s, k, seq)
                for c2 in ("live_own", "future"):  # a class without a candidate yet
                    if t is None:
                        c, t = c2, target(c2, s, k, seq)
                px[i] = to_i64(t)
                cls[i] = CLS[c]
                if c == "future":
                    pending.append((k, i, s, seq, 0.9 if last_seq - seq < near else 0.5))
                res, _ = book.submit(one(b, i, int(px[i])))
                if res[0]["status"] == ST_CANCELED:
                    tu = t & ((1 << 64) - 1)
                    del live[s][tu]
                    done[s].append(tu)
                continue
            res, fills = book.submit(one(b, i))
            r = res[0]
            if seq:
                last_new = seq
            if r["status"] == ST_REJECTED:
                if int(r["reason"]) in REJECTS and seq:
                    rejected[s].append(seq)
                continue
            for m in fills["maker_seq"].tolist():
                if m not in book.live and m in live[s]:
                    del live[s][m]
                    filled[s].append(m)
            if seq in book.live:
                live[s][seq] = None
            else:
                never[s].append(seq)
                if int(r["remaining_qty"]) > 0:
                    never_rem[s].append(seq)
        pxs.append(px)
        classes.append(cls)
        live_end.append(set(book.live))
    assert sum(len(d) for d in live) == len(book.live)
    # second pass: half of the future targets become the seq of a LIMIT of the same symbol, issued up to 200 seqs
    # later, that rests at the end of its batch (a later batch preferred). A future target is not live at its
    # cancel whatever it is, so the books above stay as they are.
    for k, i, s, own, look in pending:
        if rng.random() < look:
            cand = [t for t in range(own + 1, own + 201) if ahead.get(t, (0, -1))[1] == s and t in live_end[ahead[t][0]]]
            later = [t for t in cand if ahead[t][0] > k]
            if later and rng.random() < 0.7:
                cand = later
            if cand:
                t = pick(cand)
                info["future_ahead_later" if ahead[t][0] > k else "future_ahead_same"] += 1
                pxs[k][i] = t
    out = [Arrays(b.seq, px, b.qty, b.symbol, b.kind) for b, px in zip(batches, pxs)]
    return out, classes, info


# ---- the cases the CPU model tests and the GPU tests share -----------------------------------------------

Case = namedtuple("Case", "seed levels nbatches batch tif ring seq_start far_pct skew")
S_CX = 12
BIG_RING, SMALL_RING = 1 << 22, 1024
SEQ_HIGH = (1 << 40) + 3
CASES = {
    # every path: 128 levels (k_match_reg, the grouped walks), 1,024 (deep, the aggregate hot walk), 2,048 (k_match_hot)
    "l128_tif": Case(1101, 128, 8, 1500, True, BIG_RING, SEQ_HIGH, 2, True),
    "l128_plain": Case(1102, 128, 8, 1500, False, BIG_RING, 1, 2, True),
    "l1024_tif": Case(1103, 1024, 8, 1500, True, BIG_RING, SEQ_HIGH, 2, True),
    "l1024_plain": Case(1104, 1024, 8, 1500, False, BIG_RING, 1, 2, True),
    "l2048_tif": Case(1105, 2048, 8, 1500, True, BIG_RING, SEQ_HIGH, 2, True),
    "l2048_plain": Case(1106, 2048, 8, 1500, False, BIG_RING, 1, 2, True),
    # a 1,024-entry seq ring that wraps more than five times: groups of four 200-record batches (a group spans
    # fewer than 1,024 seqs), 800-record batches on the deep path; more far LIMITs, which live long enough to be
    # cancelled when the ring has forgotten them
    "ring128_tif": Case(1107, 128, 48, 200, True, SMALL_RING, SEQ_HIGH, 6, True),
    "ring128_plain": Case(1108, 128, 48, 200, False, SMALL_RING, SEQ_HIGH, 6, True),
    "ring1024_tif": Case(1109, 1024, 12, 800, True, SMALL_RING, SEQ_HIGH, 6, True),
    "ring1024_plain": Case(1110, 1024, 12, 800, False, SMALL_RING, SEQ_HIGH, 6, True),
    # what the cancel walk keeps: no far LIMITs, no TIF verdicts, no symbol above 128 records per batch, so
    # nearly every symbol stays on k_agg_gwalk_cx for whole groups (its own target lookups answer the cancels)
    "walk128_plain": Case(1111, 128, 8, 1200, False, BIG_RING, SEQ_HIGH, 0, False),
    "walkring128_plain": Case(1112, 128, 48, 200, False, SMALL_RING, SEQ_HIGH, 0, False),
}
RING_CASES = tuple(n for n, c in CASES.items() if c.ring == SMALL_RING)


def polite(name):
    """The case's stream before the overlay: (base prices, batches)."""
    c = CASES[name]
    base, batches = tm.tif_stream(c.seed, S_CX, c.levels, c.nbatches, c.batch, far_pct=c.far_pct, mix=MIX_RING if c.ring == SMALL_RING else MIX, seq_start=c.seq_start,
                                  skew=c.skew)
    if not c.tif:
        batches = [Arrays(b.seq, b.price_q4, b.qty, b.symbol, b.kind & 0x0F) for b in batches]
    return base, batches


@functools.lru_cache(maxsize=None)
def stream(name):
    """(base prices, batches, classes, info) of a case. Shared: callers must not change the arrays."""
    c = CASES[name]
    base, batches = polite(name)
    batches, classes, info = overlay(c.seed + 5000, S_CX, batches, tif=c.tif, ring=c.ring)
    return base, batches, classes, info


@functools.lru_cache(maxsize=None)
def expected(name):
    """The reference's outputs for a case: ([(results, fills) per batch], resting() after each batch, the
    book after the last batch). Computed once and shared; the book must not be stepped further."""
    c = CASES[name]
    _, batches, _, _ = stream(name)
    book = TifBook(S_CX) if c.tif else PyBook(S_CX)
    outs, resting = [], []
    for b in batches:
        outs.append(book.submit(b))
        resting.append(len(book.live))
    return outs, resting, book
