"""Model of me_order_preview (include/me_engine.h) — TEST INFRASTRUCTURE ONLY.

Everything comes from `model.dump(s)` of a PyBook-family model (bids best first, then asks best first, FIFO
order inside a level); the levels are rebuilt from it as order_query_model.positions does. The time-in-force
rules are restated here from DESIGN.md §2, not taken from the models' submit():

  reject order  BAD_SYMBOL (every field 0), BAD_QTY (remaining 0), BAD_SIDE, BAD_TIF (POST_ONLY on a MARKET),
                WOULD_CROSS (a POST_ONLY LIMIT whose price reaches the opposite best); the last three leave
                remaining = qty. There is no seq, hence no BAD_SEQ.
  taking        the opposite side best price first, FIFO inside a level, while the level's price is within the
                limit (BUY: price <= limit, SELL: price >= limit; any price for a MARKET).
  GTC LIMIT     NEW / PARTIALLY_FILLED / FILLED, the remainder rests. MARKET, IOC: FILLED, or CANCELED with the
                discarded remainder. FOK: when the quantity within the limit is below qty, CANCELED with filled 0,
                remaining qty and no fill; else it executes and is FILLED. POST_ONLY: NEW, rests whole.

A query is (symbol, kind, price_q4, qty). The notional is kept as a Python int and split into two's-complement
halves at the end.
"""
from __future__ import annotations

import numpy as np

BUY, SELL = 1, 2
ST_NEW, ST_PARTIAL, ST_FILLED, ST_CANCELED, ST_REJECTED = 0, 1, 2, 3, 4
RJ_NONE, RJ_BAD_QTY, RJ_BAD_SIDE, RJ_BAD_SYMBOL, RJ_WOULD_CROSS, RJ_BAD_TIF = 0, 1, 2, 4, 8, 9
TIF_GTC, TIF_IOC, TIF_FOK, TIF_POST_ONLY = 0, 1, 2, 3
PV_HAS_OPP, PV_CROSSES, PV_RESTS = 1, 2, 4
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
M64 = (1 << 64) - 1

PREVIEW_DTYPE = np.dtype(
    [("first_price_q4", "<i8"), ("last_price_q4", "<i8"), ("opp_price_q4", "<i8"), ("notional_hi", "<i8"),
     ("notional_lo", "<u8"), ("filled_qty", "<i4"), ("remaining_qty", "<i4"), ("fill_count", "<u4"), ("levels", "<u4"),
     ("status", "u1"), ("reason", "u1"), ("flags", "u1"), ("pad", "u1", (5,))]
)
FIELDS = ("status", "reason", "filled_qty", "remaining_qty", "fill_count", "levels", "first_price_q4", "last_price_q4",
          "opp_price_q4", "notional_hi", "notional_lo", "flags")
RESULT_FIELDS = ("status", "reason", "filled_qty", "remaining_qty", "fill_count")


def notional(row) -> int:
    return (int(row["notional_hi"]) << 64) | int(row["notional_lo"])


def split128(v: int):
    """(hi, lo) of a signed 128-bit value: hi signed, lo unsigned."""
    assert -(1 << 127) <= v < (1 << 127)
    return v >> 64, v & M64


def levels_of(model, s):
    """{BUY: [(price, [(seq, qty), ...]), ...], SELL: ...} of symbol s, each side best first."""
    d = model.dump(s)
    out = {BUY: [], SELL: []}
    for seq, px, q, sd in zip(d["seq"].tolist(), d["price_q4"].tolist(), d["qty"].tolist(), d["side"].tolist()):
        lv = out[sd]
        if not lv or lv[-1][0] != px:
            lv.append((px, []))
        lv[-1][1].append((seq, q))
    for sd in (BUY, SELL):
        assert len({px for px, _ in out[sd]}) == len(out[sd]), "a price appears twice on one side of a dump"
    return out


def _within(side, market, limit, p):
    return market or (p <= limit if side == BUY else p >= limit)


def execution(opp, side, market, limit, qty):
    """The fills (maker seq, price, qty) of a taker of `qty` against the levels `opp` (best first)."""
    fills, rem = [], qty
    for p, fifo in opp:
        if rem == 0 or not _within(side, market, limit, p):
            break
        for seq, q in fifo:
            if rem == 0:
                break
            t = min(rem, q)
            fills.append((seq, p, t))
            rem -= t
    return fills


def fold(fills):
    """(filled_qty, fill_count, levels, first price, last price, notional) of fills given as (.., price, qty)
    pairs in fill order: what the execution fields of an answer describe."""
    px = [int(p) for p, _ in fills]
    return (sum(int(q) for _, q in fills), len(fills), len(set(px)), px[0] if px else 0, px[-1] if px else 0,
            sum(int(p) * int(q) for p, q in fills))


def expected(model, num_symbols, queries):
    """The answers me_order_preview owes for `queries` [(symbol, kind, price_q4, qty), ...] as PREVIEW_DTYPE."""
    books = {}
    out = np.zeros(len(queries), dtype=PREVIEW_DTYPE)
    for i, (s, kd, px, q) in enumerate(queries):
        s, kd, px, q = int(s), int(kd), int(px), int(q)
        assert not kd & 8, "a CANCEL / REDUCE kind is refused by the call, it has no answer"
        r = out[i]
        side, market, tif = kd & 3, bool(kd & 4), (kd >> 4) & 3
        if s >= num_symbols:
            r["status"], r["reason"] = ST_REJECTED, RJ_BAD_SYMBOL
            continue
        if q <= 0:
            r["status"], r["reason"] = ST_REJECTED, RJ_BAD_QTY
            continue
        r["remaining_qty"] = q
        if side not in (BUY, SELL):
            r["status"], r["reason"] = ST_REJECTED, RJ_BAD_SIDE
            continue
        if tif == TIF_POST_ONLY and market:
            r["status"], r["reason"] = ST_REJECTED, RJ_BAD_TIF
            continue
        if s not in books:
            books[s] = levels_of(model, s)
        opp = books[s][SELL if side == BUY else BUY]
        flags = 0
        if opp:
            flags |= PV_HAS_OPP
            r["opp_price_q4"] = opp[0][0]
            if _within(side, market, px, opp[0][0]):
                flags |= PV_CROSSES
        if tif == TIF_POST_ONLY:
            if flags & PV_CROSSES:
                r["status"], r["reason"] = ST_REJECTED, RJ_WOULD_CROSS
            else:
                r["status"] = ST_NEW
                flags |= PV_RESTS
            r["flags"] = flags
            continue
        if tif == TIF_FOK:
            avail = sum(sum(x for _, x in fifo) for p, fifo in opp if _within(side, market, px, p))
            if avail < q:
                r["status"], r["flags"] = ST_CANCELED, flags
                continue
        fills = execution(opp, side, market, px, q)
        filled, count, nlev, first, last, ntl = fold([(p, t) for _, p, t in fills])
        rem = q - filled
        r["filled_qty"], r["remaining_qty"], r["fill_count"], r["levels"] = filled, rem, count, nlev
        r["first_price_q4"], r["last_price_q4"] = first, last
        r["notional_hi"], r["notional_lo"] = split128(ntl)
        if market or tif != TIF_GTC:
            r["status"] = ST_FILLED if rem == 0 else ST_CANCELED
        else:
            r["status"] = ST_FILLED if rem == 0 else (ST_PARTIAL if filled else ST_NEW)
            if rem > 0:
                flags |= PV_RESTS
        r["flags"] = flags
    return out


def assert_answers_equal(got, want, ctx="", queries=None):
    assert len(got) == len(want), f"{ctx}: {len(got)} answers for {len(want)} queries"
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        if len(bad):
            k = int(bad[0])
            q = f" query {tuple(int(x) for x in queries[k])}" if queries is not None else ""
            raise AssertionError(f"{ctx}: field {f} differs at query {k}{q}: got {got[k]}, want {want[k]}; "
                                 f"{len(bad)} in all")
    assert not got["pad"].any(), f"{ctx}: pad bytes are not zero"


def assert_matches_submit(row, res, fills, ctx=""):
    """A preview row against the me_order_result `res` and the fills the same record got when it was submitted
    right afterwards: the five result fields, and the execution fields against the fold of the fills."""
    for f in RESULT_FIELDS:
        assert int(row[f]) == int(res[f]), f"{ctx}: {f}: previewed {int(row[f])}, submitted {int(res[f])}"
    filled, count, nlev, first, last, ntl = fold([(int(p), int(q)) for p, q in zip(fills["price_q4"], fills["qty"])])
    got = (int(row["filled_qty"]), int(row["fill_count"]), int(row["levels"]), int(row["first_price_q4"]),
           int(row["last_price_q4"]), notional(row))
    assert got == (filled, count, nlev, first, last, ntl), f"{ctx}: previewed execution {got}, submitted {(filled, count, nlev, first, last, ntl)}"
