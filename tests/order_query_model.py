"""Model of me_order_query (include/me_engine.h) — TEST INFRASTRUCTURE ONLY.

Everything comes from `model.dump(s)` of a PyBook-family model: bids best first, then asks best first, FIFO
order inside a level. For a resting order

  ahead    the entries of its side and price that come before it in the dump,
  better   the entries of its side at strictly better prices (the levels listed before its own).

`ahead_by_seq` computes *ahead* the other way — the live orders at the order's level with a smaller seq —
which is the same set while seqs ascend along every FIFO (the audited invariant chain.fifo_seq_order).
"""
from __future__ import annotations

import numpy as np

BUY, SELL = 1, 2
ORDER_INFO_DTYPE = np.dtype(
    [("seq", "<u8"), ("price_q4", "<i8"), ("qty_ahead", "<i8"), ("level_qty", "<i8"), ("qty_better", "<i8"),
     ("qty", "<i4"), ("orders_ahead", "<u4"), ("levels_better", "<u4"), ("symbol", "<u4"), ("side", "u1"),
     ("found", "u1"), ("pad", "u1", (6,))]
)
FIELDS = ("seq", "price_q4", "qty_ahead", "level_qty", "qty_better", "qty", "orders_ahead", "levels_better", "symbol",
          "side", "found")


def positions(model, num_symbols, symbol_ids=None):
    """seq -> (price, qty_ahead, level_qty, qty_better, qty, orders_ahead, levels_better, symbol, side) of
    every resting order, by walking each symbol's dump once."""
    out = {}
    for s in range(num_symbols):
        d = model.dump(s)
        sym = int(symbol_ids[s]) if symbol_ids is not None else s
        cols = list(zip(d["seq"].tolist(), d["price_q4"].tolist(), d["qty"].tolist(), d["side"].tolist()))
        for side in (BUY, SELL):
            rows = [(seq, px, q) for seq, px, q, sd in cols if sd == side]
            levels = []  # [(price, [(seq, qty)])] in dump order: best first
            for seq, px, q in rows:
                if not levels or levels[-1][0] != px:
                    levels.append((px, []))
                levels[-1][1].append((seq, q))
            assert len({px for px, _ in levels}) == len(levels), "a price appears twice on one side of a dump"
            qty_better = 0
            for nbetter, (px, fifo) in enumerate(levels):
                level_qty = sum(q for _, q in fifo)
                ahead_q = 0
                for nahead, (seq, q) in enumerate(fifo):
                    assert seq not in out, f"seq {seq} rests twice"
                    out[seq] = (px, ahead_q, level_qty, qty_better, q, nahead, nbetter, sym, side)
                    ahead_q += q
                qty_better += level_qty
    return out


def ahead_by_seq(model, num_symbols):
    """seq -> (qty_ahead, orders_ahead) as "the live orders at its level with a smaller seq"."""
    out = {}
    for s in range(num_symbols):
        d = model.dump(s)
        by_level = {}
        for e in d:
            by_level.setdefault((int(e["side"]), int(e["price_q4"])), []).append((int(e["seq"]), int(e["qty"])))
        for fifo in by_level.values():
            for seq, _ in fifo:
                older = [q for t, q in fifo if t < seq]
                out[seq] = (sum(older), len(older))
    return out


def expected(model, num_symbols, seqs, symbol_ids=None):
    """The answers me_order_query owes for `seqs` (any integers in [0, 2^64)), as ORDER_INFO_DTYPE."""
    pos = positions(model, num_symbols, symbol_ids)
    out = np.zeros(len(seqs), dtype=ORDER_INFO_DTYPE)
    for i, q in enumerate(seqs):
        q = int(q)
        out[i]["seq"] = q
        p = pos.get(q)
        if p is None:
            continue
        (out[i]["price_q4"], out[i]["qty_ahead"], out[i]["level_qty"], out[i]["qty_better"], out[i]["qty"],
         out[i]["orders_ahead"], out[i]["levels_better"], out[i]["symbol"], out[i]["side"]) = p
        out[i]["found"] = 1
    return out


def assert_answers_equal(got, want, ctx=""):
    assert len(got) == len(want), f"{ctx}: {len(got)} answers for {len(want)} queries"
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (f"{ctx}: field {f} differs at query {int(bad[0])} (seq {int(want['seq'][bad[0]])}): "
                               f"got {got[bad[0]]}, want {want[bad[0]]}; {len(bad)} in all")
    assert not got["pad"].any(), f"{ctx}: pad bytes are not zero"
