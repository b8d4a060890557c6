"""Structural audit of the resident book — TEST INFRASTRUCTURE ONLY.

`Engine.debug_export()` returns the device arrays of the book as the kernels left them (DESIGN.md §3,
me_layout.hpp). The book holds every fact several times; `audit(raw)` checks that the copies agree, and
rebuilds every symbol's resting orders from the raw arrays alone. Written from DESIGN.md §3 and the struct
comments of me_layout.hpp, not from the kernels: plain numpy and Python, no GPU.

    violations, logical_books = audit(raw)

`violations` is a list of Violation(name, symbol, where, detail): `name` is the invariant (the keys of
INVARIANTS), `where` the level / chunk / slot. `logical_books[s]` is symbol s's resting orders in
BOOK_ENTRY_DTYPE: bids best first, then asks best first, FIFO order inside a level: what `Engine.dump(s)` and
the models' `dump(s)` return.

AUTHORITY is the authority table of DESIGN.md §3: for every redundant field, how strong the auditor's
assertion is (the strength its strictest reader between two launches needs) and under which condition. An
exemption is a row of this table; there is no other way to switch a check off.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from matching_engine_amd._abi import (BOOK_ENTRY_DTYPE, CHUNK_SLOTS, DBG_CP_FRESH, DBG_CP_NRECL, DBG_FC_HALF,
                                      DBG_ST_RESTING)

NIL = 0xFFFFFFFF
BUY, SELL = 1, 2
C = CHUNK_SLOTS

Violation = namedtuple("Violation", "name symbol where detail")

# invariant -> what it says
INVARIANTS = {
    "level.total_nonneg": "a level's total is >= 0",
    "level.empty_iff_nil": "total == 0 <=> head == tail == NIL",
    "chain.id_range": "every chunk id of a chain is < nchunks",
    "chain.cycle": "a chain visits no chunk twice",
    "chain.ends_at_tail": "hdr.next leads from head to tail",
    "chain.prev": "hdr.prev is the chunk before (NIL at the head)",
    "chain.price": "hdr.price is the level's price",
    "chain.owner": "owner is the symbol",
    "chain.negative_qty": "no slot of a linked chunk holds a negative quantity",
    "chain.empty_chunk_linked": "every linked chunk holds >= 1 live slot",
    "chain.sum_total": "the live quantities of the chain sum to the level's total",
    "chain.fifo_seq_order": "live seqs ascend strictly along the FIFO",
    "tend.range": "1 <= tend <= 16 on an occupied level",
    "tend.covers_live": "every tail-chunk slot at index >= tend holds quantity 0",
    "sides.bid_below_ask": "-1 <= best_bid < best_ask <= L",
    "sides.level_between": "no occupied level lies strictly between best_bid and best_ask (the hints bound the best levels)",
    "sides.hint_exact": "best_bid / best_ask name an occupied level, or -1 / L on an empty side",
    "occ.bit_matches_total": "occ bit <=> total > 0",
    "far.count_le_cap": "nfar[k] <= fdir.cap",
    "far.region_in_arena": "a side's region lies inside the arena",
    "far.region_placement": "a region is the side's inline one or lies in the active half below its top",
    "far.regions_disjoint": "regions of distinct (symbol, side) are disjoint",
    "far.price_order": "far prices ascend strictly (bids) / descend strictly (asks): best last",
    "far.invariant_I": "every far bid < base, every far ask >= base + L",
    "far.total_positive": "every far entry has total > 0",
    "counts.sym_resting": "SymState.resting == the symbol's live slots",
    "counts.st_resting": "the symbols' resting counts sum to ST_RESTING",
    "counts.chunks_le_orders": "linked chunks <= resting orders",
    "partition.chunk_in_two_places": "no chunk id is in two of: level chains, free lists, fcache rows, unconsumed recl",
    "partition.free_list": "a free list is a NIL-terminated chain of ids < nchunks; nfree <= 64; fcache / recl ids < nchunks",
    "partition.live_chunk_unlinked": "every chunk holding a non-zero quantity is linked",
    "partition.free_chunk_nonzero": "a chunk on a free list, in an fcache row or in recl has all 16 quantities 0",
    "partition.beyond_high_water": "a chunk in use or parked was handed out by the pool (id below its high-water mark)",
    "lookup.ring": "every live order with seq >= horizon has loc[seq & ring_mask] == its slot",
    "lookup.old_table": "every older live order has an entry {current epoch, slot, seq} in old",
    "lookup.last_seq": "sq.last is the largest seq submitted (>= every live seq)",
    "err.zero": "the sticky error word is 0",
}

# ---- the authority table (DESIGN.md §3 holds the same rows) ---------------------------------------------------
# strength: "exact" (asserted as stated), "bound" (may err on the side its readers tolerate: asserted one-sided, the
# argument says which side), "unread" (no reader between launches under `when`: not asserted). `when` is a
# condition on the export's info.
Row = namedtuple("Row", "field writers readers strength when argument")
ANY = "any L"
AUTHORITY = (
    Row("Level.total", "every matcher's level write-back; lad_recentre; far <-> window moves",
        "every matcher (sweeps and FOK / POST_ONLY verdicts run on totals), k_book_snapshot, quote and depth scans",
        "exact", ANY, "the aggregate walks match on totals alone: a wrong total is a wrong fill"),
    Row("Level.head / tail, hdr.next / prev", "the FIFO writers of every path", "every matcher, k_book_snapshot",
        "exact", ANY, "a take walks head -> tail; an unlink reads prev"),
    Row("hdr.price, owner", "whoever links a chunk; the pool when it hands one out", "cancel / reduce lookups (verify owner, "
        "find the level by price)", "exact", ANY, "a cancel locates its level by the chunk's price"),
    Row("tend", "appends, tail unlinks", "every append (never reads the chunk)", "exact", ANY,
        "asserted as: 1..16 and no live slot at or past it; an append at a tend below a live slot would overwrite an order"),
    Row("best_bid / best_ask", "k_match wave_end, k_match_reg epilogue, k_agg_gres / k_agg_fin symbol write-back",
        "every matcher loads the pair and sweeps from it; snapshot, quote and depth scans step over empty levels from it",
        "exact", ANY, "the scans need a bound only, but a matcher that loads a hint naming an empty level starts its "
        "sweep there: asserted exact, the strictest reader"),
    Row("occ", "k_match / k_match_hot ladders, k_agg_walk lw_end, k_match_reg epilogue", "k_match next_occ / prev_occ and "
        "the occ-gated total loads, k_agg_walk's LDS copy, k_depth_scan (L > 128)", "exact", "L > 128",
        "the deep matchers search the next level through occ and the depth scan visits only set bits"),
    Row("occ", "k_match_reg epilogue, the grouped walk's lw_end", "none: k_match_reg and the grouped walks rebuild the "
        "mask from the 128 totals by ballot, the scans load every total of a block", "exact", "L <= 128",
        "no reader needs it, but both writers store the ballot of the totals and every audited image has it exact on every "
        "path, so it is asserted exact: a writer that stops maintaining it must come here and say so"),
    Row("SymState.resting, ST_RESTING", "every symbol write-back adds its change", "admission control, me_book_dump sizing",
        "exact", ANY, "admission control's bound is proven from the exact count"),
    Row("free list, fcache row, recl, chunk_top / cpool", "frees of every path; chunk_reclaim", "allocations of every path",
        "bound", ANY, "a chunk reachable from two places is handed out twice; a chunk in NO place is only lost until the "
        "next reclamation (it scans quantities), so leaks are not asserted"),
    Row("loc", "every rest", "cancel / reduce of an order with seq >= horizon", "bound", ANY,
        "a live order's entry must name its slot (else it cannot be cancelled); entries of dead orders are never deleted and "
        "every hit is verified against the slot, so they are not asserted"),
    Row("old", "k_seq_sweep rebuild", "cancel / reduce of an order older than the horizon", "bound", ANY,
        "every older live order must be on its probe path in the current epoch; entries of earlier epochs read as empty and "
        "entries of orders that died since the rebuild are harmless (every hit is verified)"),
    Row("fdir, far regions, far_ctl", "far_grow, far_collect", "every far access, k_book_snapshot, the scans", "exact", ANY,
        "two sides sharing entries corrupt each other's levels"),
    Row("sq.last", "k_seq_sweep", "k_seq_sweep's order check of the next group", "exact", ANY,
        "asserted >= every live seq from the image alone, == the stream's last seq when the caller passes it"),
)


def strength(field, info):
    """The strength AUTHORITY gives `field` for this export."""
    L = info["levels"]
    for r in AUTHORITY:
        if r.field == field and (r.when == ANY or (r.when == "L > 128") == (L > 128)):
            return r.strength
    raise KeyError(field)


def old_hash(q):
    q &= (1 << 64) - 1
    q ^= q >> 33
    q = (q * 0xff51afd7ed558ccd) & ((1 << 64) - 1)
    q ^= q >> 33
    return q


def high_water(raw):
    """Chunk ids below this have been handed out at some point (me_layout.hpp cp_hw)."""
    top = int(raw["chunk_top"][0])
    nrecl, fresh = int(raw["cpool"][DBG_CP_NRECL]), int(raw["cpool"][DBG_CP_FRESH])
    h = fresh + (top - nrecl) if top > nrecl else fresh
    return min(h, raw["info"]["nchunks"])


def audit(raw, last_seq=None):
    """(violations, logical_books) of one export. last_seq: the largest seq submitted so far, when known.
    `audit.last` keeps the last call's figures (live and old orders, linked chunks, horizon, high-water mark) for
    the tests' non-vacuity assertions."""
    info = raw["info"]
    S, L, W, NC = info["num_symbols"], info["levels"], info["level_words"], info["nchunks"]
    # the one-sided checks below are the table's "bound" rows, and nothing else is
    assert [r.field for r in AUTHORITY if r.strength != "exact"] == \
        ["free list, fcache row, recl, chunk_top / cpool", "loc", "old"], "the auditor's exemptions are AUTHORITY's rows"
    chunks = raw["chunks"]
    c_next, c_prev, c_price, c_owner = chunks["next"], chunks["prev"], chunks["price"], chunks["owner"]
    qty, seqs = chunks["qty"], chunks["seq"]
    out = []

    def bad(name, s, where, detail=""):
        assert name in INVARIANTS, name
        out.append(Violation(name, s, where, detail))

    place = {}  # chunk id -> where it was found first

    def claim(ch, s, where):
        if ch in place:
            bad("partition.chunk_in_two_places", s, f"chunk {ch}", f"{where} and {place[ch]}")
            return False
        place[ch] = where
        return True

    live_seq, live_gid = [], []  # every live order found on a chain

    def walk(s, where, price, total, head, tail, tend):
        """Check one level (window or far) and return its live orders [(seq, qty)] in FIFO order."""
        orders = []
        nlinked = 0
        if total < 0:
            bad("level.total_nonneg", s, where, f"total {total}")
        if (total == 0) != (head == NIL and tail == NIL) or (head == NIL) != (tail == NIL):
            bad("level.empty_iff_nil", s, where, f"total {total} head {head:#x} tail {tail:#x}")
        if head == NIL:
            return orders, nlinked
        ch, prev, seen, reached = head, NIL, set(), False
        while True:
            if ch >= NC:
                bad("chain.id_range" if ch != NIL else "chain.ends_at_tail", s, where, f"chunk id {ch:#x} after {prev:#x}")
                break
            if ch in seen:
                bad("chain.cycle", s, where, f"chunk {ch} again after {prev}")
                break
            seen.add(ch)
            nlinked += 1
            claim(ch, s, where)
            if int(c_prev[ch]) != prev:
                bad("chain.prev", s, f"{where} chunk {ch}", f"prev {int(c_prev[ch]):#x}, the chain came from {prev:#x}")
            if int(c_price[ch]) != price:
                bad("chain.price", s, f"{where} chunk {ch}", f"hdr.price {int(c_price[ch])}, the level's is {price}")
            if int(c_owner[ch]) != s:
                bad("chain.owner", s, f"{where} chunk {ch}", f"owner {int(c_owner[ch])}")
            q = qty[ch]
            if (q < 0).any():
                bad("chain.negative_qty", s, f"{where} chunk {ch} slot {int(np.argmax(q < 0))}", f"{q.tolist()}")
            lv = np.nonzero(q > 0)[0]
            if len(lv) == 0:
                bad("chain.empty_chunk_linked", s, f"{where} chunk {ch}")
            for i in lv:
                orders.append((int(seqs[ch][i]), int(q[i])))
                live_seq.append(int(seqs[ch][i]))
                live_gid.append(ch * C + int(i))
            if ch == tail:
                reached = True
                break
            prev, ch = ch, int(c_next[ch])
        if reached:
            if not 1 <= tend <= C:
                bad("tend.range", s, where, f"tend {tend}")
            elif (qty[tail][tend:] != 0).any():
                bad("tend.covers_live", s, f"{where} chunk {tail}", f"tend {tend}, quantities {qty[tail].tolist()}")
        got = sum(o[1] for o in orders)
        if got != total:
            bad("chain.sum_total", s, where, f"total {total}, live quantities sum to {got}")
        sq_ = [o[0] for o in orders]
        if any(b <= a for a, b in zip(sq_, sq_[1:])):
            bad("chain.fifo_seq_order", s, where, f"seqs {sq_}")
        return orders, nlinked

    # ---- the far arena's geometry -----------------------------------------------------------------------
    fcap, half, inl, fent = info["far_levels"], info["far_half"], info["far_inline"], info["far_entries"]
    ctl = raw["far_ctl"]
    act = int(ctl[DBG_FC_HALF]) & 1
    act_lo = inl + act * half
    act_top = act_lo + int(ctl[act])
    regions = []
    for s in range(S):
        for k in range(2):
            off, cap = int(raw["fdir"][s, k]["off"]), int(raw["fdir"][s, k]["cap"])
            n = int(raw["sym"][s]["nfar"][k])
            w = f"far side {k}"
            if n > cap:
                bad("far.count_le_cap", s, w, f"nfar {n} cap {cap}")
            if off + cap > fent or off + n > fent:
                bad("far.region_in_arena", s, w, f"off {off} cap {cap} n {n}, the arena holds {fent}")
            inline = off == (2 * s + k) * fcap and cap == fcap
            if not inline and not (act_lo <= off and off + cap <= act_top):
                bad("far.region_placement", s, w, f"off {off} cap {cap}: not its inline region, not in the active half "
                    f"[{act_lo}, {act_top})")
            regions.append((off, off + cap, s, k))
    regions.sort()
    for (a0, a1, s0, k0), (b0, b1, s1, k1) in zip(regions, regions[1:]):
        if b0 < a1:
            bad("far.regions_disjoint", s1, f"far side {k1}", f"[{b0}, {b1}) overlaps symbol {s0} side {k0} [{a0}, {a1})")

    # ---- per symbol ----------------------------------------------------------------------------------------
    books = []
    occ_strength = strength("occ", info)
    hint_strength = strength("best_bid / best_ask", info)
    resting_sum = 0
    for s in range(S):
        sym = raw["sym"][s]
        base, bb, ba = int(sym["base"]), int(sym["best_bid"]), int(sym["best_ask"])
        lv = raw["levels"][s]
        total, head, tail = lv["total"], lv["head"], lv["tail"]
        tend = raw["tend"][s]
        nlinked = 0
        per_level = {}
        for l in np.nonzero((total != 0) | (head != NIL) | (tail != NIL))[0]:
            l = int(l)
            o, n = walk(s, f"level {l}", base + l, int(total[l]), int(head[l]), int(tail[l]), int(tend[l]))
            per_level[l] = o
            nlinked += n
        occupied = np.nonzero(total > 0)[0]
        # sides
        if not (-1 <= bb < ba <= L):
            bad("sides.bid_below_ask", s, "sym", f"best_bid {bb} best_ask {ba}")
        between = occupied[(occupied > bb) & (occupied < ba)]
        if len(between):
            bad("sides.level_between", s, f"level {int(between[0])}", f"occupied between best_bid {bb} and best_ask {ba}")
        if hint_strength == "exact":
            bids, asks = occupied[occupied <= bb], occupied[occupied >= ba]
            tb = int(bids[-1]) if len(bids) else -1
            ta = int(asks[0]) if len(asks) else L
            if tb != bb:
                bad("sides.hint_exact", s, "best_bid", f"hint {bb}, the best occupied bid level is {tb}")
            if ta != ba:
                bad("sides.hint_exact", s, "best_ask", f"hint {ba}, the best occupied ask level is {ta}")
        # occ
        if occ_strength != "unread":
            bits = np.zeros(W * 64, dtype=bool)
            for w_ in range(W):
                word = int(raw["occ"][s, w_])
                bits[w_ * 64:(w_ + 1) * 64] = [(word >> b) & 1 for b in range(64)]
            want = np.zeros(W * 64, dtype=bool)
            want[:L] = total > 0
            wrong = np.nonzero((want & ~bits) if occ_strength == "bound" else (want != bits))[0]
            if len(wrong):
                bad("occ.bit_matches_total", s, f"level {int(wrong[0])}", f"bit {int(bits[wrong[0]])}, total "
                    f"{int(total[wrong[0]]) if wrong[0] < L else 'none'} ({len(wrong)} levels)")
        # far sides
        far_orders = [[], []]
        for k in range(2):
            off, n = int(raw["fdir"][s, k]["off"]), int(sym["nfar"][k])
            n = max(0, min(n, fent - off)) if off < fent else 0
            ent = raw["far"][off:off + n]
            px = ent["price"].astype(object)
            for i in range(n - 1):
                if not (px[i] < px[i + 1] if k == 0 else px[i] > px[i + 1]):
                    bad("far.price_order", s, f"far side {k} entry {i}", f"prices {int(px[i])}, {int(px[i + 1])}")
            for i in range(n):
                e = ent[i]
                p = int(e["price"])
                w = f"far side {k} entry {i} price {p}"
                if (k == 0 and p >= base) or (k == 1 and p < base + L):
                    bad("far.invariant_I", s, w, f"window [{base}, {base + L})")
                if int(e["total"]) <= 0:
                    bad("far.total_positive", s, w, f"total {int(e['total'])}")
                o, nl = walk(s, w, p, int(e["total"]), int(e["head"]), int(e["tail"]), int(e["tend"]))
                nlinked += nl
                far_orders[k].append((p, o))
        # counts
        n_live = sum(len(o) for o in per_level.values()) + sum(len(o) for k in range(2) for _, o in far_orders[k])
        if int(sym["resting"]) != n_live:
            bad("counts.sym_resting", s, "sym", f"resting {int(sym['resting'])}, live slots {n_live}")
        if nlinked > n_live:
            bad("counts.chunks_le_orders", s, "sym", f"{nlinked} linked chunks, {n_live} live orders")
        resting_sum += int(sym["resting"])
        # the logical book: bids best first (window from best_bid down, then far bids from the last entry), asks
        book = []
        for l in sorted((l for l in per_level if l <= bb), reverse=True):
            book += [(q, base + l, n, BUY, (0, 0, 0)) for q, n in per_level[l]]
        for p, o in reversed(far_orders[0]):
            book += [(q, p, n, BUY, (0, 0, 0)) for q, n in o]
        for l in sorted(l for l in per_level if l >= ba):
            book += [(q, base + l, n, SELL, (0, 0, 0)) for q, n in per_level[l]]
        for p, o in reversed(far_orders[1]):
            book += [(q, p, n, SELL, (0, 0, 0)) for q, n in o]
        books.append(np.array(book, dtype=BOOK_ENTRY_DTYPE) if book else np.zeros(0, dtype=BOOK_ENTRY_DTYPE))
    if resting_sum != int(raw["stats"][DBG_ST_RESTING]):
        bad("counts.st_resting", -1, "stats", f"ST_RESTING {int(raw['stats'][DBG_ST_RESTING])}, the symbols sum to {resting_sum}")

    # ---- chunk partition ------------------------------------------------------------------------------------
    linked = set(place)
    free_places = set()
    for s in range(S):
        ch, seen = int(raw["sym"][s]["free_head"]), set()
        while ch != NIL:
            if ch >= NC or ch in seen:
                bad("partition.free_list", s, "free list", f"chunk id {ch:#x} ({'again' if ch in seen else 'out of range'})")
                break
            seen.add(ch)
            if claim(ch, s, f"free list of symbol {s}"):
                free_places.add(ch)
            ch = int(c_next[ch])
        nfree = int(raw["sym"][s]["nfree"])
        if nfree > raw["fcache"].shape[1]:
            bad("partition.free_list", s, "fcache", f"nfree {nfree}")
            nfree = raw["fcache"].shape[1]
        for j in range(nfree):
            ch = int(raw["fcache"][s, j])
            if ch >= NC:
                bad("partition.free_list", s, f"fcache[{j}]", f"chunk id {ch:#x}")
            elif claim(ch, s, f"fcache row of symbol {s}"):
                free_places.add(ch)
    top, nrecl = int(raw["chunk_top"][0]), int(raw["cpool"][DBG_CP_NRECL])
    for v in range(top, min(nrecl, NC)):
        ch = int(raw["recl"][v])
        if ch >= NC:
            bad("partition.free_list", -1, f"recl[{v}]", f"chunk id {ch:#x}")
        elif claim(ch, -1, "recl"):
            free_places.add(ch)
    hw = high_water(raw)
    for ch in sorted(place):
        if ch >= hw:
            bad("partition.beyond_high_water", -1, f"chunk {ch}", f"{place[ch]}; the pool has handed out ids below {hw}")
    nonzero = np.nonzero((qty != 0).any(axis=1))[0]
    for ch in nonzero:
        ch = int(ch)
        if ch in linked:
            continue
        name = "partition.free_chunk_nonzero" if ch in free_places else "partition.live_chunk_unlinked"
        bad(name, int(c_owner[ch]) if int(c_owner[ch]) < S else -1, f"chunk {ch}",
            f"{place.get(ch, 'in no chain')}, quantities {qty[ch].tolist()}")

    # ---- order lookup ----------------------------------------------------------------------------------------
    sq = raw["sq"][info["sq_idx"]]
    horizon, last, epoch = int(sq["horizon"]), int(sq["last"]), int(sq["epoch"])
    mask, omask = info["ring_mask"], info["old_mask"]
    loc, old = raw["loc"], raw["old"]
    n_old = 0
    for q, g in zip(live_seq, live_gid):
        w = f"chunk {g // C} slot {g % C} seq {q}"
        s = int(c_owner[g // C])
        if q >= horizon:
            if int(loc[q & mask]) != g:
                bad("lookup.ring", s, w, f"loc[{q & mask}] = {int(loc[q & mask]):#x}, the order is in slot {g}")
            continue
        n_old += 1
        h, found = old_hash(q) & omask, False
        for _ in range(omask + 1):
            e = old[h]
            if int(e["epoch"]) != epoch:
                break  # empty in this epoch: a lookup stops here
            if int(e["seq"]) == q:
                found = int(e["slot"]) == g
                break
            h = (h + 1) & omask
        if not found:
            bad("lookup.old_table", s, w, f"no entry {{epoch {epoch}, slot {g}}} on its probe path (horizon {horizon})")
    mx = max(live_seq) if live_seq else 0
    if last < mx or (last_seq is not None and last != last_seq):
        bad("lookup.last_seq", -1, "sq", f"sq.last {last}, largest live seq {mx}, largest submitted {last_seq}")
    if int(raw["err"][0]) != 0:
        bad("err.zero", -1, "err", f"{int(raw['err'][0]):#x}")
    audit.last = {"old_orders": n_old, "live_orders": len(live_seq), "linked_chunks": len(linked), "horizon": horizon,
                  "high_water": hw}
    return out, books


def names(violations):
    return sorted({v.name for v in violations})


def copy_raw(raw):
    """A deep copy of an export (corruption tests change the copy)."""
    return {k: (dict(v) if k == "info" else v.copy()) for k, v in raw.items()}


def is_drained(raw):
    """After a drain: every level empty, no far level, nothing resting, no linked chunk, every chunk all-zero.
    Returns a list of what is not."""
    left = []
    lv = raw["levels"]
    if (lv["total"] != 0).any() or (lv["head"] != NIL).any() or (lv["tail"] != NIL).any():
        left.append("window levels")
    if raw["sym"]["nfar"].any():
        left.append("nfar")
    if raw["sym"]["resting"].any() or int(raw["stats"][DBG_ST_RESTING]):
        left.append("resting")
    if (raw["chunks"]["qty"] != 0).any():
        left.append("chunk quantities")
    if raw["occ"].any():
        left.append("occ")
    return left
