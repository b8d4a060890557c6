"""Raw images of model books for the book auditor (tests/book_audit.py), and single-field corruptions of them.

`build_image` lays a model book out the way me_layout.hpp describes the resident book: a window of L levels
per symbol and far levels outside it, FIFO chunks of 16 slots drawn from a shuffled pool (chunks emptied by
cancels unlinked), a seq ring with a horizon above a few live orders and an old-order table holding those (among
entries of a stale epoch), a free list, an fcache row, an unconsumed reclamation list, one far side moved into
the active half of the arena. `corrupt` changes one field of a copy: of such an image on the CPU
(tests/test_book_audit_model.py), of a real export on the GPU (tests/test_book_audit_gpu.py).
"""
import numpy as np

from matching_engine_amd import _abi
from tests import book_audit as ba
from tests.book_audit import C, NIL, copy_raw


def _nextpow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def build_image(model, L, base0, last_seq, *, ring=1 << 14, fcap=8, half=512, old_n=256, n_old=6, spare=16, seed=0):
    """The canonical raw image of `model` (a PyBook-shaped book): what Engine.debug_export() returns."""
    rng = np.random.default_rng(seed)
    S = model.S
    sides = []
    need = 0
    for s in range(S):
        bids = [(-k, [list(e) for e in f]) for k, f in model.side[s][0].levels.items()]  # best (highest) first
        asks = [(k, [list(e) for e in f]) for k, f in model.side[s][1].levels.items()]   # best (lowest) first
        sides.append((bids, asks))
        need += sum((len(f) + C - 1) // C for _, f in bids + asks)
    hwm = need + spare
    NC = hwm + 32
    ids = list(rng.permutation(hwm))
    W = L // 64
    inl = 2 * S * fcap
    raw = {
        "levels": np.zeros((S, L), dtype=_abi.DBG_LEVEL_DTYPE),
        "occ": np.zeros((S, W), dtype="<u8"),
        "tend": np.zeros((S, L), dtype="u1"),
        "sym": np.zeros(S, dtype=_abi.DBG_SYM_DTYPE),
        "chunks": np.zeros(NC, dtype=_abi.DBG_CHUNK_DTYPE),
        "fcache": np.full((S, 64), NIL, dtype="<u4"),
        "loc": np.full(ring, NIL, dtype="<u4"),
        "old": np.zeros(old_n, dtype=_abi.DBG_OLD_DTYPE),
        "sq": np.zeros(2, dtype=_abi.DBG_SQ_DTYPE),
        "far": np.zeros(inl + 2 * half, dtype=_abi.DBG_FAR_DTYPE),
        "fdir": np.zeros((S, 2), dtype=_abi.DBG_FDIR_DTYPE),
        "far_ctl": np.zeros(4, dtype="<u8"),
        "chunk_top": np.zeros(1, dtype="<u4"),
        "recl": np.zeros(NC, dtype="<u4"),
        "cpool": np.zeros(4, dtype="<u4"),
        "stats": np.zeros(8, dtype="<u8"),
        "err": np.zeros(1, dtype="<u4"),
    }
    raw["levels"]["head"] = NIL
    raw["levels"]["tail"] = NIL
    raw["chunks"]["next"] = NIL
    raw["chunks"]["prev"] = NIL
    ch_ = raw["chunks"]
    freed, live = [], []  # chunk ids emptied by cancels; (seq, slot id) of every live order

    def lay(s, price, fifo):
        """(total, head, tail, tend) of one level's chain."""
        groups = [fifo[i:i + C] for i in range(0, len(fifo), C)]
        got = [ids.pop() for _ in groups]
        keep = [(g, c) for g, c in zip(groups, got) if any(e[1] > 0 for e in g)]
        freed.extend(c for g, c in zip(groups, got) if not any(e[1] > 0 for e in g))
        assert keep
        for j, (g, c) in enumerate(keep):
            ch_[c]["next"] = keep[j + 1][1] if j + 1 < len(keep) else NIL
            ch_[c]["prev"] = keep[j - 1][1] if j else NIL
            ch_[c]["price"], ch_[c]["owner"] = price, s
            for i, e in enumerate(g):
                ch_[c]["seq"][i], ch_[c]["qty"][i] = e[0], e[1]
                if e[1] > 0:
                    live.append((e[0], int(c) * C + i))
        tend = len(groups[-1]) if keep[-1][1] == got[-1] else C
        return sum(e[1] for e in fifo), int(keep[0][1]), int(keep[-1][1]), tend

    far_sides = {}
    for s, (bids, asks) in enumerate(sides):
        base = int(base0[s])
        if bids:
            base = max(base, bids[0][0] - L + 1)
        if asks:
            base = min(base, asks[0][0])
        sym = raw["sym"][s]
        sym["base"], sym["best_bid"], sym["best_ask"], sym["free_head"] = base, -1, L, NIL
        n = 0
        for k, side in enumerate((bids, asks)):
            far = []
            for price, fifo in side:
                if not any(e[1] > 0 for e in fifo):
                    continue
                t, h, tl, te = lay(s, price, fifo)
                n += sum(1 for e in fifo if e[1] > 0)
                l = price - base
                if 0 <= l < L:
                    raw["levels"][s, l] = (t, h, tl)
                    raw["tend"][s, l] = te
                    raw["occ"][s, l >> 6] |= np.uint64(1 << (l & 63))
                    if k == 0:
                        sym["best_bid"] = max(int(sym["best_bid"]), l)
                    else:
                        sym["best_ask"] = min(int(sym["best_ask"]), l)
                else:
                    assert (price < base) == (k == 0)
                    far.append((price, t, h, tl, te, 0))
            far_sides[(s, k)] = far[::-1]  # the best level last
            sym["nfar"][k] = len(far)
        sym["resting"] = n
    # far regions: a side that outgrew its inline region, and the largest side, live in the active half (1)
    moved = {max(far_sides, key=lambda sk: len(far_sides[sk]))} | {sk for sk, f in far_sides.items() if len(f) > fcap}
    top = 0
    for (s, k), f in far_sides.items():
        off, cap = (2 * s + k) * fcap, fcap
        if (s, k) in moved:
            cap = max(2 * fcap, _nextpow2(len(f)))
            off, top = inl + half + top, top + cap
        raw["fdir"][s, k] = (off, cap, 0)
        if f:
            raw["far"][off:off + len(f)] = np.array(f, dtype=_abi.DBG_FAR_DTYPE)
    assert top <= half
    raw["far_ctl"][:3] = (0, top, 1)
    # free chunks: a free list (symbol 0), an fcache row (symbol 1), the unconsumed part of the reclamation's list;
    # two stay in no place at all (a reclamation would find them)
    free = freed + [int(c) for c in ids[2:]]
    assert len(free) >= 12
    fl, fc, rl = free[:4], free[4:8], free[8:]
    for a, b in zip(fl, fl[1:] + [NIL]):
        ch_[a]["next"] = b
    raw["sym"][0]["free_head"] = fl[0]
    raw["fcache"][1, :len(fc)] = fc
    raw["sym"][1]["nfree"] = len(fc)
    consumed = 3
    used = [g // C for _, g in live[:consumed]]
    raw["recl"][:len(used)] = used
    raw["recl"][consumed:consumed + len(rl)] = rl
    raw["chunk_top"][0] = consumed
    raw["cpool"][:2] = (consumed + len(rl), hwm)
    for c in free:
        ch_[c]["qty"] = 0
    # the seq ring and the old-order table
    live.sort()
    horizon = live[min(n_old, len(live) - 1)][0] if live else 1
    epoch = 3
    raw["sq"][0] = (1, max(horizon - 1, 0), epoch - 1, (0, 0, 0))
    raw["sq"][1] = (horizon, last_seq, epoch, (0, 0, 0))
    stale = rng.integers(0, old_n, old_n // 4)
    raw["old"]["epoch"][stale] = epoch - 1
    raw["old"]["seq"][stale] = rng.integers(1, 1 << 20, len(stale))
    for q, g in live:
        if q >= horizon:
            assert raw["loc"][q & (ring - 1)] == NIL, "ring too small for the stream"
            raw["loc"][q & (ring - 1)] = g
        else:
            h = ba.old_hash(q) & (old_n - 1)
            while raw["old"][h]["epoch"] == epoch:
                h = (h + 1) & (old_n - 1)
            raw["old"][h] = (epoch, g, q)
            raw["loc"][q & (ring - 1)] = g ^ 1  # (overwritten since: nobody reads the ring below the horizon)
    raw["stats"][_abi.DBG_ST_RESTING] = int(raw["sym"]["resting"].sum())
    raw["info"] = dict(num_symbols=S, levels=L, level_words=W, nchunks=NC, ring_mask=ring - 1, old_mask=old_n - 1,
                       far_levels=fcap, far_half=half, far_inline=inl, far_entries=inl + 2 * half, sq_idx=1,
                       chunk_slots=C, fcache_row=64, n_far_ctl=4, n_cpool=4, n_stats=8)
    return raw


# ---- single-field corruptions -----------------------------------------------------------------------------------
# Each finds its own target in the image (so the GPU suite can apply them to real exports) and changes one field
# of the host copy. `Targets` gathers the targets once.

class Targets:
    def __init__(self, raw):
        self.raw = raw
        lv = raw["levels"]
        self.occ = [(int(s), int(l)) for s, l in zip(*np.nonzero(lv["total"] > 0))]
        self.multi = [(s, l) for s, l in self.occ if lv[s, l]["head"] != lv[s, l]["tail"]]
        self.empty = [(int(s), int(l)) for s, l in zip(*np.nonzero(lv["total"] == 0))]
        self.far = [(s, k) for s in range(len(raw["sym"])) for k in range(2) if raw["sym"][s]["nfar"][k] > 0]

    def level(self, multi=False):
        return (self.multi if multi else self.occ)[0]

    def head(self, multi=False):
        s, l = self.level(multi)
        return int(self.raw["levels"][s, l]["head"])

    def live_slot(self, two=False):
        """(chunk, slot) of a live order on a window level (two: in a chunk with >= 2 live orders)."""
        q = self.raw["chunks"]["qty"]
        for s, l in self.occ:
            c = int(self.raw["levels"][s, l]["head"])
            lv = np.nonzero(q[c] > 0)[0]
            if len(lv) >= (2 if two else 1):
                return s, l, c, [int(i) for i in lv]
        raise LookupError

    def far_entry(self, k=None, n=1):
        for s, kk in self.far:
            if (k is None or kk == k) and self.raw["sym"][s]["nfar"][kk] >= n:
                return s, kk, int(self.raw["fdir"][s, kk]["off"]), int(self.raw["sym"][s]["nfar"][kk])
        raise LookupError

    def both_sides(self, gap=1):
        for s, y in enumerate(self.raw["sym"]):
            if y["best_bid"] >= 1 and y["best_ask"] < self.raw["info"]["levels"] and y["best_ask"] - y["best_bid"] > gap:
                return s
        raise LookupError


def _total(d):
    def f(raw, t):
        s, l = t.level()
        raw["levels"][s, l]["total"] += d
    return f


def _zero_live_slot(raw, t):
    _, _, c, lv = t.live_slot(two=True)
    raw["chunks"][c]["qty"][lv[0]] = 0


def _negative_total(raw, t):
    s, l = t.empty[0]
    raw["levels"][s, l]["total"] = -5


def _head_of_empty(raw, t):
    s, l = t.empty[0]
    raw["levels"][s, l]["head"] = t.head()


def _chunk_field(field, value, multi=False, second=False):
    def f(raw, t):
        c = t.head(multi)
        if second:
            c = int(raw["chunks"][c]["next"])
        raw["chunks"][c][field] = value(raw, c) if callable(value) else value
    return f


def _negative_qty(raw, t):
    _, _, c, lv = t.live_slot()
    raw["chunks"][c]["qty"][lv[0]] *= -1


def _empty_chunk_linked(raw, t):
    s, l = t.level(multi=True)
    c = t.head(multi=True)
    raw["levels"][s, l]["total"] -= int(raw["chunks"][c]["qty"].sum())
    raw["chunks"][c]["qty"] = 0


def _swap_seqs(raw, t):
    _, _, c, lv = t.live_slot(two=True)
    sq = raw["chunks"][c]["seq"]
    sq[lv[0]], sq[lv[1]] = sq[lv[1]], sq[lv[0]]


def _tend(value):
    def f(raw, t):
        s, l = t.level()
        raw["tend"][s, l] = value
    return f


def _tend_short(raw, t):
    for s, l in t.occ:
        te, tl = int(raw["tend"][s, l]), int(raw["levels"][s, l]["tail"])
        if te >= 2 and raw["chunks"][tl]["qty"][te - 1] > 0:
            raw["tend"][s, l] = te - 1
            return
    raise LookupError


def _bid_above_ask(raw, t):
    s = t.both_sides()
    raw["sym"][s]["best_bid"] = raw["sym"][s]["best_ask"]


def _hint(field, d, gap=1):
    def f(raw, t):
        raw["sym"][t.both_sides(gap)][field] += d
    return f


def _occ_flip(raw, t):
    s, l = t.level()
    raw["occ"][s, l >> 6] ^= np.uint64(1 << (l & 63))


def _occ_stray(raw, t):
    s, l = t.empty[0]
    raw["occ"][s, l >> 6] |= np.uint64(1 << (l & 63))


def _nfar_over_cap(raw, t):
    s, k, _, n = t.far_entry()
    raw["fdir"][s, k]["cap"] = n - 1


def _region_outside(raw, t):
    s, k, _, _ = t.far_entry()
    raw["fdir"][s, k]["off"] = raw["info"]["far_entries"] - 1


def _region_inactive_half(raw, t):
    s, k, _, _ = t.far_entry()
    act = int(raw["far_ctl"][2]) & 1
    raw["fdir"][s, k]["off"] = raw["info"]["far_inline"] + (act ^ 1) * raw["info"]["far_half"]


def _regions_overlap(raw, t):
    f = raw["fdir"]
    f[1, 0]["off"] = f[0, 1]["off"] + 1 if f[0, 1]["off"] != f[1, 0]["off"] + 1 else f[0, 1]["off"]


def _far_swap(raw, t):
    _, _, off, n = t.far_entry(n=2)
    raw["far"][[off + n - 2, off + n - 1]] = raw["far"][[off + n - 1, off + n - 2]]


def _far_bid_in_window(raw, t):
    s, _, off, n = t.far_entry(k=0)
    e = raw["far"][off + n - 1]  # the best far bid: still the highest, so the order holds
    e["price"] = raw["sym"][s]["base"]
    c = int(e["head"])
    while c != NIL:
        raw["chunks"][c]["price"] = e["price"]
        c = int(raw["chunks"][c]["next"])


def _far_total_zero(raw, t):
    _, _, off, _ = t.far_entry()
    raw["far"][off]["total"] = 0


def _resting(d):
    def f(raw, t):
        y = raw["sym"][t.level()[0]]
        y["resting"] = int(y["resting"]) + d
    return f


def _st_resting(raw, t):
    raw["stats"][_abi.DBG_ST_RESTING] -= 1


def _all_chunks_dead(raw, t):
    s = t.level()[0]
    mine = (raw["chunks"]["owner"] == s) & (raw["chunks"]["qty"] > 0).any(axis=1)
    raw["chunks"]["qty"][mine] = 0


def _fcache_push(pick):
    def f(raw, t):
        s = int(np.argmin(raw["sym"]["nfree"]))
        n = int(raw["sym"][s]["nfree"])
        raw["fcache"][s, n] = pick(raw, t)
        raw["sym"][s]["nfree"] = n + 1
    return f


def _free_chunk(raw):
    """A chunk on some free list or fcache row, or the first unconsumed one of the reclamation's list."""
    s = np.nonzero(raw["sym"]["nfree"] > 0)[0]
    if len(s):
        return int(raw["fcache"][s[0], 0])
    s = np.nonzero(raw["sym"]["free_head"] != NIL)[0]
    if len(s):
        return int(raw["sym"][s[0]]["free_head"])
    if raw["chunk_top"][0] < raw["cpool"][0]:
        return int(raw["recl"][raw["chunk_top"][0]])
    raise LookupError


def _free_list_cycle(raw, t):
    s = int(np.nonzero(raw["sym"]["free_head"] != NIL)[0][0])
    c = int(raw["sym"][s]["free_head"])
    raw["chunks"][c]["next"] = c


def _unlinked_live(raw, t):
    raw["chunks"][raw["info"]["nchunks"] - 1]["qty"][3] = 7


def _free_nonzero(raw, t):
    raw["chunks"][_free_chunk(raw)]["qty"][5] = 2


def _ring_order(raw):
    """(seq, slot id, ring index) of a live order at or above the horizon."""
    hz = int(raw["sq"][raw["info"]["sq_idx"]]["horizon"])
    q, sq = raw["chunks"]["qty"], raw["chunks"]["seq"]
    c, i = np.nonzero((q > 0) & (sq >= hz))
    return int(sq[c[0], i[0]]), int(c[0]) * C + int(i[0]), int(sq[c[0], i[0]]) & raw["info"]["ring_mask"]


def _loc_other_slot(raw, t):
    _, g, r = _ring_order(raw)
    assert raw["loc"][r] == g
    raw["loc"][r] = g ^ 1


def _old_entry(raw):
    sqs = raw["sq"][raw["info"]["sq_idx"]]
    q, sq = raw["chunks"]["qty"], raw["chunks"]["seq"]
    for h, e in enumerate(raw["old"]):
        if e["epoch"] == sqs["epoch"] and e["seq"] < sqs["horizon"] and e["slot"] // C < len(q) and \
                q[e["slot"] // C, e["slot"] % C] > 0 and sq[e["slot"] // C, e["slot"] % C] == e["seq"]:
            return h
    raise LookupError


def _old_missing(raw, t):
    raw["old"][_old_entry(raw)]["seq"] += 1 << 50


def _old_stale_epoch(raw, t):
    raw["old"][_old_entry(raw)]["epoch"] -= 1


def _old_wrong_slot(raw, t):
    raw["old"][_old_entry(raw)]["slot"] ^= 1


def _last_seq(raw, t):
    raw["sq"][raw["info"]["sq_idx"]]["last"] = 1


def _err(raw, t):
    raw["err"][0] = 4


NC_OF = lambda raw, c: raw["info"]["nchunks"] + 5  # noqa: E731
CORRUPTIONS = {
    # name: (the invariant that must report it, the change)
    "total + 1": ("chain.sum_total", _total(+1)),
    "total - 1": ("chain.sum_total", _total(-1)),
    "a live slot zeroed without the total": ("chain.sum_total", _zero_live_slot),
    "a negative total": ("level.total_nonneg", _negative_total),
    "head of an empty level not NIL": ("level.empty_iff_nil", _head_of_empty),
    "tail of an occupied level NIL": ("level.empty_iff_nil", lambda raw, t: raw["levels"][t.level()].__setitem__("tail", NIL)),
    "prev broken": ("chain.prev", _chunk_field("prev", NIL, multi=True, second=True)),
    "prev of the head not NIL": ("chain.prev", _chunk_field("prev", 0)),
    "a cycle": ("chain.cycle", _chunk_field("next", lambda raw, c: c, multi=True)),
    "next out of range": ("chain.id_range", _chunk_field("next", NC_OF, multi=True)),
    "the chain stops before the tail": ("chain.ends_at_tail", _chunk_field("next", NIL, multi=True)),
    "a chunk's price off by one": ("chain.price", _chunk_field("price", lambda raw, c: raw["chunks"][c]["price"] + 1)),
    "owner changed": ("chain.owner", _chunk_field("owner", lambda raw, c: raw["chunks"][c]["owner"] ^ 1)),
    "a negative quantity": ("chain.negative_qty", _negative_qty),
    "an all-zero chunk left linked": ("chain.empty_chunk_linked", _empty_chunk_linked),
    "two seqs of a FIFO swapped": ("chain.fifo_seq_order", _swap_seqs),
    "tend 0 on an occupied level": ("tend.range", _tend(0)),
    "tend 17": ("tend.range", _tend(17)),
    "tend one short of a live slot": ("tend.covers_live", _tend_short),
    "a bid above an ask": ("sides.bid_below_ask", _bid_above_ask),
    "best_bid one worse": ("sides.level_between", _hint("best_bid", -1)),
    "best_ask one worse": ("sides.level_between", _hint("best_ask", +1)),
    "best_bid on an empty level": ("sides.hint_exact", _hint("best_bid", +1, gap=2)),
    "occ bit of an occupied level cleared": ("occ.bit_matches_total", _occ_flip),
    "occ bit of an empty level set": ("occ.bit_matches_total", _occ_stray),
    "nfar > cap": ("far.count_le_cap", _nfar_over_cap),
    "a region past the arena": ("far.region_in_arena", _region_outside),
    "a region in the inactive half": ("far.region_placement", _region_inactive_half),
    "two fdir regions overlapping": ("far.regions_disjoint", _regions_overlap),
    "far prices swapped": ("far.price_order", _far_swap),
    "a far bid inside the window": ("far.invariant_I", _far_bid_in_window),
    "a far entry with total 0": ("far.total_positive", _far_total_zero),
    "resting + 1": ("counts.sym_resting", _resting(+1)),
    "resting - 1": ("counts.sym_resting", _resting(-1)),
    "ST_RESTING - 1": ("counts.st_resting", _st_resting),
    "every chunk of a symbol emptied": ("counts.chunks_le_orders", _all_chunks_dead),
    "a linked chunk also in an fcache row": ("partition.chunk_in_two_places", _fcache_push(lambda raw, t: t.head())),
    "the same chunk in two free places": ("partition.chunk_in_two_places", _fcache_push(lambda raw, t: _free_chunk(raw))),
    "a free list that loops": ("partition.free_list", _free_list_cycle),
    "nfree 65": ("partition.free_list", lambda raw, t: raw["sym"][0].__setitem__("nfree", 65)),
    "a quantity in a chunk no chain holds": ("partition.live_chunk_unlinked", _unlinked_live),
    "a quantity in a parked chunk": ("partition.free_chunk_nonzero", _free_nonzero),
    "a parked chunk the pool never handed out": ("partition.beyond_high_water",
                                                 _fcache_push(lambda raw, t: raw["info"]["nchunks"] - 2)),
    "a loc entry pointing at another slot": ("lookup.ring", _loc_other_slot),
    "an old order missing from old": ("lookup.old_table", _old_missing),
    "an old entry of a stale epoch": ("lookup.old_table", _old_stale_epoch),
    "an old entry naming another slot": ("lookup.old_table", _old_wrong_slot),
    "sq.last behind the stream": ("lookup.last_seq", _last_seq),
    "err set": ("err.zero", _err),
}


def corrupt(raw, name):
    """A corrupted deep copy of `raw` and the invariant that must report it."""
    inv, fn = CORRUPTIONS[name]
    bad = copy_raw(raw)
    fn(bad, Targets(bad))
    return bad, inv
