"""One book for every reader of the resting book — TEST INFRASTRUCTURE ONLY.

The snapshot, the depth feed, the order query, the preview and the mass cancel all walk a side's window levels
outward from the best and then its far levels from the best end (matching_engine_amd/csrc/me_bookread.hpp).
`scenario(L)` builds the book whose levels sit where such a walk can go wrong: on both sides of 64-level block
boundaries, at the first and last bit of occupancy words, on both sides of the 64-word (4,096-level) boundary of
a load of occupancy words, near both window edges, and on more far levels than one 64-entry block holds.

  symbol 0   one bid at level 1 (it keeps the window where it is), asks at ASK_LEVELS clipped to [2, L - 3],
             70 far ask levels at base + L - 1 + 10 (k + 1)
  symbol 1   the mirror image: one ask at level L - 2, bids at L - 1 - l, 70 far bid levels at base - 10 (k + 1)
  symbol 2   both sides sparse, 70 far bid levels and 5 far ask levels; the second batch cancels a window ask
             level and two far bid levels (in different 64-entry blocks) that lie between live ones
  symbol 3   empty

tests/test_book_readers_model.py checks against the CPU oracle that the orders rest where this says;
tests/test_book_readers_gpu.py runs every reader over the book.
"""
from __future__ import annotations

from tests import tif_model as tm
from tests.big_qty import Script

BUY, SELL = 1, 2
S = 4
LS = (128, 1024, 8192)  # 8192 levels = 128 occupancy words: a walk takes two 64-word loads
NFAR = 70
ASK_LEVELS = (2, 3, 62, 63, 64, 65, 127, 128, 4094, 4095, 4096, 4097)


def ask_levels(L):
    return [l for l in sorted(set(ASK_LEVELS) | {L - 65, L - 64, L - 3}) if 2 <= l <= L - 3]


class Scenario:
    """batches: the records (tif_model.Arrays); window[(symbol, side)] / far[(symbol, side)]: the prices that
    hold live orders behind the LAST batch, best first; cancelled: [(symbol, side, price)] emptied by the
    second batch; seqs: every seq used."""


def scenario(L):
    sn = Scenario()
    sn.L, sn.S = L, S
    sn.base = tm.base_prices(S, L)
    b = [int(x) for x in sn.base]
    sn.window = {(s, side): [] for s in range(S) for side in (BUY, SELL)}
    sn.far = {(s, side): [] for s in range(S) for side in (BUY, SELL)}
    sc = Script()

    def rest(s, side, px, q, n=1):
        inside = b[s] <= px < b[s] + L
        (sn.window if inside else sn.far)[(s, side)].append(px)
        return [sc.new(s, side, px, q + j) for j in range(n)]

    lv = ask_levels(L)
    rest(0, BUY, b[0] + 1, 2)
    rest(1, SELL, b[1] + L - 2, 2)
    for i, l in enumerate(lv):  # (two orders on every third level: FIFOs longer than one)
        rest(0, SELL, b[0] + l, 3 + i, 2 if i % 3 == 0 else 1)
        rest(1, BUY, b[1] + L - 1 - l, 4 + i, 2 if i % 3 == 0 else 1)
    for k in range(NFAR):
        rest(0, SELL, b[0] + L - 1 + 10 * (k + 1), 1 + k % 7)
        rest(1, BUY, b[1] - 10 * (k + 1), 2 + k % 5)
    # symbol 2: sparse on both sides
    for l in (2, 33, L // 4 - 1, L // 4, L // 2 - 10):
        rest(2, BUY, b[2] + l, 5 + l % 3, 2 if l == L // 4 else 1)
    gone_ask = rest(2, SELL, b[2] + L // 2 + 20, 9, 2)
    for l in (L // 2 + 10, 3 * L // 4 - 1, 3 * L // 4, L - 3):
        rest(2, SELL, b[2] + l, 6 + l % 4)
    fb2 = [rest(2, BUY, b[2] - 10 * (k + 1), 1 + k % 4)[0] for k in range(NFAR)]
    for k in range(5):
        rest(2, SELL, b[2] + L - 1 + 7 * (k + 1), 3 + k)
    b0 = sc.take()
    sn.cancelled = [(2, SELL, b[2] + L // 2 + 20), (2, BUY, b[2] - 10 * 2), (2, BUY, b[2] - 10 * 67)]
    for t in gone_ask + [fb2[1], fb2[66]]:
        sc.cancel(2, t)
    b1 = sc.take()
    for s, side, px in sn.cancelled:
        (sn.window if b[s] <= px < b[s] + L else sn.far)[(s, side)].remove(px)
    for key in list(sn.window):  # best first
        sn.window[key].sort(reverse=key[1] == BUY)
        sn.far[key].sort(reverse=key[1] == BUY)
    sn.batches = [b0, b1]
    sn.seqs = list(range(1, sc.next))
    return sn
