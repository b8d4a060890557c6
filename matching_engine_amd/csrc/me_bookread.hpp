// me_bookread.hpp — how the kernels of me_snapshot.hip read a resting book between launches (device only).
//
// A side's levels in priority order are its WINDOW levels outward from the best-level hint (a bound, DESIGN.md
// §4: asks ascend, bids descend), then its FAR levels from the end of their array (the best is last, me_far.hpp;
// by Invariant I a window level always beats a far level). Four rules hold for every reader:
//   the total decides   a level counts when its total is > 0: an occupancy bit over a total <= 0 and a dead far
//                       entry are stepped over;
//   window before far   far levels follow only once the window is exhausted;
//   the best far is last
//   checked before use  a side's FarDir region {off, cap} is checked against the arena before it is dereferenced
//                       (far_side), a chunk id against nchunks, and a chain walk ends after nchunks steps.
//
// walk_window is the wave-level window walk: 64 gate words a round, the blocks of 64 levels under non-zero
// words one after the other, lane order = priority order. A deep window's gate words are its occupancy words,
// 64 words = 4,096 levels per load, so that only blocks with a set bit are visited and only the totals under
// set bits are loaded; a window of L <= 128 has all-ones gate words (two blocks at most, every total loaded).
// walk_far is the same for the far levels: 64 entries a block from the end, lane order = priority order.
// The block-level kernels (k_book_snapshot, k_purge) gather a pass of levels with the whole workgroup instead
// and share what follows the gather: far_nth, chain_live and chunk_entries.
#pragma once
#include "me_layout.hpp"
#include "me_wave.hpp"

namespace me {

// The bits of occupancy word wi that are levels of [lo, hi] (lo <= hi).
__device__ __forceinline__ unsigned long long word_range(int wi, int lo, int hi) {
  unsigned long long m = ~0ull;
  if (wi == (lo >> 6)) m &= ~0ull << (lo & 63);
  if (wi == (hi >> 6)) m &= ~0ull >> (63 - (hi & 63));
  return m;
}

// Window levels from .. to of symbol s, both inside [0, L), `from` the end nearer the best (asks: from <= to,
// bids: from >= to; the other way round: no level). f(l, gate) gets every block of 64 levels whose gate word
// is non-zero: this lane's level index and whether its gate bit is set (clear: not a level of the walk, nothing
// to load). A word's bids go from its top bit down, so lane order is priority order on both sides. f returns
// true to end the walk, and so does walk_window then. Wave-uniform control flow, no LDS.
template <class F>
__device__ __forceinline__ bool walk_window(const BookDev& bk, uint32_t s, bool bid, int from, int to, F&& f) {
  const int lane = lane_id();
  const int lo = bid ? to : from, hi = bid ? from : to;
  if (lo > hi) return false;
  const unsigned long long* oc = bk.occ + (size_t)s * bk.Lwords;
  const bool deep = bk.L > 128u;
  const int wlo = lo >> 6, whi = hi >> 6;
  const int bit = bid ? 63 - lane : lane;
  for (int w0 = bid ? whi : wlo; bid ? w0 >= wlo : w0 <= whi; w0 += bid ? -64 : 64) {
    const int wi = bid ? w0 - lane : w0 + lane;
    unsigned long long word = 0ull;
    if (wi >= wlo && wi <= whi) word = (deep ? oc[wi] : ~0ull) & word_range(wi, lo, hi);
    for (unsigned long long nz = __ballot(word != 0ull); nz; nz &= nz - 1ull) {
      const int j = __builtin_ctzll(nz);
      const unsigned long long g = rl64(word, j);
      if (f((bid ? w0 - j : w0 + j) * 64 + bit, ((g >> bit) & 1ull) != 0ull)) return true;
    }
  }
  return false;
}

// A side's far levels: lv[0, n), the best last. n = min(the symbol's count hint, the region's capacity).
struct FarSide {
  gptr<FarLevel> lv;
  uint32_t n;
};
// Side k of symbol s (s < S), `hint` the symbol's count of its levels. False: the region does not lie inside
// the arena (a corrupt FarDir); fs is empty then. Branch-free (a caller that can skip the 16-B FarDir load for
// a hint of 0 does so itself).
__device__ __forceinline__ bool far_side(const BookDev& bk, uint32_t s, uint32_t k, uint32_t hint, FarSide& fs) {
  const FarDir fd = bk.fdir[(size_t)s * 2u + k];
  const uint32_t n = min(hint, fd.cap);
  const unsigned long long end = far_arena_entries(bk);
  const bool ok = fd.off <= end && n <= end - fd.off;
  fs.lv = (gptr<FarLevel>)(bk.far + fd.off);  // (never dereferenced when n == 0)
  fs.n = ok ? n : 0u;
  return ok;
}
// Entry i counted from the best (i < fs.n).
__device__ __forceinline__ FarLevel far_nth(const FarSide& fs, uint32_t i) { return fs.lv[fs.n - 1u - i]; }

// The `count` best entries of fs (count <= fs.n), best first, 64 a block: f(e) gets this lane's entry (all
// zero: none, the total decides anyway) and returns true to end the walk. Wave-uniform control flow.
template <class F>
__device__ __forceinline__ bool walk_far(const FarSide& fs, uint32_t count, F&& f) {
  const uint32_t lane = (uint32_t)lane_id();
  for (uint32_t i0 = 0; i0 < count; i0 += 64u) {
    FarLevel e{};
    if (i0 + lane < count) e = far_nth(fs, i0 + lane);
    if (f(e)) return true;
  }
  return false;
}

// Live slots of the chain head .. tail (one thread; head NIL: none), four int4 loads a chunk. False: the chain
// is broken — it leaves [0, nchunks), ends before its tail or takes more than nchunks steps; c then holds the
// count up to the break. (One exit: a return from inside the loop costs the callers some 40 SGPR spills.)
__device__ __forceinline__ bool chain_live(const BookDev& bk, uint32_t head, uint32_t tail, uint32_t& c) {
  c = 0;
  bool ok = true;
  uint32_t ch = head, guard = 0;
  while (ch != NIL) {
    if (ch >= bk.nchunks || ++guard > bk.nchunks) {
      ok = false;
      break;
    }
    const int4* qv = reinterpret_cast<const int4*>(bk.chunks[ch].qty);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int4 v = qv[u];
      c += (v.x > 0) + (v.y > 0) + (v.z > 0) + (v.w > 0);
    }
    if (ch == tail) break;
    ch = bk.chunks[ch].hdr.next;
    ok = ch != NIL;
  }
  return ok;
}

// The live slots of chunk c, in slot order, as entries out[o ..]; an entry at or past cap is counted, not
// written. Returns o behind them.
__device__ __forceinline__ unsigned long long chunk_entries(const Chunk& c, long long price, bool bid, me_book_entry* out,
                                                            unsigned long long o, unsigned long long cap) {
  for (int u = 0; u < ME_C; ++u) {
    const int qq = c.qty[u];
    if (qq <= 0) continue;
    if (o < cap) {
      me_book_entry e;
      e.seq = c.seq[u];
      e.price_q4 = price;
      e.qty = qq;
      e.side = bid ? ME_SIDE_BUY : ME_SIDE_SELL;
      e.pad[0] = e.pad[1] = e.pad[2] = 0;
      out[o] = e;
    }
    ++o;
  }
  return o;
}

}  // namespace me
