// me_snapshot.hip — device book snapshots (GetOrderBook, src/server/matching_engine_service.cpp:123-129;
// OrderBookResponse = repeated Order, proto/matching_engine.proto:16-23,57-60).
//
// k_book_snapshot: one 1024-thread workgroup per (symbol, side) of the request. It walks the side's
// price levels best first — the window from the best level outward, then the far levels (best last
// in their array) — and, for the first `depth` non-empty ones, writes each level's aggregate
// (price, total, order count) and every resting order of its FIFO (seq, price, qty, side) in
// priority order. Levels are taken in passes of up to SNAP_P: the pass's levels are found by a
// block-wide compaction of the window's totals, every thread then walks ONE level's chunk chain to
// count its live slots, a block scan turns the counts into output offsets, and a second walk writes
// the orders. Chains are short (a chunk holds 16 slots), so a pass costs a few chunk-load latencies
// however deep the book is: a 10,000-level side is five passes of one launch.
//
// Bytes per resting order: one 256-B chunk read per 16 orders (twice: count + write) + 24 B out;
// per level 16 B (window) or 32 B (far) read + 24 B out. HBM-bound in principle, latency-bound in
// practice (dependent chunk loads).
//
// The rules every reader kernel of this file follows, and the walks they share, are in me_bookread.hpp.
#include <hip/hip_runtime.h>

#include "me_bookread.hpp"
#include "me_far.hpp"
#include "me_launch.hpp"
#include "me_layout.hpp"
#include "me_wave.hpp"

namespace me {

constexpr int SNAP_T = 1024;  // threads per workgroup
constexpr int SNAP_P = 2048;  // levels per pass (LDS: 24 B each + counts)


__device__ __forceinline__ uint32_t snap_block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t incl = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  uint32_t before = 0, tot = 0;
  for (int k = 0; k < SNAP_T / 64; ++k) {
    const uint32_t x = wsum[k];
    if (k < w) before += x;
    tot += x;
  }
  __syncthreads();
  total = tot;
  return before + incl - v;
}

__global__ __launch_bounds__(SNAP_T) void k_book_snapshot(BookDev bk, SnapReq rq) {
  __shared__ long long p_price[SNAP_P];
  __shared__ long long p_total[SNAP_P];
  __shared__ uint32_t p_head[SNAP_P];
  __shared__ uint32_t p_tail[SNAP_P];
  __shared__ uint32_t p_off[SNAP_P];
  __shared__ uint32_t wsum[SNAP_T / 64];
  __shared__ int s_cur;          // window cursor (next level to look at)
  __shared__ uint32_t s_far;     // far levels taken so far
  __shared__ uint32_t s_np;      // levels in this pass
  const int tid = threadIdx.x;
  const uint32_t q = blockIdx.x >> 1, side = blockIdx.x & 1u;
  const uint32_t s = rq.sym[q];
  const int L = (int)bk.L;
  const SymState st = bk.sym[s];
  const Level* lv = bk.levels + (size_t)s * L;
  FarSide fs;
  if (!far_side(bk, s, side, st.nfar[side], fs) && tid == 0) atomicOr(rq.err, 1u);  // (no far levels then)
  const size_t reg = (size_t)q * 2 + side;
  me_level* lv_out = rq.lv + reg * rq.depth;
  me_book_entry* ord_out = rq.ord ? rq.ord + reg * rq.ocap : nullptr;
  if (tid == 0) {
    s_cur = side == 0 ? min(st.best_bid, L - 1) : max(st.best_ask, 0);
    s_far = 0;
  }
  __syncthreads();
  uint32_t found = 0;
  unsigned long long norders = 0;
  while (found < rq.depth) {
    const uint32_t want = min((uint32_t)SNAP_P, rq.depth - found);
    if (tid == 0) s_np = 0;
    __syncthreads();
    // ---- this pass's levels: window levels in scan order, then far levels
    for (;;) {
      const int cur = s_cur;
      const uint32_t np = s_np;
      const bool win_left = side == 0 ? cur >= 0 : cur < L;
      if (np >= want || !win_left) break;
      const int l = side == 0 ? cur - tid : cur + tid;
      const bool inwin = side == 0 ? l >= 0 : l < L;
      const long long tot = inwin ? lv[l].total : 0;
      const uint32_t nz = tot > 0;
      uint32_t all = 0;
      const uint32_t pos = snap_block_excl_scan(nz, wsum, all);
      if (nz && np + pos < want) {
        const Level x = lv[l];
        p_price[np + pos] = st.base + l;
        p_total[np + pos] = x.total;
        p_head[np + pos] = x.head;
        p_tail[np + pos] = x.tail;
      }
      // the cursor moves past the last level taken (or the whole block when it all fits)
      __syncthreads();
      if (tid == 0) {
        const uint32_t take = min(all, want - np);
        s_np = np + take;
      }
      if (nz && np + pos + 1 == want) s_cur = side == 0 ? l - 1 : l + 1;  // the pass filled at l
      __syncthreads();
      if (tid == 0 && s_np < want) s_cur = side == 0 ? cur - SNAP_T : cur + SNAP_T;
      __syncthreads();
    }
    {
      const uint32_t np = s_np;
      const uint32_t fr = s_far;
      const uint32_t nf = min(want - np, fs.n - fr);
      for (uint32_t j = tid; j < nf; j += SNAP_T) {
        const FarLevel f = far_nth(fs, fr + j);
        p_price[np + j] = f.price;
        p_total[np + j] = f.total;
        p_head[np + j] = f.head;
        p_tail[np + j] = f.tail;
      }
      __syncthreads();
      if (tid == 0) {
        s_np = np + nf;
        s_far = fr + nf;
      }
      __syncthreads();
    }
    const uint32_t np = s_np;
    if (np == 0) break;
    // ---- count every level's live orders (one thread per level), scan, write
    uint32_t cnt[SNAP_P / SNAP_T];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < SNAP_P / SNAP_T; ++k) {
      const uint32_t i = (uint32_t)tid * (SNAP_P / SNAP_T) + k;
      uint32_t c = 0;
      if (i < np && !chain_live(bk, p_head[i], p_tail[i], c)) atomicOr(rq.err, 1u);
      cnt[k] = c;
      mine += c;
    }
    uint32_t pass_total = 0;
    uint32_t off = snap_block_excl_scan(mine, wsum, pass_total);
#pragma unroll
    for (int k = 0; k < SNAP_P / SNAP_T; ++k) {
      const uint32_t i = (uint32_t)tid * (SNAP_P / SNAP_T) + k;
      if (i < np) {
        p_off[i] = off;
        me_level o;
        o.price_q4 = p_price[i];
        o.total_qty = p_total[i];
        o.order_count = cnt[k];
        o.pad = 0;
        lv_out[found + i] = o;
      }
      off += cnt[k];
    }
    if (ord_out) {
#pragma unroll
      for (int k = 0; k < SNAP_P / SNAP_T; ++k) {
        const uint32_t i = (uint32_t)tid * (SNAP_P / SNAP_T) + k;
        if (i >= np || !cnt[k]) continue;
        unsigned long long o = norders + p_off[i];
        uint32_t ch = p_head[i], guard = 0;
        while (ch != NIL && ch < bk.nchunks && ++guard <= bk.nchunks) {
          const Chunk& c = bk.chunks[ch];
          o = chunk_entries(c, p_price[i], side == 0, ord_out, o, rq.ocap);
          if (ch == p_tail[i]) break;
          ch = c.hdr.next;
        }
      }
    }
    norders += pass_total;
    found += np;
    __syncthreads();
    if (np < want) break;  // both sources exhausted
  }
  if (tid == 0) {
    rq.nlv[reg] = found;
    rq.nord[reg] = norders;
  }
}

// ---- the feeds' event ring (FeedRing, me_layout.hpp): the two steps both emit passes share -----------
// Does a job of `total` events fit the free part of the log, given the tail it starts from?
template <class Ev>
__device__ __forceinline__ bool feed_fits(const FeedRing<Ev>& r, unsigned long long tail, unsigned long long total) {
  const unsigned long long used = tail - r.consumed;  // (consumed <= tail: the host reads only logged events)
  return used <= r.cap && total <= r.cap - used;
}

// The end of a job, run by exactly one thread once every event of the job is behind a system-scope fence
// (the caller's business). The mirror is pinned host memory written with plain vector stores; the tail goes
// last, behind a fence, so a host that reads the tail first never sees an unwritten event.
template <class Ev>
__device__ __forceinline__ void feed_publish(const FeedRing<Ev>& r, unsigned long long tail, unsigned long long total,
                                             bool fit) {
  const unsigned long long jobs = r.ctl[FR_JOBS] + 1ull;
  const unsigned long long deferred = r.ctl[FR_DEFERRED] + (fit ? 0ull : 1ull);
  const unsigned long long ntail = fit ? tail + total : tail;
  r.ctl[FR_TAIL] = ntail;
  r.ctl[FR_JOBS] = jobs;
  r.ctl[FR_DEFERRED] = deferred;
  r.ctl[FR_PENDING] = fit ? 0ull : 1ull;
  volatile unsigned long long* h = r.hctl;
  h[FR_JOBS] = jobs;
  h[FR_DEFERRED] = deferred;
  h[FR_PENDING] = fit ? 0ull : 1ull;
  __threadfence_system();
  h[FR_TAIL] = ntail;
}

// ---- top-of-book change feed (me_quotes_*, include/me_engine.h; StreamMarketData, proto:32,62-69) ----
// Two launches behind every match launch of an engine with the feed on.
//
// k_quote_scan: one lane per symbol. It reads the symbol's state (64 B), walks each side of the window
// from the best-level hint to the first occupied level (one 16-B Level when the hint is exact; an empty
// level is stepped over, as k_book_snapshot does), falls back to the side's best far level (the last
// occupied entry of its region: 16 B FarDir + 32 B FarLevel) only when the window side is empty, and
// compares with the published quote (40 B). A symbol that differs writes its quote to `cand`; every
// wave writes its ballot word. ~136 B read per symbol with an idle far side, 40 B written per change.
//
// k_quote_emit: one workgroup. It prefixes the words' popcounts (S / 64 words: 1,563 at 100,000
// symbols, two block scans), checks the total against the free part of the log, and — only if it fits —
// writes the events in symbol order (a wave per word, a lane per set bit: position = the word's offset
// + the bits below the lane) and updates the published quotes. Every writing thread fences (system scope)
// behind its events; after the block's barrier thread 0 runs feed_publish.
__device__ __forceinline__ bool quote_far_best(const BookDev& bk, uint32_t s, uint32_t side, uint32_t nfar,
                                               long long& px, long long& qty) {
  if (!nfar) return false;
  FarSide fs;
  far_side(bk, s, side, nfar, fs);  // (a region outside the arena: no far level, the feed has no error word)
  for (uint32_t n = fs.n; n; --n) {
    const long long t = fs.lv[n - 1].total;
    if (t > 0) {
      px = fs.lv[n - 1].price;
      qty = t;
      return true;
    }
  }
  return false;
}

__global__ __launch_bounds__(256) void k_quote_scan(BookDev bk, QuoteDev q) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const int L = (int)bk.L;
  bool changed = false;
  if (s < bk.S) {
    const SymState st = bk.sym[s];
    const Level* lv = bk.levels + (size_t)s * L;
    QuoteTop c;
    c.bid_px = c.ask_px = c.bid_qty = c.ask_qty = 0;
    c.flags = 0;
    c.pad = 0;
    int lb = min(st.best_bid, L - 1);
    long long t = 0;
    while (lb >= 0 && (t = lv[lb].total) <= 0) --lb;
    if (lb >= 0) {
      c.bid_px = st.base + lb;
      c.bid_qty = t;
      c.flags |= ME_QUOTE_HAS_BID;
    } else if (quote_far_best(bk, s, 0u, st.nfar[0], c.bid_px, c.bid_qty)) {
      c.flags |= ME_QUOTE_HAS_BID;
    }
    int la = max(max(st.best_ask, 0), lb + 1);
    t = 0;
    while (la < L && (t = lv[la].total) <= 0) ++la;
    if (la < L) {
      c.ask_px = st.base + la;
      c.ask_qty = t;
      c.flags |= ME_QUOTE_HAS_ASK;
    } else if (quote_far_best(bk, s, 1u, st.nfar[1], c.ask_px, c.ask_qty)) {
      c.flags |= ME_QUOTE_HAS_ASK;
    }
    const QuoteTop p = q.pub[s];
    changed = c.flags != p.flags || c.bid_px != p.bid_px || c.ask_px != p.ask_px || c.bid_qty != p.bid_qty ||
              c.ask_qty != p.ask_qty;
    if (changed) q.cand[s] = c;
  }
  const unsigned long long m = __ballot(changed);
  const uint32_t w = s >> 6;
  if ((threadIdx.x & 63u) == 0u && w < q.nw) q.mask[w] = m;
}

__global__ __launch_bounds__(SNAP_T) void k_quote_emit(BookDev bk, QuoteDev q) {
  __shared__ uint32_t wsum[SNAP_T / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  // changed symbols before every word, and in all
  uint32_t run = 0;
  for (uint32_t base = 0; base < q.nw; base += SNAP_T) {
    const uint32_t w = base + tid;
    const uint32_t pc = w < q.nw ? (uint32_t)__popcll(q.mask[w]) : 0u;
    uint32_t tot = 0;
    const uint32_t ex = snap_block_excl_scan(pc, wsum, tot);
    if (w < q.nw) q.woff[w] = run + ex;
    run += tot;
  }
  const FeedRing<me_quote>& r = q.ring;
  const unsigned long long tail = r.ctl[FR_TAIL];
  const bool fit = feed_fits(r, tail, run);
  __syncthreads();  // the offsets are written, the tail is read
  if (fit && run) {
    for (uint32_t w = wv; w < q.nw; w += SNAP_T / 64) {
      const unsigned long long m = q.mask[w];
      if (!((m >> lane) & 1ull)) continue;
      const uint32_t s = w * 64u + lane;
      const uint32_t pos = q.woff[w] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      const QuoteTop c = q.cand[s];
      me_quote ev;
      ev.bid_price_q4 = c.bid_px;
      ev.ask_price_q4 = c.ask_px;
      ev.bid_qty = c.bid_qty;
      ev.ask_qty = c.ask_qty;
      ev.batches = r.batches;
      ev.symbol = bk.gsym ? bk.gsym[s] : s;
      ev.flags = c.flags;
      r.log[(tail + pos) % r.cap] = ev;
      q.pub[s] = c;
    }
    __threadfence_system();
  }
  __syncthreads();  // every writer has fenced
  if (tid == 0) feed_publish(r, tail, run, fit);
}

// The feed's job: scan + emit on st (behind the match launch whose quotes it takes).
hipError_t launch_quotes(hipStream_t st, const BookDev& bk, const QuoteDev& q) {
  hipLaunchKernelGGL(k_quote_scan, dim3((bk.S + 255u) / 256u), dim3(256), 0, st, bk, q);
  hipLaunchKernelGGL(k_quote_emit, dim3(1), dim3(SNAP_T), 0, st, bk, q);
  return hipGetLastError();
}

// ---- depth feed: top-D price-level changes (me_depth_*, include/me_engine.h) -------------------------
// Three launches behind every match launch of an engine with the depth feed on.
//
// k_depth_scan: one wave per (symbol, side), four per workgroup. It gathers the side's view — the D best
// occupied levels, window first, then far — diffs it against the published view and writes the side's
// candidate events (at their ranks), its candidate view and its event count. A side whose window is empty
// by the hints, with no far level and an empty published view, costs the 64-B state and one count.
//   Both parts come in blocks of 64 levels in priority order (walk_window, walk_far: me_bookread.hpp); a
// ballot of total > 0 and a popcount of the lanes below compact a block's occupied levels into the view.
// The ask walk starts no lower than one level above the best bid found (a bid walk wanting one level), as
// k_quote_scan's does.
//   The diff stages both lists (<= 32 entries each, sorted) in LDS: lanes 0..31 own the new view's
// entries, lanes 32..63 the published ones; each runs down the other list once for "is my price there,
// with which total" and "how many of its entries beat my price". A new entry emits a SET unless published
// with the same total, a published one a DELETE unless its price survives; an event's rank is the emitting
// entries of its own list before it plus those of the other list with a better price: one ballot and
// two popcounts, nothing is sorted.
//
// k_depth_offsets: one workgroup. Block scans, 1,024 counts a round with the running total carried from
// round to round, turn the 2S counts into offsets and the job's total; the fit test is feed_fits; it
// leaves {tail, total, fit} for the emit pass.
//
// k_depth_emit: spread over the grid, at most 2,048 waves, each over a run of consecutive sides. Only when
// the job fits, a wave copies the events of its changed sides to log[(tail + offset + rank) % cap] and their
// candidate views over the published ones. A wave that wrote events fences once (system scope) behind all of
// them, not once per side, and every workgroup counts itself done on a device-scope counter; the last one
// runs feed_publish.
constexpr int DEPTH_WAVES = 4;
constexpr uint32_t DEPTH_EMIT_WAVES = 2048;  // waves of the emit pass at most (8 per CU)

__device__ __forceinline__ void depth_wave_order() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// One block of a side's levels, lane order = priority order: this lane's price and total (<= 0: none). The
// occupied ones go to view[found ..]. True when the view is full.
__device__ __forceinline__ bool depth_take(DepthLvl* view, uint32_t want, uint32_t& found, long long px, long long t) {
  const unsigned long long m = __ballot(t > 0);
  const uint32_t at = found + (uint32_t)__popcll(m & lanemask_lt());
  if (t > 0 && at < want) {
    DepthLvl x;
    x.price = px;
    x.qty = t;
    view[at] = x;
  }
  found = min(want, found + (uint32_t)__popcll(m));
  return found >= want;
}

__global__ __launch_bounds__(DEPTH_WAVES * 64) void k_depth_scan(BookDev bk, DepthDev d) {
  __shared__ DepthLvl s_new[DEPTH_WAVES][ME_DEPTH_MAX];
  __shared__ DepthLvl s_pub[DEPTH_WAVES][ME_DEPTH_MAX];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t sidx = blockIdx.x * DEPTH_WAVES + wv;
  if (sidx >= 2u * bk.S) return;  // (whole waves leave: the kernel has no block barrier)
  const uint32_t s = sidx >> 1;
  const bool bid = (sidx & 1u) == 0u;
  const uint32_t D = d.D;
  const int L = (int)bk.L;
  const SymState st = bk.sym[s];
  const uint32_t nfar_hint = st.nfar[bid ? 0 : 1];
  const bool win = bid ? st.best_bid >= 0 : st.best_ask < L;
  const uint32_t np = min(d.npub[sidx], D);
  if (!win && !nfar_hint && !np) {  // idle: nothing rests by the hints, nothing is published
    if (lane == 0) d.nev[sidx] = 0;
    return;
  }
  DepthLvl* nv = s_new[wv];
  DepthLvl* pv = s_pub[wv];
  // the published view and the far region's place do not depend on the walk: their loads go out ahead of it
  DepthLvl pubv{};
  if (lane < np) pubv = d.pub[(size_t)sidx * D + lane];
  FarSide fs{};
  if (nfar_hint) far_side(bk, s, bid ? 0u : 1u, nfar_hint, fs);  // (a region outside the arena: no far levels, no error word)
  // ---- gather the view
  uint32_t n = 0;
  if (win) {
    const Level* lv = bk.levels + (size_t)s * L;
    const int bb = min(st.best_bid, L - 1);
    int from = bb, to = 0;
    if (!bid) {  // the best bid found (a walk wanting one level): the ask walk starts above it
      int lb = -1;
      walk_window(bk, s, true, bb, 0, [&](int l, bool gate) {
        const unsigned long long m = __ballot(gate && lv[l].total > 0);
        if (m) lb = rli32(l, __builtin_ctzll(m));
        return m != 0ull;
      });
      from = max(max(st.best_ask, 0), lb + 1);
      to = L - 1;
    }
    walk_window(bk, s, bid, from, to,
                [&](int l, bool gate) { return depth_take(nv, D, n, st.base + l, gate ? lv[l].total : 0); });
  }
  // complete it from the far levels, occupied ones only
  if (n < D) walk_far(fs, fs.n, [&](const FarLevel& f) { return depth_take(nv, D, n, f.price, f.total); });
  if (lane < np) pv[lane] = pubv;
  depth_wave_order();
  // ---- diff: lanes 0..31 own the new entries, lanes 32..63 the published ones
  const bool is_new = lane < 32u;
  const uint32_t idx = lane & 31u;
  const uint32_t mine_n = is_new ? n : np, other_n = is_new ? np : n;
  const DepthLvl* other = is_new ? pv : nv;
  const bool valid = idx < mine_n;
  DepthLvl me_{};
  if (valid) me_ = is_new ? nv[idx] : pv[idx];
  bool there = false;
  long long there_qty = 0;
  uint32_t better = 0;  // entries of the other list with a better price (they form its head: it is sorted)
  for (uint32_t k = 0; k < other_n; ++k) {
    const DepthLvl o = other[k];
    if (o.price == me_.price) {
      there = true;
      there_qty = o.qty;
    }
    better += bid ? o.price > me_.price : o.price < me_.price;
  }
  const bool emits = valid && (is_new ? !(there && there_qty == me_.qty) : !there);
  const unsigned long long em = __ballot(emits);
  const uint32_t em_new = (uint32_t)em, em_pub = (uint32_t)(em >> 32);
  const uint32_t ne = (uint32_t)__popcll(em);
  if (emits) {
    const uint32_t own = is_new ? em_new : em_pub, oth = is_new ? em_pub : em_new;
    const uint32_t rank = (uint32_t)__popc(own & ((1u << idx) - 1u)) +
                          (uint32_t)__popc(oth & (better >= 32u ? ~0u : (1u << better) - 1u));
    DepthLvl ev;
    ev.price = me_.price;
    ev.qty = is_new ? me_.qty : 0;
    d.cev[(size_t)sidx * 2u * D + rank] = ev;
  }
  if (ne) {
    if (lane < n) d.cand[(size_t)sidx * D + lane] = nv[lane];
    if (lane == 0) d.ncand[sidx] = n;
  }
  if (lane == 0) d.nev[sidx] = ne;
}

__global__ __launch_bounds__(SNAP_T) void k_depth_offsets(BookDev bk, DepthDev d) {
  __shared__ uint32_t wsum[SNAP_T / 64];
  const uint32_t tid = threadIdx.x;
  const uint32_t ns = 2u * bk.S;
  uint32_t run = 0;
  for (uint32_t base = 0; base < ns; base += SNAP_T) {  // `run` carries the rounds before this one
    const uint32_t i = base + tid;
    const uint32_t c = i < ns ? d.nev[i] : 0u;
    uint32_t tot = 0;
    const uint32_t ex = snap_block_excl_scan(c, wsum, tot);
    if (i < ns) d.off[i] = run + ex;
    run += tot;
  }
  if (tid == 0) {
    unsigned long long* ctl = d.ring.ctl;
    const unsigned long long tail = ctl[FR_TAIL];
    ctl[DJ_TAIL] = tail;
    ctl[DJ_TOTAL] = run;
    ctl[DJ_FIT] = feed_fits(d.ring, tail, run) ? 1ull : 0ull;
  }
}

__global__ __launch_bounds__(DEPTH_WAVES * 64) void k_depth_emit(BookDev bk, DepthDev d, uint32_t spw) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t ns = 2u * bk.S, D = d.D;
  const FeedRing<me_depth_event>& r = d.ring;
  const bool fit = r.ctl[DJ_FIT] != 0ull;
  const unsigned long long total = r.ctl[DJ_TOTAL];
  if (fit && total) {
    const unsigned long long tail = r.ctl[DJ_TAIL];
    // this wave's sides [lo, hi): 64 counts per load, then the changed sides one after the other
    const uint32_t lo = min(ns, (blockIdx.x * DEPTH_WAVES + wv) * spw), hi = min(ns, lo + spw);
    bool wrote = false;
    for (uint32_t base = lo; base < hi; base += 64u) {
      const uint32_t i = base + lane;
      const uint32_t c = i < hi ? d.nev[i] : 0u;
      unsigned long long m = __ballot(c != 0u);
      wrote |= m != 0ull;
      while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1ull;
        const uint32_t sidx = base + (uint32_t)j, s = sidx >> 1;
        const uint32_t ne = min((uint32_t)__shfl((int)c, j, 64), 2u * D);
        if (lane < ne) {
          const DepthLvl x = d.cev[(size_t)sidx * 2u * D + lane];
          me_depth_event ev;
          ev.price_q4 = x.price;
          ev.qty = x.qty;
          ev.batches = r.batches;
          ev.symbol = bk.gsym ? bk.gsym[s] : s;
          ev.side = (sidx & 1u) ? ME_SIDE_SELL : ME_SIDE_BUY;
          ev.pad[0] = ev.pad[1] = ev.pad[2] = 0;
          r.log[(tail + d.off[sidx] + lane) % r.cap] = ev;
        }
        // (the published view is read by the next job's scan only, a later launch: no fence for it)
        const uint32_t nc = min(d.ncand[sidx], D);
        if (lane < nc) d.pub[(size_t)sidx * D + lane] = d.cand[(size_t)sidx * D + lane];
        if (lane == 0) d.npub[sidx] = nc;
      }
    }
    if (wrote) __threadfence_system();  // one fence per wave, behind all the events it wrote
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long before = atomicAdd(&r.ctl[DJ_DONE], 1ull);
    if (before + 1ull == gridDim.x) {  // the last workgroup: every event of the job is behind a fence
      __threadfence_system();
      r.ctl[DJ_DONE] = 0ull;
      feed_publish(r, r.ctl[DJ_TAIL], total, fit);
    }
  }
}

// The depth feed's job: scan + offsets + emit on st (behind the match launch whose books it reads). The emit
// pass runs at most DEPTH_EMIT_WAVES waves, each over a run of consecutive sides: its cost is the events it
// writes and one system-scope fence per wave that wrote any, not one per side.
hipError_t launch_depth(hipStream_t st, const BookDev& bk, const DepthDev& d) {
  const uint32_t ns = 2u * bk.S;
  const uint32_t grid = (ns + DEPTH_WAVES - 1u) / DEPTH_WAVES;
  const uint32_t spw = (ns + DEPTH_EMIT_WAVES - 1u) / DEPTH_EMIT_WAVES;  // sides per emit wave (>= 1)
  const uint32_t ewaves = (ns + spw - 1u) / spw;
  hipLaunchKernelGGL(k_depth_scan, dim3(grid), dim3(DEPTH_WAVES * 64), 0, st, bk, d);
  hipLaunchKernelGGL(k_depth_offsets, dim3(1), dim3(SNAP_T), 0, st, bk, d);
  hipLaunchKernelGGL(k_depth_emit, dim3((ewaves + DEPTH_WAVES - 1u) / DEPTH_WAVES), dim3(DEPTH_WAVES * 64), 0, st, bk, d,
                     spw);
  return hipGetLastError();
}

// ---- trade feed: per-symbol trade summaries (me_trades_*, include/me_engine.h) -----------------------
// Three launches behind every match launch of an engine with the trade feed on (two at enable and catch-up
// time: no fold). Right behind a match launch, record i of a batch owns scratch[start .. start + fill_count)
// in fill order on every matching path, so one fold covers them all. The start is fstart[i] behind a launch
// of the sort path (deep windows: what k_tape_compact reads) and res[i].tape_offset behind a bucketed launch
// (L <= 128: the match job leaves it there until the group's tape job, one launch on, replaces it with the
// tape offset — me_side.hpp aux_tape_tile reads the same word).
//
// k_trade_fold: one lane per record, a workgroup over TF_T * TF_ITERS consecutive records of one batch
// (grid.y = the batch's position in the group). A record without fills costs its 8-B count and start.
// Otherwise the lane reads its symbol and its run and forms the run's volume, high, low and count and the
// keys of its first and last fill (trade_key, me_layout.hpp); a run longer than 64 fills is read by the
// whole wave, 64 fills a step. The symbol's raw words take six 64-bit integer updates (add, min, max). They
// go to the workgroup's LDS table first (TF_TABLE): slot symbol % TF_SLOTS, claimed by a CAS on its tag, so
// that a workgroup sends every symbol it met to HBM once, six atomics on the symbol's own 64-B line, when
// it is done; a symbol that finds its slot held by another goes to HBM at once. When every active lane of a
// wave holds the same symbol (TF_WAVE) the wave reduces first and one lane goes on. Sums and min / max do
// not depend on arrival order: the words are deterministic. A record whose run does not lie inside the
// scratch, or whose symbol is >= S, is skipped.
//
// k_trade_scan: one lane per symbol. A symbol whose job count is non-zero fetches the two fills its keys
// name from their batches' scratch, merges the job into its pending summary (open only when that is empty),
// adds to its cumulative pair and puts the job words back to their identities. Every wave then ballots
// "pending non-empty" into its mask word.
//
// k_trade_emit: k_quote_emit's shape — prefix the popcounts, feed_fits, and only if the job fits write the
// events in symbol order and empty the pending summaries (never the cumulative pair); every writer fences
// at system scope, and after the barrier thread 0 runs feed_publish.
__device__ __forceinline__ unsigned long long trade_wave_min(unsigned long long x) {
  for (int d = 32; d >= 1; d >>= 1) x = min(x, (unsigned long long)__shfl_xor(x, d, 64));
  return x;
}
__device__ __forceinline__ unsigned long long trade_wave_max(unsigned long long x) {
  for (int d = 32; d >= 1; d >>= 1) x = max(x, (unsigned long long)__shfl_xor(x, d, 64));
  return x;
}

constexpr uint32_t TF_T = 1024;     // threads of a fold workgroup
constexpr uint32_t TF_ITERS = 16;   // records per thread: a workgroup folds TF_T * TF_ITERS records of one batch
constexpr uint32_t TF_SLOTS = 1024; // slots of the workgroup's LDS table (48 KB of words + 4 KB of tags)
enum : uint32_t { TF_WAVE = 1u, TF_TABLE = 2u };  // TradeDev::wave_reduce bits (ME_TRADE_FOLD)

__device__ __forceinline__ void trade_words_global(unsigned long long* w, unsigned long long kf, unsigned long long kl,
                                                   unsigned long long hi, unsigned long long lo, unsigned long long vol,
                                                   unsigned long long cnt) {
  atomicMin(&w[TJ_FIRST], kf);
  atomicMax(&w[TJ_LAST], kl);
  atomicMax(&w[TJ_HIGH], hi);
  atomicMin(&w[TJ_LOW], lo);
  atomicAdd(&w[TJ_VOLUME], vol);
  atomicAdd(&w[TJ_COUNT], cnt);
}

__global__ __launch_bounds__(TF_T) void k_trade_fold(TradeDev t, TradeLaunch tl, uint32_t S) {
  __shared__ unsigned long long tab[TF_SLOTS][6];  // TJ_FIRST .. TJ_COUNT of the symbol in tag[slot]
  __shared__ uint32_t tag[TF_SLOTS];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t pos = blockIdx.y;
  const TradeBatch& b = tl.b[pos];
  const bool table = (t.wave_reduce & TF_TABLE) != 0u;
  if (table) {
    for (uint32_t k = threadIdx.x; k < TF_SLOTS; k += TF_T) {
      tag[k] = NIL;
      tab[k][TJ_FIRST] = ~0ull;
      tab[k][TJ_LAST] = 0ull;
      tab[k][TJ_HIGH] = 0ull;
      tab[k][TJ_LOW] = ~0ull;
      tab[k][TJ_VOLUME] = 0ull;
      tab[k][TJ_COUNT] = 0ull;
    }
    __syncthreads();
  }
  const uint32_t r0 = blockIdx.x * (TF_T * TF_ITERS);
  for (uint32_t it = 0; it < TF_ITERS; ++it) {
    const uint32_t w0 = r0 + it * TF_T;
    if (w0 >= b.n) break;  // (the same for the whole workgroup)
    const uint32_t i = w0 + threadIdx.x;
    uint32_t fc = 0, s = 0, f0 = 0;
    if (i < b.n) {
      fc = b.res[i].fill_count;
      f0 = b.res[i].tape_offset;  // (the same 8 B: a bucketed launch leaves the run's start here)
    }
    bool active = fc != 0u;
    if (active) {
      s = b.sym[i];
      if (b.fstart) f0 = b.fstart[i];
      active = s < S && (unsigned long long)f0 <= tl.scratch_cap && (unsigned long long)fc <= tl.scratch_cap - f0;
    }
    const unsigned long long am = __ballot(active);
    if (!am) continue;  // (the whole wave: there is no barrier inside the loop)
    unsigned long long vol = 0, hi = 0, lo = ~0ull;
    if (active && fc <= 64u) {
      for (uint32_t k = 0; k < fc; ++k) {
        const me_fill& f = b.scratch[(size_t)f0 + k];
        const unsigned long long p = trade_bias(f.price_q4);
        vol += (unsigned long long)(long long)f.qty;
        hi = max(hi, p);
        lo = min(lo, p);
      }
    }
    // runs longer than 64 fills, one after the other: the whole wave reads them, 64 fills a step
    for (unsigned long long m = __ballot(active && fc > 64u); m; m &= m - 1ull) {
      const int j = __builtin_ctzll(m);
      const uint32_t jf0 = (uint32_t)__shfl((int)f0, j, 64), jfc = (uint32_t)__shfl((int)fc, j, 64);
      unsigned long long v = 0, h = 0, l = ~0ull;
      for (uint32_t k = lane; k < jfc; k += 64u) {
        const me_fill& f = b.scratch[(size_t)jf0 + k];
        const unsigned long long p = trade_bias(f.price_q4);
        v += (unsigned long long)(long long)f.qty;
        h = max(h, p);
        l = min(l, p);
      }
      v = (unsigned long long)wave_sum((long long)v);
      h = trade_wave_max(h);
      l = trade_wave_min(l);
      if ((int)lane == j) {
        vol = v;
        hi = h;
        lo = l;
      }
    }
    unsigned long long kf = ~0ull, kl = 0ull, cnt = 0ull;
    if (active) {
      kf = trade_key(pos, i, 0u);
      kl = trade_key(pos, i, fc - 1u);
      cnt = fc;
    }
    // one symbol in the whole wave: reduce, and the first active lane goes on alone
    const int lead = __builtin_ctzll(am);
    bool issue = active;
    if ((t.wave_reduce & TF_WAVE) && (am & (am - 1ull))) {
      const uint32_t s0 = (uint32_t)__shfl((int)s, lead, 64);
      if (!__ballot(active && s != s0)) {
        vol = (unsigned long long)wave_sum((long long)vol);  // (inactive lanes hold the identities)
        cnt = (unsigned long long)wave_sum((long long)cnt);
        hi = trade_wave_max(hi);
        lo = trade_wave_min(lo);
        kf = trade_wave_min(kf);
        kl = trade_wave_max(kl);
        issue = (int)lane == lead;
      }
    }
    if (issue) {
      bool mine = false;
      const uint32_t slot = s & (TF_SLOTS - 1u);
      if (table) {  // the slot is this symbol's if it is free or already holds it; else straight to HBM
        const uint32_t was = atomicCAS(&tag[slot], NIL, s);
        mine = was == NIL || was == s;
      }
      if (mine) {
        atomicMin(&tab[slot][TJ_FIRST], kf);
        atomicMax(&tab[slot][TJ_LAST], kl);
        atomicMax(&tab[slot][TJ_HIGH], hi);
        atomicMin(&tab[slot][TJ_LOW], lo);
        atomicAdd(&tab[slot][TJ_VOLUME], vol);
        atomicAdd(&tab[slot][TJ_COUNT], cnt);
      } else {
        trade_words_global(t.jw + (size_t)s * TJ_N, kf, kl, hi, lo, vol, cnt);
      }
    }
  }
  if (!table) return;
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < TF_SLOTS; k += TF_T) {
    const uint32_t s = tag[k];
    if (s == NIL || s >= S || !tab[k][TJ_COUNT]) continue;
    trade_words_global(t.jw + (size_t)s * TJ_N, tab[k][TJ_FIRST], tab[k][TJ_LAST], tab[k][TJ_HIGH], tab[k][TJ_LOW],
                       tab[k][TJ_VOLUME], tab[k][TJ_COUNT]);
  }
}

// The fill a key names, or false when the key does not name one of this launch (never the case for a key
// the fold wrote: it took them from records it had checked).
__device__ __forceinline__ bool trade_fill_at(const TradeLaunch& tl, unsigned long long key, me_fill& out) {
  const uint32_t fill = (uint32_t)key;
  const unsigned long long up = key >> TK_FILL_BITS;
  const uint32_t pos = tl.nb == 1u ? 0u : (uint32_t)(up >> TK_REC_BITS);
  const uint32_t rec = tl.nb == 1u ? (uint32_t)up : (uint32_t)(up & ((1u << TK_REC_BITS) - 1u));
  if (pos >= tl.nb) return false;
  const TradeBatch& b = tl.b[pos];
  if (rec >= b.n) return false;
  const unsigned long long at = (unsigned long long)(b.fstart ? b.fstart[rec] : b.res[rec].tape_offset) + fill;
  if (at >= tl.scratch_cap) return false;
  out = b.scratch[at];
  return true;
}

__global__ __launch_bounds__(256) void k_trade_scan(TradeDev t, TradeLaunch tl, uint32_t S) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  bool pending = false;
  if (s < S) {
    unsigned long long* w = t.jw + (size_t)s * TJ_N;
    const unsigned long long cnt = w[TJ_COUNT];
    unsigned long long have = t.pend[s].trades;
    if (cnt) {
      me_fill first, last;
      if (trade_fill_at(tl, w[TJ_FIRST], first) && trade_fill_at(tl, w[TJ_LAST], last)) {
        TradePend p = t.pend[s];
        const long long hi = trade_unbias(w[TJ_HIGH]), lo = trade_unbias(w[TJ_LOW]);
        if (!p.trades) {
          p.open_px = first.price_q4;
          p.high_px = hi;
          p.low_px = lo;
          p.volume = 0;
        } else {
          p.high_px = max(p.high_px, hi);
          p.low_px = min(p.low_px, lo);
        }
        p.taker_seq = last.taker_seq;
        p.maker_seq = last.maker_seq;
        p.last_px = last.price_q4;
        p.last_qty = last.qty;
        p.pad = 0;
        p.volume += (long long)w[TJ_VOLUME];
        p.trades += cnt;
        t.pend[s] = p;
        TradeCum c = t.cum[s];
        c.volume += (long long)w[TJ_VOLUME];
        c.trades += cnt;
        t.cum[s] = c;
        have = p.trades;
      }
      w[TJ_FIRST] = ~0ull;
      w[TJ_LAST] = 0ull;
      w[TJ_HIGH] = 0ull;
      w[TJ_LOW] = ~0ull;
      w[TJ_VOLUME] = 0ull;
      w[TJ_COUNT] = 0ull;
    }
    pending = have != 0ull;
  }
  const unsigned long long m = __ballot(pending);
  const uint32_t wd = s >> 6;
  if ((threadIdx.x & 63u) == 0u && wd < t.nw) t.mask[wd] = m;
}

__global__ __launch_bounds__(SNAP_T) void k_trade_emit(BookDev bk, TradeDev t) {
  __shared__ uint32_t wsum[SNAP_T / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  uint32_t run = 0;
  for (uint32_t base = 0; base < t.nw; base += SNAP_T) {
    const uint32_t w = base + tid;
    const uint32_t pc = w < t.nw ? (uint32_t)__popcll(t.mask[w]) : 0u;
    uint32_t tot = 0;
    const uint32_t ex = snap_block_excl_scan(pc, wsum, tot);
    if (w < t.nw) t.woff[w] = run + ex;
    run += tot;
  }
  const FeedRing<me_trade>& r = t.ring;
  const unsigned long long tail = r.ctl[FR_TAIL];
  const bool fit = feed_fits(r, tail, run);
  __syncthreads();  // the offsets are written, the tail is read
  if (fit && run) {
    for (uint32_t w = wv; w < t.nw; w += SNAP_T / 64) {
      const unsigned long long m = t.mask[w];
      if (!((m >> lane) & 1ull)) continue;
      const uint32_t s = w * 64u + lane;
      const uint32_t pos = t.woff[w] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      const TradePend p = t.pend[s];
      const TradeCum c = t.cum[s];
      me_trade ev;
      ev.taker_seq = p.taker_seq;
      ev.maker_seq = p.maker_seq;
      ev.last_price_q4 = p.last_px;
      ev.open_price_q4 = p.open_px;
      ev.high_price_q4 = p.high_px;
      ev.low_price_q4 = p.low_px;
      ev.volume = p.volume;
      ev.trades = p.trades;
      ev.cum_volume = c.volume;
      ev.cum_trades = c.trades;
      ev.batches = r.batches;
      ev.last_qty = p.last_qty;
      ev.symbol = bk.gsym ? bk.gsym[s] : s;
      r.log[(tail + pos) % r.cap] = ev;
      t.pend[s].trades = 0ull;  // empty (the next job's scan reads it: a later launch)
    }
    __threadfence_system();
  }
  __syncthreads();  // every writer has fenced
  if (tid == 0) feed_publish(r, tail, run, fit);
}

// The trade feed's job on st: the fold of the launch's fills (tl.nb batches, behind their match launch; none
// at enable / catch-up time), then scan + emit.
hipError_t launch_trades(hipStream_t st, const BookDev& bk, const TradeDev& t, const TradeLaunch& tl) {
  if (tl.nb && tl.nmax)
    hipLaunchKernelGGL(k_trade_fold, dim3((tl.nmax + TF_T * TF_ITERS - 1u) / (TF_T * TF_ITERS), tl.nb), dim3(TF_T), 0,
                       st, t, tl, bk.S);
  hipLaunchKernelGGL(k_trade_scan, dim3((bk.S + 255u) / 256u), dim3(256), 0, st, t, tl, bk.S);
  hipLaunchKernelGGL(k_trade_emit, dim3(1), dim3(SNAP_T), 0, st, bk, t);
  return hipGetLastError();
}

// ---- trigger book: stop and stop-limit orders (me_stops_*, include/me_engine.h) -----------------------
// Three launches behind every match launch of an engine with live stops (none otherwise: the host knows).
//
// The fold is k_trade_fold as it is, through a TradeDev view whose jw words are the trigger book's own: after
// it, a symbol's TJ_COUNT says whether it traded in this launch and TJ_HIGH / TJ_LOW hold its biased extremes.
//
// k_stop_scan: one lane per table entry of [0, top). A live entry reads its symbol's count (a symbol without
// a fill triggers nothing: the count decides, not the min / max identities) and compares its biased stop
// price with the high (BUY: high >= stop) or the low (SELL: low <= stop). Every wave ballots into its mask
// word. 48 B per entry plus the symbol's 64-B line, which the entries of a symbol share in L2.
//
// k_stop_emit: k_trade_emit's shape — prefix the popcounts, feed_fits (always true: the host keeps a ring
// slot for every live stop, me_stops.hpp), write the events at tail + pos in table order and clear the
// entries' state; every writer fences at system scope, and after the barrier the job words of every symbol
// that traded go back to their identities and thread 0 runs feed_publish.
__global__ __launch_bounds__(256) void k_stop_scan(StopDev sd) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool trig = false;
  if (i < sd.top) {
    const StopEnt& e = sd.tab[i];
    const uint32_t s = e.s.symbol;
    if (e.live && s < sd.S) {
      const unsigned long long* w = sd.jw + (size_t)s * TJ_N;
      if (w[TJ_COUNT]) {
        const unsigned long long p = trade_bias(e.s.stop_px_q4);
        trig = (e.s.kind & 3u) == ME_SIDE_BUY ? w[TJ_HIGH] >= p : w[TJ_LOW] <= p;
      }
    }
  }
  const unsigned long long m = __ballot(trig);
  if ((threadIdx.x & 63u) == 0u && i < sd.top) sd.mask[i >> 6] = m;  // (i: the word's first entry)
}

__global__ __launch_bounds__(SNAP_T) void k_stop_emit(StopDev sd) {
  __shared__ uint32_t wsum[SNAP_T / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t nw = (sd.top + 63u) / 64u;
  uint32_t run = 0;
  for (uint32_t base = 0; base < nw; base += SNAP_T) {
    const uint32_t w = base + tid;
    const uint32_t pc = w < nw ? (uint32_t)__popcll(sd.mask[w]) : 0u;
    uint32_t tot = 0;
    const uint32_t ex = snap_block_excl_scan(pc, wsum, tot);
    if (w < nw) sd.woff[w] = run + ex;
    run += tot;
  }
  const FeedRing<me_stop_event>& r = sd.ring;
  const unsigned long long tail = r.ctl[FR_TAIL];
  const bool fit = feed_fits(r, tail, run);
  __syncthreads();  // the offsets are written, the tail is read
  if (fit && run) {
    for (uint32_t w = wv; w < nw; w += SNAP_T / 64) {
      const unsigned long long m = sd.mask[w];
      if (!((m >> lane) & 1ull)) continue;
      const uint32_t i = w * 64u + lane;
      const uint32_t pos = sd.woff[w] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      const me_stop s = sd.tab[i].s;
      const unsigned long long* jw = sd.jw + (size_t)s.symbol * TJ_N;
      me_stop_event ev;
      ev.id = s.id;
      ev.stop_px_q4 = s.stop_px_q4;
      ev.limit_px_q4 = s.limit_px_q4;
      ev.trigger_px_q4 = trade_unbias((s.kind & 3u) == ME_SIDE_BUY ? jw[TJ_HIGH] : jw[TJ_LOW]);
      ev.batches = r.batches;
      ev.qty = s.qty;
      ev.symbol = s.symbol;
      ev.kind = s.kind;
      for (int k = 0; k < 15; ++k) ev.pad[k] = 0;
      r.log[(tail + pos) % r.cap] = ev;
      sd.tab[i].live = 0;
    }
    __threadfence_system();
  }
  __syncthreads();  // every writer has fenced and has read its symbol's words
  for (uint32_t s = tid; s < sd.S; s += SNAP_T) {
    unsigned long long* w = sd.jw + (size_t)s * TJ_N;
    if (!w[TJ_COUNT]) continue;  // (the count rises with every other word: untouched words are identities)
    w[TJ_FIRST] = ~0ull;
    w[TJ_LAST] = 0ull;
    w[TJ_HIGH] = 0ull;
    w[TJ_LOW] = ~0ull;
    w[TJ_VOLUME] = 0ull;
    w[TJ_COUNT] = 0ull;
  }
  if (tid == 0) feed_publish(r, tail, run, fit);
}

// The trigger book's job on st, behind the match launch whose nb batches tl names.
hipError_t launch_stops(hipStream_t st, const StopDev& sd, const TradeLaunch& tl) {
  if (tl.nb && tl.nmax) {
    TradeDev t{};  // the fold reads jw and wave_reduce alone
    t.jw = sd.jw;
    t.wave_reduce = TF_WAVE | TF_TABLE;
    hipLaunchKernelGGL(k_trade_fold, dim3((tl.nmax + TF_T * TF_ITERS - 1u) / (TF_T * TF_ITERS), tl.nb), dim3(TF_T), 0,
                       st, t, tl, sd.S);
  }
  if (sd.top) hipLaunchKernelGGL(k_stop_scan, dim3((sd.top + 255u) / 256u), dim3(256), 0, st, sd);
  hipLaunchKernelGGL(k_stop_emit, dim3(1), dim3(SNAP_T), 0, st, sd);
  return hipGetLastError();
}

// k_stop_cancel: one lane per id. The table ascends by id over [0, top), dead entries included, so a binary
// search finds the one entry that can hold the id; a live one is cleared and answers 1. The ids of a call are
// distinct (the host checks that they ascend): no two lanes touch one entry.
__global__ __launch_bounds__(256) void k_stop_cancel(StopDev sd, const uint64_t* ids, uint32_t n, uint8_t* found) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= n) return;
  const uint64_t id = ids[q];
  uint32_t lo = 0, hi = sd.top;  // the first entry with an id >= id lies in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (sd.tab[mid].s.id < id) lo = mid + 1u;
    else hi = mid;
  }
  uint8_t f = 0;
  if (lo < sd.top && sd.tab[lo].s.id == id && sd.tab[lo].live) {
    sd.tab[lo].live = 0;
    f = 1;
  }
  found[q] = f;
}

hipError_t launch_stop_cancel(hipStream_t st, const StopDev& sd, const uint64_t* ids, uint32_t n, uint8_t* found) {
  if (n) hipLaunchKernelGGL(k_stop_cancel, dim3((n + 255u) / 256u), dim3(256), 0, st, sd, ids, n, found);
  return hipGetLastError();
}

// The stable compaction of the table (an add that reaches the append end, and me_stops_dump): k_stop_live
// ballots "live" per entry, k_stop_compact — one workgroup, k_stop_emit's prefix — scatters the live entries
// to dst in table order and writes their number to *count. dst is the table's other buffer: never sd.tab.
__global__ __launch_bounds__(256) void k_stop_live(StopDev sd) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const unsigned long long m = __ballot(i < sd.top && sd.tab[i].live);
  if ((threadIdx.x & 63u) == 0u && i < sd.top) sd.mask[i >> 6] = m;
}

__global__ __launch_bounds__(SNAP_T) void k_stop_compact(StopDev sd, StopEnt* dst, uint32_t* count) {
  __shared__ uint32_t wsum[SNAP_T / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t nw = (sd.top + 63u) / 64u;
  uint32_t run = 0;
  for (uint32_t base = 0; base < nw; base += SNAP_T) {
    const uint32_t w = base + tid;
    const uint32_t pc = w < nw ? (uint32_t)__popcll(sd.mask[w]) : 0u;
    uint32_t tot = 0;
    const uint32_t ex = snap_block_excl_scan(pc, wsum, tot);
    if (w < nw) sd.woff[w] = run + ex;
    run += tot;
  }
  __syncthreads();  // the offsets are written
  for (uint32_t w = wv; w < nw; w += SNAP_T / 64) {
    const unsigned long long m = sd.mask[w];
    if (!((m >> lane) & 1ull)) continue;
    // (pos <= the entry's own index < top <= cap: inside dst)
    const uint32_t pos = sd.woff[w] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    StopEnt e = sd.tab[w * 64u + lane];
    for (int k = 0; k < 7; ++k) e.s.pad[k] = 0;
    dst[pos] = e;
  }
  if (tid == 0) *count = run;
}

hipError_t launch_stop_compact(hipStream_t st, const StopDev& sd, StopEnt* dst, uint32_t* count) {
  if (sd.top) hipLaunchKernelGGL(k_stop_live, dim3((sd.top + 255u) / 256u), dim3(256), 0, st, sd);
  hipLaunchKernelGGL(k_stop_compact, dim3(1), dim3(SNAP_T), 0, st, sd, dst, count);
  return hipGetLastError();
}

// ---- order query (me_order_query, include/me_engine.h) -----------------------------------------------
// k_order_query: one wave per queried seq, four per workgroup, read-only. The wave
//   1. finds the order's slot as cancel_order does (me_kernels.hip): the seq ring's entry, verified (chunk id
//      in range, the slot holds the seq, quantity > 0); on someone else's entry and a seq below the horizon,
//      the old-order table of the current epoch, verified the same way. Between launches HBM is the book:
//      no on-chip copy exists;
//   2. walks hdr.prev from the order's chunk to the level's head: lanes 0..15 hold a chunk's quantities and
//      add the live ones (in the order's own chunk only the slots below its own). One dependent HBM round
//      trip per chunk; every id is checked against nchunks before it is dereferenced and the walk ends
//      after nchunks steps at the latest;
//   3. finds the level: price - base inside [0, L) is a window level, a bid at or below best_bid, an ask at
//      or above best_ask; any other price is a far level of side price < base ? bid : ask (Invariant I),
//      located by far_rank. The walk must have ended at that level's head;
//   4. adds up the better levels of the side: the occupied window levels between the side's best hint and
//      the order's level (all of the side's window levels for a far order: a window level always beats a far
//      level) and, for a far order, the occupied far entries behind its own (the best is last): walk_window
//      over a bounded range and walk_far (me_bookread.hpp), as per-lane partial sums.
// Whatever does not fit (an id out of range, the step bound, a level that is not there, a head that is not
// the walk's end) sets the request's error word and answers found = 0; nothing is read out of bounds.
constexpr int OQ_WAVES = 4;

__global__ __launch_bounds__(OQ_WAVES * 64) void k_order_query(BookDev bk, OrderQueryReq rq) {
  const int lane = lane_id();
  const uint32_t qi = blockIdx.x * OQ_WAVES + (threadIdx.x >> 6);
  if (qi >= rq.n) return;  // (whole waves leave: the kernel has no block barrier)
  const unsigned long long tgt = rl64(rq.seqs[qi], 0);
  const uint32_t NC = bk.nchunks;
  me_order_info o{};
  o.seq = tgt;
  // ---- 1. the slot
  uint32_t g = NIL;
  int q = 0;
  if (tgt != 0ull) {
    const SeqState sqs = bk.sq[bk.sq_idx];
    const unsigned long long horizon = rl64(sqs.horizon, 0);
    const uint32_t epoch = rl32(sqs.epoch, 0);
    uint32_t cand = rl32(bk.loc[tgt & bk.ring_mask], 0);
    for (int pass = 0;; ++pass) {
      if (cand != NIL && cand / ME_C < NC) {
        const unsigned long long sq = rl64(cs_at(bk.chunks, cand), 0);
        if (sq == tgt) {  // the order's slot: live or dead, it never moves
          q = rli32(cq_at(bk.chunks, cand), 0);
          if (q > 0) g = cand;
          break;
        }
      }
      // the ring entry is someone else's: only an order older than the horizon can still be live
      if (pass != 0 || tgt >= horizon) break;
      cand = old_lookup((gptr<const OldEnt>)bk.old, bk.old_mask, epoch, tgt);
      if (cand == NIL) break;
    }
  }
  bool bad = false;
  if (g != NIL) {
    const uint32_t ch0 = g / ME_C, slot = g % ME_C;
    const long long price = rli64(bk.chunks[ch0].hdr.price, 0);
    const uint32_t s = rl32(bk.chunks[ch0].owner, 0);
    // ---- 2. the place in the level: back to the head
    long long a_qty = 0, a_cnt = 0;  // per-lane partial sums
    uint32_t cur = ch0, steps = 0;
    for (;;) {
      const uint32_t prv = rl32(bk.chunks[cur].hdr.prev, 0);
      const int qv = lane < ME_C ? bk.chunks[cur].qty[lane] : 0;
      if (qv > 0 && (cur != ch0 || (uint32_t)lane < slot)) {
        a_qty += qv;
        a_cnt += 1;
      }
      if (prv == NIL) break;
      if (prv >= NC || ++steps >= NC) {
        bad = true;
        break;
      }
      cur = prv;
    }
    bad = bad || s >= bk.S;
    if (!bad) {
      // ---- 3. the level
      const SymState st = bk.sym[s];
      const long long base = rli64(st.base, 0);
      const int L = (int)bk.L;
      const int bb = min(rli32(st.best_bid, 0), L - 1), ba = max(rli32(st.best_ask, 0), 0);
      const unsigned long long off = (unsigned long long)price - (unsigned long long)base;
      long long b_qty = 0, b_cnt = 0;  // per-lane partial sums
      const auto better = [&](long long t) {
        b_qty += t > 0 ? t : 0;
        b_cnt += t > 0;
        return false;
      };
      const Level* lv = bk.levels + (size_t)s * L;
      const auto window = [&](int lo, int hi) {  // (in no particular order: as asks)
        walk_window(bk, s, false, lo, hi, [&](int l, bool gate) { return better(gate ? lv[l].total : 0); });
      };
      long long level_qty = 0;
      uint32_t head = NIL;
      bool bid = false;
      if (off < (unsigned long long)L) {
        const int lvl = (int)off;
        const Level x = lv[lvl];
        level_qty = rli64(x.total, 0);
        head = rl32(x.head, 0);
        bid = lvl <= bb;
        if (bid == (lvl >= ba)) bad = true;  // between the hints (or both): no level of either side
        // ---- 4. better: strictly between the side's best hint and the order's level
        if (!bad) window(bid ? lvl + 1 : ba, bid ? bb : lvl - 1);
      } else {
        bid = price < base;
        const uint32_t k = bid ? 0u : 1u;
        FarSide fs;
        far_side(bk, s, k, bid ? st.nfar[0] : st.nfar[1], fs);  // (a bad region is an empty one: the level is not there)
        const uint32_t pos = fs.n ? far_rank(fs.lv, fs.n, price, k) : 0u;
        if (pos >= fs.n) {
          bad = true;
        } else {
          const FarLevel e = far_get(fs.lv, pos);
          level_qty = e.total;
          head = e.head;
          bad = e.price != price;
        }
        if (!bad) {  // every window level of the side, and the far entries behind the order's
          window(bid ? 0 : ba, bid ? bb : L - 1);
          walk_far(fs, fs.n - 1u - pos, [&](const FarLevel& e) { return better(e.total); });
        }
      }
      bad = bad || head != cur;  // the walk ended at another chunk than the level's first
      if (!bad) {
        o.price_q4 = price;
        o.qty_ahead = wave_sum(a_qty);
        o.level_qty = level_qty;
        o.qty_better = wave_sum(b_qty);
        o.qty = q;
        o.orders_ahead = (uint32_t)wave_sum(a_cnt);
        o.levels_better = (uint32_t)wave_sum(b_cnt);
        o.symbol = bk.gsym ? bk.gsym[s] : s;
        o.side = bid ? ME_SIDE_BUY : ME_SIDE_SELL;
        o.found = 1;
      }
    }
  }
  if (lane == 0) {
    if (bad) atomicOr(rq.err, 1u);
    rq.out[qi] = o;
  }
}

hipError_t launch_order_query(hipStream_t st, const BookDev& bk, const OrderQueryReq& rq) {
  if (!rq.n) return hipSuccess;
  hipLaunchKernelGGL(k_order_query, dim3((rq.n + OQ_WAVES - 1u) / OQ_WAVES), dim3(OQ_WAVES * 64), 0, st, bk, rq);
  return hipGetLastError();
}

// ---- order preview (me_order_preview, include/me_engine.h) -------------------------------------------
// k_order_preview: one wave per hypothetical NEW record, four per workgroup, read-only, no LDS. After the
// matcher's rejects (BAD_SYMBOL, BAD_QTY, BAD_SIDE, BAD_TIF, in that order) the wave walks the side the record
// would trade against, best level first, in blocks of up to 64 levels, lane order = priority order: the window
// outward from the side's best hint, then the far levels (walk_window, walk_far: me_bookread.hpp; a far region
// outside the arena sets the error word). pv_block does the rest. A level counts when its total is > 0 (the
// total decides). The first such level is the opposite best. The limit clips by
// price: every lane compares its level's own price with the limit, a signed int64 compare — no price
// difference is ever formed, so any int64 limit and any window base are exact — and the first counted level
// beyond the limit ends the walk (prices only get worse behind it; by Invariant I that also keeps a limit
// short of the window's far edge away from the far levels). A wave_incl_scan of the totals finds where the
// running sum reaches the quantity wanted: lane i takes min(max(want - before_i, 0), total_i). Every lane
// that takes anything adds price x taken to the notional as a 128-bit product from 64-bit halves, and the
// wave then walks that level's FIFO for fill_count (pv_chain): lanes 0..15 hold a chunk's quantities, a scan
// counts the live makers whose running quantity starts below what is taken there — all of them on a level
// consumed whole. One dependent HBM round trip per chunk; every chunk id is checked against nchunks before
// it is dereferenced, a walk ends after nchunks steps at the latest and must cover the quantity by the
// level's tail; a violation sets the request's error word, nothing is read out of bounds.
//   A POST_ONLY needs the opposite best alone: the same walk wanting nothing. A FOK walks twice: first the
// totals only (no chain, nothing committed), and only when they cover its quantity the walk that counts.
constexpr int PV_WAVES = 4;

struct PvWalk {  // wave-uniform
  long long limit;
  long long want;  // quantity still to take
  bool buy, market;
  bool count;      // walk the chains of the levels taken (fill_count)
  bool has_opp, bad;
  long long opp_px, first_px, last_px;
  unsigned long long nlo;  // notional: low half ...
  long long nhi;           // ... and high half
  uint32_t levels, fills;
};

// fill_count of one level: the live makers from the head whose running quantity starts below `need`.
__device__ __forceinline__ void pv_chain(const BookDev& bk, PvWalk& w, uint32_t head, uint32_t tail, long long need) {
  const int lane = lane_id();
  const uint32_t NC = bk.nchunks;
  uint32_t ch = head, steps = 0;
  for (;;) {
    if (ch >= NC || ++steps > NC) {  // (NIL too)
      w.bad = true;
      return;
    }
    const int qv = lane < ME_C ? bk.chunks[ch].qty[lane] : 0;
    const uint32_t nx = rl32(bk.chunks[ch].hdr.next, 0);
    const long long uq = qv > 0 ? qv : 0;
    const long long incl = wave_incl_scan(uq);
    w.fills += (uint32_t)__popcll(__ballot(uq > 0 && incl - uq < need));
    const long long live = rli64(incl, 63);
    if (live >= need) return;
    need -= live;
    if (ch == tail) {  // the chain holds less than the level's total says
      w.bad = true;
      return;
    }
    ch = nx;
  }
}

// One block of the walk: this lane's level (total <= 0: none). True when the walk is over.
__device__ __forceinline__ bool pv_block(const BookDev& bk, PvWalk& w, long long price, long long total, uint32_t head,
                                         uint32_t tail) {
  const int lane = lane_id();
  const bool occ = total > 0;
  const unsigned long long mo = __ballot(occ);
  if (!mo) return false;
  if (!w.has_opp) {
    w.has_opp = true;
    w.opp_px = rli64(price, __builtin_ctzll(mo));
  }
  const bool beyond = occ && !w.market && (w.buy ? price > w.limit : price < w.limit);
  const unsigned long long mb = __ballot(beyond);
  const bool in = occ && (!mb || lane < __builtin_ctzll(mb));
  const long long t = in ? total : 0;
  const long long incl = wave_incl_scan(t);
  long long take = w.want - (incl - t);
  take = take < 0 ? 0 : (take < t ? take : t);
  const unsigned long long mt = __ballot(take > 0);
  if (mt) {
    if (!w.levels) w.first_px = rli64(price, __builtin_ctzll(mt));
    w.last_px = rli64(price, 63 - __builtin_clzll(mt));
    w.levels += (uint32_t)__popcll(mt);
    // price x take, take <= INT32_MAX: the signed 128-bit product from 64-bit halves, summed over the wave in
    // three 64-bit columns (the low half as two 32-bit columns: 64 of them cannot carry out of 64 bits)
    const unsigned long long plo = (unsigned long long)price * (unsigned long long)take;
    const long long phi = __mul64hi(price, take);
    const unsigned long long c0 = (unsigned long long)wave_sum((long long)(plo & 0xFFFFFFFFull));
    const unsigned long long c1 = (unsigned long long)wave_sum((long long)(plo >> 32));
    const unsigned long long chi = (unsigned long long)wave_sum(phi);
    const unsigned long long lo = c0 + (c1 << 32);
    const unsigned long long hi = chi + (c1 >> 32) + (lo < c0 ? 1ull : 0ull);
    const unsigned long long nlo = w.nlo + lo;
    w.nhi = (long long)((unsigned long long)w.nhi + hi + (nlo < lo ? 1ull : 0ull));
    w.nlo = nlo;
    if (w.count) {
      for (unsigned long long m = mt; m; m &= m - 1ull) {
        const int j = __builtin_ctzll(m);
        pv_chain(bk, w, rl32(head, j), rl32(tail, j), rli64(take, j));
      }
    }
    const long long got = rli64(incl, 63);
    w.want -= got < w.want ? got : w.want;
  }
  return mb != 0ull || w.want == 0;
}

// The whole walk of symbol s's side opposite to the record: window, then far levels.
__device__ __forceinline__ void pv_walk(const BookDev& bk, uint32_t s, PvWalk& w) {
  const SymState st = bk.sym[s];
  const int L = (int)bk.L;
  const bool bid = !w.buy;  // a SELL walks the bids
  const Level* lv = bk.levels + (size_t)s * L;
  const bool done = walk_window(bk, s, bid, bid ? min(st.best_bid, L - 1) : max(st.best_ask, 0), bid ? 0 : L - 1,
                                [&](int l, bool gate) {
                                  Level x;
                                  x.total = 0;
                                  x.head = x.tail = NIL;
                                  if (gate) x = lv[l];
                                  return pv_block(bk, w, st.base + l, x.total, x.head, x.tail);
                                });
  if (done) return;
  FarSide fs;
  if (!far_side(bk, s, bid ? 0u : 1u, bid ? st.nfar[0] : st.nfar[1], fs)) w.bad = true;
  walk_far(fs, fs.n, [&](const FarLevel& f) { return pv_block(bk, w, f.price, f.total, f.head, f.tail); });
}

__global__ __launch_bounds__(PV_WAVES * 64) void k_order_preview(BookDev bk, PreviewReq rq) {
  const int lane = lane_id();
  const uint32_t qi = blockIdx.x * PV_WAVES + (threadIdx.x >> 6);
  if (qi >= rq.n) return;  // (whole waves leave: the kernel has no block barrier)
  const uint32_t s = rl32(rq.sym[qi], 0);
  const uint32_t kd = rl32((uint32_t)rq.kind[qi], 0);
  const long long px = rli64(rq.px[qi], 0);
  const int qty = rli32(rq.qty[qi], 0);
  const uint32_t side = kd & 3u, tif = kd_tif(kd);
  const bool market = (kd & 4u) != 0u;
  me_preview o{};
  bool bad = false;
  uint32_t rj = ME_RJ_NONE;
  if (s >= bk.S)
    rj = ME_RJ_BAD_SYMBOL;
  else if (qty <= 0)
    rj = ME_RJ_BAD_QTY;
  else if (side != (uint32_t)ME_SIDE_BUY && side != (uint32_t)ME_SIDE_SELL)
    rj = ME_RJ_BAD_SIDE;
  else if (tif == (uint32_t)ME_TIF_POST_ONLY && market)
    rj = ME_RJ_BAD_TIF;
  if (rj != ME_RJ_NONE) {
    o.status = ME_ST_REJECTED;
    o.reason = (uint8_t)rj;
    o.remaining_qty = rj == ME_RJ_BAD_SYMBOL || rj == ME_RJ_BAD_QTY ? 0 : qty;
  } else {
    PvWalk w;
    for (bool again = false;; again = true) {  // (a second time only for a fillable FOK: the walk that counts)
      w = PvWalk{};
      w.limit = px;
      w.buy = side == (uint32_t)ME_SIDE_BUY;
      w.market = market;
      w.want = tif == (uint32_t)ME_TIF_POST_ONLY ? 0 : qty;
      w.count = again || tif == (uint32_t)ME_TIF_GTC || tif == (uint32_t)ME_TIF_IOC;
      pv_walk(bk, s, w);
      if (again || tif != (uint32_t)ME_TIF_FOK || w.want != 0 || w.bad) break;
    }
    const bool has_opp = w.has_opp;
    const long long opp_px = w.opp_px;
    const bool crosses = has_opp && (market || (w.buy ? opp_px <= px : opp_px >= px));
    const bool exec = w.count;  // w describes an execution
    bad = w.bad;
    o.remaining_qty = qty;
    if (tif == (uint32_t)ME_TIF_POST_ONLY) {
      o.status = crosses ? ME_ST_REJECTED : ME_ST_NEW;
      o.reason = crosses ? ME_RJ_WOULD_CROSS : ME_RJ_NONE;
      if (!crosses) o.flags |= ME_PV_RESTS;
    } else if (!exec) {  // a killed FOK
      o.status = ME_ST_CANCELED;
    } else {
      const int rem = (int)w.want;
      o.filled_qty = qty - rem;
      o.remaining_qty = rem;
      o.fill_count = w.fills;
      o.levels = w.levels;
      o.first_price_q4 = w.first_px;
      o.last_price_q4 = w.last_px;
      o.notional_hi = w.nhi;
      o.notional_lo = w.nlo;
      if (market || tif != (uint32_t)ME_TIF_GTC) {
        o.status = rem == 0 ? ME_ST_FILLED : ME_ST_CANCELED;
      } else {
        o.status = rem == 0 ? ME_ST_FILLED : (rem < qty ? ME_ST_PARTIALLY_FILLED : ME_ST_NEW);
        if (rem > 0) o.flags |= ME_PV_RESTS;
      }
    }
    if (has_opp) {
      o.flags |= ME_PV_HAS_OPP;
      o.opp_price_q4 = opp_px;
    }
    if (crosses) o.flags |= ME_PV_CROSSES;
  }
  if (lane == 0) {
    if (bad) atomicOr(rq.err, 1u);
    rq.out[qi] = o;
  }
}

hipError_t launch_order_preview(hipStream_t st, const BookDev& bk, const PreviewReq& rq) {
  if (!rq.n) return hipSuccess;
  hipLaunchKernelGGL(k_order_preview, dim3((rq.n + PV_WAVES - 1u) / PV_WAVES), dim3(PV_WAVES * 64), 0, st, bk, rq);
  return hipGetLastError();
}

// ---- mass cancel (me_mass_cancel, include/me_engine.h) -----------------------------------------------
// k_purge<REMOVE>: k_book_snapshot's shape, one 1024-thread workgroup per (request, side), over ALL of the
// side's levels, in passes of up to PURGE_P. The window levels of a pass come from the occupancy words, not
// from the totals (a window has up to 2^20 levels): every thread takes one word of the side's range, going
// outward from the best level; a block scan of the popcounts places the words' levels in the pass, and the
// words that still fit it — a prefix, whole words only — are taken; the cursor stops at the first that does
// not. Windows of L <= 128 form their (at most two) words from the totals, as the scans do. (The two block
// gathers stay apart because their units differ: k_book_snapshot compacts level totals, 1,024 levels a round,
// and stops inside a round at `depth`; this one places whole occupancy words, 65,536 levels a round. What
// follows a gather is shared: far_nth, chain_live, chunk_entries, me_bookread.hpp.) Far levels
// follow once the window is exhausted, best (last) first. Every thread then walks the chains of two levels
// of the pass to count their live slots, and a block scan turns the counts into output offsets.
//   REMOVE = false writes the side's count and nothing else. REMOVE = true walks each chain a second time:
// it writes the live slots in slot order to out, zeroes all 16 quantities of every chunk (a freed chunk is
// zero in HBM before it is listed anywhere), pushes the whole chain onto the symbol's free list (an atomic
// exchange of free_head with the chain's head, then tail.next = the old head: both sides of a symbol may
// push at once, nothing pops during the launch), writes Level{0, NIL, NIL} and clears the level's occ bit.
// Thread 0 ends the side: best_bid = -1 / best_ask = L, nfar = 0, and the removed count off the symbol's
// resting count and ST_RESTING (atomics: the other side's workgroup does the same). FarDir, fcache, nfree,
// the seq ring and the old-order table are not touched: their entries are verified against the slot, whose
// quantity is now 0. A chain that leaves [0, nchunks), takes more than nchunks steps or ends before its
// tail sets the error word and is left alone; the host runs the count pass first and removes nothing then.
constexpr int PURGE_P = 2048;  // levels per pass (LDS: 20 B each)

__device__ __forceinline__ unsigned long long purge_occ_word(const BookDev& bk, const Level* lv,
                                                             const unsigned long long* oc, int wi) {
  if (bk.L > 128u) return oc[wi];
  unsigned long long w = 0;
  for (int b = 0; b < 64; ++b) {
    const int l = wi * 64 + b;
    if (l < (int)bk.L && lv[l].total > 0) w |= 1ull << b;
  }
  return w;
}

template <bool REMOVE>
__global__ __launch_bounds__(SNAP_T) void k_purge(BookDev bk, PurgeReq rq) {
  __shared__ long long p_price[PURGE_P];
  __shared__ uint32_t p_head[PURGE_P];  // NIL: nothing to walk (an empty or a corrupt level)
  __shared__ uint32_t p_tail[PURGE_P];
  __shared__ int p_lvl[PURGE_P];        // window level, -1 for a far level
  __shared__ uint32_t wsum[SNAP_T / 64];
  __shared__ int s_cur;                 // window cursor: the next occ word to look at
  __shared__ uint32_t s_far;            // far levels taken so far
  __shared__ uint32_t s_np;             // levels in this pass
  __shared__ uint32_t s_first;          // first thread of a round whose word did not fit the pass
  const int tid = threadIdx.x;
  const uint32_t q = blockIdx.x >> 1, side = blockIdx.x & 1u;
  const size_t reg = blockIdx.x;
  const bool bid = side == 0u;
  const uint32_t s = rq.sym[q];
  if (!((rq.sides[q] >> side) & 1u) || s >= bk.S) {  // (ME_SIDE_BUY = 1, ME_SIDE_SELL = 2: bit `side`)
    if (!REMOVE && tid == 0) rq.cnt[reg] = 0ull;
    return;
  }
  if (REMOVE && rq.cnt[reg] == 0ull) return;  // the count pass found the side empty: its hints say so already
  const int L = (int)bk.L;
  const SymState st = bk.sym[s];
  Level* lv = bk.levels + (size_t)s * L;
  unsigned long long* oc = bk.occ + (size_t)s * bk.Lwords;
  FarSide fs;
  if (!far_side(bk, s, side, st.nfar[side], fs)) {
    if (tid == 0) {
      atomicOr(rq.err, 1u);
      if (!REMOVE) rq.cnt[reg] = 0ull;
    }
    return;
  }
  // the side's window levels [lo, hi] (none: lo > hi), words [wlo, whi]
  const int lo = bid ? 0 : max(st.best_ask, 0);
  const int hi = bid ? min(st.best_bid, L - 1) : L - 1;
  const int wlo = lo >> 6, whi = hi >> 6;
  if (tid == 0) {
    s_cur = lo <= hi ? (bid ? whi : wlo) : (bid ? wlo - 1 : whi + 1);
    s_far = 0;
  }
  __syncthreads();
  const unsigned long long obase = REMOVE ? rq.off[reg] : 0ull;
  unsigned long long norders = 0;
  for (;;) {
    if (tid == 0) s_np = 0;
    __syncthreads();
    // ---- this pass's window levels
    for (;;) {
      const int cur = s_cur;
      const uint32_t np = s_np;
      if (bid ? cur < wlo : cur > whi) break;
      __syncthreads();  // everyone holds cur and np
      if (tid == 0) s_first = SNAP_T;
      const int wi = bid ? cur - tid : cur + tid;
      unsigned long long word = 0;
      if (wi >= wlo && wi <= whi) word = purge_occ_word(bk, lv, oc, wi) & word_range(wi, lo, hi);
      const uint32_t pc = (uint32_t)__popcll(word);
      uint32_t all = 0;
      const uint32_t pos = snap_block_excl_scan(pc, wsum, all);
      // pos + pc ascends with the thread: the words taken are a prefix of the round
      if (np + pos + pc > (uint32_t)PURGE_P) {
        atomicMin(&s_first, (uint32_t)tid);
      } else if (pc) {
        atomicMax(&s_np, np + pos + pc);
        uint32_t at = np + pos;
        for (unsigned long long m = word; m;) {  // in priority order: bids from the top bit down
          const int b = bid ? 63 - __builtin_clzll(m) : __builtin_ctzll(m);
          m &= ~(1ull << b);
          p_lvl[at++] = wi * 64 + b;
        }
      }
      __syncthreads();
      const uint32_t first = s_first;
      if (tid == 0) s_cur = bid ? cur - (int)first : cur + (int)first;
      __syncthreads();
      if (first < (uint32_t)SNAP_T) break;  // the pass is full
    }
    const uint32_t nw = s_np;
    for (uint32_t i = tid; i < nw; i += SNAP_T) {
      const int l = p_lvl[i];
      const Level x = lv[l];
      p_price[i] = st.base + l;
      p_head[i] = x.total > 0 ? x.head : NIL;  // (the total decides, as in the scans)
      p_tail[i] = x.tail;
    }
    // ---- far levels, once the window is exhausted
    const bool win_done = bid ? s_cur < wlo : s_cur > whi;
    const uint32_t fr = s_far;
    const uint32_t nf = win_done ? min((uint32_t)PURGE_P - nw, fs.n - fr) : 0u;
    for (uint32_t j = tid; j < nf; j += SNAP_T) {
      const FarLevel f = far_nth(fs, fr + j);
      p_lvl[nw + j] = -1;
      p_price[nw + j] = f.price;
      p_head[nw + j] = f.total > 0 ? f.head : NIL;
      p_tail[nw + j] = f.tail;
    }
    __syncthreads();
    if (tid == 0) s_far = fr + nf;
    const uint32_t np = nw + nf;
    if (np == 0) break;
    // ---- count every level's live orders (two levels per thread), scan
    uint32_t cnt[PURGE_P / SNAP_T];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < PURGE_P / SNAP_T; ++k) {
      const uint32_t i = (uint32_t)tid * (PURGE_P / SNAP_T) + k;
      uint32_t c = 0;
      if (i < np && !chain_live(bk, p_head[i], p_tail[i], c)) {  // a broken chain is left alone
        atomicOr(rq.err, 1u);
        p_head[i] = NIL;  // (this thread's own entry)
        c = 0;
      }
      cnt[k] = c;
      mine += c;
    }
    uint32_t pass_total = 0;
    uint32_t off = snap_block_excl_scan(mine, wsum, pass_total);
    if (REMOVE) {
#pragma unroll
      for (int k = 0; k < PURGE_P / SNAP_T; ++k) {
        const uint32_t i = (uint32_t)tid * (PURGE_P / SNAP_T) + k;
        if (i < np && p_head[i] != NIL) {
          unsigned long long o = obase + norders + off;
          const uint32_t head = p_head[i], tail = p_tail[i];
          uint32_t ch = head;
          for (;;) {  // (the count walk went head -> tail inside [0, nchunks))
            Chunk& c = bk.chunks[ch];
            const uint32_t nxt = c.hdr.next;
            o = chunk_entries(c, p_price[i], bid, rq.out, o, rq.cap);
            int4* qv = reinterpret_cast<int4*>(c.qty);
#pragma unroll
            for (int u = 0; u < 4; ++u) qv[u] = make_int4(0, 0, 0, 0);
            if (ch == tail) break;
            ch = nxt;
          }
          const uint32_t old = atomicExch(&bk.sym[s].free_head, head);
          bk.chunks[tail].hdr.next = old;
          const int l = p_lvl[i];
          if (l >= 0) {
            Level z;
            z.total = 0;
            z.head = NIL;
            z.tail = NIL;
            lv[l] = z;
            atomicAnd(&oc[l >> 6], ~(1ull << (l & 63)));
          }
        }
        off += cnt[k];
      }
    }
    norders += pass_total;
    __syncthreads();
  }
  if (tid == 0) {
    if (!REMOVE) {
      rq.cnt[reg] = norders;
    } else {
      SymState* ss = bk.sym + s;
      if (bid) {
        ss->best_bid = -1;
        ss->nfar[0] = 0;
      } else {
        ss->best_ask = L;
        ss->nfar[1] = 0;
      }
      atomicSub(&ss->resting, (uint32_t)norders);
      atomicAdd(&bk.stats[ST_RESTING], 0ull - norders);
    }
  }
}

hipError_t launch_purge(hipStream_t st, const BookDev& bk, const PurgeReq& rq, bool remove) {
  if (!rq.n) return hipSuccess;
  if (remove)
    hipLaunchKernelGGL(k_purge<true>, dim3(rq.n * 2), dim3(SNAP_T), 0, st, bk, rq);
  else
    hipLaunchKernelGGL(k_purge<false>, dim3(rq.n * 2), dim3(SNAP_T), 0, st, bk, rq);
  return hipGetLastError();
}

hipError_t launch_book_snapshot(hipStream_t st, const BookDev& bk, const SnapReq& rq) {
  if (!rq.nsym || !rq.depth) return hipSuccess;
  hipLaunchKernelGGL(k_book_snapshot, dim3(rq.nsym * 2), dim3(SNAP_T), 0, st, bk, rq);
  return hipGetLastError();
}

}  // namespace me
