// me_side.hpp — the pipeline's two side jobs as device code: the bucket job sorts a
// batch's records into per-symbol buckets, the tape job copies a group's fills from scratch to the tape.
// Shared by their two users: the side waves of k_match_reg<false> (me_match_reg.hip aux_jobs) and the
// side kernels k_side / k_side_fill (me_side.hip). Templates over the user's argument block GA, held in
// LDS and read where used (ldsu / ldsg, me_wave.hpp); they touch G.ax and G.bk.err only.
#pragma once
#include <hip/hip_runtime.h>

#include "me_layout.hpp"
#include "me_wave.hpp"

namespace me {

// (pipelined path: no fill start of its own — the tape job reads a record's scratch start from its
// result's tape_offset, see aux_tape_tile)
__device__ __forceinline__ void reject_bad_at(gptr<me_order_result> res, uint32_t i) {
  me_order_result r;
  r.filled_qty = 0;
  r.remaining_qty = 0;
  r.fill_count = 0;
  r.tape_offset = 0;
  r.status = ME_ST_REJECTED;
  r.reason = ME_RJ_BAD_SYMBOL;
  r.pad[0] = r.pad[1] = 0;
  res[i] = r;
}

// Bucket job: records [r0, r1) of bucket job j, one returning atomic per record on its bin's counter.
template <class GA>
__device__ __forceinline__ void aux_bucket(const GA& G, uint32_t j, uint32_t r0, uint32_t r1) {
  const int lane = lane_id();
  const AuxBucket& J = G.ax.b[j];
  const gptr<const uint32_t> sym = ldsg(J.sym);
  const gptr<const uint64_t> seq = ldsg(J.seq);
  const gptr<const int64_t> px = ldsg(J.px);
  const gptr<const int32_t> qty = ldsg(J.qty);
  const gptr<const uint8_t> kind = ldsg(J.kind);
  const gptr<uint32_t> bcnt = ldsg(J.bcnt);
  const gptr<BkRec> brec = ldsg(J.b_rec);
  const uint32_t S = ldsu(G.ax.S);
  const gptr<me_order_result> bres = ldsg(J.bres);
  bool order_ok = true;
  for (uint32_t i0 = r0; i0 < r1; i0 += 64) {
    const uint32_t i = i0 + (uint32_t)lane;
    if (i < r1) {
      const uint32_t k = kind[i];
      // API precondition (the seq ring relies on it): seqs ascending through the batch (seq_follows)
      if (i > 0) order_ok &= seq_follows(seq[i - 1], seq[i], k);
      const uint32_t b = min(sym[i], S);
      if (b == S) {  // unknown symbol: rejected here, never bucketed (the batch's result set is free)
        reject_bad_at(bres, i);
        continue;
      }
      const uint64_t sq = seq[i];  // the payload loads are in flight while the atomic returns
      const int64_t p = px[i];
      const int32_t q = qty[i];
      const uint32_t r = atomicAdd(&bcnt[(size_t)b * BK_CNT_STRIDE], 1u);
      if (r < (uint32_t)BK_CAP) {
        const size_t d = (size_t)b * BK_CAP + r;
        brec[d].seq = sq;
        brec[d].px = p;
        brec[d].qty = q;
        brec[d].ok = i | ((k & BK_KIND_BITS) << BK_KIND_SHIFT);
      }
    }
  }
  if (__ballot(!order_ok) && lane == 0) atomicOr(ldsg(G.bk.err), ERR_SEQ_ORDER);
}

// Tape job j, one TILE_TAPE-record tile per wave: tape offsets of its records and the copy of their
// fills from scratch into the batch's tape (ordered by taker seq).
template <class GA>
__device__ __forceinline__ void aux_tape_tile(const GA& G, uint32_t jb, uint32_t t, uint32_t ntiles,
                                              uint32_t tn) {
  const int lane = lane_id();
  const AuxTape& J = G.ax.t[jb];
  const gptr<const uint32_t> tile_sum = ldsg(J.tile_sum);
  const gptr<me_order_result> res = ldsg(J.res);
  const gptr<const me_fill> scratch = ldsg(J.scratch);
  const gptr<me_fill> tape = ldsg(J.tape);
  const gptr<me_order_result> hres = ldsg(J.hres);
  const bool host = hres != nullptr;  // a host batch: soft tape cap, results and scratch starts kept
  const unsigned long long cap = ldsu(J.cap);
  long long acc = 0;  // fills of the earlier tiles
  for (uint32_t u = (uint32_t)lane; u < t; u += 64) acc += tile_sum[u];
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  const unsigned long long base = (unsigned long long)rli64(acc, 0);
  const uint32_t r0 = t * TILE_TAPE;
  const uint32_t cnt = min((uint32_t)TILE_TAPE, tn - r0);
  uint32_t c[TILE_TAPE / 64], src[TILE_TAPE / 64];
  long long loc = 0;
#pragma unroll
  for (int k = 0; k < TILE_TAPE / 64; ++k) {  // lane holds records 4*lane .. 4*lane+3 of the tile
    const uint32_t j = (uint32_t)(lane * (TILE_TAPE / 64) + k);
    // the match job left the record's scratch start in tape_offset (same line as fill_count)
    c[k] = j < cnt ? res[r0 + j].fill_count : 0u;
    src[k] = j < cnt ? res[r0 + j].tape_offset : 0u;
    loc += c[k];
  }
  const long long incl = wave_incl_scan(loc);
  const uint32_t total = (uint32_t)rli64(incl, 63);
  uint32_t o = (uint32_t)(incl - loc);
#pragma unroll
  for (int k = 0; k < TILE_TAPE / 64; ++k) {
    const uint32_t j = (uint32_t)(lane * (TILE_TAPE / 64) + k);
    if (j < cnt) res[r0 + j].tape_offset = (uint32_t)(base + o);
    o += c[k];
  }
  if (host) {  // the slot's copy of the final results; the scratch starts stay for me_collect's spill
    const gptr<uint32_t> fst = ldsg(J.fstart);
    uint32_t o3 = (uint32_t)(incl - loc);
#pragma unroll
    for (int k = 0; k < TILE_TAPE / 64; ++k) {
      const uint32_t j = (uint32_t)(lane * (TILE_TAPE / 64) + k);
      if (j < cnt) {
        me_order_result r = res[r0 + j];  // written by the match job of an earlier launch
        r.tape_offset = (uint32_t)(base + o3);
        hres[r0 + j] = r;
        fst[r0 + j] = src[k];
      }
      o3 += c[k];
    }
  } else if (base + total > cap) {
    if (lane == 0) atomicOr(ldsg(G.bk.err), ERR_SCRATCH_OOM);
    return;
  }
  // The tile's fills are one contiguous tape run [base, base + total): lane i copies fill f0 + i, found
  // by a binary search over the lanes' exclusive offsets (one record per lane), so every store
  // instruction writes 64 consecutive 32-B records — whole lines in HBM, full-size PCIe writes when
  // the tape is a host slot's pinned buffer.
  static_assert(TILE_TAPE == 64, "one record per lane");
  {
    const uint32_t ex = (uint32_t)(incl - loc);
    for (uint32_t f0 = 0; f0 < total; f0 += 64) {
      const uint32_t f = f0 + (uint32_t)lane;
      int lo = 0;  // last lane whose exclusive offset is <= f: the record that owns fill f
#pragma unroll
      for (int step = 32; step >= 1; step >>= 1) {
        const uint32_t e = (uint32_t)__shfl((int)ex, min(lo + step, 63), 64);
        if (lo + step < 64 && e <= f) lo += step;
      }
      const uint32_t s0 = (uint32_t)__shfl((int)src[0], lo, 64);
      const uint32_t e0 = (uint32_t)__shfl((int)ex, lo, 64);
      if (f < total && base + f < cap) tape[base + f] = scratch[s0 + (f - e0)];
    }
  }
  if (t == ntiles - 1 && lane == 0) {
    *ldsg(J.tape_count) = base + total;
    atomicAdd(ldsg(G.ax.fills_acc), base + total);
    if (host) *ldsg(J.err_out) = __hip_atomic_load(ldsg(G.bk.err), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace me
