// me_side.hip — k_side and k_side_fill: the pipeline's side jobs (me_side.hpp) in launches of their own,
// where no match job runs beside them — on a stream of their own beside the grouped walk, as the
// pipeline's fill and drain launches, and as the early fill. Compiled once, with the
// register kernel's flags (Makefile REGFLAGS).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "me_launch.hpp"
#include "me_layout.hpp"
#include "me_side.hpp"
#include "me_wave.hpp"

namespace me {

// ---- launches with no match job: the side jobs alone ------------------------------------------
// The pipeline's first launch of a run (bucket only) and its last (tape only) have no matching waves to
// hide behind: in k_match_reg they ran on its 4 side waves per CU (one 145-KB workgroup per CU), 74 and
// 87 us for a 20-batch group at config 2. k_side carries only the side jobs' arguments in LDS.
//  * bucket: one workgroup per SB_REC records of a batch counts its records per symbol in LDS, then
//    reserves each symbol's run with ONE returning global atomic (device-scope atomics execute at the
//    memory side, one request each: one per record capped the fill launch at ~20 G records/s), then
//    writes the records at run + rank. A bucket's order is free (the match wave sorts by batch index).
//    Needs (S + 1) counters in LDS; above SB_SMAX symbols the waves bucket 64-record blocks with one
//    atomic per record as the pipelined launch does.
//  * tape: tiles dealt round-robin to the tape waves over a list flattened across the group's batches.
struct SideArgs {
  struct {
    uint32_t* err;
  } bk;
  AuxDev ax;
};
#ifndef ME_SIDE_THREADS
#define ME_SIDE_THREADS 512
#endif
#ifndef ME_SB_REC
#define ME_SB_REC 2048  // records per bucket workgroup: same box, config 2's driver shape 1,818-1,836M at 4,096,
                        // 1,911-1,918M at 2,048, 1,804-1,820M at 1,024; 640 steps 2,561 / 2,604 / 2,572M; config
                        // 3 1,301 / 1,317M (profiles/r4/sb) — the group's walk + resolve 549 -> 514 us
#endif
constexpr int SIDE_THREADS = ME_SIDE_THREADS;
constexpr int SIDE_WAVES = SIDE_THREADS / 64;
#ifndef ME_TAPE_XCD
#define ME_TAPE_XCD 1  // tape tiles: each half of a batch's tape on one XCD (1) or dealt over all (0); profiles/r5/tx
#endif
constexpr uint32_t SB_REC = ME_SB_REC;             // records per bucket workgroup
constexpr uint32_t SB_PER = SB_REC / SIDE_THREADS;  // records per thread
constexpr uint32_t SB_SMAX = 16383;                // symbols bucketed through an LDS histogram (64 KB)

// Units [off, off + cnt) of a list flattened over batches, dealt round-robin to waves: wave a's first.
__device__ __forceinline__ uint32_t flat_first(uint32_t off, uint32_t a, uint32_t A) {
  return off + (a + A - off % A) % A;
}

// The early fill's launch (me_engine.cpp early_fill): bucket jobs only, at most FILL_NB of them — a
// ~0.8-KB argument block instead of SideArgs' ~5.7 KB (the host's launch call is the early fill's cost:
// ~13 us per launch with SideArgs).
constexpr uint32_t FILL_NB = 8;
struct FillArgs {
  struct {
    uint32_t* err;
  } bk;
  struct {
    uint32_t S, nb;
    AuxBucket b[FILL_NB];
  } ax;
};

// Bucket records [r0, r1) of bucket job j with a workgroup histogram (cnt: S + 1 LDS counters).
template <class GA>
__device__ __forceinline__ void side_bucket_wg(const GA& G, uint32_t j, uint32_t r0, uint32_t r1, uint32_t* cnt) {
  const uint32_t tid = threadIdx.x;
  const AuxBucket& J = G.ax.b[j];
  const uint32_t S = ldsu(G.ax.S);
  const gptr<const uint32_t> sym = ldsg(J.sym);
  const gptr<const uint64_t> seq = ldsg(J.seq);
  const gptr<const int64_t> px = ldsg(J.px);
  const gptr<const int32_t> qty = ldsg(J.qty);
  const gptr<const uint8_t> kind = ldsg(J.kind);
  const gptr<uint32_t> bcnt = ldsg(J.bcnt);
  const gptr<BkRec> brec = ldsg(J.b_rec);
  const gptr<me_order_result> bres = ldsg(J.bres);
  for (uint32_t b = tid; b <= S; b += SIDE_THREADS) cnt[b] = 0u;
  {  // the tile sums of this record range, and the batch's scratch top, start at zero
    const gptr<uint32_t> z = ldsg(J.zero_tile_sum);
    const uint32_t t1 = min((r1 + TILE_TAPE - 1) / TILE_TAPE, ldsu(J.zero_tiles));
    for (uint32_t t = r0 / TILE_TAPE + tid; t < t1; t += SIDE_THREADS) z[t] = 0u;
    if (r0 == 0 && tid == 0) *ldsg(J.zero_top) = 0ull;
  }
  __syncthreads();
  uint32_t bin[SB_PER], rank[SB_PER];
  uint64_t sq[SB_PER];
  int64_t p[SB_PER];
  int32_t q[SB_PER];
  uint32_t k8[SB_PER];
  bool order_ok = true;
#pragma unroll
  for (uint32_t k = 0; k < SB_PER; ++k) {
    const uint32_t i = r0 + k * SIDE_THREADS + tid;
    bin[k] = S;
    if (i < r1) {
      bin[k] = min(sym[i], S);
      sq[k] = seq[i];
      p[k] = px[i];
      q[k] = qty[i];
      k8[k] = kind[i];
      // API precondition (the seq ring relies on it): seqs ascending through the batch (seq_follows)
      if (i > 0) order_ok &= seq_follows(seq[i - 1], sq[k], k8[k]);
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < SB_PER; ++k) {
    const uint32_t i = r0 + k * SIDE_THREADS + tid;
    if (i < r1 && bin[k] == S) reject_bad_at(bres, i);  // unknown symbol: rejected here, never bucketed
    if (bin[k] < S) rank[k] = atomicAdd(&cnt[bin[k]], 1u);
  }
  if (__ballot(!order_ok) && lane_id() == 0) atomicOr(ldsg(G.bk.err), ERR_SEQ_ORDER);
  __syncthreads();
  for (uint32_t b = tid; b < S; b += SIDE_THREADS) {
    const uint32_t c = cnt[b];
    if (c) cnt[b] = atomicAdd(&bcnt[(size_t)b * BK_CNT_STRIDE], c);
  }
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < SB_PER; ++k) {
    if (bin[k] >= S) continue;
    const uint32_t r = cnt[bin[k]] + rank[k];
    if (r < (uint32_t)BK_CAP) {
      const uint32_t i = r0 + k * SIDE_THREADS + tid;
      const size_t d = (size_t)bin[k] * BK_CAP + r;
      brec[d].seq = sq[k];
      brec[d].px = p[k];
      brec[d].qty = q[k];
      brec[d].ok = i | ((k8[k] & BK_KIND_BITS) << BK_KIND_SHIFT);
    }
  }
}

// Grid: 8 x the most units a batch has; batch j on the blocks b = j (mod 8), its units in turn (k_side's
// xseq form, one batch per XCD).
__global__ __launch_bounds__(SIDE_THREADS) void k_side_fill(FillArgs args) {
  __shared__ FillArgs G;
  extern __shared__ uint32_t side_cnt[];
  static_assert(sizeof(FillArgs) % 8 == 0, "FillArgs copy");
  for (uint32_t i = threadIdx.x; i < sizeof(FillArgs) / 8; i += SIDE_THREADS)
    reinterpret_cast<unsigned long long*>(&G)[i] = reinterpret_cast<const unsigned long long*>(&args)[i];
  __syncthreads();
  const uint32_t nb = ldsu(G.ax.nb), x = blockIdx.x % 8u, k = blockIdx.x / 8u;
  for (uint32_t j = x; j < nb; j += 8) {
    const uint32_t n = ldsu(G.ax.b[j].n), r0 = k * SB_REC;
    if (r0 >= n) continue;  // (uniform over the workgroup)
    side_bucket_wg(G, j, r0, min(n, r0 + SB_REC), side_cnt);
    __syncthreads();  // the LDS counters are zeroed again by the next batch
  }
}

// Grid: [0, nbu) bucket workgroups (histogram path; 0 on the per-record path), then tape workgroups.
__global__ __launch_bounds__(SIDE_THREADS) void k_side(SideArgs args, uint32_t nbu) {
  __shared__ SideArgs G;
  extern __shared__ uint32_t side_cnt[];
  static_assert(sizeof(SideArgs) % 8 == 0, "SideArgs copy");
  for (uint32_t i = threadIdx.x; i < sizeof(SideArgs) / 8; i += SIDE_THREADS)
    reinterpret_cast<unsigned long long*>(&G)[i] = reinterpret_cast<const unsigned long long*>(&args)[i];
  __syncthreads();
  const int lane = lane_id();
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nb = ldsu(G.ax.nb);
  if (blockIdx.x < nbu) {  // histogram bucket unit: batch j, records [u * SB_REC, ...)
    // Blocks b and b + 8 share an XCD (round-robin placement; speed only): every unit of batch j runs
    // on blocks b = j (mod 8), so the runs its workgroups write side by side into one bucket array
    // meet in one L2 and leave it as whole lines, not as partial lines from several XCDs.
    const uint32_t x = blockIdx.x % 8u, k = blockIdx.x / 8u;
    if (ldsu(G.ax.xseq)) {
      // beside a walk (off the critical path): unit k of each of the XCD's batches in turn, so one
      // batch's buckets (1.5 MB at config 2) are being filled per L2 at a time, not four batches' 6 MB
      // whose partial lines the 4-MB L2 evicts before the later units complete them (profiles/r4/xs)
      for (uint32_t j = x; j < nb; j += 8) {
        const uint32_t n = ldsu(G.ax.b[j].n), r0 = k * SB_REC;
        if (r0 >= n) continue;  // (uniform over the workgroup)
        side_bucket_wg(G, j, r0, min(n, r0 + SB_REC), side_cnt);
        __syncthreads();  // the LDS counters are zeroed again by the next batch
      }
      return;
    }
    uint32_t off = 0;
    for (uint32_t j = x; j < nb; j += 8) {
      const uint32_t n = ldsu(G.ax.b[j].n), nu = (n + SB_REC - 1) / SB_REC;
      if (k < off + nu) {
        const uint32_t r0 = (k - off) * SB_REC;
        side_bucket_wg(G, j, r0, min(n, r0 + SB_REC), side_cnt);
        return;
      }
      off += nu;
    }
    return;
  }
  const uint32_t A = (gridDim.x - nbu) * SIDE_WAVES, a = (blockIdx.x - nbu) * SIDE_WAVES + wv;
  uint32_t off = 0;
  if (nbu == 0) {  // per-record bucket path (too many symbols for the LDS histogram)
    for (uint32_t j = 0; j < nb; ++j) {
      const AuxBucket& J = G.ax.b[j];
      const uint32_t zt = ldsu(J.zero_tiles);
      const gptr<uint32_t> z = ldsg(J.zero_tile_sum);
      for (uint32_t i = a * 64u + (uint32_t)lane; i < zt; i += A * 64u) z[i] = 0u;
      if (a == 0 && lane == 0) *ldsg(J.zero_top) = 0ull;
      const uint32_t n = ldsu(J.n), nblk = (n + 63u) / 64u;
      for (uint32_t u = flat_first(off, a, A); u < off + nblk; u += A) {
        const uint32_t r0 = (u - off) * 64u;
        aux_bucket(G, j, r0, min(n, r0 + 64u));
      }
      off += nblk;
    }
  }
  const uint32_t nt = ldsu(G.ax.nt);
#if ME_TAPE_XCD
  // Each half of a batch's tape on one XCD (blocks b = x mod 8 under round-robin placement; speed only): a
  // 128-B line of a symbol's scratch slab holds fills of takers ~16 tiles apart, so the tiles that read it
  // meet in one L2 instead of fetching the line once per XCD. Halves, not batches, keep the XCDs balanced.
  if (gridDim.x - nbu >= 8u) {
    const uint32_t x = blockIdx.x % 8u;
    const uint32_t b0 = nbu + (x + 8u - nbu % 8u) % 8u;  // the first tape block on XCD x
    const uint32_t AX = ((gridDim.x - b0 + 7u) / 8u) * SIDE_WAVES, ax = ((blockIdx.x - b0) / 8u) * SIDE_WAVES + wv;
    for (uint32_t v = x; v < 2u * nt; v += 8u) {
      const uint32_t j = v >> 1, h = v & 1u;
      const uint32_t tn = ldsu(G.ax.t[j].tn);
      const uint32_t ntiles = (tn + TILE_TAPE - 1) / TILE_TAPE, half = (ntiles + 1u) / 2u;
      const uint32_t t0 = h * half, t1 = min(ntiles, t0 + half);
      for (uint32_t t = t0 + ax; t < t1; t += AX) aux_tape_tile(G, j, t, ntiles, tn);
    }
    return;
  }
#endif
  off = 0;
  for (uint32_t j = 0; j < nt; ++j) {
    const uint32_t tn = ldsu(G.ax.t[j].tn);
    const uint32_t ntiles = (tn + TILE_TAPE - 1) / TILE_TAPE;
    for (uint32_t u = flat_first(off, a, A); u < off + ntiles; u += A) aux_tape_tile(G, j, u - off, ntiles, tn);
    off += ntiles;
  }
}


// ---- host entries -----------------------------------------------------------------------------
// The early fill (bucket jobs of at most FILL_NB batches, symbols within the LDS histogram); done = false:
// not this launch's shape, nothing was launched (the caller uses launch_side).
hipError_t launch_side_fill(hipStream_t st, uint32_t* err, const AuxDev& ax, bool& done) {
  done = false;
  if (ax.nb == 0 || ax.nb > FILL_NB || ax.S > SB_SMAX || ax.nt) return hipSuccess;
  FillArgs FA{};
  FA.bk.err = err;
  FA.ax.S = ax.S;
  FA.ax.nb = ax.nb;
  uint32_t per = 0;
  for (uint32_t j = 0; j < ax.nb; ++j) {
    FA.ax.b[j] = ax.b[j];
    per = max(per, (ax.b[j].n + SB_REC - 1) / SB_REC);
  }
  hipLaunchKernelGGL(k_side_fill, dim3(8u * max(per, 1u)), dim3(SIDE_THREADS), (size_t)(ax.S + 1) * sizeof(uint32_t),
                     st, FA);
  done = true;
  return hipGetLastError();
}

// The side jobs of ax, all waves on them: k_side. ev0 / ev1 (optional) bracket the kernel.
hipError_t launch_side(hipStream_t st, uint32_t* err, const AuxDev& ax, hipEvent_t ev0, hipEvent_t ev1) {
  if (ax.nb > (uint32_t)ME_GMAX || ax.nt > (uint32_t)ME_GMAX) return hipErrorInvalidValue;
  SideArgs SA{};
  SA.bk.err = err;
  SA.ax = ax;
  uint32_t nbr = 0, ntr = 0;
  for (uint32_t j = 0; j < ax.nb; ++j) nbr += ax.b[j].n;
  for (uint32_t j = 0; j < ax.nt; ++j) ntr += ax.t[j].tn;
  const bool hist = ax.S <= SB_SMAX;
  uint32_t nbu = 0;
  if (hist) {  // 8 x the most units any XCD's batches have (batch j on blocks = j mod 8)
    uint32_t per[8] = {};
    for (uint32_t j = 0; j < ax.nb; ++j) {
      const uint32_t nu = (ax.b[j].n + SB_REC - 1) / SB_REC;
      per[j % 8] = ax.xseq ? max(per[j % 8], nu) : per[j % 8] + nu;  // xseq: the batches in turn
    }
    for (uint32_t x = 0; x < 8; ++x) nbu = max(nbu, 8u * per[x]);
  }
  // the waves after the bucket workgroups: tape tiles (and per-record bucket blocks without hist)
  const uint32_t units = max(hist ? 0u : (nbr + 63u) / 64u, (ntr + TILE_TAPE - 1) / TILE_TAPE);
  const uint32_t twg = min((units + SIDE_WAVES - 1) / SIDE_WAVES, max(ax.nwg, 1u) * 4u);
  const uint32_t sgrid = max(nbu + twg, 1u);
  const size_t lds = hist ? (size_t)(ax.S + 1) * sizeof(uint32_t) : 0;
  hipExtLaunchKernelGGL(k_side, dim3(sgrid), dim3(SIDE_THREADS), lds, st, ev0, ev1, 0, SA, nbu);
  return hipGetLastError();
}

}  // namespace me
