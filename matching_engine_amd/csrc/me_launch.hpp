// me_launch.hpp — the host entries of the kernel units: one declaration per launch_* function (and
// sort_tile), included by the .hip file that defines it and by its callers. Every entry enqueues on the
// given stream and returns the launch's hipError_t; none synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "me_layout.hpp"

namespace me {

// ---- me_kernels.hip
uint32_t sort_tile(uint32_t n);
hipError_t launch_sort_pass(hipStream_t st, const uint32_t* keys_in, const uint32_t* idx_in, uint32_t n,
                            uint32_t clamp_key, int shift, int dbits, uint32_t* hist, uint32_t* tot,
                            uint32_t* keys_out, uint32_t* idx_out, uint32_t* zero_buf,
                            uint32_t zero_words, unsigned long long* scratch_top, uint32_t* bin_start,
                            const uint64_t* seq, const uint8_t* kind, uint32_t* err);
hipError_t launch_seq_sweep(hipStream_t st, const BookDev& bk, const uint64_t* const* seq, const uint8_t* const* kind,
                            const uint32_t* n, uint32_t ng, uint32_t in_idx, uint32_t grid, uint32_t launch);
hipError_t launch_match(hipStream_t st, const BookDev& bk, const BatchDev& bt, hipEvent_t ev0, hipEvent_t ev1,
                        const HotLaunch& hot);
// the L <= 128 dispatcher: picks the register kernel's build, or the grouped aggregate path
hipError_t launch_match_reg(hipStream_t st, const BookDev& bk, const BatchDev* bt, uint32_t ng, const AuxDev& ax,
                            hipEvent_t ev0, hipEvent_t ev1, const HotLaunch* hot);
hipError_t launch_tape(hipStream_t st, const BatchDev& bt, me_fill* tape, unsigned long long tape_cap,
                       unsigned long long* tape_count, unsigned long long* fills_acc, uint32_t* err,
                       me_order_result* hres, uint32_t* err_out);
hipError_t launch_tape_spill(hipStream_t st, const me_order_result* res, const uint32_t* fstart, uint32_t n,
                             const me_fill* scratch, unsigned long long cap, me_fill* spill);
hipError_t launch_init_levels(hipStream_t st, Level* levels, size_t count);
hipError_t launch_init_chunks(hipStream_t st, Chunk* chunks, size_t count);

// ---- me_side.hip: the side jobs of ax alone (err: the book's error word)
hipError_t launch_side(hipStream_t st, uint32_t* err, const AuxDev& ax, hipEvent_t ev0, hipEvent_t ev1);
hipError_t launch_side_fill(hipStream_t st, uint32_t* err, const AuxDev& ax, bool& done);

// ---- me_agg.hip
hipError_t launch_agg(hipStream_t hs, const BookDev& bk, const BatchDev& bt, const AggDev& ag);
hipError_t launch_agg_group(hipStream_t st, const BookDev& bk, const BatchDev* bt, uint32_t ng, const AggDev& ag);

// ---- me_snapshot.hip
hipError_t launch_book_snapshot(hipStream_t st, const BookDev& bk, const SnapReq& rq);
hipError_t launch_quotes(hipStream_t st, const BookDev& bk, const QuoteDev& q);
hipError_t launch_depth(hipStream_t st, const BookDev& bk, const DepthDev& d);
hipError_t launch_trades(hipStream_t st, const BookDev& bk, const TradeDev& t, const TradeLaunch& tl);
// the trigger book: its job behind a match launch; a cancel by id (found [n]); the stable compaction of the
// table's live entries into dst (count [1] receives how many)
hipError_t launch_stops(hipStream_t st, const StopDev& sd, const TradeLaunch& tl);
hipError_t launch_stop_cancel(hipStream_t st, const StopDev& sd, const uint64_t* ids, uint32_t n, uint8_t* found);
hipError_t launch_stop_compact(hipStream_t st, const StopDev& sd, StopEnt* dst, uint32_t* count);
hipError_t launch_order_query(hipStream_t st, const BookDev& bk, const OrderQueryReq& rq);
hipError_t launch_order_preview(hipStream_t st, const BookDev& bk, const PreviewReq& rq);
// the mass cancel's passes: remove = false counts (read-only), true removes
hipError_t launch_purge(hipStream_t st, const BookDev& bk, const PurgeReq& rq, bool remove);

// ---- me_match_reg.hip, one namespace per build (ng >= 1; launch_match_reg above picks one). Visible
// only under ME_LAUNCH_REG_VARIANTS, which that dispatcher's file and the defining file set: no other
// caller names a build
#ifdef ME_LAUNCH_REG_VARIANTS
namespace rc64 {
hipError_t launch_match_reg(hipStream_t st, const BookDev& bk, const BatchDev* bt, uint32_t ng, const AuxDev& ax,
                            hipEvent_t ev0, hipEvent_t ev1);
hipError_t launch_match_reg_cont(hipStream_t st, const BookDev& bk, const BatchDev* bt, uint32_t ng, hipEvent_t ev1);
}  // namespace rc64
namespace rc128 {
hipError_t launch_match_reg(hipStream_t st, const BookDev& bk, const BatchDev* bt, uint32_t ng, const AuxDev& ax,
                            hipEvent_t ev0, hipEvent_t ev1);
hipError_t launch_match_reg_cont(hipStream_t st, const BookDev& bk, const BatchDev* bt, uint32_t ng, hipEvent_t ev1);
}  // namespace rc128
#endif

}  // namespace me
