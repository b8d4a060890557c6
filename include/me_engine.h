/*
 * me_engine.h — C-ABI of the MI355X batched matching core.
 *
 * This is the drop-in boundary between the (C++) submit-order host side and the
 * gfx950 HIP kernels. Plain C: no exceptions cross it, every call returns an int
 * status (0 = ok), buffers are caller-owned unless stated, no torch types.
 *
 * What each entry point replaces in the reference (julien-mrty/Matching_Engine,
 * paths relative to the reference root):
 *
 *   me_service_*        MatchingEngineServiceImpl (include/server/matching_engine_service.hpp:9-30,
 *                       src/server/matching_engine_service.cpp:17-121): ctor seeds the OID counter,
 *                       me_service_submit_order == SubmitOrder (validate :66-83 -> OID :85 ->
 *                       Order::FromRaw/normalize_to_q4 :89-97 -> persist :99-104 -> response :107-114).
 *                       Persistence is deferred to the batched flush (me_service_flush).
 *   me_normalize_to_q4  normalize_to_q4 (include/domain/price.hpp:15-29), exceptions mapped to codes.
 *   me_create/...       the engine slot include/engine/model.hpp (0 bytes in the reference): there is no
 *                       reference matcher; matching semantics are defined in DESIGN.md §2 and pinned by
 *                       the CPU oracle under oracle/.
 *   me_book_snapshot    GetOrderBook (src/server/matching_engine_service.cpp:123-129, a stub returning an
 *                       empty OrderBookResponse) and Storage::best_bid/best_ask
 *                       (src/storage/storage.cpp:212-252, broken: always nullopt).
 *   me_fill             FillRow (include/storage/storage.hpp:11-17) + fills table (src/storage/storage.cpp:53-63).
 *   ME_ST_*             OrderUpdate.Status (proto/matching_engine.proto:79-85).
 */
#ifndef ME_ENGINE_H
#define ME_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- domain encodings --------------------------------------------------------------- */
/* Side (proto/matching_engine.proto:5-9; include/domain/side.hpp:8-9 static_asserts 1/2). */
enum { ME_SIDE_UNSPECIFIED = 0, ME_SIDE_BUY = 1, ME_SIDE_SELL = 2 };
/* OrderType (proto/matching_engine.proto:11-14). Any value != LIMIT is treated as MARKET,
 * mirroring type_str / the LIMIT-only price check (matching_engine_service.cpp:50,78). */
enum { ME_TYPE_LIMIT = 0, ME_TYPE_MARKET = 1 };
/* Operation carried by a batch record. CANCEL is a build extension (no reference RPC).
 * A REDUCE has no op value of its own: it is a CANCEL record (bit 3) whose type bit (bit 2) is set as
 * well, ME_KIND_REDUCE below. */
enum { ME_OP_NEW = 0, ME_OP_CANCEL = 1 };
/* OrderUpdate.Status (proto/matching_engine.proto:79-85). */
enum {
  ME_ST_NEW = 0,
  ME_ST_PARTIALLY_FILLED = 1,
  ME_ST_FILLED = 2,
  ME_ST_CANCELED = 3,
  ME_ST_REJECTED = 4
};
/* Why a batch record was rejected by the matcher (me_order_result.reason). */
enum {
  ME_RJ_NONE = 0,
  ME_RJ_BAD_QTY = 1,       /* qty <= 0 (the service rejects these before they reach a batch) */
  ME_RJ_BAD_SIDE = 2,      /* side not BUY/SELL (reference: CHECK side IN (1,2) -> "DB insert failed") */
  ME_RJ_OUT_OF_WINDOW = 3, /* retired: every int64 price is accepted (never produced) */
  ME_RJ_BAD_SYMBOL = 4,    /* symbol id >= num_symbols */
  ME_RJ_UNKNOWN_ORDER = 5, /* CANCEL / REDUCE target is not a live resting order of this symbol */
  ME_RJ_BAD_SEQ = 6,       /* seq == 0 (no OID is 0: the counter starts at 1, storage.cpp:254-267) */
  ME_RJ_CAPACITY = 7,      /* service only: a LIMIT the shard could not admit while its books hold
                              max_resting orders (me_service.h; never produced by the engine) */
  ME_RJ_WOULD_CROSS = 8,   /* a POST_ONLY LIMIT whose price reaches the opposite side's best price */
  ME_RJ_BAD_TIF = 9        /* POST_ONLY on a MARKET */
};
/* Time in force / execution instruction of a NEW record (bits 4-5 of the kind byte, DESIGN.md §2;
 * build extension, the reference has none). CANCEL records ignore it.
 *   GTC        a LIMIT rests its remainder, a MARKET drops it (the behaviour without the bits).
 *   IOC        crosses exactly as a LIMIT at its price would; the remainder is discarded and never
 *              rests: FILLED, or CANCELED with remaining_qty = the discarded part (the MARKET
 *              convention). A no-op on a MARKET.
 *   FOK        fillable when the opposite side's resting quantity at prices within the limit (any price
 *              for a MARKET) is >= qty, judged on the book as it stands at that record: then it
 *              executes like the IOC / MARKET and ends FILLED. Else it is killed: no fill, the book
 *              unchanged, CANCELED, filled_qty 0, remaining_qty = qty, fill_count 0, reason NONE.
 *   POST_ONLY  LIMIT only. REJECTED with ME_RJ_WOULD_CROSS (filled_qty 0, remaining_qty = qty, the book
 *              unchanged) when the opposite best price is within its limit; else it rests whole (NEW)
 *              and is an ordinary resting order from then on. On a MARKET: REJECTED, ME_RJ_BAD_TIF.
 * Reject order: BAD_QTY, BAD_SIDE, BAD_SEQ (BAD_SYMBOL ahead of them all), then BAD_TIF, then WOULD_CROSS. */
enum { ME_TIF_GTC = 0, ME_TIF_IOC = 1, ME_TIF_FOK = 2, ME_TIF_POST_ONLY = 3 };

/* kind byte of a batch record: bits 0-1 side, bit 2 type (1 = MARKET), bit 3 op (1 = CANCEL),
 * bits 4-5 time in force (ME_TIF_*; 0 = GTC), bits 6-7 reserved and ignored. */
#define ME_KIND(side, type, op) ((uint8_t)(((side) & 3) | (((type) & 1) << 2) | (((op) & 1) << 3)))
#define ME_KIND_TIF(side, type, op, tif) ((uint8_t)(ME_KIND(side, type, op) | (((tif) & 3) << 4)))

/* REDUCE (build extension): a record whose kind has bits 3 and 2 both set takes `qty` off
 * the resting order whose seq is in price_q4 and leaves it where it is. Side and time-in-force bits are
 * ignored, as on a CANCEL, and the seq rule is the CANCEL's. With the target holding r and qty = d:
 *   d <= 0    REJECTED / ME_RJ_BAD_QTY, whether or not the target lives (after BAD_SYMBOL, before
 *             UNKNOWN_ORDER).
 *   no live resting order of this symbol has that seq: REJECTED / ME_RJ_UNKNOWN_ORDER, as for a CANCEL.
 *   d >= r    exactly a CANCEL: ME_ST_CANCELED, remaining_qty = r (the quantity removed).
 *   d <  r    the order keeps its slot, its seq and its place in the level's FIFO and holds r - d; the
 *             level total drops by d, the resting count is unchanged. ME_ST_NEW, remaining_qty = r - d
 *             (what still rests), filled_qty 0, fill_count 0, reason NONE. The status tells the two
 *             outcomes apart; the quantity removed is d here.
 * A REDUCE never rests and admission control does not count it. There is no increase and no price change:
 * those lose time priority by definition and stay "cancel + new order". */
#define ME_KIND_REDUCE ((uint8_t)0x0D)

/* Slots per FIFO chunk (one wave-wide load of a level's queue). */
#define ME_CHUNK_SLOTS 16

/* Error codes returned by every entry point. */
enum {
  ME_OK = 0,
  ME_E_INVALID = -1,   /* bad argument / config */
  ME_E_HIP = -2,       /* HIP runtime failure (no device, launch failure, ...) */
  ME_E_CAPACITY = -3,  /* a batch refused by admission control (max_resting; not sticky), or a
                          fixed-capacity pool (chunks, far levels, ...) overflowed inside a batch (sticky) */
  ME_E_STATE = -4,     /* engine in a failed state (a previous capacity/HIP error) */
  ME_E_SQLITE = -5     /* persistence failure */
};

/* ---- domain helper ------------------------------------------------------------------- */
/* normalize_to_q4 (include/domain/price.hpp:15-29). Returns 0 and *out on success,
 * 1 for invalid_argument("scale out of range"), 2 for overflow_error("overflow"),
 * 3 for overflow_error("underflow"). */
int me_normalize_to_q4(int64_t price, int32_t scale, int64_t* out);

/* Build record (no reference counterpart): "src=<16 hex> arch=gfx950", the first 16 hex digits of
 * the sha256 of the product sources and headers the library was compiled from (Makefile
 * DIGEST_SRCS order, restated by tools/src_digest.py). */
const char* me_build_info(void);

/* ---- the batched matching engine (one shard = one GPU) ------------------------------- */
typedef struct me_engine me_engine;

typedef struct me_config {
  int32_t device;              /* HIP device ordinal */
  uint32_t num_symbols;        /* local symbols of this shard, ids 0..num_symbols-1 */
  uint32_t levels;             /* L: price levels of each symbol's on-chip WINDOW (power of two, 64..2^20).
                                  Prices are not limited to it: levels outside live in far arrays and the
                                  window re-centres as the market moves */
  uint32_t max_batch;          /* largest n accepted by me_submit_batch* */
  uint64_t max_resting;        /* resting orders the scratch/tape bound is sized for. Admission control:
                                  a batch is accepted only while (resting orders) + (records that may
                                  rest — GTC and POST_ONLY LIMITs — accepted and not yet matched) + (its
                                  records that may rest; every record of a device batch) <= max_resting,
                                  else me_submit_* return ME_E_CAPACITY for that batch, NOT sticky: nothing
                                  of it was enqueued and the engine stays usable (me_admission_read) */
  uint64_t max_chunks;         /* FIFO chunk pool (ME_CHUNK_SLOTS slots each, 256 B); 0 = max_resting + 32*S + 64,
                                  enough for any book shape and any movement of liquidity between symbols:
                                  free chunks go back to a shared pool (me_chunk_stats) */
  uint64_t seq_ring;           /* seq-ring entries for cancels (power of two, 0 = 2^28). Any u64 seq is
                                  accepted; one launch group (batches_per_launch batches) must span fewer
                                  than seq_ring seqs */
  const int64_t* base_price;   /* [num_symbols] initial window base (price_q4 of level 0) per symbol */
  const uint32_t* symbol_ids;  /* optional [num_symbols] ids written to me_fill.symbol (NULL = local id) */
  uint32_t batches_per_launch; /* L <= 128: device batches matched per kernel launch, 1..32 (0 = 32). Back-to-back
                                  me_submit_batch_device calls fill a group; me_sync flushes a partial one */
  uint32_t far_levels;         /* far levels (price levels outside the window) each symbol and side holds in
                                  its inline region, 0 = 256. Not a limit: a side that outgrows it moves to
                                  the far arena, sized from max_resting so it never runs out (me_far_stats) */
  uint32_t host_slots;         /* pinned slots of the host-batch pipeline (me_submit_host), 0 = enough to keep
                                  four launch groups in flight (4 * batches_per_launch + 1); allocated on use */
  uint64_t host_tape_cap;      /* fills a slot holds (0 = 2 * max_batch + 4096). A longer tape is recovered at
                                  me_collect while its batch's scratch is intact (collected before 3 further
                                  launch groups were submitted), else that collect fails with ME_E_CAPACITY */
} me_config;

/* One batch in structure-of-arrays form. Seqs (= numeric OIDs) ascend across the whole stream of an
 * engine: a NEW record's seq is above every earlier record's, a CANCEL record's is at least the
 * previous record's (a cancel never rests, so it may repeat the last OID instead of taking one).
 * Checked on the device: a violation fails the batch with ME_E_INVALID. */
typedef struct me_order_soa {
  const uint64_t* seq;      /* numeric OID of the record */
  const int64_t* price_q4;  /* NEW: normalized Q4 price (ignored for MARKET); CANCEL, REDUCE: target seq */
  const int32_t* qty;       /* NEW: quantity (wire int32, proto:44); CANCEL: ignored; REDUCE: quantity to take off */
  const uint32_t* symbol;   /* local symbol id */
  const uint8_t* kind;      /* ME_KIND(side, type, op) / ME_KIND_TIF(side, type, op, tif) */
} me_order_soa;

/* One trade (32 B): the maker rests, the taker crosses; price is the maker's level. */
typedef struct me_fill {
  uint64_t taker_seq;
  uint64_t maker_seq;
  int64_t price_q4;
  int32_t qty;
  uint32_t symbol;
} me_fill;

/* Per-record outcome (20 B). For CANCEL records: status CANCELED and remaining_qty = the
 * quantity removed from the book, or REJECTED/UNKNOWN_ORDER. For REDUCE records: the same, or status NEW
 * and remaining_qty = what the target still holds (ME_KIND_REDUCE above). */
typedef struct me_order_result {
  int32_t filled_qty;
  int32_t remaining_qty;  /* GTC / POST_ONLY LIMIT: resting remainder; MARKET, IOC, FOK: discarded remainder */
  uint32_t fill_count;
  uint32_t tape_offset;   /* index of this record's first fill in the batch tape */
  uint8_t status;         /* ME_ST_* */
  uint8_t reason;         /* ME_RJ_* */
  uint8_t pad[2];
} me_order_result;

/* One price level of a snapshot. */
typedef struct me_level {
  int64_t price_q4;
  int64_t total_qty;
  uint32_t order_count;
  uint32_t pad;
} me_level;

/* One resting order of a full book dump, in priority order (bids best-first, then asks best-first). */
typedef struct me_book_entry {
  uint64_t seq;
  int64_t price_q4;
  int32_t qty;
  uint8_t side;  /* ME_SIDE_BUY / ME_SIDE_SELL */
  uint8_t pad[3];
} me_book_entry;

/* Creation fails (NULL) without a usable HIP device; the reason is then in me_last_error(NULL,..). */
me_engine* me_create(const me_config* cfg);
void me_destroy(me_engine* e);

/* Host-memory batch, synchronous: me_submit_host + me_collect + copy-out.
 * out_fills must hold the tape (me_fill_bound(e, n) records always suffice; NULL skips the copy);
 * out_results holds n records (or NULL). *n_fills receives the tape length. */
int me_submit_batch(me_engine* e, const me_order_soa* batch, size_t n, me_fill* out_fills,
                    size_t fills_cap, size_t* n_fills, me_order_result* out_results);
/* Upper bound on the tape length of one batch of n records (resting capacity + 2n). */
uint64_t me_fill_bound(const me_engine* e, size_t n);

/* ---- pipelined host batches (the time-slice path of SubmitOrder) -----------
 * me_submit_host stages the batch in the next of the engine's pinned slots (skipped when the batch
 * already lives there, see me_host_inputs), copies it to HBM on the engine's H2D stream and enqueues
 * it behind everything submitted before; it returns at once with a ticket (0, 1, 2, ...). The H2D of
 * batch k+1, the match of batch k and the PCIe writes of batch k-1's results and tape (by the tape
 * job, straight into the slot's pinned block) overlap.
 * me_collect waits for the ticket's batch (launching a partial group first when it is still waiting
 * for one) and points into the slot's pinned outputs: valid until the next me_collect (the engine holds
 * the last collected slot back; only a submit that finds every other slot busy takes it). A slot is
 * reused only after its ticket was collected (else ME_E_STATE). Not
 * thread-safe, like every other entry point: serialize calls on one engine. */
int me_submit_host(me_engine* e, const me_order_soa* batch, size_t n, uint64_t* ticket);
int me_collect(me_engine* e, uint64_t ticket, const me_fill** fills, size_t* n_fills,
               const me_order_result** results, size_t* n_results);
/* Writable pinned arrays for the n-record batch the next me_submit_host will take (zero-copy
 * staging: fill them, then pass the same pointers to me_submit_host). ME_E_STATE while that slot's
 * previous ticket is uncollected. */
typedef struct me_order_soa_w {
  uint64_t* seq;
  int64_t* price_q4;
  int32_t* qty;
  uint32_t* symbol;
  uint8_t* kind;
} me_order_soa_w;
int me_host_inputs(me_engine* e, size_t n, me_order_soa_w* out);
/* Allocate the first nslots host slots now (0 = all of them) instead of on first use — a server's
 * start-up, so no pinned allocation lands in the request path. */
int me_host_reserve(me_engine* e, uint32_t nslots);
/* The engine's configuration as created, defaults resolved (base_price / symbol_ids NULL). */
int me_get_config(const me_engine* e, me_config* out);

/* Device-resident batch (pointers in HBM), enqueued on the engine stream, asynchronous. The batch
 * buffers must stay valid until the next me_sync (or any call that reads outputs or the book).
 * Outputs stay on the device until me_fetch_outputs (me_fetch_outputs / me_fetch_group_outputs /
 * me_copy_*_device read the most recent batch and fail with ME_E_INVALID when it was a host batch). */
int me_submit_batch_device(me_engine* e, const me_order_soa* dev_batch, size_t n);
/* The same with the count of the batch's records that may rest known to the caller
 * (me_submit_batch_device counts every record of a device batch as one that may rest): admission control
 * takes n_limits, which must be at least the batch's NEW records of type LIMIT with time in force GTC or
 * POST_ONLY (IOC and FOK never rest and need not be counted; fewer than that can overflow the scratch
 * bound: a loud, sticky ME_E_CAPACITY). The cluster's shards use it (the root counted them while
 * splitting). */
int me_submit_device_limits(me_engine* e, const me_order_soa* dev_batch, size_t n, uint64_t n_limits);
/* Wait for all enqueued work; returns ME_E_CAPACITY if a pool overflowed in any batch. */
int me_sync(me_engine* e);
/* Copy the last batch's tape/results to host memory (synchronous). */
int me_fetch_outputs(me_engine* e, me_fill* out_fills, size_t fills_cap, size_t* n_fills,
                     me_order_result* out_results, size_t n_results);
/* Batches of the most recent launch group (1..batches_per_launch; the last batch is the last one of
 * it) and the outputs of its k-th batch (synchronous, like me_fetch_outputs). */
uint32_t me_last_group_size(const me_engine* e);
int me_fetch_group_outputs(me_engine* e, uint32_t k, me_fill* out_fills, size_t fills_cap, size_t* n_fills,
                           me_order_result* out_results, size_t n_results);
/* Device-to-device copy of the last batch's tape into dst (HBM), on the engine stream;
 * *n_fills is the synchronous tape length. */
int me_copy_tape_device(me_engine* e, void* dst, size_t cap_fills, size_t* n_fills);
/* Device-to-device copy of the last batch's n_results per-record results (batch order) into dst
 * (HBM), on the engine stream. With me_copy_tape_device: the per-GPU payload of the RCCL gather to
 * the persistence root (matching_engine_amd/gather.py). */
int me_copy_results_device(me_engine* e, void* dst, size_t n_results);

/* Device memory helpers so a C/Python caller can keep batches resident without torch. */
int me_device_alloc(me_engine* e, size_t bytes, void** dptr);
int me_device_free(me_engine* e, void* dptr);
int me_memcpy_h2d(me_engine* e, void* dst, const void* src, size_t bytes);
/* Use an external hipStream_t (e.g. torch's current stream); NULL restores the engine's own. */
int me_set_stream(me_engine* e, void* hip_stream);

/* GetOrderBook: top `depth` levels per side, best first (one device snapshot launch). */
int me_book_snapshot(me_engine* e, uint32_t symbol, me_level* bids, me_level* asks, size_t depth,
                     size_t* n_bids, size_t* n_asks);
/* GetOrderBook in the reference's shape (OrderBookResponse = repeated Order, proto:16-23,57-60), from
 * ONE device snapshot launch (k_book_snapshot, one workgroup per side): every resting order of the
 * top `depth` levels of each side, best level first and FIFO order within a level, plus the levels'
 * aggregates (bid_levels / ask_levels hold `depth` entries). Any output may be NULL; the counts are
 * exact even when a cap is short (entries past it are not written). */
int me_book_orders(me_engine* e, uint32_t symbol, uint32_t depth, me_book_entry* bids, size_t bids_cap,
                   size_t* n_bids, me_book_entry* asks, size_t asks_cap, size_t* n_asks, me_level* bid_levels,
                   me_level* ask_levels, size_t* n_bid_levels, size_t* n_ask_levels);
/* The top `depth` levels per side of EVERY symbol of the shard in one launch — the periodic book
 * snapshot a multi-GPU deployment gathers to its persistence root: levels[(s * 2 + side) * depth + k]
 * (side 0 bids, 1 asks; best first; zeros past the side's levels), counts[s * 2 + side] = levels written. */
int me_book_levels_all(me_engine* e, uint32_t depth, me_level* levels, uint32_t* counts);
/* Full resting state of one symbol (side, price, FIFO). *n receives the count even when cap is short. */
int me_book_dump(me_engine* e, uint32_t symbol, me_book_entry* out, size_t cap, size_t* n);
/* Resting orders over all symbols (device counter). */
int me_resting_count(me_engine* e, uint64_t* n);

/* ---- order query: what a resting order still holds and where it stands (no reference counterpart) ----
 * One answer per seq, from ONE launch of a read-only kernel (k_order_query, one wave per seq; DESIGN.md §2,
 * §4) over the books at the point me_book_dump brings the pipeline to (me_sync runs first). In terms of
 * me_book_dump's order (bids best first, then asks best first, FIFO inside a level): AHEAD are the entries
 * of the order's side and price that come before it, BETTER the entries of its side at strictly better
 * prices. level_qty >= qty_ahead + qty always. The three quantities are int64, as level totals are.
 * found = 0 (every field but seq zero) for seq 0, a seq never submitted or beyond the stream's last, the
 * seq of a record that never rested (MARKET, IOC, FOK, a rejected record, a CANCEL or REDUCE record) and an
 * order that was filled, cancelled or reduced to nothing; these are not told apart. A partially filled or
 * partially reduced order is found with its smaller qty and its unchanged place. */
typedef struct me_order_info { /* 64 B */
  uint64_t seq;           /* echoed */
  int64_t price_q4;
  int64_t qty_ahead;      /* live quantity in front of it in its own level's FIFO */
  int64_t level_qty;      /* its level's total, its own quantity included */
  int64_t qty_better;     /* total resting at the strictly better price levels of its side */
  int32_t qty;            /* what it still holds (> 0 when found) */
  uint32_t orders_ahead;  /* live orders in front of it in its level's FIFO */
  uint32_t levels_better; /* occupied price levels of its side strictly better than its own */
  uint32_t symbol;        /* me_fill.symbol id space (symbol_ids when given) */
  uint8_t side;           /* ME_SIDE_BUY / ME_SIDE_SELL */
  uint8_t found;          /* 1: a live resting order has this seq */
  uint8_t pad[6];         /* zero */
} me_order_info;
/* Synchronous: one H2D copy of the seqs, one launch, one D2H copy of the answers (device buffers grown on
 * demand). Seqs are unique over an engine's stream, so no symbol is named; duplicates in seqs are
 * independent queries. n == 0: ME_OK, nothing is launched. n > 2^24, or seqs / out NULL with n > 0:
 * ME_E_INVALID. A failed engine answers what me_sync answers. A FIFO chain that does not lead back to its
 * level's head: ME_E_STATE "corrupt FIFO chain", as the snapshot calls. */
int me_order_query(me_engine* e, const uint64_t* seqs, size_t n, me_order_info* out);

/* ---- order preview: what a record would execute against the books now (no reference counterpart) -----
 * The question asked BEFORE sending an order (an impact quote, a pre-trade check): query i is the NEW record
 * (q->symbol[i], q->kind[i], q->price_q4[i], q->qty[i]); q->seq is ignored and may be NULL. The answer is what
 * that record would get if it were the only next record of the stream, on the books at the point me_book_dump
 * brings the pipeline to (me_sync runs first, so a partial group is launched and matched), from ONE launch of
 * a read-only kernel (k_order_preview, one wave per query). Queries are independent: none
 * sees another's effect, duplicates are independent queries. The call changes no book, no seq state, no
 * counter and no feed; it consumes no seq and is no batch (the feeds' `batches` stamps do not advance).
 * status, reason, filled_qty, remaining_qty and fill_count equal, field for field, the me_order_result the
 * matcher gives that record (every time in force on LIMIT and MARKET, the MARKET / IOC remainder convention,
 * a killed FOK, WOULD_CROSS, BAD_TIF, and BAD_SYMBOL / BAD_QTY / BAD_SIDE in the matcher's reject order;
 * BAD_SEQ cannot occur: there is no seq). first / last price, notional, levels, fill_count and filled_qty
 * describe the fills the record would produce and are all zero when it produces none (a killed FOK, any
 * reject, nothing crossing). flags and opp_price_q4 describe the opposite side as it is now on every accepted
 * answer, a killed FOK and a WOULD_CROSS reject; they are zero on every other reject.
 * ADMISSION CONTROL IS NOT CONSULTED: ME_PV_RESTS says the remainder would rest if the record were admitted,
 * it does not promise room under max_resting. */
#define ME_PV_HAS_OPP 1u  /* the opposite side holds at least one order; opp_price_q4 is valid */
#define ME_PV_CROSSES 2u  /* HAS_OPP and (MARKET, or the LIMIT's price reaches opp_price_q4) */
#define ME_PV_RESTS   4u  /* accepted GTC / POST_ONLY LIMIT with remaining_qty > 0: that remainder would rest */
typedef struct me_preview { /* 64 B */
  int64_t first_price_q4;  /* price of the first fill (= opp_price_q4 whenever fill_count > 0) */
  int64_t last_price_q4;   /* price of the last fill: the worst price reached */
  int64_t opp_price_q4;    /* best price of the opposite side now (me_quote's rule: window level, else best far level) */
  int64_t notional_hi;     /* sum over the fills of price_q4 * qty as a signed 128-bit integer: high half ... */
  uint64_t notional_lo;    /* ... and low half (two's complement). Exact for any int64 price */
  int32_t filled_qty, remaining_qty;  /* exactly me_order_result's */
  uint32_t fill_count;     /* exactly me_order_result's: makers touched */
  uint32_t levels;         /* distinct price levels the fills come from */
  uint8_t status, reason;  /* exactly me_order_result's (ME_ST_*, ME_RJ_*) */
  uint8_t flags;           /* ME_PV_* */
  uint8_t pad[5];          /* zero */
} me_preview;
/* Synchronous: one H2D copy of the four arrays, one launch, one D2H copy of the answers (device buffers grown
 * on demand, as me_order_query's). n == 0: ME_OK, nothing is launched. n > 2^24, or any of q, q->symbol,
 * q->kind, q->price_q4, q->qty, out NULL with n > 0: ME_E_INVALID. Any kind with bit 3 set (a CANCEL or
 * REDUCE; checked on the host before anything is copied): ME_E_INVALID, nothing launched, nothing answered.
 * The argument checks come first: a failed engine given a bad argument or a CANCEL kind answers ME_E_INVALID;
 * given valid arguments it answers what me_sync answers. A FIFO chain that cannot be walked: ME_E_STATE "corrupt
 * FIFO chain", as the snapshot calls. Over a cluster: me_cluster_order_preview (me_cluster.h), and the
 * me_matcher's order_preview hook. */
int me_order_preview(me_engine* e, const me_order_soa* q, size_t n, me_preview* out);

/* ---- mass cancel: empty the named sides of the named symbols' books (no reference counterpart) -------
 * A halt, a delisting, the end-of-session purge, a kill switch: every resting order of sides[i]
 * (ME_SIDE_BUY = 1, ME_SIDE_SELL = 2, 3 = both) of symbols[i] is removed, window levels and far levels
 * alike, by a stand-alone kernel beside the matching kernels (k_purge): a read-only count
 * launch, one D2H copy of the counts, and — only if anything rests there and fits — one remove launch.
 * When: on the books at the point me_book_dump brings the pipeline to (me_sync runs first, so a partial
 * group is launched and matched); tickets of me_submit_host submitted before stay collectable afterwards
 * with the outputs they would have had. Stream position: the call consumes no seq, does not touch the seq
 * state and is no batch (the feeds' `batches` stamps do not advance).
 * out receives the removed orders request by request; inside a request in me_book_dump's order restricted to
 * the sides asked for (bids best first, then asks best first, FIFO inside a level), qty = what the order
 * still held. counts (or NULL) is [n][2]: counts[2 i] bids, counts[2 i + 1] asks removed for request i.
 * *n_out receives the total. All or nothing: when cap (0 for out == NULL) cannot take every order, nothing
 * is changed, *n_out still holds the exact number needed and the call returns ME_E_CAPACITY — not sticky,
 * the engine stays usable, as after a refused batch. n == 0: ME_OK, nothing is launched.
 * ME_E_INVALID with nothing changed: symbols or sides NULL with n > 0, a symbol >= num_symbols, a sides
 * value outside 1..3, the same symbol named twice, n > num_symbols. A failed engine answers what me_sync
 * answers; a chain that does not lead to its level's tail: ME_E_STATE "corrupt FIFO chain", nothing removed.
 * Afterwards: a CANCEL or REDUCE naming a removed seq is REJECTED / ME_RJ_UNKNOWN_ORDER, me_order_query
 * answers found = 0 for it, me_book_dump of a fully purged symbol is empty, a one-sided purge leaves the
 * other side's dump as it was, the window base does not move, and every later record behaves as if the same
 * orders had been removed by individual CANCEL records. The removed orders leave the resting count of
 * admission control at once (max_resting): a batch refused before the call can be admitted after it.
 * Feeds: with the quote and / or depth feed on, their jobs run once behind the remove launch (quote, then
 * depth), exactly as behind a match launch; a purged side comes out as a quote with its flag clear and as
 * DELETEs of its published view. The trade feed logs nothing: there are no fills.
 * Unlike the order query and the preview, the call exists on an engine only: not on a cluster, not behind a
 * me_matcher (it changes the books and is all-or-nothing on a capacity that would be summed over the shards). */
int me_mass_cancel(me_engine* e, const uint32_t* symbols, const uint8_t* sides, size_t n, me_book_entry* out,
                   size_t cap, size_t* n_out, uint64_t* counts /* [n][2] or NULL */);

/* ---- top-of-book change feed (StreamMarketData, proto/matching_engine.proto:32,62-69) ---------------
 * A symbol's QUOTE is (has_bid, bid_price_q4, bid_qty, has_ask, ask_price_q4, ask_qty): per side the
 * price of the best occupied level and that level's total resting quantity (int64, as level totals
 * are). A side with no resting order has its flag clear and price and quantity 0; price 0 and negative
 * prices are legitimate, so the flag, not the price, says whether a side is absent. The best level is
 * the window's best level of that side when the window holds one, else the side's best far level
 * (a window level always beats a far level of the same side).
 *
 * The feed is CONFLATED PER LAUNCH GROUP: after every match launch (a group of up to batches_per_launch
 * batches when levels <= 128, a single batch on deeper windows) a device job compares every symbol's
 * quote with the one last published for it and logs one me_quote for each symbol that differs.
 * Events of one job ascend by local symbol id, jobs appear in launch order; quotes a symbol passed
 * through inside a group are not observable. The published state starts as "both sides absent", and
 * enabling the feed runs the job once at that point of the stream: enabling on resting books yields one
 * event per symbol with a non-empty side. `batches` is the number of batches (host and device) the
 * engine had matched when the quote was taken; a batch's ordinal is its 1-based position among all
 * batches submitted to the engine (ticket t of an engine fed only by me_submit_host: t + 1).
 *
 * The log is a bounded ring in pinned memory and never loses a change: a job whose changed symbols do
 * not fit into the free part of the log (judged by the events the host had read when the job was
 * enqueued) logs nothing, leaves the published quotes untouched and counts as deferred; its changes
 * stay pending and come out, conflated, with a later job. After me_sync and reads until *left == 0,
 * replaying every event ever read gives exactly the current top of every book. */
typedef struct me_quote { /* 48 B */
  int64_t bid_price_q4, ask_price_q4;
  int64_t bid_qty, ask_qty;
  uint64_t batches;
  uint32_t symbol; /* the id space of me_fill.symbol (symbol_ids when given) */
  uint32_t flags;  /* bit 0 has_bid, bit 1 has_ask */
} me_quote;
#define ME_QUOTE_HAS_BID 1u
#define ME_QUOTE_HAS_ASK 2u
/* cap_events = 0 turns the feed off (an engine that never enables it launches exactly what it launched
 * without it); else the log's capacity in events, raised to at least num_symbols so that one job always
 * fits an empty log; more than max(64 * num_symbols, 2^24) events (pinned host memory, 48 B each) is
 * refused with ME_E_INVALID. Enabling waits for the work in flight and for its own first job (no partial group is
 * launched), so the read after it holds the whole initial state. Enabling an enabled feed starts it
 * afresh (published state "both sides absent", unread events dropped). */
int me_quotes_enable(me_engine* e, uint64_t cap_events);
/* Hands out logged events in order, at most `cap` of them (out may be NULL when cap is 0); *n = events
 * copied, *left = events logged and still unread. It launches no partial group and does not wait for
 * jobs in flight: it returns what the device has logged so far. After me_collect(t) returned, every event
 * with batches <= t's ordinal is there; after me_sync, every event. One exception: a read that leaves the
 * log empty while a deferral is outstanding waits for the work in flight and, if that still holds, runs
 * one catch-up job; its events follow in the same call as far as `cap` allows and count in *left beyond
 * that, so "read until *left == 0" also drains deferred changes. *n and *left are written on every return, also a
 * failing one: the caller always knows how many events it holds. ME_E_INVALID while the feed is off. */
int me_quotes_read(me_engine* e, me_quote* out, size_t cap, size_t* n, size_t* left);
/* Jobs run, events logged and jobs deferred since the feed was enabled, as of the work the device has
 * finished (exact after me_sync). Any pointer may be NULL. ME_E_INVALID while the feed is off. */
int me_quotes_stats(me_engine* e, uint64_t* groups, uint64_t* events, uint64_t* deferred);

/* ---- depth feed: top-N price-level changes (market by price) ----------------------------------------
 * The VIEW of (symbol, side) at depth D is that side's D best occupied price levels, best first, each as
 * (price_q4, total_qty): window levels first, then far levels in price order (the order me_book_snapshot
 * produces; DESIGN.md §3 Invariant I). D is fixed when the feed is enabled, 1 <= D <= ME_DEPTH_MAX. A
 * side with fewer than D levels has a shorter view. total_qty is int64, as level totals are; price 0 and
 * negative prices are prices, and a real level always has total_qty > 0.
 *
 * THE FEED DESCRIBES THE VIEW, NOT THE BOOK. It is conflated per launch group exactly like the quote feed
 * above: after every match launch, at enable time and as a catch-up, a device job compares every side's
 * view with the view last published for it. For a side that differs it logs
 *   SET    (qty = the new total) for every price of the new view that the published view lacks or holds
 *          with another total, and
 *   DELETE (qty = 0) for every price of the published view that the new view lacks.
 * A level that better levels pushed out of the top D is deleted although it still rests; when it comes
 * back into the top D it is SET again. Events of one job ascend by local symbol id, bids before asks;
 * inside a side they run in priority order with SETs and DELETEs merged (descending price for bids,
 * ascending for asks). Jobs appear in launch order.
 *
 * Carried over from the quote feed unchanged: the published state starts empty and enabling runs one job
 * at that point of the stream; `batches` has me_quote.batches' meaning; events are readable after
 * me_collect(t) (those stamped <= t's ordinal) and after me_sync (all); a job whose events do not fit
 * the free part of the log writes nothing, leaves the published views untouched and counts as deferred;
 * a read that leaves the log empty while a deferral is outstanding runs a catch-up job. After me_sync and
 * reads until *left == 0, applying every event ever read to a {price: qty} map per (symbol, side) gives
 * exactly the top D levels of every book. The two feeds are independent: either, both or neither may be
 * on; with both on the quote job runs first, and its events are what they are without the depth feed. */
#define ME_DEPTH_MAX 32
typedef struct me_depth_event { /* 32 B */
  int64_t price_q4;
  int64_t qty;      /* 0 = the level left the view */
  uint64_t batches;
  uint32_t symbol;  /* me_fill.symbol id space */
  uint8_t side;     /* ME_SIDE_BUY / ME_SIDE_SELL */
  uint8_t pad[3];   /* zero */
} me_depth_event;
/* depth == 0 or cap_events == 0 turns the feed off. depth > ME_DEPTH_MAX is ME_E_INVALID. The log's
 * capacity is raised to at least 4 * depth * num_symbols events, the most one job can emit (2 * depth per
 * side), so that one job always fits an empty log; a resulting capacity above 2^26 events (pinned host
 * memory, 32 B each) is refused with ME_E_INVALID. Enabling waits for the work in flight and for its own
 * first job and launches no partial group; enabling an enabled feed starts it afresh. A failing call
 * leaves the feed off. */
int me_depth_enable(me_engine* e, uint32_t depth, uint64_t cap_events);
/* me_quotes_read's contract, for me_depth_event: at most `cap` events in order (out may be NULL when cap
 * is 0); *n = events copied, *left = events logged and still unread; launches no partial group and waits
 * for no job in flight, except that a read that leaves the log empty while a deferral is outstanding
 * waits for the work in flight and, if that still holds, runs one catch-up job whose events follow in the
 * same call as far as `cap` allows. *n and *left are written on every return. ME_E_INVALID while the feed
 * is off. */
int me_depth_read(me_engine* e, me_depth_event* out, size_t cap, size_t* n, size_t* left);
/* Jobs run, events logged and jobs deferred since the feed was enabled (exact after me_sync). Any pointer
 * may be NULL. ME_E_INVALID while the feed is off. */
int me_depth_stats(me_engine* e, uint64_t* groups, uint64_t* events, uint64_t* deferred);

/* ---- trade feed: per-symbol trade summaries (what traded) --------------------------------------------
 * A TRADE is one me_fill. TAPE ORDER is the order of the stream: batches in submit order, inside a batch
 * its records in batch order, inside a record its fills in fill order — the order me_collect and
 * me_fetch_outputs hand out.
 *
 * The feed is conflated per launch group exactly like the quote feed above: after every match launch a
 * device job folds that launch's fills into a per-symbol PENDING summary and then logs one me_trade for
 * every symbol whose pending summary is non-empty, ascending by local symbol id; jobs appear in launch
 * order. An event covers every fill of its symbol since the symbol's previous event (or since enable):
 * open is the price of the earliest of them in tape order, the five last-fill fields (taker_seq, maker_seq,
 * last_price_q4, last_qty, symbol) are the latest me_fill whole, high / low run over all of them, volume
 * and trades are their sums. cum_volume / cum_trades count the symbol's fills since me_trades_enable, this
 * event included. A symbol that did not trade gets no event. Fills matched before me_trades_enable are not
 * counted; there is no initial state, and enabling runs one job that logs nothing (stats: 1 job, 0 events).
 *
 * Carried over from the quote feed unchanged: `batches` has me_quote.batches' meaning; events are readable
 * after me_collect(t) (those stamped <= t's ordinal) and after me_sync (all); a job whose events do not fit
 * the free part of the log writes nothing and counts as deferred: its fills stay in the pending summaries
 * and come out, merged into one event per symbol, with a later job or with the catch-up job of a read that
 * leaves the log empty. After me_sync and reads until *left == 0, for every symbol: the sums of volume and
 * of trades over its events equal its last event's cum_volume / cum_trades and the fold of every fill of
 * that symbol on the tapes since enable, and its last event's last-fill fields are its last fill on the tapes.
 *
 * The three feeds are independent: any subset may be on. With several on the order is quote job, depth
 * job, trade job; the other feeds' events, and every result, tape and book, are what they are without it.
 * There is no notional / VWAP field: price x qty does not fit int64 for arbitrary int64 prices. */
typedef struct me_trade { /* 96 B */
  uint64_t taker_seq, maker_seq; /* the LAST fill the event covers: with last_price_q4 / last_qty / symbol, that me_fill */
  int64_t last_price_q4;
  int64_t open_price_q4;         /* price of the FIRST fill the event covers */
  int64_t high_price_q4, low_price_q4;
  int64_t volume;                /* sum of qty over the event's fills */
  uint64_t trades;               /* fills the event covers (>= 1) */
  int64_t cum_volume;            /* this symbol since me_trades_enable, this event included */
  uint64_t cum_trades;
  uint64_t batches;              /* me_quote.batches' meaning */
  int32_t last_qty;
  uint32_t symbol;               /* me_fill.symbol id space (symbol_ids when given) */
} me_trade;
/* me_quotes_enable's rules: cap_events = 0 turns the feed off (an engine that never enables it launches
 * exactly what it launched without it); else the log's capacity in events, raised to at least num_symbols
 * so that one job always fits an empty log; more than max(64 * num_symbols, 2^24) events (pinned host
 * memory, 96 B each) is refused with ME_E_INVALID. Enabling waits for the work in flight and for its own
 * first job and launches no partial group; enabling an enabled feed starts it afresh (pending summaries
 * and cumulative counts zero, unread events dropped). A failing call leaves the feed off. */
int me_trades_enable(me_engine* e, uint64_t cap_events);
/* me_quotes_read's contract, for me_trade: at most `cap` events in order (out may be NULL when cap is 0);
 * *n = events copied, *left = events logged and still unread; launches no partial group and waits for no
 * job in flight, except that a read that leaves the log empty while a deferral is outstanding waits for
 * the work in flight and, if that still holds, runs one catch-up job whose events follow in the same call
 * as far as `cap` allows. *n and *left are written on every return. ME_E_INVALID while the feed is off. */
int me_trades_read(me_engine* e, me_trade* out, size_t cap, size_t* n, size_t* left);
/* Jobs run, events logged and jobs deferred since the feed was enabled (exact after me_sync). Any pointer
 * may be NULL. ME_E_INVALID while the feed is off. */
int me_trades_stats(me_engine* e, uint64_t* groups, uint64_t* events, uint64_t* deferred);

/* ---- stop and stop-limit orders: a trigger book on the device (no reference counterpart) --------------
 * A STOP waits outside the book until its symbol trades through its stop price; it then leaves the trigger
 * table and comes out as one me_stop_event, the NEW record it becomes (a MARKET: a stop; a LIMIT: a
 * stop-limit) ready to be submitted. A stop never rests in a price level and no matching path knows it: the
 * table is judged by a device job behind every match launch, like the feeds' jobs above.
 *
 * TRIGGER. A BUY stop triggers when a fill of its symbol has price_q4 >= stop_px_q4, a SELL stop when a fill
 * has price_q4 <= stop_px_q4. The feed is conflated per launch group exactly like the trade feed: the job
 * behind a match launch judges every live stop against its symbol's highest and lowest fill price of THAT
 * launch; a symbol without a fill in the launch triggers nothing, whatever the stop price (INT64_MIN and
 * INT64_MAX are stop prices like any other). Only fills of batches SUBMITTED AFTER THE ADD count:
 * me_stops_add first enqueues everything already submitted (a partial group goes out as it is; nothing is
 * waited for) and then copies the stops into the table in stream order. THERE IS NO "ALREADY THROUGH THE
 * MARKET" CHECK: a stop whose price earlier trades have already passed waits for the next fill that
 * satisfies it. A mass cancel produces no fills and triggers nothing; stops of a purged symbol stay until
 * the caller cancels them.
 *
 * THE ENGINE DOES NOT INJECT THE ORDER. Seqs are the host's to allocate and must ascend, so the caller turns
 * events into NEW records with fresh seqs in a later batch (kind, limit_px_q4, qty and symbol are the record's
 * kind, price, quantity and symbol). A cascade — a triggered sell trades lower and triggers the next stop —
 * therefore advances one job per step.
 *
 * Events of one job come in table order, which is ascending id (across symbols); jobs come in launch order.
 * The event ring holds cap_stops events and never defers, by construction: me_stops_add keeps
 * added - cancelled - events read + n <= cap_stops, so every live stop has a free slot waiting for its event.
 * With the feature on, a job (its fold of the launch's fills included) is enqueued only while
 * added - cancelled - events read > 0; an engine that never enables it launches exactly what it launched
 * before. Job order with several feeds on: quote, depth, trade, stops; the other feeds' events, and every
 * result, tape and book, are what they are without it.
 * The service carries stops to its clients (me_service.h: me_service_stops_enable, _submit_stop, _cancel_stop):
 * ids of their own, a `stops` table and restart recovery. Out of scope: the cluster, trailing stops. */
typedef struct me_stop { /* 40 B */
  uint64_t id;          /* the caller's, non-zero, ascending over every add since me_stops_enable */
  int64_t stop_px_q4;
  int64_t limit_px_q4;  /* the price of the record it becomes; ignored for a MARKET and echoed as given */
  int32_t qty;          /* > 0 */
  uint32_t symbol;      /* LOCAL symbol id (< num_symbols), echoed as given */
  uint8_t kind;         /* ME_KIND_TIF(side, type, ME_OP_NEW, tif) of the record it becomes */
  uint8_t pad[7];       /* ignored; zero in dumps */
} me_stop;
typedef struct me_stop_event { /* 64 B */
  uint64_t id;
  int64_t stop_px_q4;
  int64_t limit_px_q4;
  int64_t trigger_px_q4; /* the launch's highest fill price of the symbol for a BUY stop, its lowest for a SELL */
  uint64_t batches;      /* me_quote.batches' meaning */
  int32_t qty;
  uint32_t symbol;       /* the local id as given */
  uint8_t kind;
  uint8_t pad[15];       /* zero */
} me_stop_event;
/* cap_stops = 0 turns the feature off and drops everything (table, unread events, counts); else the most
 * stops that may be live or triggered-and-unread at once: the table's and the event ring's size (48 B of HBM
 * twice and 64 B of pinned host memory per stop). More than 2^22 is ME_E_INVALID. Enabling again starts
 * afresh (ids may start over); a failing call leaves the feature off. No job runs at enable time. */
int me_stops_enable(me_engine* e, uint64_t cap_stops);
/* All or nothing, validated on the host before anything is enqueued. ME_E_INVALID, nothing added: stops
 * NULL with n > 0; an id that is zero, not above the one before it in the call, or not above every id added
 * since enable; symbol >= num_symbols; a side other than BUY / SELL; qty <= 0; the op bit (bit 3) set; MARKET
 * together with POST_ONLY; the feature off. ME_E_CAPACITY, nothing added, NOT sticky (the engine stays
 * usable): added - cancelled - events read + n > cap_stops; cancel stops or read events and try again.
 * When the table's append end cannot take n more entries the call waits for the work in flight and compacts
 * the table first (dead entries go, the order stays). The call returns once the copy into the table is done.
 * n == 0: ME_OK. */
int me_stops_add(me_engine* e, const me_stop* stops, size_t n);
/* me_sync runs first, so a stop that the batches submitted so far trigger HAS triggered: it answers
 * found[i] = 0 and its event is in the ring. found[i] = 1: the stop was live and is gone without an event.
 * An id never added, already triggered or already cancelled answers 0. ids must be strictly ascending, else
 * ME_E_INVALID and nothing changes (also: ids or found NULL with n > 0, n > 2^22, the feature off). One
 * launch, one lane per id (k_stop_cancel: a binary search over the table, which ascends by id). */
int me_stops_cancel(me_engine* e, const uint64_t* ids, size_t n, uint8_t* found);
/* me_trades_read's contract without the catch-up clause (there is no deferral to catch up on): at most `cap`
 * events in order (out may be NULL when cap is 0); *n = events copied, *left = events logged and still
 * unread; launches no partial group, drains nothing and waits for no job in flight. After me_collect(t)
 * returned, every event with batches <= t's ordinal is there; after me_sync, every event. *n and *left are
 * written on every return. ME_E_INVALID while the feature is off. */
int me_stops_read(me_engine* e, me_stop_event* out, size_t cap, size_t* n, size_t* left);
/* jobs run and events logged since enable, as of the work the device has finished, and live = added -
 * cancelled - events (all three exact after me_sync). Any pointer may be NULL. ME_E_INVALID while the
 * feature is off; ME_E_STATE "stop job deferred" should a job ever have found the ring full (the bound above
 * broken: not reachable). */
int me_stops_stats(me_engine* e, uint64_t* jobs, uint64_t* events, uint64_t* live);
/* The live stops in table order (ascending id) after me_sync: what a caller persists. *n is exact even when
 * cap is short (entries past it are not written; out may be NULL when cap is 0). The pass is the table's
 * compaction. ME_E_INVALID while the feature is off. */
int me_stops_dump(me_engine* e, me_stop* out, size_t cap, size_t* n);
/* Every me_stops_* call: argument checks come first; a failed engine then answers what me_sync answers. */

/* Kernel timing. period >= 1: every period-th match-kernel launch records its own start and end
 * (hipExtLaunchKernelGGL events: no marker packets, though each timed launch still costs the
 * stream a few microseconds, hence the sampling); period <= 0: off. Resets the counters below. */
int me_timing_enable(me_engine* e, int period);
/* match_ms / launches: sum and count of the timed match-kernel durations; orders: records of the
 * timed launches; fills: fills of ALL batches since enable; pipeline_ms: device time per batch,
 * start-to-start from the first to the last timed launch (0 with fewer than two). */
int me_timing_read(me_engine* e, double* match_ms, double* pipeline_ms, uint64_t* launches,
                   uint64_t* fills, uint64_t* orders);

/* Event counters since me_create: handoffs = symbols the register-window kernel handed to its
 * continuation launch (a far price level, a re-centre, a cancel of a far or very old order, a FOK,
 * POST_ONLY or REDUCE record). */
int me_stats_read(me_engine* e, uint64_t* handoffs);
/* The same for deep windows (L > 128): hot_handoffs = hot symbols whose walk (k_agg_walk / k_match_hot) gave
 * the rest of a batch to the generic record loop (k_match_hot_cont): a cancel, a price outside the window, a
 * taker while far levels exist, a FOK or POST_ONLY record, a REDUCE, no room in the walk's pools. */
int me_hot_stats_read(me_engine* e, uint64_t* hot_handoffs);

/* Far levels (price levels outside a symbol's window; unbounded since round 5): moves =
 * sides that outgrew their region and moved to a larger one in the far arena, collections = the
 * arena's copying collections (k_seq_sweep), arena_used = entries taken from the active half. Any
 * pointer may be NULL. No reference counterpart (the reference keeps no book). */
int me_far_stats(me_engine* e, uint64_t* moves, uint64_t* collections, uint64_t* arena_used);

/* The FIFO chunk pool: reclaims = reclamations so far (k_seq_sweep returned every symbol's free chunks
 * to the shared pool ahead of a launch group that could otherwise have run out), high_water = chunk ids
 * ever handed out, pool = max_chunks. Any pointer may be NULL. No reference counterpart. */
int me_chunk_stats(me_engine* e, uint64_t* reclaims, uint64_t* high_water, uint64_t* pool);

/* The matching paths the engine runs now (no reference counterpart: the reference has one CPU path).
 * *flags bit 0 (ME_PATH_GROUPED_AGG): launch groups of windows <= 128 levels go through the aggregate
 * path (k_agg_gwalk2); bit 1 (ME_PATH_HOT_AGG): hot symbols of deeper windows do. */
#define ME_PATH_GROUPED_AGG 1u
#define ME_PATH_HOT_AGG 2u
#define ME_PATH_GROUPED_CANCELS 4u /* the grouped walk covers cancels (k_agg_gwalk_cx) */
int me_paths_read(const me_engine* e, uint32_t* flags);

/* Admission control state (any pointer may be NULL): resting = resting orders of every symbol after
 * all enqueued work (waits for it); bound = the host's current upper bound (resting orders once every
 * accepted record is matched); exact_counts = times a submit had to take an exact count (flush + sync)
 * because the published count was too stale or too close to max_resting. */
int me_admission_read(me_engine* e, uint64_t* resting, uint64_t* bound, uint64_t* exact_counts);
/* Would a batch with n_rest records that may rest (GTC / POST_ONLY LIMITs) be admitted now? (*ok = 1/0;
 * nothing is enqueued.) A submit from the same thread right after a 1 is admitted. Shards that must accept
 * a slice all-or-none (cluster.ShardedMatcher) ask every engine first. */
int me_admission_check(me_engine* e, uint64_t n_rest, int* ok);

/* ---- raw export of the resident book: DIAGNOSTIC (tests/book_audit.py) -----------------
 * Not part of the service boundary and no reference counterpart: the device arrays of the book exactly as
 * the kernels left them, for an offline audit of their redundant fields. Both calls first bring the pipeline
 * to the point me_book_dump does (every enqueued batch matched, the stream idle); the copy is a plain
 * device-to-host copy, no kernel runs. The layout of the entries is me_layout.hpp's, not an ABI: me_debug_info
 * reports sizeof of every exported struct so that a reader fails loudly when one drifts. */
enum {
  ME_DBG_LEVELS = 0, /* Level [S][L] */
  ME_DBG_OCC,        /* u64 [S][L / 64] */
  ME_DBG_TEND,       /* u8 [S][L] */
  ME_DBG_SYM,        /* SymState [S] */
  ME_DBG_CHUNKS,     /* Chunk [nchunks] */
  ME_DBG_FCACHE,     /* u32 [S][fcache_row] */
  ME_DBG_LOC,        /* u32 [ring_mask + 1] */
  ME_DBG_OLD,        /* OldEnt [old_mask + 1] */
  ME_DBG_SQ,         /* SeqState [2]; the matchers read entry me_debug_info.sq_idx */
  ME_DBG_FAR,        /* FarLevel [far_entries] */
  ME_DBG_FDIR,       /* FarDir [S][2] */
  ME_DBG_FAR_CTL,    /* u64 [n_far_ctl] */
  ME_DBG_CHUNK_TOP,  /* u32 [1] */
  ME_DBG_RECL,       /* u32 [nchunks] */
  ME_DBG_CPOOL,      /* u32 [n_cpool] */
  ME_DBG_STATS,      /* u64 [n_stats] */
  ME_DBG_ERR,        /* u32 [1] */
  ME_DBG_ARRAYS
};
typedef struct me_debug_info {
  uint64_t num_symbols, levels, level_words, nchunks, ring_mask, old_mask;
  uint64_t far_levels;  /* inline far entries per (symbol, side) */
  uint64_t far_half;    /* entries of each arena half */
  uint64_t far_inline;  /* end of the inline regions = start of half 0 */
  uint64_t far_entries; /* far_inline + 2 * far_half */
  uint64_t sq_idx, chunk_slots, fcache_row, n_far_ctl, n_cpool, n_stats;
  uint64_t sizeof_level, sizeof_symstate, sizeof_chunk, sizeof_farlevel, sizeof_fardir, sizeof_oldent,
      sizeof_seqstate;
} me_debug_info;
int me_debug_layout(me_engine* e, me_debug_info* out);
/* Array `which` (ME_DBG_*) into dst[0, cap); *bytes (may be NULL) receives its size. cap smaller than the
 * array: ME_E_INVALID, nothing copied (dst NULL and cap 0 ask for the size alone and return ME_OK). */
int me_debug_export(me_engine* e, uint32_t which, void* dst, size_t cap, size_t* bytes);

/* Last error text of e (or of the last failed me_create when e == NULL). */
int me_last_error(const me_engine* e, char* buf, size_t cap);

/* ---- synthetic order streams (bench + tests; stands in for the reference client CLI) --- */
typedef struct me_gen_params {
  uint32_t config;          /* 1..5, SURVEY.md §8(d) */
  uint64_t seed;
  uint32_t num_symbols;     /* global symbols */
  uint32_t levels;          /* window L per symbol (must cover the price spread) */
  int32_t spread_ticks;     /* LIMIT offsets U[-spread, +spread] around the symbol mid */
  int32_t max_qty;          /* qty ~ U[1, max_qty] */
  uint32_t market_pct;      /* % MARKET among new orders */
  uint32_t cancel_pct;      /* % CANCEL among records */
  double zipf_s;            /* > 0: Zipf(s) symbol popularity, 0 = uniform */
  int32_t market_qty_mult;  /* > 0: MARKET qty = U[1, market_qty_mult] * max_qty (sweeps) */
  uint64_t seq_start;       /* first seq of the stream (0 = 1) */
  int32_t drift_step;       /* > 0: a symbol's mid moves drift_step ticks (in its own fixed direction) ... */
  uint32_t drift_every;     /* ... every drift_every records of that symbol */
  uint32_t far_pct;         /* % of LIMITs priced far away: mid +- U[levels, 64 * levels] ticks */
} me_gen_params;

typedef struct me_gen me_gen;
me_gen* me_gen_create(const me_gen_params* p);
void me_gen_destroy(me_gen* g);
/* Per-symbol window base (level 0 price) for all num_symbols global symbols. */
int me_gen_base_prices(const me_gen* g, int64_t* out);
/* Next n records of the global stream (already normalized, global symbol ids, seq from 1).
 * Any pointer may be NULL. */
int me_gen_next(me_gen* g, size_t n, uint64_t* seq, int64_t* price_q4, int32_t* qty,
                uint32_t* symbol, uint8_t* kind);
/* Pre-seed records (config 4): `per_side` resting orders per side per symbol at distinct levels. */
int me_gen_seed_book(me_gen* g, uint32_t symbol, uint32_t per_side, uint64_t* seq, int64_t* price_q4,
                     int32_t* qty, uint8_t* kind);
/* shard of a global symbol: splitmix64(symbol) % shards. */
uint32_t me_shard_of(uint32_t symbol, uint32_t shards);

#ifdef __cplusplus
}
#endif
#endif /* ME_ENGINE_H */
