/*
 * me_service.h — the SubmitOrder drop-in: MatchingEngineServiceImpl's request path re-hosted on
 * the batched GPU core (C-ABI, plain C structs mirroring the proto messages, no gRPC types).
 *
 *   me_service_create         MatchingEngineServiceImpl(db_path) + Impl ctor
 *                             (src/server/matching_engine_service.cpp:17-22, :36): opens/creates the
 *                             SQLite DB with the reference pragmas + schema (src/storage/storage.cpp:9-69)
 *                             and seeds the OID counter from MAX(OID)+1 (storage.cpp:254-267).
 *   me_service_submit_order   SubmitOrder (matching_engine_service.cpp:41-121): identical validation
 *                             order and strings (:66-83), OID allocation (:85, consumed even when
 *                             normalisation throws), normalize_to_q4 (:89-97), side CHECK -> "DB insert
 *                             failed" with order_id set (:107-111). The order joins the open time slice.
 *                             Any non-empty symbol is accepted (:66-71): a new one takes the engine's
 *                             next unused book, or an idle symbol's book once all are taken (below);
 *                             only when every book holds orders is it refused (grpc_status 8
 *                             RESOURCE_EXHAUSTED, "symbol capacity exhausted", no OID).
 *   me_service_flush          the time-slice batcher: matches every slice submitted so far on the engine
 *                             (me_submit_host / me_collect) and ingests each in ONE SQLite transaction
 *                             (orders rows as insert_new_order writes them carrying the matched status
 *                             and remainder, fills rows, maker / cancel-target updates) — the batched
 *                             rewrite of storage.cpp:78-208. Matching and persistence run outside the
 *                             submit lock: SubmitOrder never waits for a flush.
 *   me_service_start          background flusher: a slice closes at slice_orders records or once it is
 *                             interval_us old, and is flushed without any caller.
 *   me_service_book           GetOrderBook (matching_engine_service.cpp:123-129) from the GPU book.
 *   me_service_cancel_order   CancelOrder — a build extension (the reference has no cancel RPC; SURVEY
 *                             §8(f) row 4): queues a cancel record for a resting order into the slice.
 *   me_service_market_data    StreamMarketData's MarketDataUpdate (proto:60-67) from the GPU book.
 *   me_service_updates        StreamOrderUpdates (proto/matching_engine.proto:34,71-91): drains the
 *                             OrderUpdate events the flushes produced, optionally for one client_id.
 *   me_service_submit_stop    stop and stop-limit orders — a build extension (the trigger book of me_engine.h
 *                             behind me_service_stops_enable): ids "SID-<n>", me_service_cancel_stop,
 *                             me_service_stop_updates, a `stops` table and restart recovery (further down).
 *
 * Restart: the reference resumes only its OID counter from the DB (matching_engine_service.cpp:18-22,
 * storage.cpp:254-267). me_service_create does that and also rebuilds the books: every order the DB
 * shows resting (status NEW / PARTIALLY_FILLED, remaining_quantity > 0) is replayed into the backend
 * in OID order with its remainder, before the first SubmitOrder is matched, so it keeps its price-time
 * priority, can trade and can be cancelled.
 *
 * Symbols: any non-empty symbol is accepted (:66-71). The backend holds a fixed number of books; when
 * every book is taken, a new symbol takes over a book with no resting order and no record on its way
 * (the old symbol's book is reclaimed). Only when every book is in use is the order refused
 * (RESOURCE_EXHAUSTED, no OID).
 *
 * Capacity: a slice the backend refuses (its books near max_resting) is split and matched in parts;
 * a single LIMIT that still does not fit is answered in-band with an OrderUpdate REJECTED (reason
 * ME_RJ_CAPACITY) instead of stalling every later slice behind it. Deliberate deviation from the
 * reference, which has no capacity: admission counts every GTC / POST_ONLY LIMIT as one that may rest
 * (whether it fills is only known once matched), so near max_resting a marketable LIMIT that would have
 * filled completely is refused too. max_resting is a deployment parameter sized to HBM; a deployment sizes it
 * above its resting high-water mark.
 */
#ifndef ME_SERVICE_H
#define ME_SERVICE_H

#include "me_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* OrderRequest (proto/matching_engine.proto:37-45). */
typedef struct me_order_request {
  const char* client_id;
  const char* symbol;
  int32_t order_type; /* OrderType; != LIMIT is MARKET */
  int32_t side;       /* Side */
  int64_t price;      /* raw scaled integer */
  int32_t scale;
  int32_t quantity;
} me_order_request;

/* OrderResponse (proto:47-51) + the gRPC status code of the call. */
typedef struct me_order_response {
  char order_id[32];      /* "OID-<n>", empty when none was allocated */
  int32_t success;
  int32_t grpc_status;    /* 0 OK; 2 UNKNOWN: normalize_to_q4 threw (price.hpp:16,23-24) */
  char error_message[64];
} me_order_response;

typedef struct me_service me_service;

/* engine: the shard the slices are matched on (NULL: submit works, flush fails loudly). The service
 * drives it from its own threads: no other caller may use the engine while the service lives.
 * symbols[num_symbols]: symbol strings pre-assigned to the engine's local ids 0..num_symbols-1; later
 * symbols take the following ids, up to the engine's num_symbols.
 * db_path: SQLite file (NULL: no persistence). Destroy does not flush: flush first. */
me_service* me_service_create(me_engine* engine, const char* const* symbols, uint32_t num_symbols,
                              const char* db_path);
void me_service_destroy(me_service* s);

/* A sharded deployment's matcher (matching_engine_amd/cluster.py): symbols live on
 * several engines (one per GPU, splitmix64(symbol) % G); the service on the persistence root hands
 * it each slice and gets back the merged outputs, exactly what one engine holding every symbol
 * would produce (me_collect's shapes: tape ordered by taker seq, results in slice order). */
typedef struct me_matcher {
  void* ctx;
  uint32_t num_symbols;  /* symbol ids it takes (the service interns up to this many) */
  uint32_t max_batch;    /* largest slice */
  uint64_t max_resting;  /* resting orders it holds at most (me_fill_bound's bound: max_resting + 2n) */
  /* Match one slice; outputs valid until the next call. ME_E_CAPACITY: refused, nothing of it was
   * applied (admission control; the slice stays queued). Any other nonzero: the slice is lost (the
   * service fails). */
  int (*match)(void* ctx, const me_order_soa* slice, size_t n, const me_fill** fills, size_t* n_fills,
               const me_order_result** results);
  /* me_book_orders' contract for one symbol (depth 0: the whole book). */
  int (*book)(void* ctx, uint32_t symbol, uint32_t depth, me_book_entry* bids, size_t bids_cap, size_t* n_bids,
              me_book_entry* asks, size_t asks_cap, size_t* n_asks, me_level* bid_levels, me_level* ask_levels,
              size_t* n_bid_levels, size_t* n_ask_levels);
  /* Optional, both or neither: match split in two, so the service keeps two slices in flight (slice k+1
   * is submitted before slice k is collected). submit applies the slice and returns a ticket
   * (ME_E_CAPACITY: refused, nothing applied); collect returns that ticket's outputs (valid until the
   * next collect). Tickets are collected in submission order, at most two outstanding. */
  int (*submit)(void* ctx, const me_order_soa* slice, size_t n, uint64_t* ticket);
  int (*collect)(void* ctx, uint64_t ticket, const me_fill** fills, size_t* n_fills, const me_order_result** results);
  /* Optional (NULL: no feed): me_quotes_read's contract over the matcher's books — top-of-book change events
   * in order, at most cap of them, *left = events still unread. `symbol` is the id space of `match`; `batches`
   * must count the slices the matcher has matched (slice k of this service is stamped k, from 1): the service
   * names an event's symbol by it (me_service_market_stream). */
  int (*quotes)(void* ctx, me_quote* out, size_t cap, size_t* n, size_t* left);
  /* All optional (NULL: the service answers as it does without the facility). depth_enable / depth and
   * trades_enable / trades: me_depth_enable's / me_depth_read's and me_trades_enable's / me_trades_read's
   * contracts over the matcher's books, `symbol` and `batches` as in `quotes` (slice numbers). order_query /
   * order_preview: me_order_query's / me_order_preview's contracts in the id space of `match`. */
  int (*depth_enable)(void* ctx, uint32_t depth, uint64_t cap_events);
  int (*depth)(void* ctx, me_depth_event* out, size_t cap, size_t* n, size_t* left);
  int (*trades_enable)(void* ctx, uint64_t cap_events);
  int (*trades)(void* ctx, me_trade* out, size_t cap, size_t* n, size_t* left);
  int (*order_query)(void* ctx, const uint64_t* seqs, size_t n, me_order_info* out);
  int (*order_preview)(void* ctx, const me_order_soa* q, size_t n, me_preview* out);
  /* Optional, all four or none (else the matcher has no stop orders: me_service_stops_enable answers
   * ME_E_INVALID): me_stops_enable's / me_stops_add's / me_stops_cancel's / me_stops_read's contracts over the
   * matcher's books. me_stop.symbol is in the id space of `match`; me_stop_event.batches counts slices, as
   * `quotes` documents. A matcher built by older code must be zero-initialised up to sizeof(me_matcher). */
  int (*stops_enable)(void* ctx, uint64_t cap_stops);
  int (*stops_add)(void* ctx, const me_stop* stops, size_t n);
  int (*stops_cancel)(void* ctx, const uint64_t* ids, size_t n, uint8_t* found);
  int (*stops_read)(void* ctx, me_stop_event* out, size_t cap, size_t* n, size_t* left);
} me_matcher;

/* The service over a matcher instead of an engine (same contract otherwise). NULL on a bad matcher. The
 * matcher must outlive the service: me_service_destroy (like an unsubscribe) turns the depth and trade feeds
 * it enabled off through depth_enable / trades_enable, and stop orders off through stops_enable(ctx, 0). */
me_service* me_service_create_matcher(const me_matcher* m, const char* const* symbols, uint32_t num_symbols,
                                      const char* db_path);

/* Always returns 0 (the RPC itself succeeded or failed in-band, like the reference). */
int me_service_submit_order(me_service* s, const me_order_request* req, me_order_response* resp);

/* SubmitOrder with a time in force (ME_TIF_*, me_engine.h; build extension: the reference's OrderRequest
 * carries none, so me_order_request stays as it is). me_service_submit_order is this call with
 * ME_TIF_GTC. After the reference's own validations (same strings, same order) a tif outside 0..3, or
 * POST_ONLY on a MARKET, is answered in-band: success = 0, "invalid time in force", no OID. An IOC or
 * FOK never rests (no live entry, nothing to cancel): its remainder or kill arrives as an OrderUpdate
 * CANCELED with the discarded quantity; a POST_ONLY that would cross as REJECTED. The orders row carries
 * the final state, as a MARKET's does; a restart rebuilds resting orders as plain LIMITs (only GTC and
 * POST_ONLY orders ever rest). */
int me_service_submit_order_tif(me_service* s, const me_order_request* req, int32_t tif, me_order_response* resp);

/* n SubmitOrder calls in order (what a server's handler threads do one request at a time), for
 * drivers and benchmarks holding many requests at once; resps[i] answers reqs[i]. */
int me_service_submit_orders(me_service* s, const me_order_request* reqs, size_t n, me_order_response* resps);

/* Submitted orders not matched yet (the open slice, closed slices, the slice being matched). */
size_t me_service_pending(const me_service* s);
/* Next OID number the service will allocate. */
uint64_t me_service_next_oid(const me_service* s);

/* Match and persist every slice submitted before the call, oldest first (matching runs on the calling
 * thread, ahead of the service's persister thread by at most 4 slices, so the engine overlaps
 * SQLite); returns once every matched slice's OrderUpdates are out and its transaction committed.
 * Any output may be NULL;
 * the outputs cover the records this call matched, in submission order (tape offsets into the
 * concatenated tape): *n_results records, out_seq[i] their numeric OIDs. The capacities are checked
 * before anything is matched (results_cap >= me_service_pending, fills_cap >= me_fill_bound of it),
 * else ME_E_INVALID and nothing happens.
 * A slice the engine accepted is never matched again. When its transaction fails (e.g. SQLITE_BUSY
 * past the 5 s busy timeout) the matched slice is kept in memory, later slices still match, and every
 * later flush first retries the kept ones in order; the call returns ME_E_SQLITE meanwhile
 * (me_service_unpersisted counts the records waiting). */
int me_service_flush(me_service* s, me_fill* out_fills, size_t fills_cap, size_t* n_fills,
                     me_order_result* out_results, uint64_t* out_seq, size_t results_cap, size_t* n_results);
/* Matched records whose SQLite transaction has not committed yet (queued for the persister, or kept
 * after a failed transaction). me_service_pending + me_service_unpersisted is 0 exactly when every
 * submitted order is matched and committed. */
size_t me_service_unpersisted(const me_service* s);
/* Background flusher (one thread): a slice closes at slice_orders records (0 or more than the
 * engine's max_batch: max_batch) or once it is interval_us old (0: 1000), and is flushed at once.
 * Errors go to me_service_last_error. me_service_stop joins it and waits for the persister to
 * finish what it matched. */
int me_service_start(me_service* s, uint32_t interval_us, uint32_t slice_orders);
int me_service_stop(me_service* s);

/* Level view of GetOrderBook for a symbol string (top depth levels per side, aggregates; depth 0:
 * no levels). */
int me_service_book(me_service* s, const char* symbol, me_level* bids, me_level* asks, size_t depth,
                    size_t* n_bids, size_t* n_asks);

/* Order (proto/matching_engine.proto:16-23): one resting order of an OrderBookResponse. */
typedef struct me_book_order {
  char order_id[32];  /* "OID-<n>" */
  char client_id[64]; /* the submitting client ("" for orders that did not come through this service) */
  int64_t price;      /* Q4 */
  int32_t scale;      /* 4 */
  int32_t quantity;   /* the resting (unfilled) quantity */
  int32_t side;       /* ME_SIDE_BUY / ME_SIDE_SELL */
  int32_t pad;
} me_book_order;

/* GetOrderBook (matching_engine_service.cpp:123-129) in the reference's shape: OrderBookResponse
 * {repeated Order bids; repeated Order asks} (proto:57-60), bids best price first, asks best price
 * first, FIFO (time) order within a price; from one device snapshot launch (me_book_orders). depth:
 * price levels per side (0: the whole book, as OrderBookRequest carries no depth). Counts are exact
 * even when a cap is short; unknown symbol: empty. */
int me_service_order_book(me_service* s, const char* symbol, uint32_t depth, me_book_order* bids, size_t bids_cap,
                          size_t* n_bids, me_book_order* asks, size_t asks_cap, size_t* n_asks);

/* CancelOrder request (build extension, mirrors OrderRequest's conventions). */
typedef struct me_cancel_request {
  const char* client_id;
  const char* symbol;
  const char* order_id; /* "OID-<n>" of the order to cancel */
} me_cancel_request;

/* Validation (first failing check wins, in-band like SubmitOrder :66-83): "symbol is required",
 * "order_id is invalid" (not "OID-<n>", n >= 1), "order belongs to another client" (the target is a
 * resting or pending order of a different client_id). An accepted cancel consumes NO OID: its stream
 * position is the last OID allocated (a cancel record may repeat the previous seq, me_engine.h), so
 * accepted orders keep the reference's gap-free OID sequence. It answers success=1 with order_id = the
 * TARGET's id; whether it removed anything arrives as an OrderUpdate after the flush (CANCELED with
 * the removed quantity, or REJECTED when the target was not resting on that symbol). */
int me_service_cancel_order(me_service* s, const me_cancel_request* req, me_order_response* resp);

/* ReduceOrder request (build extension): take `quantity` off a resting order and leave it where it is in
 * its price level's queue (me_engine.h ME_KIND_REDUCE; an increase or a price change stays "cancel + new
 * order"). */
typedef struct me_reduce_request {
  const char* client_id;
  const char* symbol;
  const char* order_id; /* "OID-<n>" of the order to reduce */
  int32_t quantity;     /* the quantity to take off, > 0 */
} me_reduce_request;

/* CancelOrder's contract with one more in-band check after "symbol is required": "quantity must be > 0"
 * (SubmitOrder's text). The same owner rule, no OID consumed, success=1 with order_id = the TARGET's id.
 * The outcome arrives as an OrderUpdate after the flush: when `quantity` is below what the target holds,
 * one update for the TARGET to its owner with the target's own status (NEW if it never traded, else
 * PARTIALLY_FILLED), fill price and quantity 0 and remaining_quantity = what still rests; when it covers
 * the target, exactly a cancel's CANCELED (remaining = removed qty); REJECTED to the requester when the
 * target was not resting on that symbol. The orders row keeps its status and its remaining_quantity drops
 * by `quantity`; a restart rebuilds the book from it, so the order comes back reduced and in its place. */
int me_service_reduce_order(me_service* s, const me_reduce_request* req, me_order_response* resp);

/* OrderStatus (build extension): what a client's resting orders still hold and where they stand in their
 * queues, from one me_order_query (me_engine.h) for all n ids. The cancel RPC's conventions: ids are
 * "OID-<n>", n >= 1, and only the owner learns anything.
 *   ME_OS_NOT_RESTING  the id is malformed, the order is unknown, it stopped resting (filled, cancelled,
 *                      reduced to nothing, a MARKET / IOC / FOK), or it belongs to ANOTHER client: the call
 *                      does not reveal that such an order exists. Every field but order_id and scale is 0.
 *   ME_OS_PENDING      the caller's order is known to the service but the engine has no resting order of that
 *                      id: it sits in a slice not matched yet, or its closing update is on its way. quantity =
 *                      the remainder the service knows; no position.
 *   ME_OS_RESTING      side, quantity (what it still holds), price (Q4) and the position fields exactly as
 *                      me_order_info defines them.
 * out[i] answers order_ids[i] (order_id echoed, truncated to fit). The call matches what was flushed before
 * it (me_order_query's me_sync) but flushes no open slice. A service over a me_matcher asks its `order_query`
 * hook; a matcher without one has no order query: ME_E_INVALID. n == 0: ME_OK. */
enum { ME_OS_NOT_RESTING = 0, ME_OS_PENDING = 1, ME_OS_RESTING = 2 };
typedef struct me_order_status { /* 88 B */
  char order_id[32];
  int32_t state; /* ME_OS_* */
  int32_t side, scale /* 4 */, quantity /* remaining */;
  int64_t price, qty_ahead, level_qty, qty_better;
  uint32_t orders_ahead, levels_better;
} me_order_status;
int me_service_order_status(me_service* s, const char* client_id, const char* const* order_ids, size_t n,
                            me_order_status* out);

/* PreviewOrder (build extension): what SubmitOrder with this request and time in force would execute against
 * the book now, from one me_order_preview (me_engine.h) — nothing is submitted. The request passes
 * me_service_submit_order_tif's validations and Q4 normalisation: one that SubmitOrder would refuse in-band
 * returns ME_E_INVALID with SubmitOrder's message in me_service_last_error. No OID is taken, nothing is
 * persisted, nothing enters a slice and no book is claimed. The answer is taken on what was flushed before the
 * call (me_order_preview's me_sync); like me_service_order_status it flushes no open slice, so orders still
 * pending in a slice are not in the book it sees. A symbol name that has no book is answered as an empty book
 * (a LIMIT rests whole, a MARKET / IOC / FOK fills nothing) without touching the engine. Admission control is
 * not consulted (me_order_preview). A service over a me_matcher asks its `order_preview` hook; a matcher
 * without one has no preview: ME_E_INVALID. */
int me_service_preview_order(me_service* s, const me_order_request* req, int32_t tif, me_preview* out);

/* Mass cancel (build extension): an operator's action — a halt, a delisting, the end-of-session purge — so
 * there is no owner check. Every resting order of `sides` (ME_SIDE_BUY = 1, ME_SIDE_SELL = 2, 3 = both) of the
 * n named symbols is removed by ONE me_mass_cancel; symbols == NULL means every symbol that has a book. The open
 * slice is closed and everything pending flushed first, so the purge takes what was submitted before the call.
 * Every removed order's owner gets one OrderUpdate, CANCELED with remaining_quantity = the quantity removed —
 * a cancel's update exactly; the rows' status is persisted in one transaction through the path matched slices
 * take (a failed transaction: ME_E_SQLITE, kept and retried at the next flush), so a restart does not bring
 * the orders back; me_service_order_status then answers ME_OS_NOT_RESTING for them, and a book left empty
 * counts as idle: a new symbol may take it (me_service_stats: reclaimed_books). *n_cancelled (or NULL)
 * receives the number of orders removed. ME_E_INVALID with nothing changed: a name that has no book, a name
 * given twice, a NULL name, sides outside 1..3, and a service over a me_matcher (it has no mass cancel).
 * Stop orders are left alone, as me_mass_cancel leaves them: a purge produces no fill and triggers nothing, and
 * the stops of a purged symbol stay armed (and keep its book) until their owners cancel them. */
int me_service_mass_cancel(me_service* s, const char* const* symbols, size_t n, int32_t sides, uint64_t* n_cancelled);

/* OrderUpdate (proto:71-91). Events per flushed record, in slice order: for each fill the maker's
 * update then the taker's (fill price/qty, remaining after the fill, PARTIALLY_FILLED / FILLED);
 * then a closing taker update when no fill closed it (NEW resting, CANCELED market / IOC remainder or
 * FOK kill, REJECTED — a POST_ONLY that would cross included); a cancel record emits CANCELED
 * (remaining = removed qty) or REJECTED for its target; a reduce record the same, or its target's own
 * status with the reduced remainder (me_service_reduce_order). */
typedef struct me_order_update {
  char order_id[32];
  char client_id[64];
  char symbol[32];
  int32_t status;            /* ME_ST_* */
  int32_t scale;             /* 4: prices are Q4 */
  int64_t fill_price;        /* Q4, 0 without a fill */
  int32_t fill_quantity;
  int32_t remaining_quantity;
} me_order_update;

/* Drain up to cap queued updates (client_id NULL or "": every client; else only that client's,
 * leaving the others queued). *n = updates written; returns ME_OK. */
int me_service_updates(me_service* s, const char* client_id, me_order_update* out, size_t cap, size_t* n);
/* Events dropped because the queue held 2^24 undrained updates (the oldest go first; each drop also
 * sets me_service_last_error). One count for the OrderUpdate queue and the stop update queue
 * (me_service_stop_updates), which has the same bound. */
uint64_t me_service_updates_dropped(const me_service* s);
/* Books handed from an idle symbol to a new one since create, and resting orders replayed into the
 * books from the DB at create (restart recovery). */
int me_service_stats(const me_service* s, uint64_t* reclaimed_books, uint64_t* recovered_orders);

/* MarketDataUpdate (proto:60-67) for StreamMarketData, from the GPU book: best bid / ask (Q4,
 * scale 4) and the total quantity resting there (saturated to int32). The reference's
 * Storage::best_bid / best_ask SQL (storage.cpp:212-252) query side=0 / side=1, which the schema's
 * CHECK side IN (1,2) never admits, so they always return nullopt; here a missing side reads 0
 * with has_bid / has_ask = 0 (proto3 default). Unknown symbol: both sides missing. */
typedef struct me_market_data {
  int64_t best_bid;
  int64_t best_ask;
  int32_t scale;
  int32_t bid_size;
  int32_t ask_size;
  int32_t has_bid;
  int32_t has_ask;
  int32_t pad;
} me_market_data;

int me_service_market_data(me_service* s, const char* symbol, me_market_data* out);

/* StreamMarketData (proto/matching_engine.proto:32, MarketDataUpdate :62-69) as a change stream instead of
 * the poll above: one update per symbol whose top of book changed in a matched slice, from the backend's
 * quote feed (me_quotes_*, me_engine.h) — nothing is snapshotted and the pipeline is not drained.
 * md follows me_service_market_data's conventions (scale 4, sizes saturated to int32, has_* flags). */
typedef struct me_market_update {
  char symbol[32];
  me_market_data md;
} me_market_update;
/* on != 0: enable the backend's feed — me_quotes_enable on the service's engine (the engine must have been
 * fresh when the service was created: the service matches event stamps with the slices it submitted), or
 * the matcher's `quotes` hook — and queue the books' current tops (one update per symbol with a non-empty
 * side; after restart recovery: the recovered books). ME_E_INVALID with neither. It waits for a running
 * flush. on == 0: the stream stops and queued updates are dropped. */
int me_service_market_subscribe(me_service* s, int on);
/* Drain up to cap queued updates (symbol NULL or "": every symbol; else only that symbol's, leaving the
 * others queued, as me_service_updates does for clients). After each matched slice the flush path reads
 * the backend's events and queues them. The queue conflates: a symbol has at most one pending update, a
 * newer one overwrites its payload and keeps its place, so the queue is bounded by the number of symbols
 * and nothing is ever dropped. An event is named by the symbol that owned its book at the slice the event
 * belongs to (its `batches` stamp), so a book handed from an idle symbol to a new one never reports one
 * symbol's quote under the other's name. *n = updates written; ME_E_INVALID when not subscribed. */
int me_service_market_stream(me_service* s, const char* symbol, me_market_update* out, size_t cap, size_t* n);

/* The depth stream: the top-D book of every symbol whose top D levels changed in a matched slice, from the
 * engine's depth feed (me_depth_*, me_engine.h). The engine sends deltas, the service materialises views: it
 * applies the events to a view it keeps per symbol, so its queue is bounded by the number of symbols. */
typedef struct me_depth_level {
  int64_t price;
  int32_t size; /* saturated to int32 */
  int32_t pad;
} me_depth_level;
typedef struct me_depth_book {
  char symbol[32];
  int32_t scale; /* 4 */
  uint32_t n_bids, n_asks;
  uint32_t pad;
  me_depth_level bids[ME_DEPTH_MAX], asks[ME_DEPTH_MAX]; /* best first */
} me_depth_book;
/* depth in 1..ME_DEPTH_MAX: me_depth_enable on the service's own engine (which must have been fresh when the
 * service was created, as for me_service_market_subscribe) and queue the books as they stand; it waits for a
 * running flush. A service backed by a me_matcher uses its `depth_enable` / `depth` hooks; a matcher without
 * them has no depth feed: ME_E_INVALID. depth == 0: the stream
 * stops, the views and the queue are dropped. Independent of me_service_market_subscribe. */
int me_service_depth_subscribe(me_service* s, uint32_t depth);
/* Hand out the whole current top-D book of up to cap changed symbols, in first-change order (symbol NULL or
 * "": every symbol; else only that symbol's book, the others stay queued). A symbol has at most one pending
 * book: a newer change refreshes it in place and nothing is dropped. An emptied book is delivered once, with
 * both counts 0. A book's events are named by the symbol that owned it at the slice they belong to, as
 * me_service_market_stream's are. *n = books written; ME_E_INVALID when not subscribed. */
int me_service_depth_stream(me_service* s, const char* symbol, me_depth_book* out, size_t cap, size_t* n);

/* The trade stream: one summary per symbol that traded in a matched slice, from the engine's trade feed
 * (me_trades_*, me_engine.h): last trade price and size, open / high / low and the traded volume and count of
 * the fills the update covers, and the symbol's totals since the subscription. Prices are Q4 (scale 4).
 * volume and the cumulative fields are int64 / uint64 and never saturate; there is no notional or VWAP field
 * (price x quantity does not fit int64 for arbitrary int64 prices). */
typedef struct me_trade_update {
  char symbol[32];
  int32_t scale;     /* 4 */
  int32_t last_size; /* quantity of the last fill */
  int64_t last_price;
  int64_t open_price, high_price, low_price;
  int64_t volume;    /* over the fills this update covers */
  uint64_t trades;
  int64_t cum_volume; /* this symbol NAME since me_service_trades_subscribe, this update included */
  uint64_t cum_trades;
} me_trade_update;
/* on != 0: me_trades_enable on the service's own engine (which must have been fresh when the service was
 * created, as for me_service_market_subscribe); fills matched before are not counted and nothing is queued. It
 * waits for a running flush. A service backed by a me_matcher uses its `trades_enable` / `trades` hooks; a
 * matcher without them has no trade feed: ME_E_INVALID. on == 0: the
 * stream stops, queued updates and the totals are dropped. Independent of the market and depth streams. */
int me_service_trades_subscribe(me_service* s, int on);
/* Drain up to cap queued updates (symbol NULL or "": every symbol; else only that symbol's, the others stay
 * queued). After each matched slice the flush path reads the engine's events and queues them. The queue
 * conflates: a symbol has at most one pending update; a newer event merges into it — last price and size are
 * the newer event's, open is kept, high / low widen, volume and trades add — and keeps its place. An event is
 * named by the symbol that owned its book at the slice the event belongs to (its `batches` stamp), and the
 * cumulative fields are summed per symbol name from the events' own volume and trades: a book handed from an
 * idle symbol to a new one reports each name's own totals, not the book's. *n = updates written;
 * ME_E_INVALID when not subscribed. */
int me_service_trades_stream(me_service* s, const char* symbol, me_trade_update* out, size_t cap, size_t* n);

/* ---- stop and stop-limit orders (build extension; the trigger book of me_engine.h, me_stops_*) --------------
 * A stop waits outside the book until its symbol trades through its stop price (BUY: a fill at or above it,
 * SELL: at or below it) and then becomes an ordinary order of its owner: a MARKET (a stop) or a LIMIT (a
 * stop-limit). The backend judges the stops in the job behind every match launch; what the service adds per
 * slice is one read of its event ring.
 *
 * IDS. Stops have their own id space, "SID-<n>", counted from 1 (after a restart: from the highest id the
 * `stops` table holds, plus 1); n is the backend's me_stop.id. The order a stop becomes takes the next OID when
 * its event is processed, not before: seqs ascend along the stream, and OIDs stay gap-free.
 *
 * STREAM POSITION. A stop operation (SubmitStop, CancelStop) closes the open slice if it holds records and
 * attaches to the boundary in front of the next slice; consecutive operations share one boundary. The flush
 * path applies a boundary's operations in submission order right before it submits the slice behind it — runs
 * of adds as one stops_add, runs of cancels as one stops_cancel (ids sorted; an id named twice in a run is
 * answered CANCEL_REJECTED the second time) — so a stop sees the fills of every order submitted after it and
 * of none submitted before it (me_stops_add's rule). A boundary with no slice behind it is applied by
 * me_service_flush and, on its interval, by the background flusher. A slice split after a capacity refusal has
 * the boundary in front of its first part only. Slices already in flight are collected before a boundary that
 * holds a cancel is applied. me_service_pending counts records only.
 *
 * TRIGGER. After every collected slice, and after every stops_cancel, the backend's events are read until none
 * is left; an event is processed once the slice it is stamped with has been collected (two slices are in
 * flight, and a later slice's events may already be readable: the outcome does not depend on that). The stamps
 * are matched as me_service_market_subscribe matches them: the engine must have been fresh when the service was
 * created, and recovery slices count. For each event, in ring order: the next OID is allocated, the NEW record
 * (the event's kind, limit price, quantity and symbol) joins the open slice under the stop's client, and a
 * TRIGGERED update is queued. From then on the order is an ordinary order: its OrderUpdates go to the stop's
 * owner, it can be cancelled and reduced while it rests. me_service_flush does not chase a cascade: the
 * injected orders stay pending (me_service_pending() > 0) for the next flush or the background flusher — one
 * step per flush, as in the engine. With batches_per_launch > 1 the engine judges the stops once per launch
 * group: slices of one flush that share a group share a job, so trigger_price is the group's extreme and the
 * events of the group come in stop id order.
 * THERE IS NO "ALREADY THROUGH THE MARKET" CHECK (me_engine.h): a stop waits for the next qualifying fill.
 *
 * PERSISTENCE. me_service_stops_enable creates the table `stops` (stop_id INTEGER PRIMARY KEY — the n of
 * "SID-n" —, client_id, symbol, side, order_type, tif, stop_price and limit_price (Q4), quantity, status
 * (ME_SS_ARMED / _TRIGGERED / _CANCELED), order_id, trigger_price, updated_ts); a database that never enables
 * stops keeps the reference's schema. Rows go through the persister in order with the matched slices: the ARMED
 * insert and the CANCELED update in the transaction of the slice behind their boundary, TRIGGERED (with
 * order_id and trigger_price) in the transaction that carries the triggered order's `orders` row. A crash
 * between the trigger and that commit therefore leaves the stop ARMED and no order: it is re-armed at the
 * restart and, there being no already-through-the-market check, waits for the next qualifying fill. A failed
 * transaction is kept and retried like a slice's. Without a database everything works, in memory only. */

/* cap_stops > 0: turn stop orders on — the backend's stops_enable(cap_stops) (an engine, or a matcher's four
 * hooks; a matcher without them: ME_E_INVALID; more than 2^22: ME_E_INVALID) — create the table, seed the SID
 * counter from MAX(stop_id) + 1 over all rows (never backwards within one service: a SID handed out before an
 * off / on is not issued again), and re-add the rows the database shows ARMED in ascending id
 * through stops_add (the books were rebuilt at create): they count into me_service_stop_stats' `recovered` and
 * keep their symbols' books. More ARMED rows than cap_stops, or more symbols than books: ME_E_CAPACITY and
 * stop orders stay off. Already on: ME_E_STATE. cap_stops == 0: off — the backend's table and events are
 * dropped, queued stop updates too; the rows stay (a later enable re-arms them). It waits for a running flush. */
int me_service_stops_enable(me_service* s, uint64_t cap_stops);

typedef struct me_stop_request {
  const char* client_id;
  const char* symbol;
  int32_t order_type, side; /* of the order the stop becomes */
  int64_t price;            /* its limit price; ignored for a MARKET */
  int64_t stop_price;       /* same scale */
  int32_t scale, quantity, tif; /* ME_TIF_* */
} me_stop_request;
/* Always returns 0; the first failing check wins, answered in-band, and a refused request takes no SID and no
 * OID: (1) "stop orders are not enabled"; (2) SubmitOrder's checks, its strings and order ("symbol is
 * required", "quantity must be > 0", "price must be > 0 for LIMIT"); (3) "invalid time in force" as
 * me_service_submit_order_tif gives it; (4) normalize_to_q4 of price (LIMIT only) and of stop_price with
 * `scale`: grpc_status 2 and SubmitOrder's text ("scale out of range", "overflow", "underflow"); then a side
 * other than BUY / SELL: "DB insert failed" (SubmitOrder's answer to it; here before any id exists); (5)
 * "stop capacity exhausted", grpc_status 8, when the stops accepted and not yet cancel-confirmed or
 * trigger-processed, plus this one, exceed cap_stops — the service mirrors the engine's bound on the host, so
 * the backend's add is never refused (should it be, the service fails: ME_E_* from the flush, not an answer);
 * (6) the book claim as SubmitOrder does it: "symbol capacity exhausted", grpc_status 8. Accepted: success = 1,
 * order_id = "SID-<n>"; the stop is QUEUED until its boundary is applied, then ARMED (one ARMED update). A book
 * with a QUEUED or ARMED stop is not idle: no other symbol takes it over. */
int me_service_submit_stop(me_service* s, const me_stop_request* req, me_order_response* resp);

typedef struct me_stop_cancel_request {
  const char* client_id;
  const char* stop_id; /* "SID-<n>" */
} me_stop_cancel_request;
/* Always returns 0. In-band, first failing check wins: "stop orders are not enabled", "stop_id is invalid" (not
 * "SID-<n>", n >= 1), "stop belongs to another client" (a QUEUED or ARMED stop of a different client_id). An
 * accepted cancel consumes no id and answers success = 1 with order_id = the TARGET's id; its outcome arrives as
 * a stop update once its boundary is applied: CANCELED when the backend found the stop live (found = 1), else
 * CANCEL_REJECTED (already triggered, already cancelled, or an id nobody owns, which is queued like any other).
 * The backend's events are read and processed before the outcomes are queued: the owner of a stop that had
 * triggered sees TRIGGERED before the rejection. */
int me_service_cancel_stop(me_service* s, const me_stop_cancel_request* req, me_order_response* resp);

enum { ME_SS_ARMED = 0, ME_SS_TRIGGERED = 1, ME_SS_CANCELED = 2, ME_SS_CANCEL_REJECTED = 3, ME_SS_QUEUED = 4 };
typedef struct me_stop_update { /* 200 B */
  char stop_id[32];   /* "SID-<n>" */
  char order_id[32];  /* "OID-<n>" once TRIGGERED, else "" */
  char client_id[64]; /* the stop's owner; of a CANCEL_REJECTED: the requester */
  char symbol[32];    /* "" in a CANCEL_REJECTED of a stop the service no longer holds */
  int32_t state;      /* ME_SS_* */
  int32_t scale;      /* 4 */
  int64_t stop_price, limit_price, trigger_price; /* Q4; trigger_price 0 until TRIGGERED */
  int32_t quantity;
  uint8_t kind;       /* ME_KIND_TIF of the order the stop becomes */
  uint8_t pad[3];
} me_stop_update;
/* me_service_updates' contract for the stop updates: drain up to cap of them (client_id NULL or "": every
 * client's; else only that client's, the others stay queued). *n = updates written; returns ME_OK. The queue
 * holds 2^24 undrained updates; beyond that the oldest go first, each drop counted by
 * me_service_updates_dropped and the first one reported in me_service_last_error. */
int me_service_stop_updates(me_service* s, const char* client_id, me_stop_update* out, size_t cap, size_t* n);
/* The caller's stops that are QUEUED or ARMED, in ascending stop id (client_id NULL or "": every client's).
 * *n is exact even when cap is short (entries past it are not written; out may be NULL when cap is 0). */
int me_service_stops(me_service* s, const char* client_id, me_stop_update* out, size_t cap, size_t* n);
/* live: stops QUEUED or ARMED now; triggered: events processed since the enable; recovered: ARMED rows re-added
 * from the database by the enable. Any pointer may be NULL. All 0 while stop orders are off. */
int me_service_stop_stats(const me_service* s, uint64_t* live, uint64_t* triggered, uint64_t* recovered);

int me_service_last_error(const me_service* s, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ME_SERVICE_H */
