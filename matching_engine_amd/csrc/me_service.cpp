// me_service.cpp — SubmitOrder re-hosted on the batched core (include/me_service.h).
//
// Per order (host, synchronous, the reference's exact contract):
//   validate (matching_engine_service.cpp:66-83) -> "OID-<n>" (:85, :29-32) -> normalize_to_q4
//   (:89-97, price.hpp:15-29) -> side CHECK (storage.cpp:32) -> response (:107-114)
// and the order joins the open time slice (SoA). A slice closes when it reaches the slice size or
// (with the background flusher, me_service_start) when it is older than the interval; closed slices
// are matched on the engine and persisted, in stream order, OUTSIDE the submit lock — SubmitOrder
// only ever waits for another SubmitOrder. Persistence is ONE SQLite transaction per slice (the
// batched rewrite of storage.cpp:78-208): each order's row as insert_new_order writes it (incl.
// order_type=1, storage.cpp:106) carrying its matched status and remainder in the same INSERT,
// update_order_status-style updates for makers and cancel targets, and fills rows through the
// corrected add_fill statement (5 columns, 5 placeholders; the reference's has 6, storage.cpp:190).
//
// Two stages run concurrently: the flushing thread matches slice k+1 while the persister thread
// (which alone owns the DB) emits slice k's OrderUpdates and commits its transaction, so the engine
// (or the sharded matcher's gather) overlaps SQLite instead of waiting for it.
//
// Locks (always taken in this order, never the other way round):
//   flush_mu  one flusher at a time: slices are matched in stream order
//   eng_mu    every engine call (the engine is single-threaded): flush matching, book reads
//   mu        the open slice, the closed-slice queue, the symbol table, the OID counter; the stops held, the
//             SID counter (the flush thread takes it after eng_mu, or without it, to turn stop events into
//             orders: never the other way round)
//   pq_mu     the matched-slice queue between the two stages
//   live_mu   resting orders' owners and remainders (cancel ownership, OrderUpdate bookkeeping)
//   upd_mu    the OrderUpdate queue
//   ref_mu    per-book reference counts (which books an idle symbol may hand over)
//   err_mu    the last error text
//
// The flusher keeps two slices in flight: slice k+1 is submitted to the backend (its own engine or a
// sharded deployment's matcher: one table of calls, Backend below) before slice k is collected, so the
// backend's work on k+1 overlaps the collect of k and its hand-off to the persister.
//
// SQLite is loaded at run time (dlopen libsqlite3.so.0) so the library has no build-time
// dependency on a sqlite3 header.
#include <dlfcn.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <list>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "me_engine.h"
#include "me_service.h"
#include "me_service_feed.hpp"
#include "me_service_stops.hpp"
#include "me_stops.hpp"

namespace {

// ---- minimal sqlite3 C API (dlopen) -------------------------------------------------------
struct sqlite3;
struct sqlite3_stmt;
constexpr int SQLITE_OK = 0, SQLITE_ROW = 100, SQLITE_DONE = 101;
constexpr int SQLITE_OPEN_READWRITE = 0x2, SQLITE_OPEN_CREATE = 0x4, SQLITE_OPEN_FULLMUTEX = 0x10000;
using destructor_t = void (*)(void*);
const destructor_t SQLITE_TRANSIENT = reinterpret_cast<destructor_t>(-1);

struct Sql {
  void* h = nullptr;
  int (*open_v2)(const char*, sqlite3**, int, const char*) = nullptr;
  int (*close)(sqlite3*) = nullptr;
  int (*exec)(sqlite3*, const char*, void*, void*, char**) = nullptr;
  int (*prepare_v2)(sqlite3*, const char*, int, sqlite3_stmt**, const char**) = nullptr;
  int (*bind_int64)(sqlite3_stmt*, int, long long) = nullptr;
  int (*bind_text)(sqlite3_stmt*, int, const char*, int, destructor_t) = nullptr;
  int (*step)(sqlite3_stmt*) = nullptr;
  int (*reset)(sqlite3_stmt*) = nullptr;
  int (*finalize)(sqlite3_stmt*) = nullptr;
  long long (*column_int64)(sqlite3_stmt*, int) = nullptr;
  const unsigned char* (*column_text)(sqlite3_stmt*, int) = nullptr;
  const char* (*errmsg)(sqlite3*) = nullptr;
  int (*busy_timeout)(sqlite3*, int) = nullptr;

  bool load(std::string& err) {
    if (h) return true;
    h = dlopen("libsqlite3.so.0", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libsqlite3.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) {
      err = "libsqlite3 not found";
      return false;
    }
#define SYM(f, n)                                  \
  f = reinterpret_cast<decltype(f)>(dlsym(h, n));  \
  if (!f) {                                        \
    err = std::string("sqlite symbol missing: ") + n; \
    return false;                                  \
  }
    SYM(open_v2, "sqlite3_open_v2");
    SYM(close, "sqlite3_close");
    SYM(exec, "sqlite3_exec");
    SYM(prepare_v2, "sqlite3_prepare_v2");
    SYM(bind_int64, "sqlite3_bind_int64");
    SYM(bind_text, "sqlite3_bind_text");
    SYM(step, "sqlite3_step");
    SYM(reset, "sqlite3_reset");
    SYM(finalize, "sqlite3_finalize");
    SYM(column_int64, "sqlite3_column_int64");
    SYM(column_text, "sqlite3_column_text");
    SYM(errmsg, "sqlite3_errmsg");
    SYM(busy_timeout, "sqlite3_busy_timeout");
#undef SYM
    return true;
  }
};

Sql g_sql;
std::mutex g_sql_mu;

inline int64_t now_ms() {
  using namespace std::chrono;
  return duration_cast<milliseconds>(system_clock::now().time_since_epoch()).count();
}
inline int64_t mono_us() {
  using namespace std::chrono;
  return duration_cast<microseconds>(steady_clock::now().time_since_epoch()).count();
}

// storage.cpp:26-69, verbatim schema semantics.
const char* kSchema =
    "CREATE TABLE IF NOT EXISTS orders ("
    "  order_id TEXT PRIMARY KEY, client_id TEXT NOT NULL, symbol TEXT NOT NULL,"
    "  side INTEGER NOT NULL CHECK (side IN (1,2)), order_type INTEGER NOT NULL, price INTEGER,"
    "  quantity INTEGER NOT NULL CHECK (quantity > 0), status INTEGER NOT NULL,"
    "  remaining_quantity INTEGER NOT NULL, created_ts INTEGER NOT NULL, updated_ts INTEGER NOT NULL);"
    "CREATE INDEX IF NOT EXISTS idx_orders_symbol_side ON orders(symbol, side);"
    "CREATE INDEX IF NOT EXISTS idx_orders_client ON orders(client_id);"
    "CREATE TABLE IF NOT EXISTS fills ("
    "  id INTEGER PRIMARY KEY AUTOINCREMENT, order_id TEXT NOT NULL, symbol TEXT NOT NULL,"
    "  fill_price INTEGER NOT NULL, fill_quantity INTEGER NOT NULL, event_ts INTEGER NOT NULL,"
    "  FOREIGN KEY(order_id) REFERENCES orders(order_id));"
    "CREATE INDEX IF NOT EXISTS idx_fills_order ON fills(order_id);";

struct Pending {
  std::string client;
  std::string symbol;
  int32_t side;
  bool cancel;      // CancelOrder / ReduceOrder record (build extensions): target = the order it names
  uint64_t target;
  bool reduce = false;  // of a cancel-type record: a ReduceOrder (ME_KIND_REDUCE), taking d off its target
  int32_t d = 0;
};

// The symbol id of a cancel whose symbol holds no book: out of the backend's range, so the record is
// rejected (BAD_SYMBOL -> an OrderUpdate REJECTED) without taking a book for it.
constexpr uint32_t kNoBook = 0xFFFFFFFFu;

// A stop order the service holds: QUEUED (accepted, its boundary not applied yet) or ARMED (in the backend's
// table). It leaves the table when its cancel is confirmed or its event is processed.
struct Stop {
  std::string client;
  std::string symbol;
  uint32_t sid = 0;  // its book (reference-counted like a live order's: a book with a stop is never handed over)
  int32_t side = 0, type = 0, tif = 0;
  int64_t stop_px = 0, limit_px = 0;
  int32_t qty = 0;
  uint8_t kind = 0;
  bool armed = false;
};

// One stop operation at a slice boundary, in submission order. An add carries the stop as accepted; a cancel
// the requester, and what the service knew of the target when it was asked (for the rejection's update).
struct StopOp {
  bool cancel = false;
  bool unknown = false;  // a cancel of an id not issued yet when it was accepted: rejected without asking
  uint64_t id = 0;
  std::string client;  // add: the owner; cancel: the requester
  Stop stop;           // add: the stop; cancel: the target as known at the request (symbol "" if unknown)
};

// A change to the `stops` table that commits with a slice's transaction.
struct StopRow {
  int32_t state = 0;  // ME_SS_ARMED: insert (from `stop`); ME_SS_CANCELED / ME_SS_TRIGGERED: update
  uint64_t id = 0;
  uint64_t oid = 0;   // TRIGGERED: the order the stop became (a record of the same slice)
  int64_t trigger_px = 0;
  std::string client;
  Stop stop;
};

// One time slice: the SoA handed to the engine + the host-only fields persistence needs.
struct Slice {
  std::vector<uint64_t> seq;
  std::vector<int64_t> px;
  std::vector<int32_t> qty;
  std::vector<uint32_t> sid;
  std::vector<uint8_t> kind;
  std::vector<Pending> meta;
  std::vector<StopOp> pre;     // the boundary in front of the slice: applied right before it is submitted
  std::vector<StopRow> srows;  // stop rows of its transaction: its boundary's, and its triggered orders'
  int64_t opened_us = 0;
  bool recovery = false;  // resting orders replayed from the DB at create: their rows already exist
  size_t size() const { return seq.size(); }
  // The first k records become their own slice; this one keeps the rest. The boundary (and its rows) stays in
  // front of the first part; a triggered stop's row goes with its order's record.
  Slice take_prefix(size_t k) {
    Slice p;
    p.opened_us = opened_us;
    p.recovery = recovery;
    p.pre = std::move(pre);
    pre.clear();
    const uint64_t last = k ? seq[k - 1] : 0;
    std::vector<StopRow> rest;
    for (auto& r : srows) (r.state != ME_SS_TRIGGERED || r.oid <= last ? p.srows : rest).push_back(std::move(r));
    srows = std::move(rest);
    auto cut = [k](auto& src, auto& dst) {
      dst.assign(std::make_move_iterator(src.begin()), std::make_move_iterator(src.begin() + k));
      src.erase(src.begin(), src.begin() + k);
    };
    cut(seq, p.seq);
    cut(px, p.px);
    cut(qty, p.qty);
    cut(sid, p.sid);
    cut(kind, p.kind);
    cut(meta, p.meta);
    return p;
  }
};

// A matched slice on its way to the DB (outputs copied out of the engine's buffers). One whose
// transaction failed stays at the head of the queue, in order, until a later flush commits it.
struct Matched {
  Slice sl;
  std::vector<me_order_result> res;
  std::vector<me_fill> tape;
  int64_t ts;
};

// An order the OrderUpdate stream still reports on, and whose owner may cancel it: every accepted
// LIMIT order from SubmitOrder until it stops resting.
struct Live {
  std::string client;
  std::string symbol;
  int32_t remaining;
  uint32_t sid;  // its book (reference-counted: a book with live orders is never handed over)
  bool filled = false;  // it has traded: a reduce reports it PARTIALLY_FILLED, else NEW
};

constexpr size_t kMaxQueuedUpdates = size_t(1) << 24;  // oldest events are dropped beyond this
constexpr int kRows = 64;  // rows per multi-row INSERT (11 * 64 parameters < SQLite's 999 floor)
constexpr size_t kMaxMatchedAhead = 4;  // matched slices the flusher may run ahead of the persister

// ---- the backend: everything the service asks of what matches its slices -------------------------
// Built in two places, backend_of(me_engine*) and backend_of(const me_matcher*); the rest of the file calls
// through it and never asks which of the two it fronts. A facility the backend lacks is a NULL pointer
// (`book` NULL: no backend at all). The reads and enables follow me_engine.h's contracts of the same names.
struct Backend {
  void* ctx = nullptr;
  // submit / collect, both or neither: a slice now, its outputs later (two slices in flight). Without them
  // `match` does both at once and one slice is in flight.
  decltype(me_matcher::submit) submit = nullptr;
  decltype(me_matcher::collect) collect = nullptr;
  decltype(me_matcher::match) match = nullptr;
  decltype(me_matcher::book) book = nullptr;
  int (*quotes_enable)(void*, uint64_t cap_events) = nullptr;  // NULL with `quotes` set: the feed needs no enabling
  decltype(me_matcher::quotes) quotes = nullptr;
  decltype(me_matcher::depth_enable) depth_enable = nullptr;
  decltype(me_matcher::depth) depth = nullptr;
  decltype(me_matcher::trades_enable) trades_enable = nullptr;
  decltype(me_matcher::trades) trades = nullptr;
  decltype(me_matcher::order_query) order_query = nullptr;
  decltype(me_matcher::order_preview) order_preview = nullptr;
  decltype(me_matcher::stops_enable) stops_enable = nullptr;  // the four together, or no stop orders
  decltype(me_matcher::stops_add) stops_add = nullptr;
  decltype(me_matcher::stops_cancel) stops_cancel = nullptr;
  decltype(me_matcher::stops_read) stops_read = nullptr;
  int (*mass_cancel)(void*, const uint32_t* symbols, const uint8_t* sides, size_t n, me_book_entry* out, size_t cap,
                     size_t* n_out, uint64_t* counts) = nullptr;
  std::string (*last_error)(void*) = nullptr;
  uint64_t (*fill_bound)(const Backend&, uint64_t n) = nullptr;  // fills n records can produce at most
  uint32_t num_symbols = UINT32_MAX;  // books it holds (local ids 0 .. num_symbols-1)
  uint32_t max_batch = 0;             // largest slice
  uint64_t max_resting = 0;           // (a matcher's fill bound)
  uint64_t seq_span = 1ull << 20;     // seqs one restart-recovery chunk may span
  // A failed submit other than ME_E_CAPACITY: the slice was taken and is lost (the service fails). Else only
  // ME_OK is "accepted" and every failure is a refusal that applied nothing.
  bool failure_loses_slice = false;
  // The depth and trade feeds and the stop orders the service turned on go off when it is destroyed (the
  // backend outlives it).
  bool feeds_off_at_destroy = false;
};

template <auto F, class... A>
int eng_call(void* e, A... a) {
  return F(static_cast<me_engine*>(e), a...);
}

Backend backend_of(me_engine* e) {
  Backend b;
  if (!e) return b;
  b.ctx = e;
  b.submit = eng_call<me_submit_host>;
  b.collect = [](void* e, uint64_t t, const me_fill** f, size_t* nf, const me_order_result** r) {
    size_t nr = 0;
    return me_collect(static_cast<me_engine*>(e), t, f, nf, r, &nr);
  };
  b.book = [](void* e, uint32_t sid, uint32_t depth, me_book_entry* bids, size_t bids_cap, size_t* n_bids,
              me_book_entry* asks, size_t asks_cap, size_t* n_asks, me_level* bl, me_level* al, size_t* nbl,
              size_t* nal) {
    if (!depth) depth = 0xFFFFFFFFu;  // the whole book: every window level plus the far levels
    return me_book_orders(static_cast<me_engine*>(e), sid, depth, bids, bids_cap, n_bids, asks, asks_cap, n_asks, bl,
                          al, nbl, nal);
  };
  b.quotes_enable = eng_call<me_quotes_enable>;
  b.quotes = eng_call<me_quotes_read>;
  b.depth_enable = eng_call<me_depth_enable>;
  b.depth = eng_call<me_depth_read>;
  b.trades_enable = eng_call<me_trades_enable>;
  b.trades = eng_call<me_trades_read>;
  b.order_query = eng_call<me_order_query>;
  b.order_preview = eng_call<me_order_preview>;
  b.stops_enable = eng_call<me_stops_enable>;
  b.stops_add = eng_call<me_stops_add>;
  b.stops_cancel = eng_call<me_stops_cancel>;
  b.stops_read = eng_call<me_stops_read>;
  b.mass_cancel = eng_call<me_mass_cancel>;
  b.last_error = [](void* e) {
    char t[512];
    me_last_error(static_cast<me_engine*>(e), t, sizeof t);
    return std::string(t);
  };
  b.fill_bound = [](const Backend& b, uint64_t n) { return me_fill_bound(static_cast<me_engine*>(b.ctx), n); };
  me_config c{};
  if (me_get_config(e, &c) == ME_OK) {
    b.num_symbols = c.num_symbols;
    b.max_batch = c.max_batch;
    // one launch group must span fewer seqs than the seq ring: a recovery chunk stays below half of it
    if (c.seq_ring) b.seq_span = std::max<uint64_t>(c.seq_ring / 2, 1);
  }
  // the flusher keeps two slices in flight, and me_collect holds the last collected slot back: three
  // warm pinned slots, so no slot is pinned inside the serving path
  me_host_reserve(e, 3);
  return b;
}

Backend backend_of(const me_matcher* m) {
  Backend b;
  b.ctx = m->ctx;
  if (m->submit && m->collect) {
    b.submit = m->submit;
    b.collect = m->collect;
  }
  b.match = m->match;
  b.book = m->book;
  b.quotes = m->quotes;  // (a matcher has no quote enable)
  b.depth_enable = m->depth_enable;
  b.depth = m->depth;
  b.trades_enable = m->trades_enable;
  b.trades = m->trades;
  b.order_query = m->order_query;
  b.order_preview = m->order_preview;
  if (m->stops_enable && m->stops_add && m->stops_cancel && m->stops_read) {
    b.stops_enable = m->stops_enable;
    b.stops_add = m->stops_add;
    b.stops_cancel = m->stops_cancel;
    b.stops_read = m->stops_read;
  }
  b.last_error = [](void*) { return std::string("matcher failed"); };
  b.fill_bound = [](const Backend& b, uint64_t n) { return b.max_resting + 2 * n; };
  b.num_symbols = m->num_symbols;
  b.max_batch = m->max_batch;
  b.max_resting = m->max_resting;
  b.failure_loses_slice = true;
  b.feeds_off_at_destroy = true;
  return b;
}

}  // namespace

struct me_service {
  Backend be;
  size_t slice_max = 0;         // records per slice (the backend's max_batch, or me_service_start's)
  // --- mu
  std::mutex mu;
  std::unordered_map<std::string, uint32_t> sym;
  std::vector<std::string> names;
  uint64_t next_id = 1;
  Slice open;
  std::deque<Slice> closed;
  size_t closed_records = 0;
  size_t inflight_records = 0;  // taken off `closed`, not yet in pq (being matched)
  // --- flush_mu
  std::mutex flush_mu;
  // --- pq_mu: matched slices, oldest first, until committed (the persister thread owns the DB)
  std::mutex pq_mu;
  std::condition_variable pq_cv;
  std::deque<Matched> pq;
  size_t pq_emitted = 0;    // slices at the head of pq whose OrderUpdates are out
  size_t pq_records = 0;
  bool pq_stalled = false;  // the head's transaction failed: retried when the next flush starts
  bool pq_stop = false;
  std::string pq_err;
  std::thread persister;
  // --- eng_mu
  std::mutex eng_mu;
  // --- live_mu / upd_mu
  std::mutex live_mu;
  std::unordered_map<uint64_t, Live> live;
  std::mutex upd_mu;
  std::deque<me_order_update> updates;
  uint64_t updates_dropped = 0;
  // --- ref_mu: per book, live-table entries of its symbol + its records not yet emitted. A book at 0
  // holds no resting order and has nothing on its way: a new symbol may take it over.
  std::mutex ref_mu;
  std::vector<int64_t> sref;
  std::vector<uint32_t> idle;     // books whose count reached 0 (checked again when taken) ...
  std::vector<uint8_t> in_idle;   // ... each at most once: a book's count returns to 0 again and again
  uint64_t reclaimed = 0;
  uint64_t recovered = 0;
  // --- md_mu: the three change streams (me_service_market_ / _depth_ / _trades_ subscribe and stream). Lock
  // order: flush_mu, eng_mu, md_mu. Each is a me::ServiceFeed (me_service_feed.hpp): one pending item per
  // symbol name in first-change order, and its own history of which symbol owned a book from which slice on.
  std::mutex md_mu;
  me::ServiceFeed<me_market_update, sizeof(me_market_update::symbol) - 1> md;  // the pending quote
  // The backend sends depth deltas, the service materialises views: dp_view holds every named symbol's top-D
  // {price: qty} per side, and dp queues the names whose view changed since it was last handed out.
  struct DepthView {
    std::map<int64_t, int64_t> side[2];  // [0] bids, [1] asks, ascending price
  };
  struct Changed {};
  me::ServiceFeed<Changed, sizeof(me_depth_book::symbol) - 1> dp;
  std::unordered_map<std::string, DepthView> dp_view;
  // The pending trade update, and the names' totals since the subscription.
  me::ServiceFeed<me_trade_update, sizeof(me_trade_update::symbol) - 1> tr;
  std::unordered_map<std::string, std::pair<int64_t, uint64_t>> tr_cum;
  uint64_t nsub = 0;  // slices the backend accepted since create (eng_mu): slice k's events are stamped k
  // --- stop orders (me_service_stops.hpp). mu: whether they are on, the SID counter, the stops held, the
  // capacity mirror. flush_mu: the events read and held back, the slices collected. upd_mu: the stop updates.
  uint64_t stops_cap = 0;  // 0: off
  uint64_t next_sid = 1;
  std::map<uint64_t, Stop> stops;  // QUEUED and ARMED, ascending id
  me::StopLedger stop_ledger;
  uint64_t stops_triggered = 0;
  uint64_t stops_recovered = 0;
  me::StopHold stop_hold;
  uint64_t ncol = 0;  // slices collected since create: an event is due once its stamp is <= ncol
  std::deque<me_stop_update> stop_updates;
  // --- background flusher
  std::thread flusher;
  std::condition_variable cv;  // with mu
  bool stop = false;
  int64_t interval_us = 0;
  // --- persistence (the persister thread; create/destroy otherwise)
  sqlite3* db = nullptr;
  sqlite3_stmt* st_ins = nullptr;
  sqlite3_stmt* st_upd = nullptr;
  sqlite3_stmt* st_fill = nullptr;
  sqlite3_stmt* st_maker = nullptr;
  sqlite3_stmt* st_reduce = nullptr;  // an earlier slice's order, reduced in place: remaining only
  sqlite3_stmt* st_ins_k = nullptr;   // kRows-row INSERT INTO orders
  sqlite3_stmt* st_fill_k = nullptr;  // kRows-row INSERT INTO fills
  sqlite3_stmt* st_stop_ins = nullptr;  // the `stops` table (me_service_stops_enable prepares them)
  sqlite3_stmt* st_stop_upd = nullptr;
  bool failed = false;  // the engine lost a slice it had accepted: nothing more can be matched
  // --- err_mu
  mutable std::mutex err_mu;
  std::string err;

  int fail(int code, const std::string& m) {
    std::lock_guard<std::mutex> lk(err_mu);
    err = m;
    return code;
  }
  std::string sql_err(const char* what) { return std::string(what) + ": " + (db ? g_sql.errmsg(db) : "no db"); }
};

static void close_db(me_service* s) {
  for (sqlite3_stmt* st : {s->st_ins, s->st_upd, s->st_fill, s->st_maker, s->st_reduce, s->st_ins_k, s->st_fill_k,
                           s->st_stop_ins, s->st_stop_upd})
    if (st) g_sql.finalize(st);
  s->st_ins = s->st_upd = s->st_fill = s->st_maker = s->st_reduce = s->st_ins_k = s->st_fill_k = nullptr;
  s->st_stop_ins = s->st_stop_upd = nullptr;
  if (s->db) g_sql.close(s->db);
  s->db = nullptr;
}

static void persister_main(me_service* s);
static bool has_backend(const me_service* s);

static bool sql_ok(int rc) { return rc == SQLITE_OK || rc == SQLITE_DONE || rc == SQLITE_ROW; }

static bool open_db(me_service* s, const char* path, std::string& err) {
  {
    std::lock_guard<std::mutex> lk(g_sql_mu);
    if (!g_sql.load(err)) return false;
  }
  auto chk = [&](int rc, const char* what) {
    if (sql_ok(rc)) return true;
    err = s->sql_err(what);
    return false;
  };
  if (!chk(g_sql.open_v2(path, &s->db, SQLITE_OPEN_READWRITE | SQLITE_OPEN_CREATE | SQLITE_OPEN_FULLMUTEX, nullptr),
           "open"))
    return false;
  g_sql.busy_timeout(s->db, 5000);  // storage.cpp:14
  // storage.cpp:17-24 pragmas, then the schema
  if (!chk(g_sql.exec(s->db, "PRAGMA journal_mode=WAL;", nullptr, nullptr, nullptr), "pragma") ||
      !chk(g_sql.exec(s->db, "PRAGMA synchronous=NORMAL;", nullptr, nullptr, nullptr), "pragma") ||
      !chk(g_sql.exec(s->db, "PRAGMA foreign_keys=ON;", nullptr, nullptr, nullptr), "pragma") ||
      !chk(g_sql.exec(s->db, kSchema, nullptr, nullptr, nullptr), "schema"))
    return false;
  // load_next_oid_seq (storage.cpp:254-267)
  sqlite3_stmt* q = nullptr;
  if (!chk(g_sql.prepare_v2(s->db,
                            "SELECT COALESCE(MAX(CAST(SUBSTR(order_id, 5) AS INTEGER)), 0) + 1 "
                            "FROM orders WHERE order_id LIKE 'OID-%'",
                            -1, &q, nullptr),
           "prepare oid"))
    return false;
  if (g_sql.step(q) == SQLITE_ROW) s->next_id = (uint64_t)g_sql.column_int64(q, 0);
  g_sql.finalize(q);
  // cached statements (the reference prepares a fresh one per call, storage.cpp:95)
  const char* ins =
      "INSERT INTO orders(order_id, client_id, symbol, side, order_type, price, quantity, status,"
      " remaining_quantity, created_ts, updated_ts) VALUES (?,?,?,?,?,?,?,?,?,?,?)";
  const char* upd = "UPDATE orders SET status=?, remaining_quantity=?, updated_ts=? WHERE order_id=?";
  const char* fill = "INSERT INTO fills(order_id, symbol, fill_price, fill_quantity, event_ts) VALUES (?,?,?,?,?)";
  const char* maker =
      "UPDATE orders SET remaining_quantity=remaining_quantity-?, status=CASE WHEN remaining_quantity-?=0 "
      "THEN 2 ELSE 1 END, updated_ts=? WHERE order_id=?";
  const char* reduce = "UPDATE orders SET remaining_quantity=remaining_quantity-?, updated_ts=? WHERE order_id=?";
  // multi-row forms: one statement step per kRows rows
  auto rows = [](const char* head, const char* tuple) {
    std::string q(head);
    for (int r = 0; r < kRows; ++r) q += (r ? "," : "") + std::string(tuple);
    return q;
  };
  const std::string ins_k = rows("INSERT INTO orders(order_id, client_id, symbol, side, order_type, price, quantity, "
                                 "status, remaining_quantity, created_ts, updated_ts) VALUES ",
                                 "(?,?,?,?,?,?,?,?,?,?,?)");
  const std::string fill_k =
      rows("INSERT INTO fills(order_id, symbol, fill_price, fill_quantity, event_ts) VALUES ", "(?,?,?,?,?)");
  return chk(g_sql.prepare_v2(s->db, ins, -1, &s->st_ins, nullptr), "prepare insert") &&
         chk(g_sql.prepare_v2(s->db, upd, -1, &s->st_upd, nullptr), "prepare update") &&
         chk(g_sql.prepare_v2(s->db, fill, -1, &s->st_fill, nullptr), "prepare fill") &&
         chk(g_sql.prepare_v2(s->db, maker, -1, &s->st_maker, nullptr), "prepare maker") &&
         chk(g_sql.prepare_v2(s->db, reduce, -1, &s->st_reduce, nullptr), "prepare reduce") &&
         chk(g_sql.prepare_v2(s->db, ins_k.c_str(), -1, &s->st_ins_k, nullptr), "prepare insert rows") &&
         chk(g_sql.prepare_v2(s->db, fill_k.c_str(), -1, &s->st_fill_k, nullptr), "prepare fill rows");
}

// ---- per-book reference counts ----------------------------------------------------------------
static void ref_add(me_service* s, uint32_t sid, int64_t d) {
  if (sid == kNoBook || d == 0) return;
  std::lock_guard<std::mutex> lr(s->ref_mu);
  if (sid >= s->sref.size()) return;
  int64_t& r = s->sref[sid];
  r += d;
  if (r == 0 && !s->in_idle[sid]) {
    s->in_idle[sid] = 1;
    s->idle.push_back(sid);
  }
}

// Symbol string -> local book id (mu held). The reference accepts any non-empty symbol
// (matching_engine_service.cpp:66-71) and keeps it forever; the backend holds sym_cap books. A new
// symbol takes the next unused book, else a book whose symbol has no live order and no record on its
// way (its count is 0 under ref_mu, and only this thread, holding mu, could raise it): the old symbol's
// book is empty, so handing it over changes no order's outcome; the window re-centres on the new
// symbol's first rest. False only when every book is in use.
static bool intern(me_service* s, const std::string& symbol, uint32_t& sid) {
  auto it = s->sym.find(symbol);
  if (it != s->sym.end()) {
    sid = it->second;
    return true;
  }
  std::lock_guard<std::mutex> lr(s->ref_mu);
  if (s->names.size() < s->be.num_symbols) {
    sid = (uint32_t)s->names.size();
    s->names.push_back(symbol);
    s->sym.emplace(symbol, sid);
    s->sref.push_back(0);
    s->in_idle.push_back(0);
    return true;
  }
  while (!s->idle.empty()) {
    const uint32_t c = s->idle.back();
    s->idle.pop_back();
    if (c < s->in_idle.size()) s->in_idle[c] = 0;
    if (c >= s->sref.size() || s->sref[c] != 0) continue;  // busy again since it went idle
    s->sym.erase(s->names[c]);
    s->names[c] = symbol;
    s->sym.emplace(symbol, c);
    s->reclaimed++;
    sid = c;
    return true;
  }
  return false;
}

static int flush_closed(me_service* s, bool take_open, size_t limit, struct FlushOut* out, bool wait);

// Restart recovery: the orders the DB shows resting (status NEW / PARTIALLY_FILLED, remaining > 0) as
// LIMIT records in OID order, with their remainders — replayed into the backend before any new
// order, so each keeps its place in its level's FIFO. Chunks of at most slice_max records spanning
// fewer than half the engine's seq ring, each matched alone (one launch group must span fewer seqs than
// the seq ring, and old resting orders can be sparse).
static bool load_resting(me_service* s, std::string& err) {
  sqlite3_stmt* q = nullptr;
  if (!sql_ok(g_sql.prepare_v2(s->db,
                               "SELECT order_id, client_id, symbol, side, price, remaining_quantity, status FROM orders "
                               "WHERE status IN (0, 1) AND remaining_quantity > 0 AND order_id LIKE 'OID-%' "
                               "ORDER BY CAST(SUBSTR(order_id, 5) AS INTEGER)",
                               -1, &q, nullptr))) {
    err = s->sql_err("prepare recovery");
    return false;
  }
  const size_t cap = s->slice_max ? s->slice_max : 65536;
  // a recovery chunk is matched alone (flush_closed collects it before the next submit), so one launch
  // group spans only its own OIDs: below half the engine's seq ring (a matcher: 2^20)
  const uint64_t span = s->be.seq_span;
  bool ok = true;
  std::lock_guard<std::mutex> lk(s->mu);
  Slice cur;
  cur.recovery = true;
  auto close_chunk = [&] {
    if (!cur.size()) return;
    s->closed_records += cur.size();
    s->closed.push_back(std::move(cur));
    cur = Slice{};
    cur.recovery = true;
  };
  for (int rc; (rc = g_sql.step(q)) == SQLITE_ROW;) {
    const char* oid_s = (const char*)g_sql.column_text(q, 0);
    const char* cl = (const char*)g_sql.column_text(q, 1);
    const char* sy = (const char*)g_sql.column_text(q, 2);
    const uint64_t oid = oid_s ? strtoull(oid_s + 4, nullptr, 10) : 0;
    const int32_t side = (int32_t)g_sql.column_int64(q, 3);
    const int64_t px = g_sql.column_int64(q, 4);
    const long long rem = g_sql.column_int64(q, 5);
    if (!oid || (side != ME_SIDE_BUY && side != ME_SIDE_SELL) || rem <= 0 || rem > INT32_MAX) continue;
    const std::string symbol = sy ? sy : "";
    uint32_t sid = 0;
    if (!intern(s, symbol, sid)) {
      err = "restart recovery: the DB holds resting orders on more symbols than the backend has books";
      ok = false;
      break;
    }
    if (cur.size() >= cap || (cur.size() && oid - cur.seq.front() >= span)) close_chunk();
    cur.seq.push_back(oid);
    cur.px.push_back(px);
    cur.qty.push_back((int32_t)rem);
    cur.sid.push_back(sid);
    cur.kind.push_back(ME_KIND(side, ME_TYPE_LIMIT, ME_OP_NEW));
    cur.meta.push_back(Pending{cl ? cl : "", symbol, side, false, 0});
    {
      std::lock_guard<std::mutex> lv(s->live_mu);
      // (PARTIALLY_FILLED in the row: it traded in an earlier run)
      s->live[oid] = Live{cl ? cl : "", symbol, (int32_t)rem, sid, g_sql.column_int64(q, 6) == ME_ST_PARTIALLY_FILLED};
    }
    ref_add(s, sid, 1);
    s->recovered++;
  }
  g_sql.finalize(q);
  close_chunk();
  return ok;
}

static me_service* create(const Backend& be, const char* const* symbols, uint32_t num_symbols, const char* db_path) {
  me_service* s = new me_service();
  s->be = be;
  s->slice_max = be.max_batch;
  for (uint32_t i = 0; i < num_symbols; ++i) {
    s->names.emplace_back(symbols[i]);
    s->sym.emplace(s->names.back(), i);
    s->sref.push_back(0);
    s->in_idle.push_back(1);
  }
  for (uint32_t i = num_symbols; i-- > 0;) s->idle.push_back(i);  // nothing rests on them yet
  if (s->names.size() > s->be.num_symbols) s->fail(ME_E_INVALID, "me_service_create: more symbols than the engine holds");
  std::string err;
  if (db_path && !open_db(s, db_path, err)) {
    // keep the object so the caller can read the error; persistence is disabled
    close_db(s);
    s->fail(ME_E_SQLITE, "me_service_create: " + err);
  }
  s->persister = std::thread(persister_main, s);
  if (s->db && has_backend(s)) {  // rebuild the books from the DB before the first SubmitOrder
    if (!load_resting(s, err)) {
      s->failed = true;
      s->fail(ME_E_CAPACITY, "me_service_create: " + err);
    } else {
      std::lock_guard<std::mutex> lf(s->flush_mu);
      const int rc = flush_closed(s, false, SIZE_MAX, nullptr, true);
      if (rc != ME_OK) {
        s->failed = true;
        std::string e;
        {
          std::lock_guard<std::mutex> le(s->err_mu);
          e = s->err;
        }
        s->fail(rc, "me_service_create: restart recovery failed: " + e);
      }
    }
  }
  return s;
}

extern "C" me_service* me_service_create(me_engine* engine, const char* const* symbols, uint32_t num_symbols,
                                         const char* db_path) {
  return create(backend_of(engine), symbols, num_symbols, db_path);
}

extern "C" me_service* me_service_create_matcher(const me_matcher* m, const char* const* symbols,
                                                 uint32_t num_symbols, const char* db_path) {
  if (!m || !m->match || !m->book || !m->max_batch) return nullptr;
  return create(backend_of(m), symbols, num_symbols, db_path);
}

// (a service created without an engine takes orders and answers every call that needs a backend with an error)
static bool has_backend(const me_service* s) { return s->be.book != nullptr; }

static std::string backend_err(me_service* s) { return s->be.last_error(s->be.ctx); }

// A slice handed to the backend and not collected yet.
struct Inflight {
  Slice sl;
  uint64_t ticket = 0;
  bool done = false;  // outputs already here (a matcher without submit / collect matches at once)
  std::vector<me_order_result> res;
  std::vector<me_fill> tape;
  // Stop updates of a boundary applied while this slice was in flight: queued once the slice is collected and
  // its events processed, where a backend with one slice in flight queues them (the stream's order, not the
  // pipeline's).
  std::vector<me_stop_update> post;
};

// Hand one slice to the backend (eng_mu held). accepted = the backend took it (a later failure loses
// it); ME_E_CAPACITY with accepted false: refused, nothing of it was applied.
static int backend_submit(me_service* s, Inflight& f, bool& accepted) {
  const Backend& be = s->be;
  Slice& sl = f.sl;
  const size_t n = sl.size();
  me_order_soa b{sl.seq.data(), sl.px.data(), sl.qty.data(), sl.sid.data(), sl.kind.data()};
  const me_fill* tape = nullptr;
  const me_order_result* res = nullptr;
  size_t nf = 0;
  const int rc = be.submit ? be.submit(be.ctx, &b, n, &f.ticket) : be.match(be.ctx, &b, n, &tape, &nf, &res);
  accepted = be.failure_loses_slice ? rc != ME_E_CAPACITY : rc == ME_OK;
  if (rc != ME_OK || be.submit) return rc;
  // matched at once, and the output views stay valid until the backend's next call: copy them out under eng_mu
  f.res.assign(res, res + n);
  f.tape.assign(tape, tape + nf);
  f.done = true;
  return ME_OK;
}

// The outputs of an accepted slice (eng_mu held), copied out of the backend's buffers.
static int backend_collect(me_service* s, Inflight& f) {
  if (f.done) return ME_OK;
  const me_fill* tape = nullptr;
  const me_order_result* res = nullptr;
  size_t nf = 0;
  const int rc = s->be.collect(s->be.ctx, f.ticket, &tape, &nf, &res);
  if (rc != ME_OK) return rc;
  f.res.assign(res, res + f.sl.size());
  f.tape.assign(tape, tape + nf);
  f.done = true;
  return ME_OK;
}

static void put(char* dst, size_t cap, const std::string& v) {
  size_t k = v.size() < cap - 1 ? v.size() : cap - 1;
  memcpy(dst, v.data(), k);
  dst[k] = 0;
}

// ---- the change streams: quotes (md), depth (dp), trades (tr) -----------------------------------
static int md_pull(me_service* s);
static int dp_pull(me_service* s);
static int tr_pull(me_service* s);

// f(feed, its pull) for each of the three, in the order they are read after a slice.
template <class F>
static void each_feed(me_service* s, F&& f) {
  f(s->md, md_pull);
  f(s->dp, dp_pull);
  f(s->tr, tr_pull);
}

// Slice number k was accepted by the backend (eng_mu held): the symbols that own its records' books from
// slice k on, in every enabled feed's own history.
static void md_note_owners(me_service* s, const Slice& sl, uint64_t k) {
  bool any = false;
  each_feed(s, [&](auto& f, auto) { any |= f.on; });
  if (!any) return;
  std::lock_guard<std::mutex> lm(s->md_mu);
  for (size_t i = 0; i < sl.size(); ++i) {
    if (sl.sid[i] == kNoBook) continue;
    each_feed(s, [&](auto& f, auto) {
      if (f.on) f.note(sl.sid[i], k, sl.meta[i].symbol);
    });
  }
}

// Read a feed's events from the backend, `room` at a time, until none is left (eng_mu held). An event is
// named by the symbol that owned its book at slice `batches` (a book no slice ever named: skipped) and
// applied under md_mu: apply(event, name); popped(name) for each owner its stamp has passed.
template <class Ev, class Feed, class Popped, class Apply>
static int feed_pull(me_service* s, Feed& f, int (*read)(void*, Ev*, size_t, size_t*, size_t*), size_t room,
                     const char* read_failed, Popped&& popped, Apply&& apply) {
  std::vector<Ev> buf(room);
  for (;;) {
    size_t n = 0, left = 0;
    const int rc = read(s->be.ctx, buf.data(), buf.size(), &n, &left);
    if (rc != ME_OK) return s->fail(rc, read_failed + backend_err(s));
    std::lock_guard<std::mutex> lm(s->md_mu);
    for (size_t i = 0; i < n; ++i)
      if (const std::string* name = f.owner_at(buf[i].symbol, buf[i].batches, popped)) apply(buf[i], *name);
    if (!left) return ME_OK;
  }
}

// Depth events set or erase a level of the name's view and queue the name. A book changes hands only when
// it is empty: the symbol that loses it ends with an empty view, whatever the conflated events said.
static int dp_pull(me_service* s) {
  auto& f = s->dp;
  return feed_pull<me_depth_event>(
      s, f, s->be.depth, 4096, "depth stream: reading the backend's depth feed failed: ",
      [&](const std::string& old_name) {
        auto old = s->dp_view.find(f.key_of(old_name));
        if (old != s->dp_view.end() && (!old->second.side[0].empty() || !old->second.side[1].empty())) {
          old->second.side[0].clear();
          old->second.side[1].clear();
          f.pending(old->first);
        }
      },
      [&](const me_depth_event& ev, const std::string& name) {
        auto& side = s->dp_view[f.key_of(name)].side[ev.side == ME_SIDE_SELL ? 1 : 0];  // views are keyed as handed out
        if (ev.qty > 0)
          side[ev.price_q4] = ev.qty;
        else
          side.erase(ev.price_q4);
        f.pending(name);
      });
}

// Quote events conflate: the newer update replaces the name's pending one, in its place.
static int md_pull(me_service* s) {
  auto sat = [](int64_t v) { return (int32_t)(v > INT32_MAX ? INT32_MAX : v); };
  return feed_pull<me_quote>(
      s, s->md, s->be.quotes, 1024, "market stream: reading the backend's quote feed failed: ",
      [](const std::string&) {},
      [&](const me_quote& q, const std::string& name) {
        me_market_update u;
        memset(&u, 0, sizeof u);
        put(u.symbol, sizeof u.symbol, name);
        u.md.scale = 4;
        if (q.flags & ME_QUOTE_HAS_BID) {
          u.md.has_bid = 1;
          u.md.best_bid = q.bid_price_q4;
          u.md.bid_size = sat(q.bid_qty);
        }
        if (q.flags & ME_QUOTE_HAS_ASK) {
          u.md.has_ask = 1;
          u.md.best_ask = q.ask_price_q4;
          u.md.ask_size = sat(q.ask_qty);
        }
        s->md.pending(name) = u;
      });
}

// Trade events merge into the name's pending update; the names' totals are summed from the events' own
// volume and trades (a reused book's device counters span two names).
static int tr_pull(me_service* s) {
  return feed_pull<me_trade>(
      s, s->tr, s->be.trades, 1024, "trade stream: reading the backend's trade feed failed: ",
      [](const std::string&) {},
      [&](const me_trade& ev, const std::string& name) {
        me_trade_update u;
        memset(&u, 0, sizeof u);
        put(u.symbol, sizeof u.symbol, name);
        auto& cum = s->tr_cum[u.symbol];  // (the name as the update carries it)
        cum.first += ev.volume;
        cum.second += ev.trades;
        u.scale = 4;
        u.last_size = ev.last_qty;
        u.last_price = ev.last_price_q4;
        u.open_price = ev.open_price_q4;
        u.high_price = ev.high_price_q4;
        u.low_price = ev.low_price_q4;
        u.volume = ev.volume;
        u.trades = ev.trades;
        u.cum_volume = cum.first;
        u.cum_trades = cum.second;
        bool fresh = false;
        me_trade_update& p = s->tr.pending(name, &fresh);
        if (!fresh) {  // merge into the pending update, which keeps its place
          u.open_price = p.open_price;
          u.high_price = std::max(u.high_price, p.high_price);
          u.low_price = std::min(u.low_price, p.low_price);
          u.volume += p.volume;
          u.trades += p.trades;
        }
        p = u;
      });
}

// Close the open slice (mu held). One without records but with a boundary in front of it closes too: a
// boundary-only slice, which the flush path applies and never submits.
static void close_open(me_service* s) {
  if (!s->open.size() && s->open.pre.empty()) return;
  s->closed_records += s->open.size();
  s->closed.push_back(std::move(s->open));
  s->open = Slice{};
  s->cv.notify_all();
}

// Append a record to the open slice (mu held); a full slice is closed and handed to the flusher.
static void append(me_service* s, uint64_t seq, int64_t px, int32_t qty, uint32_t sid, uint8_t kind, Pending&& m) {
  Slice& o = s->open;
  if (!o.size() && o.pre.empty()) o.opened_us = mono_us();  // (a boundary started the clock already)
  o.seq.push_back(seq);
  o.px.push_back(px);
  o.qty.push_back(qty);
  o.sid.push_back(sid);
  o.kind.push_back(kind);
  o.meta.push_back(std::move(m));
  if (s->slice_max && o.size() >= s->slice_max) close_open(s);
}

extern "C" int me_service_submit_order(me_service* s, const me_order_request* r, me_order_response* resp) {
  return me_service_submit_order_tif(s, r, ME_TIF_GTC, resp);
}

extern "C" int me_service_submit_order_tif(me_service* s, const me_order_request* r, int32_t tif,
                                           me_order_response* resp) {
  memset(resp, 0, sizeof(*resp));
  const char* symbol = r->symbol ? r->symbol : "";
  // --- validation (:66-83): first failing check wins, no OID
  if (!symbol[0]) {
    put(resp->error_message, sizeof resp->error_message, "symbol is required");
    return 0;
  }
  if (r->quantity <= 0) {
    put(resp->error_message, sizeof resp->error_message, "quantity must be > 0");
    return 0;
  }
  if (r->order_type == ME_TYPE_LIMIT && r->price <= 0) {
    put(resp->error_message, sizeof resp->error_message, "price must be > 0 for LIMIT");
    return 0;
  }
  // --- time in force (build extension): after the reference's own checks, no OID either
  if (tif < ME_TIF_GTC || tif > ME_TIF_POST_ONLY || (tif == ME_TIF_POST_ONLY && r->order_type != ME_TYPE_LIMIT)) {
    put(resp->error_message, sizeof resp->error_message, "invalid time in force");
    return 0;
  }
  const std::string sym(symbol);
  std::string client = r->client_id ? r->client_id : "";
  std::lock_guard<std::mutex> lk(s->mu);
  uint32_t sid = 0;
  if (!intern(s, sym, sid)) {  // the engine's books are all taken: RESOURCE_EXHAUSTED, no OID
    resp->grpc_status = 8;
    put(resp->error_message, sizeof resp->error_message, "symbol capacity exhausted");
    return 0;
  }
  // --- OID (:85), consumed even if normalisation throws below
  const uint64_t id = s->next_id++;
  int64_t q4 = 0;
  const int nr = me_normalize_to_q4(r->price, r->scale, &q4);
  if (nr != 0) {  // exception escapes the handler -> gRPC UNKNOWN, no order_id in the response
    resp->grpc_status = 2;
    put(resp->error_message, sizeof resp->error_message,
        nr == 1 ? "scale out of range" : (nr == 2 ? "overflow" : "underflow"));
    return 0;
  }
  const std::string oid = "OID-" + std::to_string(id);
  put(resp->order_id, sizeof resp->order_id, oid);
  // --- the reference's DB CHECK side IN (1,2) (storage.cpp:32) -> "DB insert failed" (:109-111)
  if (r->side != ME_SIDE_BUY && r->side != ME_SIDE_SELL) {
    resp->success = 0;
    put(resp->error_message, sizeof resp->error_message, "DB insert failed");
    return 0;
  }
  resp->success = 1;
  const bool limit = r->order_type == ME_TYPE_LIMIT;
  const uint8_t kd = ME_KIND_TIF(r->side, limit ? ME_TYPE_LIMIT : ME_TYPE_MARKET, ME_OP_NEW, tif);
  if (limit && tif != ME_TIF_IOC && tif != ME_TIF_FOK) {  // may rest: its owner, for CancelOrder and the OrderUpdate stream
    std::lock_guard<std::mutex> lv(s->live_mu);
    s->live[id] = Live{client, sym, r->quantity, sid};
  }
  ref_add(s, sid, 1);  // a resting LIMIT's live entry, or a MARKET / IOC / FOK record on its way
  append(s, id, q4, r->quantity, sid, kd, Pending{std::move(client), sym, r->side, false, 0});
  return 0;
}

extern "C" int me_service_submit_orders(me_service* s, const me_order_request* reqs, size_t n,
                                        me_order_response* resps) {
  for (size_t i = 0; i < n; ++i) me_service_submit_order(s, reqs + i, resps + i);
  return 0;
}

// "OID-<n>", n >= 1 with no trailing characters -> n; else 0.
static uint64_t parse_oid(const char* s) {
  if (!s || strncmp(s, "OID-", 4) != 0 || !s[4]) return 0;
  uint64_t v = 0;
  for (const char* p = s + 4; *p; ++p) {
    if (*p < '0' || *p > '9' || v > (UINT64_MAX - 9) / 10) return 0;
    v = v * 10 + (uint64_t)(*p - '0');
  }
  return v;
}

// CancelOrder and ReduceOrder: the same checks, owner rule, stream position and record, apart from the kind
// byte and the quantity (reduce: take d off the target; a cancel's qty is 0 and ignored).
static int cancel_or_reduce(me_service* s, const char* client_id, const char* symbol_c, const char* order_id,
                            bool reduce, int32_t d, me_order_response* resp) {
  memset(resp, 0, sizeof(*resp));
  const char* symbol = symbol_c ? symbol_c : "";
  if (!symbol[0]) {
    put(resp->error_message, sizeof resp->error_message, "symbol is required");
    return 0;
  }
  if (reduce && d <= 0) {  // SubmitOrder's check and text (:72-77)
    put(resp->error_message, sizeof resp->error_message, "quantity must be > 0");
    return 0;
  }
  const uint64_t target = parse_oid(order_id);
  if (!target) {
    put(resp->error_message, sizeof resp->error_message, "order_id is invalid");
    return 0;
  }
  const std::string client = client_id ? client_id : "";
  const std::string sym(symbol);
  std::lock_guard<std::mutex> lk(s->mu);
  {  // only the order's owner may cancel it
    std::lock_guard<std::mutex> lv(s->live_mu);
    auto it = s->live.find(target);
    if (it != s->live.end() && it->second.client != client) {
      put(resp->error_message, sizeof resp->error_message, "order belongs to another client");
      return 0;
    }
  }
  // A symbol with no book has no resting order: the record goes out with an id the backend rejects
  // (BAD_SYMBOL -> OrderUpdate REJECTED) and takes no book.
  auto it = s->sym.find(sym);
  const uint32_t sid = it != s->sym.end() ? it->second : kNoBook;
  // Stream position: the last OID allocated, consuming none (a cancel record may repeat the previous
  // record's seq, me_engine.h), so accepted orders keep the reference's gap-free OIDs (:29-32, :85).
  const uint64_t id = s->next_id - 1;
  put(resp->order_id, sizeof resp->order_id, "OID-" + std::to_string(target));
  resp->success = 1;
  ref_add(s, sid, 1);
  append(s, id, (int64_t)target, reduce ? d : 0, sid,
         reduce ? ME_KIND_REDUCE : ME_KIND(ME_SIDE_BUY, ME_TYPE_LIMIT, ME_OP_CANCEL),
         Pending{client, sym, 0, true, target, reduce, reduce ? d : 0});
  return 0;
}

extern "C" int me_service_cancel_order(me_service* s, const me_cancel_request* r, me_order_response* resp) {
  return cancel_or_reduce(s, r->client_id, r->symbol, r->order_id, false, 0, resp);
}

extern "C" int me_service_reduce_order(me_service* s, const me_reduce_request* r, me_order_response* resp) {
  return cancel_or_reduce(s, r->client_id, r->symbol, r->order_id, true, r->quantity, resp);
}

// ---- stop orders: the request path (the flush path's half is further down) ------------------------------
static_assert(sizeof(me_stop_update) == 200, "me_stop_update layout");

static me_stop_update stop_update(uint64_t id, const std::string& client, const Stop& st, int32_t state,
                                  uint64_t oid = 0, int64_t trigger_px = 0) {
  me_stop_update u;
  memset(&u, 0, sizeof u);
  put(u.stop_id, sizeof u.stop_id, me::print_sid(id));
  if (oid) put(u.order_id, sizeof u.order_id, "OID-" + std::to_string(oid));
  put(u.client_id, sizeof u.client_id, client);
  put(u.symbol, sizeof u.symbol, st.symbol);
  u.state = state;
  u.scale = 4;
  u.stop_price = st.stop_px;
  u.limit_price = st.limit_px;
  u.trigger_price = trigger_px;
  u.quantity = st.qty;
  u.kind = st.kind;
  return u;
}

// A stop operation takes its place in the stream (mu held): behind every record submitted so far, in the
// boundary in front of the next slice.
static void boundary_add(me_service* s, StopOp&& op) {
  if (s->open.size()) close_open(s);
  if (s->open.pre.empty()) s->open.opened_us = mono_us();
  s->open.pre.push_back(std::move(op));
  s->cv.notify_all();
}

extern "C" int me_service_submit_stop(me_service* s, const me_stop_request* r, me_order_response* resp) {
  if (!resp) return 0;
  memset(resp, 0, sizeof(*resp));
  if (!s || !r) {
    put(resp->error_message, sizeof resp->error_message, "stop orders are not enabled");
    return 0;
  }
  auto refuse = [&](const char* why, int32_t grpc = 0) {
    resp->grpc_status = grpc;
    put(resp->error_message, sizeof resp->error_message, why);
    return 0;
  };
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->stops_cap) return refuse("stop orders are not enabled");
  const char* symbol = r->symbol ? r->symbol : "";
  if (!symbol[0]) return refuse("symbol is required");
  if (r->quantity <= 0) return refuse("quantity must be > 0");
  const bool limit = r->order_type == ME_TYPE_LIMIT;
  if (limit && r->price <= 0) return refuse("price must be > 0 for LIMIT");
  if (r->tif < ME_TIF_GTC || r->tif > ME_TIF_POST_ONLY || (r->tif == ME_TIF_POST_ONLY && !limit))
    return refuse("invalid time in force");
  int64_t q4 = 0, stop_q4 = 0;
  int nr = limit ? me_normalize_to_q4(r->price, r->scale, &q4) : 0;
  if (nr == 0) nr = me_normalize_to_q4(r->stop_price, r->scale, &stop_q4);
  if (nr != 0) return refuse(nr == 1 ? "scale out of range" : (nr == 2 ? "overflow" : "underflow"), 2);
  if (r->side != ME_SIDE_BUY && r->side != ME_SIDE_SELL) return refuse("DB insert failed");
  if (!s->stop_ledger.room(1, s->stops_cap)) return refuse("stop capacity exhausted", 8);
  const std::string sym(symbol);
  uint32_t sid = 0;
  if (!intern(s, sym, sid)) return refuse("symbol capacity exhausted", 8);
  const uint64_t id = s->next_sid++;
  StopOp op;
  op.id = id;
  op.client = r->client_id ? r->client_id : "";
  Stop& st = op.stop;
  st.client = op.client;
  st.symbol = sym;
  st.sid = sid;
  st.side = r->side;
  st.type = limit ? ME_TYPE_LIMIT : ME_TYPE_MARKET;
  st.tif = r->tif;
  st.stop_px = stop_q4;
  st.limit_px = q4;
  st.qty = r->quantity;
  st.kind = ME_KIND_TIF(r->side, st.type, ME_OP_NEW, r->tif);
  s->stops.emplace(id, st);
  s->stop_ledger.accepted++;
  ref_add(s, sid, 1);  // the stop's own count, until its cancel is confirmed or its event processed
  put(resp->order_id, sizeof resp->order_id, me::print_sid(id));
  resp->success = 1;
  boundary_add(s, std::move(op));
  return 0;
}

extern "C" int me_service_cancel_stop(me_service* s, const me_stop_cancel_request* r, me_order_response* resp) {
  if (!resp) return 0;
  memset(resp, 0, sizeof(*resp));
  auto refuse = [&](const char* why) {
    put(resp->error_message, sizeof resp->error_message, why);
    return 0;
  };
  if (!s || !r) return refuse("stop orders are not enabled");
  std::lock_guard<std::mutex> lk(s->mu);
  if (!s->stops_cap) return refuse("stop orders are not enabled");
  const uint64_t target = me::parse_sid(r->stop_id);
  if (!target) return refuse("stop_id is invalid");
  StopOp op;
  op.cancel = true;
  op.id = target;
  op.client = r->client_id ? r->client_id : "";
  op.unknown = target >= s->next_sid;
  auto it = s->stops.find(target);
  if (it != s->stops.end()) {
    if (it->second.client != op.client) return refuse("stop belongs to another client");
    op.stop = it->second;
  }
  put(resp->order_id, sizeof resp->order_id, me::print_sid(target));
  resp->success = 1;
  boundary_add(s, std::move(op));
  return 0;
}

extern "C" int me_service_stop_updates(me_service* s, const char* client_id, me_stop_update* out, size_t cap,
                                       size_t* n) {
  if (n) *n = 0;
  if (!s || (cap && !out)) return ME_E_INVALID;
  std::lock_guard<std::mutex> lk(s->upd_mu);
  size_t k = 0;
  const bool all = !client_id || !client_id[0];
  std::deque<me_stop_update> keep;
  for (auto& u : s->stop_updates) {
    if (k < cap && (all || strncmp(u.client_id, client_id, sizeof u.client_id) == 0))
      out[k++] = u;
    else
      keep.push_back(u);
  }
  s->stop_updates.swap(keep);
  if (n) *n = k;
  return ME_OK;
}

extern "C" int me_service_stops(me_service* s, const char* client_id, me_stop_update* out, size_t cap, size_t* n) {
  if (n) *n = 0;
  if (!s || (cap && !out)) return ME_E_INVALID;
  const bool all = !client_id || !client_id[0];
  std::lock_guard<std::mutex> lk(s->mu);
  size_t k = 0;
  for (const auto& kv : s->stops) {
    if (!all && kv.second.client != client_id) continue;
    if (k < cap) out[k] = stop_update(kv.first, kv.second.client, kv.second, kv.second.armed ? ME_SS_ARMED : ME_SS_QUEUED);
    ++k;
  }
  if (n) *n = k;
  return ME_OK;
}

extern "C" int me_service_stop_stats(const me_service* s, uint64_t* live, uint64_t* triggered, uint64_t* recovered) {
  if (!s) return ME_E_INVALID;
  me_service* m = const_cast<me_service*>(s);
  std::lock_guard<std::mutex> lk(m->mu);
  if (live) *live = m->stops.size();
  if (triggered) *triggered = m->stops_triggered;
  if (recovered) *recovered = m->stops_recovered;
  return ME_OK;
}

extern "C" size_t me_service_pending(const me_service* s) {
  me_service* m = const_cast<me_service*>(s);
  std::lock_guard<std::mutex> lk(m->mu);
  return m->open.size() + m->closed_records + m->inflight_records;
}

extern "C" uint64_t me_service_next_oid(const me_service* s) {
  me_service* m = const_cast<me_service*>(s);
  std::lock_guard<std::mutex> lk(m->mu);
  return m->next_id;
}

extern "C" size_t me_service_unpersisted(const me_service* s) {
  me_service* m = const_cast<me_service*>(s);
  std::lock_guard<std::mutex> lk(m->pq_mu);
  return m->pq_records;
}

static void push_update(me_service* s, uint64_t oid, const std::string& client, const std::string& symbol,
                        int status, int64_t price, int32_t fq, int32_t remaining) {
  me_order_update u;
  memset(&u, 0, sizeof u);
  put(u.order_id, sizeof u.order_id, "OID-" + std::to_string(oid));
  put(u.client_id, sizeof u.client_id, client);
  put(u.symbol, sizeof u.symbol, symbol);
  u.status = status;
  u.scale = 4;
  u.fill_price = price;
  u.fill_quantity = fq;
  u.remaining_quantity = remaining;
  if (s->updates.size() >= kMaxQueuedUpdates) {  // nobody drains the stream: drop the oldest, loudly
    s->updates.pop_front();
    if (s->updates_dropped++ == 0)
      s->fail(ME_OK, "OrderUpdate queue full (2^24 undrained events): dropping the oldest; drain with me_service_updates");
  }
  s->updates.push_back(u);
}

// OrderUpdate events of one matched slice (order documented in me_service.h), and the live-order
// table they are computed from. Locks are taken per block of records so SubmitOrder / CancelOrder
// (which touch the live table) never wait for a whole slice.
// Book reference counts move here too: every record's own count is released once its events are
// out, and a live entry's when it stops resting (filled, cancelled, or never rested).
// A recovery slice (orders replayed from the DB at create) emits only what is new: fills and
// outcomes other than "still resting" (its NEW events went out in the earlier run).
static void emit_updates(me_service* s, const Slice& sl, const me_order_result* res, const me_fill* tape) {
  constexpr size_t kBlock = 512;
  for (size_t i0 = 0; i0 < sl.size(); i0 += kBlock) {
    std::lock_guard<std::mutex> lv(s->live_mu);
    std::lock_guard<std::mutex> lu(s->upd_mu);
    auto live_erase = [&](std::unordered_map<uint64_t, Live>::iterator it) {
      ref_add(s, it->second.sid, -1);
      s->live.erase(it);
    };
    for (size_t i = i0; i < sl.size() && i < i0 + kBlock; ++i) {
      const Pending& m = sl.meta[i];
      const me_order_result& r = res[i];
      if (m.cancel) {
        auto it = s->live.find(m.target);
        if (m.reduce && r.status == ME_ST_NEW && it != s->live.end()) {
          // reduced in place: the target's own status, to its owner; it stays live and keeps its book
          Live& tg = it->second;
          tg.remaining = r.remaining_qty;
          push_update(s, m.target, tg.client, tg.symbol, tg.filled ? ME_ST_PARTIALLY_FILLED : ME_ST_NEW, 0, 0,
                      r.remaining_qty);
        } else if (r.status == ME_ST_CANCELED && it != s->live.end()) {
          push_update(s, m.target, it->second.client, it->second.symbol, ME_ST_CANCELED, 0, 0, r.remaining_qty);
          live_erase(it);
        } else {
          push_update(s, m.target, m.client, m.symbol, r.status == ME_ST_CANCELED ? ME_ST_CANCELED : ME_ST_REJECTED,
                      0, 0, r.remaining_qty);
        }
        ref_add(s, sl.sid[i], -1);  // the cancel record itself
        continue;
      }
      const uint64_t oid = sl.seq[i];
      int32_t rem = sl.qty[i];
      for (uint32_t f = 0; f < r.fill_count; ++f) {
        const me_fill& fl = tape[r.tape_offset + f];
        auto it = s->live.find(fl.maker_seq);
        if (it != s->live.end()) {
          Live& mk = it->second;
          mk.remaining -= fl.qty;
          mk.filled = true;
          push_update(s, fl.maker_seq, mk.client, mk.symbol,
                      mk.remaining > 0 ? ME_ST_PARTIALLY_FILLED : ME_ST_FILLED, fl.price_q4, fl.qty, mk.remaining);
          if (mk.remaining <= 0) live_erase(it);
        }
        rem -= fl.qty;
        push_update(s, oid, m.client, m.symbol, rem > 0 ? ME_ST_PARTIALLY_FILLED : ME_ST_FILLED, fl.price_q4,
                    fl.qty, rem);
      }
      // never rests: a MARKET, an IOC or a FOK
      const bool market = ((sl.kind[i] >> 2) & 1u) != 0 || (((sl.kind[i] >> 4) ^ (sl.kind[i] >> 5)) & 1u) != 0;
      if (r.status == ME_ST_REJECTED || r.status == ME_ST_CANCELED ||
          (r.fill_count == 0 && r.status == ME_ST_NEW && !sl.recovery))
        push_update(s, oid, m.client, m.symbol, r.status, 0, 0, r.remaining_qty);
      if (market) {
        ref_add(s, sl.sid[i], -1);  // the MARKET / IOC / FOK record (it never rests)
        continue;
      }
      // a LIMIT's count is its live entry, created at submit: it stays while the order rests
      if (r.remaining_qty > 0 && (r.status == ME_ST_NEW || r.status == ME_ST_PARTIALLY_FILLED)) {
        auto it = s->live.find(oid);
        if (it != s->live.end()) {
          it->second.remaining = r.remaining_qty;
          it->second.filled |= r.fill_count != 0;
        } else {
          s->live[oid] = Live{m.client, m.symbol, r.remaining_qty, sl.sid[i], r.fill_count != 0};
          ref_add(s, sl.sid[i], 1);
        }
      } else {
        auto it = s->live.find(oid);
        if (it != s->live.end()) live_erase(it);
      }
    }
  }
}

extern "C" int me_service_updates(me_service* s, const char* client_id, me_order_update* out, size_t cap,
                                  size_t* n) {
  std::lock_guard<std::mutex> lk(s->upd_mu);
  size_t k = 0;
  const bool all = !client_id || !client_id[0];
  if (all) {
    for (; k < cap && !s->updates.empty(); ++k) {
      if (out) out[k] = s->updates.front();
      s->updates.pop_front();
    }
  } else {  // one pass: this client's events out (up to cap), every other event kept in order
    std::deque<me_order_update> keep;
    for (auto& u : s->updates) {
      if (k < cap && strncmp(u.client_id, client_id, sizeof u.client_id) == 0) {
        if (out) out[k] = u;
        ++k;
      } else {
        keep.push_back(u);
      }
    }
    s->updates.swap(keep);
  }
  if (n) *n = k;
  return ME_OK;
}

// One transaction for one matched slice (the persister thread). The rows end exactly as the reference's
// per-order statements would leave them — insert_new_order's row (storage.cpp:102-112, incl.
// order_type=1, storage.cpp:106), then update_order_status-style changes (storage.cpp:160-181) as
// later fills and cancels hit the order — but the slice's own orders are brought to their final
// state in memory first, so each is ONE multi-row INSERT entry and only orders of earlier slices
// take UPDATEs. Orders rows go in before fills rows (the fills' foreign key), fills rows in tape
// order (taker's row, then maker's), through the corrected add_fill statement (5 columns, 5
// placeholders; the reference's has 6, storage.cpp:190).
static bool persist(me_service* s, const Slice& sl, const me_order_result* res, const me_fill* tape, int64_t ts,
                    std::string& err) {
  if (!s->db) return true;
  const size_t n = sl.size();
  if (sl.recovery) {  // replayed resting orders: their rows exist; a consistent DB produces no change
    bool change = false;
    for (size_t i = 0; i < n && !change; ++i) change = res[i].fill_count || res[i].status != ME_ST_NEW;
    if (!change) return true;
  }
  // ---- final state of this slice's rows; changes to earlier slices' rows
  std::vector<int32_t> fst(n), frem(n);
  std::unordered_map<uint64_t, long long> ext_fill;       // earlier order -> quantity filled now
  std::vector<std::pair<uint64_t, int32_t>> ext_cancel;   // earlier order -> quantity the cancel removed
  std::vector<std::pair<uint64_t, int32_t>> ext_reduce;   // earlier order -> quantity a partial reduce took off
  auto find = [&](uint64_t q) -> long {  // row of order q in this slice (seqs ascend), or -1
    auto it = std::lower_bound(sl.seq.begin(), sl.seq.end(), q);
    if (it == sl.seq.end() || *it != q) return -1;
    const long j = (long)(it - sl.seq.begin());
    return sl.meta[j].cancel ? -1 : j;
  };
  size_t nfill = 0;
  for (size_t i = 0; i < n; ++i) {
    const Pending& m = sl.meta[i];
    if (m.cancel) {
      if (m.reduce && res[i].status == ME_ST_NEW) {  // reduced in place: the remainder shrinks, the status stays
        const long j = find(m.target);
        if (j >= 0)
          frem[j] -= m.d;
        else
          ext_reduce.emplace_back(m.target, m.d);
        continue;
      }
      if (res[i].status != ME_ST_CANCELED) continue;
      const long j = find(m.target);
      if (j >= 0) {
        fst[j] = ME_ST_CANCELED;
        frem[j] = res[i].remaining_qty;
      } else {
        ext_cancel.emplace_back(m.target, res[i].remaining_qty);
      }
      continue;
    }
    fst[i] = res[i].status;
    frem[i] = res[i].remaining_qty;  // unfilled qty (0 once FILLED)
    for (uint32_t f = 0; f < res[i].fill_count; ++f) {
      const me_fill& fl = tape[res[i].tape_offset + f];
      const long j = find(fl.maker_seq);
      if (j >= 0) {
        frem[j] -= fl.qty;
        fst[j] = frem[j] == 0 ? ME_ST_FILLED : ME_ST_PARTIALLY_FILLED;
      } else {
        ext_fill[fl.maker_seq] += fl.qty;
      }
    }
    nfill += res[i].fill_count;
  }
  std::vector<std::string> oid(n);
  for (size_t i = 0; i < n; ++i)
    if (!sl.meta[i].cancel) oid[i] = "OID-" + std::to_string(sl.seq[i]);
  bool ok = true;
  auto step = [&](sqlite3_stmt* st, const char* what) {
    const int rc = g_sql.step(st);
    g_sql.reset(st);
    if (!sql_ok(rc)) {
      err = s->sql_err(what);
      ok = false;
    }
    return ok;
  };
  if (!sql_ok(g_sql.exec(s->db, "BEGIN", nullptr, nullptr, nullptr))) {
    err = s->sql_err("begin");
    return false;
  }
  // ---- orders rows, kRows per statement (a recovery slice's rows exist: they take UPDATEs)
  if (sl.recovery) {
    for (size_t i = 0; ok && i < n; ++i) {
      if (fst[i] == ME_ST_NEW && frem[i] == sl.qty[i]) continue;
      g_sql.bind_int64(s->st_upd, 1, fst[i]);
      g_sql.bind_int64(s->st_upd, 2, frem[i]);
      g_sql.bind_int64(s->st_upd, 3, ts);
      g_sql.bind_text(s->st_upd, 4, oid[i].c_str(), -1, SQLITE_TRANSIENT);
      step(s->st_upd, "update recovered order");
    }
  } else {
    std::vector<size_t> rows;
    rows.reserve(n);
    for (size_t i = 0; i < n; ++i)
      if (!sl.meta[i].cancel) rows.push_back(i);
    auto bind_row = [&](sqlite3_stmt* st, int b, size_t i) {
      const Pending& m = sl.meta[i];
      g_sql.bind_text(st, b + 1, oid[i].c_str(), -1, nullptr);
      g_sql.bind_text(st, b + 2, m.client.c_str(), -1, nullptr);
      g_sql.bind_text(st, b + 3, m.symbol.c_str(), -1, nullptr);
      g_sql.bind_int64(st, b + 4, m.side);
      g_sql.bind_int64(st, b + 5, 1);  // order_type: the reference binds the constant 1 (storage.cpp:106)
      g_sql.bind_int64(st, b + 6, sl.px[i]);
      g_sql.bind_int64(st, b + 7, sl.qty[i]);
      g_sql.bind_int64(st, b + 8, fst[i]);
      g_sql.bind_int64(st, b + 9, frem[i]);
      g_sql.bind_int64(st, b + 10, ts);
      g_sql.bind_int64(st, b + 11, ts);
    };
    size_t k = 0;
    for (; ok && k + kRows <= rows.size(); k += kRows) {
      for (int r = 0; r < kRows; ++r) bind_row(s->st_ins_k, 11 * r, rows[k + r]);
      step(s->st_ins_k, "insert orders");
    }
    for (; ok && k < rows.size(); ++k) {
      bind_row(s->st_ins, 0, rows[k]);
      step(s->st_ins, "insert order");
    }
  }
  // ---- earlier slices' rows: partial reduces first (remaining only; fills and reduces of one order commute
  // in the remainder, but the maker statement derives FILLED from "remaining reaches 0", which holds only with
  // the reduces already in), then fills (an order is filled before it can be canceled), then cancels
  for (size_t k = 0; ok && k < ext_reduce.size(); ++k) {
    const std::string toid = "OID-" + std::to_string(ext_reduce[k].first);
    g_sql.bind_int64(s->st_reduce, 1, ext_reduce[k].second);
    g_sql.bind_int64(s->st_reduce, 2, ts);
    g_sql.bind_text(s->st_reduce, 3, toid.c_str(), -1, SQLITE_TRANSIENT);
    step(s->st_reduce, "reduce order");
  }
  for (auto it = ext_fill.begin(); ok && it != ext_fill.end(); ++it) {
    const std::string moid = "OID-" + std::to_string(it->first);
    g_sql.bind_int64(s->st_maker, 1, it->second);
    g_sql.bind_int64(s->st_maker, 2, it->second);
    g_sql.bind_int64(s->st_maker, 3, ts);
    g_sql.bind_text(s->st_maker, 4, moid.c_str(), -1, SQLITE_TRANSIENT);
    step(s->st_maker, "update maker");
  }
  for (size_t k = 0; ok && k < ext_cancel.size(); ++k) {
    const std::string toid = "OID-" + std::to_string(ext_cancel[k].first);
    g_sql.bind_int64(s->st_upd, 1, ME_ST_CANCELED);
    g_sql.bind_int64(s->st_upd, 2, ext_cancel[k].second);  // the quantity the cancel removed
    g_sql.bind_int64(s->st_upd, 3, ts);
    g_sql.bind_text(s->st_upd, 4, toid.c_str(), -1, SQLITE_TRANSIENT);
    step(s->st_upd, "cancel order");
  }
  // ---- fills rows: one FillRow per order of each trade, kRows per statement
  if (ok && nfill) {
    std::vector<std::string> moid(nfill);
    std::vector<std::pair<size_t, size_t>> fr;  // (taker row, fill index in the slice's fills)
    fr.reserve(nfill);
    size_t q = 0;
    for (size_t i = 0; i < n; ++i) {
      if (sl.meta[i].cancel) continue;
      for (uint32_t f = 0; f < res[i].fill_count; ++f, ++q) {
        moid[q] = "OID-" + std::to_string(tape[res[i].tape_offset + f].maker_seq);
        fr.emplace_back(i, res[i].tape_offset + f);
      }
    }
    auto bind_fill = [&](sqlite3_stmt* st, int b, size_t r) {  // row r: fill r / 2, taker (even) or maker
      const size_t i = fr[r / 2].first;
      const me_fill& fl = tape[fr[r / 2].second];
      const char* who = (r & 1) ? moid[r / 2].c_str() : oid[i].c_str();
      g_sql.bind_text(st, b + 1, who, -1, nullptr);
      g_sql.bind_text(st, b + 2, sl.meta[i].symbol.c_str(), -1, nullptr);
      g_sql.bind_int64(st, b + 3, fl.price_q4);
      g_sql.bind_int64(st, b + 4, fl.qty);
      g_sql.bind_int64(st, b + 5, ts);
    };
    const size_t nrows = 2 * nfill;
    size_t r = 0;
    for (; ok && r + kRows <= nrows; r += kRows) {
      for (int k = 0; k < kRows; ++k) bind_fill(s->st_fill_k, 5 * k, r + k);
      step(s->st_fill_k, "insert fills");
    }
    for (; ok && r < nrows; ++r) {
      bind_fill(s->st_fill, 0, r);
      step(s->st_fill, "insert fill");
    }
  }
  // ---- stop rows: the boundary's ARMED inserts and CANCELED updates, and TRIGGERED for the stops whose orders
  // this slice carries (their `orders` rows went in above: one transaction)
  for (size_t k = 0; ok && k < sl.srows.size() && s->st_stop_ins && s->st_stop_upd; ++k) {
    const StopRow& r = sl.srows[k];
    if (r.state == ME_SS_ARMED) {
      sqlite3_stmt* st = s->st_stop_ins;
      g_sql.bind_int64(st, 1, (long long)r.id);
      g_sql.bind_text(st, 2, r.client.c_str(), -1, SQLITE_TRANSIENT);
      g_sql.bind_text(st, 3, r.stop.symbol.c_str(), -1, SQLITE_TRANSIENT);
      g_sql.bind_int64(st, 4, r.stop.side);
      g_sql.bind_int64(st, 5, r.stop.type);
      g_sql.bind_int64(st, 6, r.stop.tif);
      g_sql.bind_int64(st, 7, r.stop.stop_px);
      g_sql.bind_int64(st, 8, r.stop.limit_px);
      g_sql.bind_int64(st, 9, r.stop.qty);
      g_sql.bind_int64(st, 10, ME_SS_ARMED);
      g_sql.bind_int64(st, 11, ts);
      step(st, "insert stop");
    } else {
      sqlite3_stmt* st = s->st_stop_upd;
      const std::string soid = r.oid ? "OID-" + std::to_string(r.oid) : "";
      g_sql.bind_int64(st, 1, r.state);
      g_sql.bind_text(st, 2, soid.c_str(), -1, SQLITE_TRANSIENT);
      g_sql.bind_int64(st, 3, r.trigger_px);
      g_sql.bind_int64(st, 4, ts);
      g_sql.bind_int64(st, 5, (long long)r.id);
      step(st, "update stop");
    }
  }
  if (!ok) {
    g_sql.exec(s->db, "ROLLBACK", nullptr, nullptr, nullptr);
    return false;
  }
  if (!sql_ok(g_sql.exec(s->db, "COMMIT", nullptr, nullptr, nullptr))) {
    err = s->sql_err("commit");
    g_sql.exec(s->db, "ROLLBACK", nullptr, nullptr, nullptr);
    return false;
  }
  return true;
}

// The persister: emits each matched slice's OrderUpdates, then commits its transaction, oldest
// first. A failed transaction stalls the queue (later slices still get their updates) until the
// next flush clears pq_stalled; on stop it drains what it can and exits.
static void persister_main(me_service* s) {
  std::unique_lock<std::mutex> lk(s->pq_mu);
  for (;;) {
    s->pq_cv.wait(lk, [&] {
      return s->pq_stop || s->pq_emitted < s->pq.size() || (!s->pq_stalled && !s->pq.empty());
    });
    if (s->pq_emitted < s->pq.size()) {
      const Matched* m = &s->pq[s->pq_emitted];  // deque elements stay put under push_back
      lk.unlock();
      emit_updates(s, m->sl, m->res.data(), m->tape.data());
      lk.lock();
      ++s->pq_emitted;
      s->pq_cv.notify_all();
      continue;
    }
    if (!s->pq_stalled && !s->pq.empty()) {
      const Matched* m = &s->pq.front();
      lk.unlock();
      std::string err;
      const bool ok = persist(s, m->sl, m->res.data(), m->tape.data(), m->ts, err);
      lk.lock();
      if (ok) {
        s->pq_records -= m->sl.size();
        s->pq.pop_front();
        --s->pq_emitted;
      } else {
        s->pq_stalled = true;
        s->pq_err = err;
      }
      s->pq_cv.notify_all();
      continue;
    }
    if (s->pq_stop) break;
  }
}

// Where a flush's caller wants the matched outputs (any pointer may be NULL). The capacities are
// checked against the pending records before anything is matched; a slice whose outputs still would
// not fit (a matcher exceeding its own fill bound) is not copied: `short_buf`, ME_E_INVALID at the end.
struct FlushOut {
  me_fill* fills = nullptr;
  size_t fills_cap = 0;
  size_t nf = 0;
  me_order_result* res = nullptr;
  uint64_t* seq = nullptr;
  size_t res_cap = 0;
  size_t nr = 0;
  bool short_buf = false;
};

// A matched slice: its outputs to the caller, the slice to the persister (stream order).
static void deliver(me_service* s, Slice&& sl, std::vector<me_order_result>&& res, std::vector<me_fill>&& tape,
                    FlushOut* out) {
  const size_t n = sl.size(), nf = tape.size();
  if (out && !out->short_buf) {
    if ((out->fills && out->nf + nf > out->fills_cap) || ((out->res || out->seq) && out->nr + n > out->res_cap)) {
      out->short_buf = true;
    } else {
      if (out->fills) memcpy(out->fills + out->nf, tape.data(), nf * sizeof(me_fill));
      if (out->res)
        for (size_t i = 0; i < n; ++i) {
          out->res[out->nr + i] = res[i];
          out->res[out->nr + i].tape_offset += (uint32_t)out->nf;
        }
      if (out->seq) memcpy(out->seq + out->nr, sl.seq.data(), n * sizeof(uint64_t));
      out->nf += nf;
      out->nr += n;
    }
  }
  Matched mt;
  mt.ts = now_ms();
  mt.sl = std::move(sl);
  mt.res = std::move(res);
  mt.tape = std::move(tape);
  {
    std::lock_guard<std::mutex> lq(s->pq_mu);
    s->pq.push_back(std::move(mt));
    s->pq_records += n;
    s->pq_cv.notify_all();
  }
  std::lock_guard<std::mutex> lk(s->mu);  // after the push: pending + unpersisted never dips to 0 early
  s->inflight_records -= n;
}

// The backend refused a slice (its books near max_resting; nothing of it applied). Rather than
// retrying the same slice forever — nothing could free capacity, since every later record (cancels
// included) is queued behind it — it is split and its halves go back to the head of the queue; a
// single LIMIT that still does not fit is answered in-band (REJECTED, ME_RJ_CAPACITY). `taken` counts
// the records of this flush's budget handed out so far.
static int on_refused(me_service* s, Slice&& sl, FlushOut* out, size_t& taken) {
  const size_t n = sl.size();
  if (sl.recovery) {  // the DB's resting orders do not fit the books: nothing sensible to do
    s->failed = true;
    {
      std::lock_guard<std::mutex> lk(s->mu);
      s->inflight_records -= n;
    }
    return s->fail(ME_E_CAPACITY, "the backend's max_resting is below the resting orders the DB holds: " +
                                      backend_err(s));
  }
  if (n == 1 && (sl.kind[0] & 0x0Cu) == 0u && (((sl.kind[0] >> 4) ^ (sl.kind[0] >> 5)) & 1u) == 0u) {  // one LIMIT that may rest (GTC / POST_ONLY) and no room to rest it
    me_order_result r{};
    r.remaining_qty = sl.qty[0];
    r.status = ME_ST_REJECTED;
    r.reason = ME_RJ_CAPACITY;
    deliver(s, std::move(sl), std::vector<me_order_result>{r}, std::vector<me_fill>{}, out);
    return ME_OK;
  }
  std::lock_guard<std::mutex> lk(s->mu);
  s->inflight_records -= n;
  s->closed_records += n;
  taken -= n;
  if (n == 1) {  // a record that cannot rest, refused by a matcher: kept queued for the next flush
    s->closed.push_front(std::move(sl));
    return s->fail(ME_E_CAPACITY, "the matcher refused a record that cannot rest; it stays queued");
  }
  Slice head = sl.take_prefix(n / 2);
  s->closed.push_front(std::move(sl));
  s->closed.push_front(std::move(head));
  return ME_OK;
}

// ---- stop orders: the flush path's half (flush_mu held throughout) --------------------------------------
static void push_stop_updates(me_service* s, const std::vector<me_stop_update>& ups) {
  if (ups.empty()) return;
  std::lock_guard<std::mutex> lu(s->upd_mu);
  for (const me_stop_update& u : ups) {
    if (s->stop_updates.size() >= kMaxQueuedUpdates) {  // nobody drains the stream: drop the oldest, loudly
      s->stop_updates.pop_front();
      if (s->updates_dropped++ == 0)  // (one count for both streams: me_service_updates_dropped)
        s->fail(ME_OK, "stop update queue full (2^24 undrained events): dropping the oldest; drain with "
                       "me_service_stop_updates");
    }
    s->stop_updates.push_back(u);
  }
}

// Read the backend's stop events until none is left (eng_mu held) into the hold-back buffer.
static int stops_pull(me_service* s) {
  me_stop_event buf[128];
  for (;;) {
    size_t n = 0, left = 0;
    const int rc = s->be.stops_read(s->be.ctx, buf, sizeof buf / sizeof buf[0], &n, &left);
    if (rc != ME_OK) return s->fail(rc, "stop orders: reading the backend's events failed: " + backend_err(s));
    s->stop_hold.push(buf, n);
    if (!left) return ME_OK;
  }
}

// Process the events whose slice has been collected, in ring order, under the submit lock (lock order:
// flush_mu, eng_mu, mu; eng_mu is not needed here): each becomes the next order of the stream.
static void stops_process(me_service* s, std::vector<me_stop_update>& ups) {
  const std::vector<me_stop_event> due = s->stop_hold.take_due(s->ncol);
  if (due.empty()) return;
  std::lock_guard<std::mutex> lk(s->mu);
  for (const me_stop_event& ev : due) {
    auto it = s->stops.find(ev.id);
    if (it == s->stops.end()) continue;  // (not reachable: every stop of the backend's table is in this one)
    const Stop st = it->second;
    const uint64_t oid = s->next_id++;
    const bool never_rests = ((ev.kind >> 2) & 1u) != 0 || (((ev.kind >> 4) ^ (ev.kind >> 5)) & 1u) != 0;
    if (!never_rests) {
      std::lock_guard<std::mutex> lv(s->live_mu);
      s->live[oid] = Live{st.client, st.symbol, ev.qty, ev.symbol};
    }
    ref_add(s, ev.symbol, 1);  // the order's count (SubmitOrder's), before the stop's goes
    StopRow row;
    row.state = ME_SS_TRIGGERED;
    row.id = ev.id;
    row.oid = oid;
    row.trigger_px = ev.trigger_px_q4;
    s->open.srows.push_back(std::move(row));  // commits with the slice that carries the order's row
    append(s, oid, ev.limit_px_q4, ev.qty, ev.symbol, ev.kind, Pending{st.client, st.symbol, st.side, false, 0});
    ref_add(s, st.sid, -1);
    s->stops.erase(it);
    s->stop_ledger.closed++;
    s->stops_triggered++;
    ups.push_back(stop_update(ev.id, st.client, st, ME_SS_TRIGGERED, oid, ev.trigger_px_q4));
  }
}

// Apply the boundary in front of a slice, in submission order: runs of adds as one stops_add, runs of cancels as
// one stops_cancel (no slice is in flight then: the caller collected them). The boundary's rows join the
// slice's transaction, its updates go to `ups`.
static int apply_boundary(me_service* s, Slice& sl, std::vector<me_stop_update>& ups) {
  const std::vector<StopOp> ops = std::move(sl.pre);
  sl.pre.clear();
  std::vector<uint8_t> is_cancel(ops.size());
  for (size_t i = 0; i < ops.size(); ++i) is_cancel[i] = ops[i].cancel;
  for (const me::StopRun& run : me::stop_runs(is_cancel)) {
    const size_t n = run.end - run.begin;
    if (!run.cancel) {
      std::vector<me_stop> recs(n);
      memset(recs.data(), 0, n * sizeof(me_stop));
      for (size_t i = 0; i < n; ++i) {
        const StopOp& op = ops[run.begin + i];
        recs[i].id = op.id;
        recs[i].stop_px_q4 = op.stop.stop_px;
        recs[i].limit_px_q4 = op.stop.limit_px;
        recs[i].qty = op.stop.qty;
        recs[i].symbol = op.stop.sid;
        recs[i].kind = op.stop.kind;
      }
      int rc;
      {
        std::lock_guard<std::mutex> le(s->eng_mu);
        rc = s->be.stops_add(s->be.ctx, recs.data(), n);
      }
      if (rc != ME_OK) {  // the host's mirror of the bound admitted them: the backend's table is not the service's
        s->failed = true;
        return s->fail(rc, "stop orders: the backend refused stops the service had admitted: " + backend_err(s));
      }
      {
        std::lock_guard<std::mutex> lk(s->mu);
        for (size_t i = 0; i < n; ++i) {
          auto it = s->stops.find(ops[run.begin + i].id);
          if (it != s->stops.end()) it->second.armed = true;
        }
      }
      for (size_t i = 0; i < n; ++i) {
        const StopOp& op = ops[run.begin + i];
        ups.push_back(stop_update(op.id, op.client, op.stop, ME_SS_ARMED));
        StopRow row;
        row.state = ME_SS_ARMED;
        row.id = op.id;
        row.client = op.client;
        row.stop = op.stop;
        sl.srows.push_back(std::move(row));
      }
      continue;
    }
    // cancels: the ids the backend may know, sorted, each once; an id from the future (never issued when the
    // cancel was accepted) is not asked about — it may name somebody's stop by now
    std::vector<uint64_t> ids;
    std::vector<size_t> at(n, SIZE_MAX);  // operation -> its index among the asked ones
    for (size_t i = 0; i < n; ++i) {
      if (ops[run.begin + i].unknown) continue;
      at[i] = ids.size();
      ids.push_back(ops[run.begin + i].id);
    }
    const me::CancelRun cr = me::cancel_run(ids.data(), ids.size());
    std::vector<uint8_t> found(cr.ids.size() + 1, 0);
    int rc;
    {
      std::lock_guard<std::mutex> le(s->eng_mu);
      rc = s->be.stops_cancel(s->be.ctx, cr.ids.data(), cr.ids.size(), found.data());
      if (rc != ME_OK) {
        s->failed = true;
        return s->fail(rc, "stop orders: the backend's stops_cancel failed: " + backend_err(s));
      }
      rc = stops_pull(s);
    }
    if (rc != ME_OK) {
      s->failed = true;  // the cancels are applied and their answers lost
      return rc;
    }
    stops_process(s, ups);  // TRIGGERED first: the owner of a stop that had triggered sees it before the rejection
    std::lock_guard<std::mutex> lk(s->mu);
    for (size_t i = 0; i < n; ++i) {
      const StopOp& op = ops[run.begin + i];
      const bool hit = at[i] != SIZE_MAX && cr.first[at[i]] && found[cr.slot[at[i]]];
      if (!hit) {
        ups.push_back(stop_update(op.id, op.client, op.stop, ME_SS_CANCEL_REJECTED));
        continue;
      }
      auto it = s->stops.find(op.id);
      if (it != s->stops.end()) {
        ref_add(s, it->second.sid, -1);
        s->stops.erase(it);
      }
      s->stop_ledger.closed++;
      ups.push_back(stop_update(op.id, op.client, op.stop, ME_SS_CANCELED));
      StopRow row;
      row.state = ME_SS_CANCELED;
      row.id = op.id;
      sl.srows.push_back(std::move(row));
    }
  }
  return ME_OK;
}

// Flush the closed slices (and the open one when take_open), oldest first, two in flight: slice k+1 is
// submitted before slice k is collected. `rec_limit` bounds the records taken (those present when the
// caller checked its output capacity). With `wait`, returns once the persister has emitted every
// matched slice and committed them (or stalled on a failed transaction: ME_E_SQLITE, the slices kept
// in order for the next flush).
static int flush_closed(me_service* s, bool take_open, size_t rec_limit, FlushOut* out, bool wait) {
  if (s->failed) return s->fail(ME_E_STATE, "service failed: the engine lost an accepted slice");
  if (!has_backend(s)) {
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->open.size() || !s->closed.empty())
      return s->fail(ME_E_STATE, "me_service_flush: no engine (HIP device required)");
  }
  {  // every flush retries the kept slices first
    std::lock_guard<std::mutex> lq(s->pq_mu);
    if (s->pq_stalled) {
      s->pq_stalled = false;
      s->pq_cv.notify_all();
    }
  }
  if (take_open) {
    std::lock_guard<std::mutex> lk(s->mu);
    close_open(s);
  }
  std::deque<Inflight> fl;  // submitted, not collected (at most two)
  auto lost = [&](int r, const std::string& what) {
    s->failed = true;
    size_t n = 0;
    for (auto& f : fl) n += f.sl.size();
    std::lock_guard<std::mutex> lk(s->mu);
    s->inflight_records -= n;
    return s->fail(r, what + backend_err(s));
  };
  // A failure before a taken slice was handed to the backend: it goes back to the head of the queue.
  auto lost_one = [&](int r, Inflight& f) {
    std::lock_guard<std::mutex> lk(s->mu);
    s->inflight_records -= f.sl.size();
    s->closed_records += f.sl.size();
    s->closed.push_front(std::move(f.sl));
    return r;
  };
  auto finish_oldest = [&]() -> int {
    int r;
    {
      std::lock_guard<std::mutex> le(s->eng_mu);
      r = backend_collect(s, fl.front());
      each_feed(s, [&](auto& f, auto pull) {
        if (r == ME_OK && f.on) (void)pull(s);  // (a failed read is in last_error; the slice is matched)
      });
      if (r == ME_OK && s->stops_cap) (void)stops_pull(s);
    }
    if (r != ME_OK) return lost(r, "engine lost an accepted slice: ");
    ++s->ncol;
    Inflight& f = fl.front();
    const std::vector<me_stop_update> post = std::move(f.post);
    deliver(s, std::move(f.sl), std::move(f.res), std::move(f.tape), out);
    fl.pop_front();
    if (s->stops_cap) {  // the events this slice was waited for: each becomes an order of the open slice
      std::vector<me_stop_update> ups;
      stops_process(s, ups);
      push_stop_updates(s, ups);
    }
    push_stop_updates(s, post);
    return ME_OK;
  };
  size_t taken = 0;
  for (;;) {
    Inflight f;
    {
      std::lock_guard<std::mutex> lk(s->mu);
      if (s->closed.empty()) break;
      if (taken >= rec_limit && s->closed.front().size()) break;  // (a boundary-only slice holds no record)
      f.sl = std::move(s->closed.front());
      s->closed.pop_front();
      s->closed_records -= f.sl.size();
      s->inflight_records += f.sl.size();
    }
    taken += f.sl.size();
    {  // bounded run-ahead: at most kMaxMatchedAhead slices wait for the DB (unless it is stalled)
      std::unique_lock<std::mutex> lq(s->pq_mu);
      s->pq_cv.wait(lq, [&] { return s->pq_stalled || s->pq.size() < kMaxMatchedAhead; });
    }
    bool accepted = false;
    int r;
    if (!f.sl.pre.empty()) {  // the boundary in front of the slice (a slice split later keeps none: applied once)
      bool any_cancel = false;
      for (const StopOp& op : f.sl.pre) any_cancel |= op.cancel;
      // a cancel's answer depends on what the slices before it triggered: they are collected first
      while (any_cancel && !fl.empty())
        if ((r = finish_oldest()) != ME_OK) return lost_one(r, f);
      std::vector<me_stop_update> ups;
      if ((r = apply_boundary(s, f.sl, ups)) != ME_OK) return lost_one(r, f);
      if (fl.empty())
        push_stop_updates(s, ups);
      else
        fl.back().post.insert(fl.back().post.end(), ups.begin(), ups.end());
    }
    if (!f.sl.size()) {  // a boundary with no slice behind it: its rows go to the persister in stream order
      while (!fl.empty())
        if ((r = finish_oldest()) != ME_OK) return r;
      if (!f.sl.srows.empty()) deliver(s, std::move(f.sl), {}, {}, out);
      continue;
    }
    {
      std::lock_guard<std::mutex> le(s->eng_mu);
      r = backend_submit(s, f, accepted);
      if (accepted) {
        ++s->nsub;
        md_note_owners(s, f.sl, s->nsub);
      }
    }
    if (r != ME_OK && !accepted) {  // refused: the slices before it go first, then it is split
      while (!fl.empty())
        if ((r = finish_oldest()) != ME_OK) return r;
      if ((r = on_refused(s, std::move(f.sl), out, taken)) != ME_OK) return r;
      continue;
    }
    if (r != ME_OK) {  // accepted and lost: the books may hold the slice, the service cannot go on
      fl.push_back(std::move(f));
      return lost(r, "engine lost an accepted slice: ");
    }
    fl.push_back(std::move(f));
    if (fl.size() > 1 || !s->be.submit)  // (a synchronous match: one slice in flight)
      if ((r = finish_oldest()) != ME_OK) return r;
    if (!fl.empty() && fl.back().sl.recovery)  // a recovery chunk is matched alone (load_resting)
      while (!fl.empty())
        if ((r = finish_oldest()) != ME_OK) return r;
  }
  while (!fl.empty()) {
    const int r = finish_oldest();
    if (r != ME_OK) return r;
  }
  if (out && out->short_buf)
    return s->fail(ME_E_INVALID, "output buffers too small for the matched slices (they were matched and persisted; "
                                 "outputs truncated to the slices that fit)");
  if (!wait) return ME_OK;
  std::unique_lock<std::mutex> lq(s->pq_mu);
  s->pq_cv.wait(lq, [&] { return s->pq_emitted == s->pq.size() && (s->pq.empty() || s->pq_stalled); });
  if (s->pq_stalled)
    return s->fail(ME_E_SQLITE, "persistence deferred (" + s->pq_err +
                                    "); the matched slices are kept and retried at the next flush");
  return ME_OK;
}

extern "C" int me_service_flush(me_service* s, me_fill* out_fills, size_t fills_cap, size_t* n_fills,
                                me_order_result* out_results, uint64_t* out_seq, size_t results_cap,
                                size_t* n_results) {
  if (n_fills) *n_fills = 0;
  if (n_results) *n_results = 0;
  std::lock_guard<std::mutex> lf(s->flush_mu);
  size_t total = 0;
  {  // the open slice closes in the same critical section that counts it: SubmitOrders after this point go
     // into a new open slice (the next flush's), so `total` is exactly what this flush matches
    std::lock_guard<std::mutex> lk(s->mu);
    close_open(s);
    total = s->closed_records;  // inflight is 0 here (flush_mu held)
  }
  // the caller's buffers are checked before anything is matched
  if ((out_results || out_seq) && total > results_cap)
    return s->fail(ME_E_INVALID, "results_cap smaller than the pending records");
  if (out_fills && has_backend(s) && fills_cap < s->be.fill_bound(s->be, total))
    return s->fail(ME_E_INVALID, "fills_cap smaller than me_fill_bound(pending records)");
  FlushOut out;
  out.fills = out_fills;
  out.fills_cap = fills_cap;
  out.res = out_results;
  out.seq = out_seq;
  out.res_cap = results_cap;
  const int rc = flush_closed(s, false, total, &out, true);
  if (n_fills) *n_fills = out.nf;
  if (n_results) *n_results = out.nr;
  return rc;
}

// The background flusher: closes the open slice once it is interval old (or the submit path closed
// it at the slice size) and flushes the closed ones.
static void flusher_main(me_service* s) {
  std::unique_lock<std::mutex> lk(s->mu);
  // after a failed flush (e.g. a matcher kept refusing a record): retry after 1 ms, doubling to 100 ms
  int64_t backoff_us = 0, retry_at = 0;
  while (!s->stop) {
    const int64_t now = mono_us();
    const bool opened = s->open.size() || !s->open.pre.empty();  // records, or a boundary waiting to be applied
    const bool due = opened && now - s->open.opened_us >= s->interval_us;
    if (due) close_open(s);
    const bool blocked = backoff_us && now < retry_at;
    if (s->closed.empty() || blocked) {
      int64_t wait = opened && !due ? s->open.opened_us + s->interval_us - now : s->interval_us;
      if (blocked) wait = std::min(wait, retry_at - now);
      s->cv.wait_for(lk, std::chrono::microseconds(wait > 0 ? wait : 1));
      continue;
    }
    lk.unlock();
    int rc;
    {
      std::lock_guard<std::mutex> lf(s->flush_mu);
      rc = flush_closed(s, false, SIZE_MAX, nullptr, false);  // errors land in me_service_last_error
    }
    lk.lock();
    if (s->failed) break;
    if (rc == ME_OK) {
      backoff_us = 0;
    } else {
      backoff_us = std::min<int64_t>(std::max<int64_t>(2 * backoff_us, 1000), 100000);
      retry_at = mono_us() + backoff_us;
    }
  }
}

extern "C" int me_service_start(me_service* s, uint32_t interval_us, uint32_t slice_orders) {
  if (!s || !has_backend(s)) return ME_E_STATE;
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->flusher.joinable()) return s->fail(ME_E_STATE, "flusher already running");
  const uint32_t mb = s->be.max_batch;  // (not the current slice_max, which this call replaces)
  s->slice_max = slice_orders && slice_orders < mb ? slice_orders : mb;
  s->interval_us = interval_us ? interval_us : 1000;
  s->stop = false;
  s->flusher = std::thread(flusher_main, s);
  return ME_OK;
}

extern "C" int me_service_stop(me_service* s) {
  if (!s) return ME_E_INVALID;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    s->stop = true;
    s->cv.notify_all();
  }
  if (s->flusher.joinable()) s->flusher.join();
  // what the flusher matched is out (updates emitted, committed or stalled) when stop returns
  std::unique_lock<std::mutex> lq(s->pq_mu);
  s->pq_cv.wait(lq, [&] { return s->pq_emitted == s->pq.size() && (s->pq.empty() || s->pq_stalled); });
  return ME_OK;
}

extern "C" void me_service_destroy(me_service* s) {
  if (!s) return;
  me_service_stop(s);
  {  // the persister commits what it can (a stalled head is given one more try), then exits
    std::lock_guard<std::mutex> lq(s->pq_mu);
    s->pq_stalled = false;
    s->pq_stop = true;
    s->pq_cv.notify_all();
  }
  if (s->persister.joinable()) s->persister.join();
  // A matcher outlives its service: the depth and trade feeds this service turned on go off with it. (An
  // engine's feeds are left on, quotes included. That looks accidental; it is what the service has always done.)
  if (s->be.feeds_off_at_destroy) {
    std::lock_guard<std::mutex> le(s->eng_mu);
    if (s->dp.on && s->be.depth_enable) (void)s->be.depth_enable(s->be.ctx, 0, 0);
    if (s->tr.on && s->be.trades_enable) (void)s->be.trades_enable(s->be.ctx, 0);
    if (s->stops_cap && s->be.stops_enable) (void)s->be.stops_enable(s->be.ctx, 0);
  }
  close_db(s);
  delete s;
}

extern "C" int me_service_book(me_service* s, const char* symbol, me_level* bids, me_level* asks, size_t depth,
                               size_t* n_bids, size_t* n_asks) {
  if (n_bids) *n_bids = 0;
  if (n_asks) *n_asks = 0;
  if (depth == 0) return ME_OK;  // no levels asked for (the backend would read 0 as "the whole book")
  uint32_t sid = 0;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    auto it = s->sym.find(symbol ? symbol : "");
    if (it == s->sym.end()) return ME_OK;  // unknown symbol: empty book (the reference's stub is always empty)
    sid = it->second;
  }
  if (!has_backend(s)) return s->fail(ME_E_STATE, "no engine");
  std::lock_guard<std::mutex> le(s->eng_mu);
  const int rc = s->be.book(s->be.ctx, sid, (uint32_t)std::min<size_t>(depth, 0xFFFFFFFFu), nullptr, 0, nullptr,
                            nullptr, 0, nullptr, bids, asks, n_bids, n_asks);
  if (rc != ME_OK) return s->fail(rc, "engine: " + backend_err(s));
  return ME_OK;
}

extern "C" int me_service_order_book(me_service* s, const char* symbol, uint32_t depth, me_book_order* bids,
                                     size_t bids_cap, size_t* n_bids, me_book_order* asks, size_t asks_cap,
                                     size_t* n_asks) {
  if (n_bids) *n_bids = 0;
  if (n_asks) *n_asks = 0;
  uint32_t sid = 0;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    auto it = s->sym.find(symbol ? symbol : "");
    if (it == s->sym.end()) return ME_OK;
    sid = it->second;
  }
  if (!has_backend(s)) return s->fail(ME_E_STATE, "no engine");
  std::vector<me_book_entry> side[2];
  size_t n[2] = {0, 0};
  {
    std::lock_guard<std::mutex> le(s->eng_mu);
    side[0].resize(std::max<size_t>(bids_cap, 1));
    side[1].resize(std::max<size_t>(asks_cap, 1));
    const int rc = s->be.book(s->be.ctx, sid, depth, bids ? side[0].data() : nullptr, bids ? side[0].size() : 0,
                              &n[0], asks ? side[1].data() : nullptr, asks ? side[1].size() : 0, &n[1], nullptr,
                              nullptr, nullptr, nullptr);
    if (rc != ME_OK) return s->fail(rc, "engine: " + backend_err(s));
  }
  me_book_order* out[2] = {bids, asks};
  const size_t caps[2] = {bids_cap, asks_cap};
  std::lock_guard<std::mutex> lv(s->live_mu);
  for (int k = 0; k < 2; ++k) {
    if (!out[k]) continue;
    for (size_t i = 0; i < n[k] && i < caps[k]; ++i) {
      const me_book_entry& e = side[k][i];
      me_book_order& o = out[k][i];
      memset(&o, 0, sizeof o);
      put(o.order_id, sizeof o.order_id, "OID-" + std::to_string(e.seq));
      auto it = s->live.find(e.seq);
      if (it != s->live.end()) put(o.client_id, sizeof o.client_id, it->second.client);
      o.price = e.price_q4;
      o.scale = 4;
      o.quantity = e.qty;
      o.side = e.side;
    }
  }
  if (n_bids) *n_bids = n[0];
  if (n_asks) *n_asks = n[1];
  return ME_OK;
}

// OrderStatus (build extension): the queue position of a client's resting orders, from one me_order_query.
// The engine is asked about every id, another client's included; the live table then decides what the caller
// may see, so an answer never tells whether somebody else's order exists.
extern "C" int me_service_order_status(me_service* s, const char* client_id, const char* const* order_ids, size_t n,
                                       me_order_status* out) {
  if (!s) return ME_E_INVALID;
  if (n > ((size_t)1 << 24)) return s->fail(ME_E_INVALID, "order status: more than 2^24 ids");
  if (n && (!order_ids || !out)) return s->fail(ME_E_INVALID, "order status: null order_ids or out");
  if (!has_backend(s)) return s->fail(ME_E_STATE, "no engine");
  if (!s->be.order_query) return s->fail(ME_E_INVALID, "order status: the backend has no order query");
  if (!n) return ME_OK;
  const std::string client = client_id ? client_id : "";
  std::vector<uint64_t> seqs(n);
  for (size_t i = 0; i < n; ++i) seqs[i] = parse_oid(order_ids[i]);
  std::vector<me_order_info> info(n);
  {
    std::lock_guard<std::mutex> le(s->eng_mu);
    const int rc = s->be.order_query(s->be.ctx, seqs.data(), n, info.data());
    if (rc != ME_OK) return s->fail(rc, "engine: " + backend_err(s));
  }
  std::lock_guard<std::mutex> lv(s->live_mu);
  for (size_t i = 0; i < n; ++i) {
    me_order_status& o = out[i];
    memset(&o, 0, sizeof o);
    put(o.order_id, sizeof o.order_id, order_ids[i] ? order_ids[i] : "");
    o.state = ME_OS_NOT_RESTING;
    o.scale = 4;
    if (!seqs[i]) continue;
    auto it = s->live.find(seqs[i]);
    if (it == s->live.end() || it->second.client != client) continue;
    const me_order_info& q = info[i];
    if (!q.found) {  // in a slice not matched yet, or its closing update is on its way
      o.state = ME_OS_PENDING;
      o.quantity = it->second.remaining;
      continue;
    }
    o.state = ME_OS_RESTING;
    o.side = q.side;
    o.quantity = q.qty;
    o.price = q.price_q4;
    o.qty_ahead = q.qty_ahead;
    o.level_qty = q.level_qty;
    o.qty_better = q.qty_better;
    o.orders_ahead = q.orders_ahead;
    o.levels_better = q.levels_better;
  }
  return ME_OK;
}

// PreviewOrder (build extension): SubmitOrder's checks in SubmitOrder's order (a refusal it would answer in-band
// is ME_E_INVALID with its message here), then one me_order_preview. Nothing of the service changes: no OID, no
// slice, no live entry, and a name without a book is not interned — its book is empty, so is its answer.
extern "C" int me_service_preview_order(me_service* s, const me_order_request* r, int32_t tif, me_preview* out) {
  if (!s) return ME_E_INVALID;
  if (!r || !out) return s->fail(ME_E_INVALID, "order preview: null request or out");
  if (!has_backend(s)) return s->fail(ME_E_STATE, "no engine");
  if (!s->be.order_preview) return s->fail(ME_E_INVALID, "order preview: the backend has no order preview");
  const char* symbol = r->symbol ? r->symbol : "";
  if (!symbol[0]) return s->fail(ME_E_INVALID, "symbol is required");
  if (r->quantity <= 0) return s->fail(ME_E_INVALID, "quantity must be > 0");
  if (r->order_type == ME_TYPE_LIMIT && r->price <= 0) return s->fail(ME_E_INVALID, "price must be > 0 for LIMIT");
  if (tif < ME_TIF_GTC || tif > ME_TIF_POST_ONLY || (tif == ME_TIF_POST_ONLY && r->order_type != ME_TYPE_LIMIT))
    return s->fail(ME_E_INVALID, "invalid time in force");
  int64_t q4 = 0;
  const int nr = me_normalize_to_q4(r->price, r->scale, &q4);
  if (nr != 0) return s->fail(ME_E_INVALID, nr == 1 ? "scale out of range" : (nr == 2 ? "overflow" : "underflow"));
  if (r->side != ME_SIDE_BUY && r->side != ME_SIDE_SELL) return s->fail(ME_E_INVALID, "DB insert failed");
  const bool limit = r->order_type == ME_TYPE_LIMIT;
  const uint8_t kd = ME_KIND_TIF(r->side, limit ? ME_TYPE_LIMIT : ME_TYPE_MARKET, ME_OP_NEW, tif);
  uint32_t sid = 0;
  bool known = false;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    auto it = s->sym.find(symbol);
    if ((known = it != s->sym.end())) sid = it->second;
  }
  if (!known) {  // an empty book: a GTC / POST_ONLY LIMIT rests whole, everything else fills nothing
    memset(out, 0, sizeof *out);
    out->remaining_qty = r->quantity;
    const bool rests = limit && (tif == ME_TIF_GTC || tif == ME_TIF_POST_ONLY);
    out->status = rests ? ME_ST_NEW : ME_ST_CANCELED;
    out->flags = rests ? ME_PV_RESTS : 0;
    return ME_OK;
  }
  const int32_t qty = r->quantity;
  me_order_soa q{};
  q.price_q4 = &q4;
  q.qty = &qty;
  q.symbol = &sid;
  q.kind = &kd;
  std::lock_guard<std::mutex> le(s->eng_mu);
  const int rc = s->be.order_preview(s->be.ctx, &q, 1, out);
  if (rc != ME_OK) return s->fail(rc, "engine: " + backend_err(s));
  return ME_OK;
}

// Mass cancel (build extension): the purge itself is one me_mass_cancel; its outcome travels to the owners and
// to the DB as a slice of CANCEL records that the engine never sees — one per removed order, answered CANCELED
// with the removed quantity — through deliver(), so updates, live table, book counts and rows move exactly as
// for cancels the clients had sent.
extern "C" int me_service_mass_cancel(me_service* s, const char* const* symbols, size_t n, int32_t sides,
                                      uint64_t* n_cancelled) {
  if (n_cancelled) *n_cancelled = 0;
  if (!s) return ME_E_INVALID;
  if (!has_backend(s)) return s->fail(ME_E_STATE, "no engine");
  if (!s->be.mass_cancel) return s->fail(ME_E_INVALID, "mass cancel: the backend has no mass cancel");
  if (sides < 1 || sides > 3) return s->fail(ME_E_INVALID, "mass cancel: sides must be 1 (buy), 2 (sell) or 3 (both)");
  std::lock_guard<std::mutex> lf(s->flush_mu);
  std::vector<uint32_t> sids;
  std::vector<std::string> names;
  size_t total = 0;
  uint64_t id = 0;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    if (symbols) {
      std::unordered_map<uint32_t, bool> seen;
      for (size_t i = 0; i < n; ++i) {
        if (!symbols[i]) return s->fail(ME_E_INVALID, "mass cancel: null symbol name");
        auto it = s->sym.find(symbols[i]);
        if (it == s->sym.end()) return s->fail(ME_E_INVALID, std::string("mass cancel: unknown symbol ") + symbols[i]);
        if (!seen.emplace(it->second, true).second)
          return s->fail(ME_E_INVALID, std::string("mass cancel: symbol named twice: ") + symbols[i]);
        sids.push_back(it->second);
        names.push_back(it->first);
      }
    } else {
      for (uint32_t c = 0; c < s->names.size(); ++c) {
        sids.push_back(c);
        names.push_back(s->names[c]);
      }
    }
    close_open(s);
    total = s->closed_records;  // inflight is 0 here (flush_mu held)
    id = s->next_id - 1;        // a cancel's stream position: the last OID allocated
  }
  int rc = flush_closed(s, false, total, nullptr, true);
  if (rc != ME_OK) return rc;
  if (sids.empty()) return ME_OK;
  std::vector<uint8_t> sd(sids.size(), (uint8_t)sides);
  std::vector<uint64_t> counts(2 * sids.size());
  std::vector<me_book_entry> ent;
  {
    std::lock_guard<std::mutex> le(s->eng_mu);
    size_t need = 0;
    rc = s->be.mass_cancel(s->be.ctx, sids.data(), sd.data(), sids.size(), nullptr, 0, &need, counts.data());
    if (rc == ME_E_CAPACITY && need) {  // sized from *n_out (nothing can rest in between: eng_mu is held)
      ent.resize(need);
      rc = s->be.mass_cancel(s->be.ctx, sids.data(), sd.data(), sids.size(), ent.data(), ent.size(), &need,
                             counts.data());
    }
    if (rc != ME_OK) return s->fail(rc, "engine: " + backend_err(s));
    ent.resize(need);
    if (s->md.on) (void)md_pull(s);  // the purge's feed events carry the last slice's stamp
    if (s->dp.on) (void)dp_pull(s);
  }
  if (n_cancelled) *n_cancelled = ent.size();
  if (ent.empty()) return ME_OK;
  Slice sl;
  std::vector<me_order_result> res(ent.size());
  size_t k = 0;
  for (size_t i = 0; i < sids.size(); ++i) {
    const size_t cnt = (size_t)(counts[2 * i] + counts[2 * i + 1]);
    ref_add(s, sids[i], (int64_t)cnt);  // the records' own counts: emit_updates releases them
    for (size_t j = 0; j < cnt && k < ent.size(); ++j, ++k) {
      const me_book_entry& e = ent[k];
      sl.seq.push_back(id);
      sl.px.push_back((int64_t)e.seq);
      sl.qty.push_back(0);
      sl.sid.push_back(sids[i]);
      sl.kind.push_back(ME_KIND(ME_SIDE_BUY, ME_TYPE_LIMIT, ME_OP_CANCEL));
      sl.meta.push_back(Pending{"", names[i], 0, true, e.seq});
      res[k].remaining_qty = e.qty;
      res[k].status = ME_ST_CANCELED;
    }
  }
  {
    std::lock_guard<std::mutex> lk(s->mu);
    s->inflight_records += sl.size();  // (deliver takes them off again)
  }
  deliver(s, std::move(sl), std::move(res), std::vector<me_fill>{}, nullptr);
  std::unique_lock<std::mutex> lq(s->pq_mu);
  s->pq_cv.wait(lq, [&] { return s->pq_emitted == s->pq.size() && (s->pq.empty() || s->pq_stalled); });
  if (s->pq_stalled)
    return s->fail(ME_E_SQLITE, "persistence deferred (" + s->pq_err +
                                    "); the matched slices are kept and retried at the next flush");
  return ME_OK;
}

extern "C" int me_service_market_data(me_service* s, const char* symbol, me_market_data* out) {
  memset(out, 0, sizeof(*out));
  out->scale = 4;
  me_level b{}, a{};
  size_t nb = 0, na = 0;
  const int rc = me_service_book(s, symbol, &b, &a, 1, &nb, &na);
  if (rc != ME_OK) return rc;
  auto sat = [](int64_t v) { return (int32_t)(v > INT32_MAX ? INT32_MAX : v); };
  if (nb) {
    out->has_bid = 1;
    out->best_bid = b.price_q4;
    out->bid_size = sat(b.total_qty);
  }
  if (na) {
    out->has_ask = 1;
    out->best_ask = a.price_q4;
    out->ask_size = sat(a.total_qty);
  }
  return ME_OK;
}

// What the three subscribe calls share. Off: the backend's feed goes off if it was on, and the feed's state
// is dropped. On: `refuse` (a message, when the backend lacks the feed or the request is out of range) answers
// ME_E_INVALID; enable(cap_events) turns the backend's feed on (with 0: off); the feed starts empty with the
// current names owning their books; `first_pull` (or NULL) then reads the books as they stand. also_reset()
// clears what the stream keeps beside the feed, under the same md_mu.
template <class Feed, class Enable, class AlsoReset>
static int feed_subscribe(me_service* s, Feed& f, bool on, const char* refuse, uint64_t cap_events, Enable&& enable,
                          const char* enable_failed, AlsoReset&& also_reset, int (*first_pull)(me_service*)) {
  std::lock_guard<std::mutex> lf(s->flush_mu);  // no slice is in flight while it is held
  std::lock_guard<std::mutex> le(s->eng_mu);
  std::vector<std::string> names;
  if (on) {
    if (refuse) return s->fail(ME_E_INVALID, refuse);
    const int rc = enable(cap_events);
    if (rc != ME_OK) return s->fail(rc, enable_failed + backend_err(s));
    std::lock_guard<std::mutex> lk(s->mu);
    names = s->names;
  } else if (f.on) {
    (void)enable(0);
  }
  {
    std::lock_guard<std::mutex> lm(s->md_mu);
    f.reset(on, on ? &names : nullptr);
    also_reset();
  }
  return on && first_pull ? first_pull(s) : ME_OK;
}

extern "C" int me_service_market_subscribe(me_service* s, int on) {
  if (!s) return ME_E_INVALID;
  const Backend& be = s->be;
  return feed_subscribe(
      s, s->md, on != 0, be.quotes ? nullptr : "market stream: the backend has no quote feed",
      std::max<uint64_t>(4ull * be.num_symbols, 1024),
      [&](uint64_t cap) { return be.quotes_enable ? be.quotes_enable(be.ctx, cap) : (int)ME_OK; },
      "market stream: me_quotes_enable failed: ", [] {}, md_pull);
}

extern "C" int me_service_market_stream(me_service* s, const char* symbol, me_market_update* out, size_t cap,
                                        size_t* n) {
  if (n) *n = 0;
  if (!s || (cap && !out)) return ME_E_INVALID;
  std::lock_guard<std::mutex> lm(s->md_mu);
  if (!s->md.on) return s->fail(ME_E_INVALID, "market stream: not subscribed (me_service_market_subscribe)");
  const size_t k = s->md.take(symbol, cap, [&](const std::string&, const me_market_update& u) { *out++ = u; });
  if (n) *n = k;
  return ME_OK;
}

extern "C" int me_service_depth_subscribe(me_service* s, uint32_t depth) {
  if (!s) return ME_E_INVALID;
  const Backend& be = s->be;
  const char* refuse = !(be.depth_enable && be.depth) ? "depth stream: the matcher has no depth feed"
                       : depth > ME_DEPTH_MAX         ? "depth stream: depth above ME_DEPTH_MAX"
                                                      : nullptr;
  // room for four jobs in which every level of every view changes (off: depth 0, no events)
  return feed_subscribe(
      s, s->dp, depth != 0, refuse, std::max<uint64_t>(16ull * depth * be.num_symbols, 4096),
      [&](uint64_t cap) { return be.depth_enable(be.ctx, depth, cap); }, "depth stream: me_depth_enable failed: ",
      [&] { s->dp_view.clear(); }, dp_pull);
}

extern "C" int me_service_depth_stream(me_service* s, const char* symbol, me_depth_book* out, size_t cap, size_t* n) {
  if (n) *n = 0;
  if (!s || (cap && !out)) return ME_E_INVALID;
  std::lock_guard<std::mutex> lm(s->md_mu);
  if (!s->dp.on) return s->fail(ME_E_INVALID, "depth stream: not subscribed (me_service_depth_subscribe)");
  auto sat = [](int64_t v) { return (int32_t)(v > INT32_MAX ? INT32_MAX : v); };
  auto fill = [&](const std::string& name, me_service::Changed) {  // the symbol's whole current view, best first
    me_depth_book& b = *out++;
    memset(&b, 0, sizeof b);
    put(b.symbol, sizeof b.symbol, name);
    b.scale = 4;
    auto v = s->dp_view.find(name);
    if (v == s->dp_view.end()) return;
    for (auto it = v->second.side[0].rbegin(); it != v->second.side[0].rend() && b.n_bids < ME_DEPTH_MAX; ++it) {
      b.bids[b.n_bids].price = it->first;
      b.bids[b.n_bids++].size = sat(it->second);
    }
    for (auto it = v->second.side[1].begin(); it != v->second.side[1].end() && b.n_asks < ME_DEPTH_MAX; ++it) {
      b.asks[b.n_asks].price = it->first;
      b.asks[b.n_asks++].size = sat(it->second);
    }
    if (!b.n_bids && !b.n_asks) s->dp_view.erase(v);  // (an emptied book is handed out once, then forgotten)
  };
  const size_t k = s->dp.take(symbol, cap, fill);
  if (n) *n = k;
  return ME_OK;
}

extern "C" int me_service_trades_subscribe(me_service* s, int on) {
  if (!s) return ME_E_INVALID;
  const Backend& be = s->be;
  // room for four jobs in which every symbol trades; no first pull: there is no initial state to read
  return feed_subscribe(
      s, s->tr, on != 0, be.trades_enable && be.trades ? nullptr : "trade stream: the matcher has no trade feed",
      std::max<uint64_t>(4ull * be.num_symbols, 1024), [&](uint64_t cap) { return be.trades_enable(be.ctx, cap); },
      "trade stream: me_trades_enable failed: ", [&] { s->tr_cum.clear(); }, nullptr);
}

extern "C" int me_service_trades_stream(me_service* s, const char* symbol, me_trade_update* out, size_t cap, size_t* n) {
  if (n) *n = 0;
  if (!s || (cap && !out)) return ME_E_INVALID;
  std::lock_guard<std::mutex> lm(s->md_mu);
  if (!s->tr.on) return s->fail(ME_E_INVALID, "trade stream: not subscribed (me_service_trades_subscribe)");
  const size_t k = s->tr.take(symbol, cap, [&](const std::string&, const me_trade_update& u) { *out++ = u; });
  if (n) *n = k;
  return ME_OK;
}

// The `stops` table (created at the first enable: a database that never enables stops keeps the reference's
// schema) and its two statements.
static bool open_stops_table(me_service* s, std::string& err) {
  if (s->st_stop_ins && s->st_stop_upd) return true;
  auto chk = [&](int rc, const char* what) {
    if (sql_ok(rc)) return true;
    err = s->sql_err(what);
    return false;
  };
  auto drop = [&] {  // both statements or neither: persist() uses the pair
    for (sqlite3_stmt** st : {&s->st_stop_ins, &s->st_stop_upd}) {
      if (*st) g_sql.finalize(*st);
      *st = nullptr;
    }
  };
  drop();
  const bool ok = chk(g_sql.exec(s->db,
                        "CREATE TABLE IF NOT EXISTS stops ("
                        "  stop_id INTEGER PRIMARY KEY, client_id TEXT NOT NULL, symbol TEXT NOT NULL,"
                        "  side INTEGER NOT NULL CHECK (side IN (1,2)), order_type INTEGER NOT NULL, tif INTEGER NOT NULL,"
                        "  stop_price INTEGER NOT NULL, limit_price INTEGER NOT NULL,"
                        "  quantity INTEGER NOT NULL CHECK (quantity > 0), status INTEGER NOT NULL,"
                        "  order_id TEXT NOT NULL DEFAULT '', trigger_price INTEGER NOT NULL DEFAULT 0,"
                        "  updated_ts INTEGER NOT NULL);",
                        nullptr, nullptr, nullptr),
             "stops schema") &&
         chk(g_sql.prepare_v2(s->db,
                              "INSERT INTO stops(stop_id, client_id, symbol, side, order_type, tif, stop_price, "
                              "limit_price, quantity, status, updated_ts) VALUES (?,?,?,?,?,?,?,?,?,?,?)",
                              -1, &s->st_stop_ins, nullptr),
             "prepare stop insert") &&
         chk(g_sql.prepare_v2(s->db, "UPDATE stops SET status=?, order_id=?, trigger_price=?, updated_ts=? WHERE stop_id=?",
                              -1, &s->st_stop_upd, nullptr),
             "prepare stop update");
  if (!ok) drop();
  return ok;
}

extern "C" int me_service_stops_enable(me_service* s, uint64_t cap_stops) {
  if (!s) return ME_E_INVALID;
  if (!has_backend(s)) return s->fail(ME_E_STATE, "no engine");
  const Backend& be = s->be;
  if (!be.stops_enable) return s->fail(ME_E_INVALID, "stop orders: the matcher has no stop hooks");
  if (cap_stops > me::STOPS_CAP_MAX) return s->fail(ME_E_INVALID, "stop orders: cap_stops above 2^22");
  std::lock_guard<std::mutex> lf(s->flush_mu);  // no slice is in flight while it is held
  if (s->failed) return s->fail(ME_E_STATE, "service failed: the engine lost an accepted slice");
  auto backend_off = [&] {
    std::lock_guard<std::mutex> le(s->eng_mu);
    (void)be.stops_enable(be.ctx, 0);
  };
  if (!cap_stops) {  // off: the backend's table and events go, and what the service held of them
    if (!s->stops_cap) return ME_OK;
    backend_off();
    {
      std::lock_guard<std::mutex> lk(s->mu);
      for (const auto& kv : s->stops) ref_add(s, kv.second.sid, -1);
      s->stops.clear();
      s->stop_ledger = me::StopLedger{};
      s->stops_cap = 0;
      s->stops_triggered = s->stops_recovered = 0;
      s->open.pre.clear();  // operations not applied yet go with it
      for (Slice& sl : s->closed) sl.pre.clear();
    }
    s->stop_hold = me::StopHold{};
    std::lock_guard<std::mutex> lu(s->upd_mu);
    s->stop_updates.clear();
    return ME_OK;
  }
  if (s->stops_cap) return s->fail(ME_E_STATE, "stop orders are already enabled");
  // the persister owns the DB while it has work: wait until it has none (or is stalled on a failed transaction)
  std::vector<std::pair<uint64_t, Stop>> armed;
  uint64_t next_sid = 1;
  if (s->db) {
    std::unique_lock<std::mutex> lq(s->pq_mu);
    s->pq_cv.wait(lq, [&] { return s->pq_emitted == s->pq.size() && (s->pq.empty() || s->pq_stalled); });
    std::string err;
    if (!open_stops_table(s, err)) return s->fail(ME_E_SQLITE, "me_service_stops_enable: " + err);
    sqlite3_stmt* q = nullptr;
    if (!sql_ok(g_sql.prepare_v2(s->db, "SELECT COALESCE(MAX(stop_id), 0) + 1 FROM stops", -1, &q, nullptr)))
      return s->fail(ME_E_SQLITE, "me_service_stops_enable: " + s->sql_err("prepare sid"));
    if (g_sql.step(q) == SQLITE_ROW) next_sid = (uint64_t)g_sql.column_int64(q, 0);
    g_sql.finalize(q);
    q = nullptr;
    if (!sql_ok(g_sql.prepare_v2(s->db,
                                 "SELECT stop_id, client_id, symbol, side, order_type, tif, stop_price, limit_price, "
                                 "quantity FROM stops WHERE status = 0 ORDER BY stop_id",
                                 -1, &q, nullptr)))
      return s->fail(ME_E_SQLITE, "me_service_stops_enable: " + s->sql_err("prepare stop recovery"));
    while (g_sql.step(q) == SQLITE_ROW) {
      Stop st;
      const char* cl = (const char*)g_sql.column_text(q, 1);
      const char* sy = (const char*)g_sql.column_text(q, 2);
      st.client = cl ? cl : "";
      st.symbol = sy ? sy : "";
      st.side = (int32_t)g_sql.column_int64(q, 3);
      st.type = g_sql.column_int64(q, 4) == ME_TYPE_LIMIT ? ME_TYPE_LIMIT : ME_TYPE_MARKET;
      st.tif = (int32_t)g_sql.column_int64(q, 5);
      st.stop_px = g_sql.column_int64(q, 6);
      st.limit_px = g_sql.column_int64(q, 7);
      const long long qty = g_sql.column_int64(q, 8);
      const long long id = g_sql.column_int64(q, 0);
      if (id <= 0 || qty <= 0 || qty > INT32_MAX || (st.side != ME_SIDE_BUY && st.side != ME_SIDE_SELL) ||
          st.tif < ME_TIF_GTC || st.tif > ME_TIF_POST_ONLY || (st.tif == ME_TIF_POST_ONLY && st.type != ME_TYPE_LIMIT) ||
          st.symbol.empty())
        continue;  // (a row this service cannot have written)
      st.qty = (int32_t)qty;
      st.kind = ME_KIND_TIF(st.side, st.type, ME_OP_NEW, st.tif);
      st.armed = true;
      armed.emplace_back((uint64_t)id, std::move(st));
    }
    g_sql.finalize(q);
  }
  if (armed.size() > cap_stops)
    return s->fail(ME_E_CAPACITY, "me_service_stops_enable: the DB holds " + std::to_string(armed.size()) +
                                      " armed stops, more than cap_stops");
  {
    std::lock_guard<std::mutex> le(s->eng_mu);
    const int rc = be.stops_enable(be.ctx, cap_stops);
    if (rc != ME_OK) return s->fail(rc, "me_service_stops_enable: the backend's stops_enable failed: " + backend_err(s));
  }
  std::vector<me_stop> recs(armed.size());
  if (!recs.empty()) memset(recs.data(), 0, recs.size() * sizeof(me_stop));
  bool books = true;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    for (size_t i = 0; books && i < armed.size(); ++i) {
      Stop& st = armed[i].second;
      if (!intern(s, st.symbol, st.sid)) {
        for (size_t j = 0; j < i; ++j) ref_add(s, armed[j].second.sid, -1);
        books = false;
        break;
      }
      ref_add(s, st.sid, 1);  // at once: the next name must not take this book over
      recs[i].id = armed[i].first;
      recs[i].stop_px_q4 = st.stop_px;
      recs[i].limit_px_q4 = st.limit_px;
      recs[i].qty = st.qty;
      recs[i].symbol = st.sid;
      recs[i].kind = st.kind;
    }
  }
  if (!books) {
    backend_off();
    return s->fail(ME_E_CAPACITY, "me_service_stops_enable: the DB holds armed stops on more symbols than the "
                                  "backend has books");
  }
  if (!recs.empty()) {
    int rc;
    {
      std::lock_guard<std::mutex> le(s->eng_mu);
      rc = be.stops_add(be.ctx, recs.data(), recs.size());
    }
    if (rc != ME_OK) {
      const std::string why = backend_err(s);
      for (auto& a : armed) ref_add(s, a.second.sid, -1);
      backend_off();
      return s->fail(rc, "me_service_stops_enable: re-adding the armed stops failed: " + why);
    }
  }
  std::lock_guard<std::mutex> lk(s->mu);
  s->stops_cap = cap_stops;
  // never backwards within one service: a SID handed out before an off / on is not issued again (the rows cover
  // only stops whose boundary was applied, and an in-memory service has no rows at all)
  s->next_sid = std::max(next_sid, s->next_sid);
  s->stop_ledger = me::StopLedger{};
  s->stop_ledger.accepted = armed.size();
  s->stops_triggered = 0;
  s->stops_recovered = armed.size();
  s->stop_hold = me::StopHold{};
  for (auto& a : armed) s->stops.emplace(a.first, std::move(a.second));
  return ME_OK;
}

extern "C" uint64_t me_service_updates_dropped(const me_service* s) {
  me_service* m = const_cast<me_service*>(s);
  std::lock_guard<std::mutex> lk(m->upd_mu);
  return m->updates_dropped;
}

extern "C" int me_service_stats(const me_service* s, uint64_t* reclaimed_books, uint64_t* recovered_orders) {
  if (!s) return ME_E_INVALID;
  me_service* m = const_cast<me_service*>(s);
  std::lock_guard<std::mutex> lk(m->mu);
  {
    std::lock_guard<std::mutex> lr(m->ref_mu);
    if (reclaimed_books) *reclaimed_books = m->reclaimed;
  }
  if (recovered_orders) *recovered_orders = m->recovered;
  return ME_OK;
}

extern "C" int me_service_last_error(const me_service* s, char* buf, size_t cap) {
  std::lock_guard<std::mutex> lk(s->err_mu);
  if (buf && cap) put(buf, cap, s->err);
  return (int)s->err.size();
}
