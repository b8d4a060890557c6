// stops_host_test.cpp — the host's arithmetic of the trigger book (csrc/me_stops.hpp) on its own: no HIP, no
// engine. Built with -fsanitize=address,undefined and run by tests/test_stops_host.py; exit 0 = pass.
//
// Every validation rule of me_stops_add, the ascending rule of me_stops_cancel, and the capacity bound
// added - cancelled - read + n <= cap at its edges and with counts above 2^32.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "me_stops.hpp"

static int g_fail = 0;
#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); \
      printf(__VA_ARGS__);                              \
      printf("\n");                                     \
      ++g_fail;                                         \
    }                                                   \
  } while (0)

static me_stop stop(uint64_t id, uint32_t symbol, uint8_t kind, int32_t qty = 1) {
  me_stop s;
  memset(&s, 0xAB, sizeof s);  // (the pad is ignored: garbage there is valid)
  s.id = id;
  s.stop_px_q4 = INT64_MIN;
  s.limit_px_q4 = INT64_MAX;
  s.qty = qty;
  s.symbol = symbol;
  s.kind = kind;
  return s;
}

static bool ok(const std::vector<me_stop>& v, uint32_t S, uint64_t last) {
  // exactly v.size() records: a read past the end is the sanitizer's to find
  return me::stops_validate(v.data(), v.size(), S, last) == nullptr;
}

int main() {
  static_assert(sizeof(me_stop) == 40 && sizeof(me_stop_event) == 64, "ABI sizes");
  const uint32_t S = 7;
  const uint8_t BUY_L = ME_KIND_TIF(ME_SIDE_BUY, ME_TYPE_LIMIT, ME_OP_NEW, ME_TIF_GTC);
  const uint8_t SELL_M = ME_KIND_TIF(ME_SIDE_SELL, ME_TYPE_MARKET, ME_OP_NEW, ME_TIF_GTC);

  // ---- the rules of an add ----
  CHECK(ok({}, S, 0), "an empty add is valid");
  CHECK(me::stops_validate(nullptr, 0, S, 0) == nullptr, "null with n == 0 is valid");
  CHECK(me::stops_validate(nullptr, 1, S, 0) != nullptr, "null with n > 0");
  CHECK(ok({stop(1, 0, BUY_L), stop(2, 6, SELL_M), stop(~0ull, 3, BUY_L)}, S, 0), "three valid stops, id 2^64 - 1 last");
  CHECK(!ok({stop(0, 0, BUY_L)}, S, 0), "id 0");
  CHECK(!ok({stop(5, 0, BUY_L), stop(5, 0, BUY_L)}, S, 0), "equal ids in a call");
  CHECK(!ok({stop(5, 0, BUY_L), stop(4, 0, BUY_L)}, S, 0), "descending ids in a call");
  CHECK(!ok({stop(5, 0, BUY_L)}, S, 5), "id equal to the highest so far");
  CHECK(!ok({stop(5, 0, BUY_L)}, S, 9), "id below the highest so far");
  CHECK(ok({stop(10, 0, BUY_L)}, S, 9), "id just above the highest so far");
  CHECK(!ok({stop(1, 0, BUY_L)}, S, ~0ull), "nothing is above 2^64 - 1");
  CHECK(ok({stop(1, S - 1, BUY_L)}, S, 0), "the last symbol");
  CHECK(!ok({stop(1, S, BUY_L)}, S, 0), "symbol == num_symbols");
  CHECK(!ok({stop(1, ~0u, BUY_L)}, S, 0), "symbol 2^32 - 1");
  CHECK(!ok({stop(1, 0, ME_KIND_TIF(ME_SIDE_UNSPECIFIED, 0, 0, 0))}, S, 0), "side 0");
  CHECK(!ok({stop(1, 0, ME_KIND_TIF(3, 0, 0, 0))}, S, 0), "side 3");
  CHECK(!ok({stop(1, 0, BUY_L, 0)}, S, 0), "qty 0");
  CHECK(!ok({stop(1, 0, BUY_L, -1)}, S, 0), "qty -1");
  CHECK(!ok({stop(1, 0, BUY_L, INT32_MIN)}, S, 0), "qty INT32_MIN");
  CHECK(ok({stop(1, 0, BUY_L, INT32_MAX)}, S, 0), "qty INT32_MAX");
  CHECK(!ok({stop(1, 0, ME_KIND_TIF(ME_SIDE_BUY, ME_TYPE_LIMIT, ME_OP_CANCEL, 0))}, S, 0), "a CANCEL kind");
  CHECK(!ok({stop(1, 0, ME_KIND_REDUCE | ME_SIDE_BUY)}, S, 0), "a REDUCE kind");
  CHECK(!ok({stop(1, 0, ME_KIND_TIF(ME_SIDE_SELL, ME_TYPE_MARKET, ME_OP_NEW, ME_TIF_POST_ONLY))}, S, 0), "MARKET + POST_ONLY");
  for (int tif = 0; tif < 4; ++tif) {
    CHECK(ok({stop(1, 0, ME_KIND_TIF(ME_SIDE_SELL, ME_TYPE_LIMIT, ME_OP_NEW, tif))}, S, 0), "LIMIT with tif %d", tif);
    if (tif != ME_TIF_POST_ONLY)
      CHECK(ok({stop(1, 0, ME_KIND_TIF(ME_SIDE_BUY, ME_TYPE_MARKET, ME_OP_NEW, tif))}, S, 0), "MARKET with tif %d", tif);
  }
  CHECK(ok({stop(1, 0, (uint8_t)(BUY_L | 0xC0))}, S, 0), "the reserved bits 6-7 are ignored");
  // all or nothing: one bad record anywhere fails the call
  for (size_t bad = 0; bad < 5; ++bad) {
    std::vector<me_stop> v;
    for (size_t i = 0; i < 5; ++i) v.push_back(stop(10 + i, (uint32_t)i, i == bad ? (uint8_t)0 : BUY_L));
    CHECK(!ok(v, S, 0), "a bad record at %zu of 5", bad);
  }

  // ---- a cancel's ids ----
  {
    const uint64_t a[] = {1, 2, ~0ull}, b[] = {1, 1}, c[] = {2, 1}, d[] = {0};
    CHECK(me::stops_ids_ascend(a, 3), "ascending ids");
    CHECK(!me::stops_ids_ascend(b, 2), "equal ids");
    CHECK(!me::stops_ids_ascend(c, 2), "descending ids");
    CHECK(me::stops_ids_ascend(d, 1) && me::stops_ids_ascend(nullptr, 0), "one id, no id");
  }

  // ---- the capacity bound ----
  {
    me::StopCounts c;
    const uint64_t cap = 8;
    CHECK(me::stops_pending(c) == 0 && me::stops_room(c, 8, cap) && !me::stops_room(c, 9, cap), "an empty table: == cap fits, cap + 1 does not");
    CHECK(me::stops_room(c, 0, cap) && !me::stops_room(c, ~0ull, cap), "n = 0 and n = 2^64 - 1");
    c.added = 8;
    CHECK(me::stops_pending(c) == 8 && me::stops_room(c, 0, cap) && !me::stops_room(c, 1, cap), "a full table");
    c.cancelled = 2;  // two cancelled: two free
    CHECK(me::stops_room(c, 2, cap) && !me::stops_room(c, 3, cap), "after two cancels");
    c.read = 3;  // three triggered and read: five free
    CHECK(me::stops_pending(c) == 3 && me::stops_room(c, 5, cap) && !me::stops_room(c, 6, cap), "after three events read");
    // triggered but unread stops still hold their slot: nothing of the device's enters the bound
    c.added = 13;
    CHECK(me::stops_pending(c) == 8 && !me::stops_room(c, 1, cap), "full again");
  }
  {  // counts above 2^32: nothing wraps at 32 bits
    me::StopCounts c;
    const uint64_t cap = 1ull << 22, big = (1ull << 32) + 12345;
    c.added = 3 * big + cap;
    c.cancelled = big;
    c.read = 2 * big;
    CHECK(me::stops_pending(c) == cap, "pending %llu", (unsigned long long)me::stops_pending(c));
    CHECK(me::stops_room(c, 0, cap) && !me::stops_room(c, 1, cap), "full at counts above 2^32");
    c.read += 1;
    CHECK(me::stops_room(c, 1, cap) && !me::stops_room(c, 2, cap), "one slot at counts above 2^32");
    c.cancelled += cap - 1;
    CHECK(me::stops_pending(c) == 0 && me::stops_room(c, cap, cap) && !me::stops_room(c, cap + 1, cap), "empty at counts above 2^32");
    CHECK(!me::stops_room(c, (1ull << 32) + 1, cap), "n above 2^32 is not taken for 1");
    c.added = ~0ull;  // the counters' own end
    c.cancelled = ~0ull - 5;
    c.read = 0;
    CHECK(me::stops_pending(c) == 5, "pending at the end of u64");
  }
  CHECK(me::STOPS_CAP_MAX == (1ull << 22), "the enable bound");

  if (g_fail) {
    printf("%d failures\n", g_fail);
    return 1;
  }
  printf("trigger book host arithmetic: ok\n");
  return 0;
}
