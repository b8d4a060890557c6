// stops_service_host_test.cpp — the service's arithmetic of stop orders (csrc/me_service_stops.hpp) on its own:
// no HIP, no SQLite, no service. Built with -fsanitize=address,undefined and run by
// tests/test_stops_service_host.py; exit 0 = pass.
//
// "SID-<n>" parsing at its edges, the capacity mirror, the runs a boundary's operations go out in (duplicates in a
// cancel run included), and the hold-back of events stamped ahead of the collected slice.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "me_service_stops.hpp"

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

// The text in a heap buffer of exactly its length + 1: a read past the terminator is the sanitizer's to find.
static uint64_t parse(const char* text) {
  std::vector<char> exact(text, text + strlen(text) + 1);
  return me::parse_sid(exact.data());
}

static void test_sid() {
  CHECK(me::parse_sid(nullptr) == 0, "null");
  const char* bad[] = {"",      "S",      "SID",     "SID-",     "SID-0",  "SID-00", "sid-1", "OID-1", "SID-1 ", " SID-1",
                       "SID--1", "SID-+1", "SID-1x",  "SID-1\n",  "SID-0x1", "SID-1.0", "SID_1", "SID-18446744073709551616",
                       "SID-99999999999999999999", "SID-184467440737095516150"};
  for (const char* b : bad) CHECK(parse(b) == 0, "'%s' must be refused", b);
  CHECK(parse("SID-1") == 1, "1");
  CHECK(parse("SID-01") == 1, "leading zero");
  CHECK(parse("SID-4294967296") == 4294967296ull, "2^32");
  CHECK(parse("SID-18446744073709551615") == UINT64_MAX, "UINT64_MAX");
  CHECK(parse("SID-18446744073709551614") == UINT64_MAX - 1, "UINT64_MAX - 1");
  CHECK(parse("SID-18446744073709551609") == UINT64_MAX - 6, "last digit below the edge");
  for (uint64_t v : std::vector<uint64_t>{1, 9, 10, 4294967295ull, 1ull << 53, UINT64_MAX})
    CHECK(me::parse_sid(me::print_sid(v).c_str()) == v, "round trip of %llu", (unsigned long long)v);
  CHECK(me::print_sid(7) == "SID-7", "print");
}

static void test_ledger() {
  me::StopLedger l;
  CHECK(l.open() == 0 && l.room(1, 1) && !l.room(1, 0) && l.room(0, 0), "empty");
  l.accepted = 2;
  CHECK(l.open() == 2 && !l.room(1, 2) && l.room(1, 3) && !l.room(2, 3) && l.room(0, 2), "two open");
  l.closed = 1;  // one triggered and processed
  CHECK(l.open() == 1 && l.room(1, 2) && !l.room(2, 2), "one closed");
  l.accepted = (1ull << 40) + 5;  // counts above 2^32 do not wrap
  l.closed = 1ull << 40;
  CHECK(l.open() == 5 && l.room(3, 8) && !l.room(4, 8), "wide counts");
  l.accepted = UINT64_MAX;
  l.closed = UINT64_MAX - 3;
  CHECK(l.open() == 3 && l.room(UINT64_MAX - 3, UINT64_MAX) && !l.room(UINT64_MAX - 2, UINT64_MAX), "the top");
  l.closed = 0;  // more open than the cap (a cap lowered by a later enable): nothing fits, nothing wraps
  CHECK(!l.room(0, 5) && !l.room(1, 5), "open above cap");
}

static void test_runs() {
  CHECK(me::stop_runs({}).empty(), "no operations");
  const std::vector<uint8_t> ops = {0, 0, 1, 1, 1, 0, 1};
  const std::vector<me::StopRun> r = me::stop_runs(ops);
  CHECK(r.size() == 4, "%zu runs", r.size());
  const size_t want[4][3] = {{0, 0, 2}, {1, 2, 5}, {0, 5, 6}, {1, 6, 7}};
  for (size_t i = 0; i < r.size() && i < 4; ++i)
    CHECK(r[i].cancel == (want[i][0] != 0) && r[i].begin == want[i][1] && r[i].end == want[i][2], "run %zu", i);
  CHECK(me::stop_runs({1}).size() == 1 && me::stop_runs({1})[0].cancel, "one cancel");
  // a cancel run with duplicates, out of order
  const std::vector<uint64_t> ids = {9, 3, 9, UINT64_MAX, 3, 3, 1};
  const me::CancelRun c = me::cancel_run(ids.data(), ids.size());
  CHECK((c.ids == std::vector<uint64_t>{1, 3, 9, UINT64_MAX}), "sorted, each once");
  CHECK((c.slot == std::vector<size_t>{2, 1, 2, 3, 1, 1, 0}), "slots");
  CHECK((c.first == std::vector<uint8_t>{1, 1, 0, 1, 0, 0, 1}), "only the first naming of an id takes the answer");
  for (size_t i = 1; i < c.ids.size(); ++i) CHECK(c.ids[i - 1] < c.ids[i], "strictly ascending");
  const me::CancelRun none = me::cancel_run(nullptr, 0);
  CHECK(none.ids.empty() && none.slot.empty() && none.first.empty(), "an empty run");
}

static me_stop_event event(uint64_t id, uint64_t batches) {
  me_stop_event e;
  memset(&e, 0, sizeof e);
  e.id = id;
  e.batches = batches;
  return e;
}

static void test_hold() {
  me::StopHold h;
  CHECK(h.take_due(100).empty() && h.held() == 0, "empty");
  // slice 3 is collected while slice 4's events are already readable
  const me_stop_event read1[] = {event(11, 3), event(12, 3), event(13, 4)};
  h.push(read1, 3);
  std::vector<me_stop_event> due = h.take_due(2);
  CHECK(due.empty() && h.held() == 3, "nothing is due before its slice is collected");
  due = h.take_due(3);
  CHECK(due.size() == 2 && due[0].id == 11 && due[1].id == 12 && h.held() == 1, "slice 3's events, in ring order");
  CHECK(h.take_due(3).empty(), "handed out once");
  const me_stop_event read2[] = {event(14, 4), event(15, 6)};
  h.push(read2, 2);
  h.push(read2, 0);  // a read that found nothing
  due = h.take_due(5);
  CHECK(due.size() == 2 && due[0].id == 13 && due[1].id == 14 && h.held() == 1, "the held event comes first");
  due = h.take_due(UINT64_MAX);
  CHECK(due.size() == 1 && due[0].id == 15 && h.held() == 0, "the rest");
}

int main() {
  test_sid();
  test_ledger();
  test_runs();
  test_hold();
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("service stop arithmetic: ok\n");
  return 0;
}
