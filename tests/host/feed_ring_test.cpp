// feed_ring_test.cpp — the host's copy-out step of a feed's event ring (csrc/me_feed.hpp) on its own: no HIP,
// no engine. Built with -fsanitize=address,undefined and run by tests/test_feed_ring_host.py; exit 0 = pass.
//
// Event i carries payload i. A ring of `cap` slots holds events [tail - cap, tail) at most; a reader at
// `consumed` must be handed consumed, consumed + 1, ... in order, whatever the slot they sit in.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "me_feed.hpp"

struct Ev {
  uint64_t payload;
  uint32_t half;  // payload's low 32 bits again: a copy that tears an event shows
  uint32_t pad;
};

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

struct Ring {
  std::vector<Ev> log;  // exactly cap slots: a read past the end is the sanitizer's to find
  uint64_t cap, tail, consumed;
  Ring(uint64_t cap_, uint64_t start) : log(cap_), cap(cap_), tail(start), consumed(start) {
    for (Ev& e : log) e = Ev{~0ull, ~0u, 0};
  }
  void write(uint64_t n) {  // the device's part: events tail .. tail + n - 1 (the caller keeps to the fit rule)
    for (uint64_t i = 0; i < n; ++i, ++tail) log[tail % cap] = Ev{tail, (uint32_t)tail, 0};
  }
  // one read into a buffer of exactly `room` events; checks count, order and what is left
  void read(uint64_t room, uint64_t want_n, uint64_t want_left, const char* what) {
    std::vector<Ev> out(room);
    const uint64_t k = me::feed_copy_out(log.data(), cap, consumed, tail, room ? out.data() : (Ev*)nullptr, room);
    CHECK(k == want_n, "%s: cap %llu: copied %llu, expected %llu", what, (unsigned long long)cap,
          (unsigned long long)k, (unsigned long long)want_n);
    for (uint64_t i = 0; i < k && i < room; ++i)
      CHECK(out[i].payload == consumed + i && out[i].half == (uint32_t)(consumed + i),
            "%s: cap %llu: event %llu holds %llu, expected %llu", what, (unsigned long long)cap,
            (unsigned long long)i, (unsigned long long)out[i].payload, (unsigned long long)(consumed + i));
    consumed += k;
    CHECK(tail - consumed == want_left, "%s: cap %llu: left %llu, expected %llu", what, (unsigned long long)cap,
          (unsigned long long)(tail - consumed), (unsigned long long)want_left);
  }
};

static void cases(uint64_t cap) {
  {
    Ring r(cap, 0);
    r.read(cap, 0, 0, "nothing to read");
    r.read(0, 0, 0, "nothing to read, room 0, null output");
    // a read that ends exactly at the ring's last slot
    r.write(cap);
    r.read(2, 2, cap - 2, "head of a full ring");
    r.read(cap - 2, cap - 2, 0, "ends at the last slot");
    CHECK(r.consumed % cap == 0, "the reader stands at slot 0 again");
    // a read that straddles the end: two copies
    r.write(cap - 2);
    r.read(cap - 3, cap - 3, 1, "up to the last slots");
    r.write(3);  // slots cap - 3 .. cap - 1 are read: 1 + 3 unread events, around the end
    r.read(cap, 4, 0, "straddles the end");
    // output room smaller than what is there, then the rest (which straddles too)
    r.write(cap);
    r.read(0, 0, cap, "room 0 with a null output");
    r.read(3, 3, cap - 3, "room smaller than available");
    r.read(cap, cap - 3, 0, "the read that takes the rest");
    r.read(1, 0, 0, "read empty again");
  }
  {
    // counts above 2^32 with a full ring: % cap on a non-power-of-two at 64 bits (a 32-bit remainder of these
    // counts names other slots: 2^32 % 5 = 1, 2^32 % 7 = 4)
    const uint64_t start = (1ull << 32) + 3 * cap + 1;
    Ring r(cap, start);
    r.write(cap);
    CHECK(r.consumed > (1ull << 32) && r.tail - r.consumed == cap, "a full ring above 2^32");
    CHECK((uint32_t)r.consumed % cap != r.consumed % cap, "the 32-bit remainder differs at cap %llu",
          (unsigned long long)cap);
    r.read(cap + 2, cap, 0, "full ring above 2^32");
    // a full ring read in chunks of 1
    r.write(cap);
    for (uint64_t i = 0; i < cap; ++i) r.read(1, 1, cap - 1 - i, "chunks of 1");
    r.read(1, 0, 0, "chunks of 1: empty");
  }
}

int main() {
  cases(5);
  cases(7);
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("feed ring copy-out: ok\n");
  return 0;
}
