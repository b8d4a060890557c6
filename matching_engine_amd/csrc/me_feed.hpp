// me_feed.hpp — the host's copy-out step of a feed's event ring (FeedRing, me_layout.hpp; Feed,
// me_engine.cpp). No HIP here: it compiles and is tested on a CPU alone (tests/host/feed_ring_test.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>

namespace me {

// Events [consumed, tail) of the ring `log` (event i at log[i % cap], consumed <= tail <= consumed + cap),
// as many as `room` holds, to `out` in order: one copy, or two when the run passes the ring's last slot.
// Returns the events copied; out may be null when room is 0.
template <class Ev>
inline uint64_t feed_copy_out(const Ev* log, uint64_t cap, uint64_t consumed, uint64_t tail, Ev* out, uint64_t room) {
  const uint64_t k = std::min(tail - consumed, room);
  const uint64_t at = consumed % cap;
  const uint64_t first = std::min(k, cap - at);
  if (first) memcpy(out, log + at, first * sizeof(Ev));
  if (k > first) memcpy(out + first, log, (k - first) * sizeof(Ev));
  return k;
}

}  // namespace me
