// me_stops.hpp — the host's arithmetic of the trigger book (me_stops_*, include/me_engine.h): the validation
// of an add and of a cancel's ids, and the capacity bound that keeps the event ring from ever deferring. No
// HIP here: it compiles and is tested on a CPU alone (tests/host/stops_host_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "me_engine.h"

namespace me {

constexpr uint64_t STOPS_CAP_MAX = 1ull << 22;  // me_stops_enable's bound; a cancel names no more ids either

// What the host knows of the table since enable. Every count is monotonic and 64 bits wide: none wraps.
struct StopCounts {
  uint64_t added = 0;      // stops ever added
  uint64_t cancelled = 0;  // stops a cancel found live
  uint64_t read = 0;       // events handed out by me_stops_read (the ring's consumed count)
  uint64_t last_id = 0;    // the highest id ever added (0: none)
};

// Stops that are live or triggered and not yet read: each owns one slot of the ring, taken or waiting. An
// upper bound on the live stops that needs nothing from the device, so the host can decide with it whether a
// job has anything to judge. (read <= triggered <= added - cancelled: never negative.)
inline uint64_t stops_pending(const StopCounts& c) { return c.added - c.cancelled - c.read; }

// May n more stops be added under a table / ring of cap entries?
inline bool stops_room(const StopCounts& c, uint64_t n, uint64_t cap) {
  const uint64_t p = stops_pending(c);
  return p <= cap && n <= cap - p;
}

// The first rule an add breaks, or null when all n stops are valid (num_symbols symbols, c.last_id the
// highest id so far). The rules are me_stops_add's, in the header's order.
inline const char* stops_validate(const me_stop* s, size_t n, uint32_t num_symbols, uint64_t last_id) {
  if (n && !s) return "null stops";
  for (size_t i = 0; i < n; ++i) {
    const me_stop& x = s[i];
    if (!x.id) return "id 0";
    if (x.id <= last_id) return i ? "ids not strictly ascending" : "id not above every id added since enable";
    last_id = x.id;
    if (x.symbol >= num_symbols) return "symbol out of range";
    const uint32_t side = x.kind & 3u;
    if (side != ME_SIDE_BUY && side != ME_SIDE_SELL) return "side must be BUY or SELL";
    if (x.qty <= 0) return "qty must be positive";
    if (x.kind & 8u) return "the op bit is set: a stop becomes a NEW record";
    if ((x.kind & 4u) && ((x.kind >> 4) & 3u) == ME_TIF_POST_ONLY) return "POST_ONLY on a MARKET";
  }
  return nullptr;
}

// A cancel's ids: strictly ascending (so each names one stop once and the lanes never race on an entry).
inline bool stops_ids_ascend(const uint64_t* ids, size_t n) {
  for (size_t i = 1; i < n; ++i)
    if (ids[i] <= ids[i - 1]) return false;
  return true;
}

}  // namespace me
