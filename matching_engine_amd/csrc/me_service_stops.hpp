// me_service_stops.hpp — the service's own arithmetic of stop orders (me_service_stops_* / _submit_stop /
// _cancel_stop, include/me_service.h): the second id space ("SID-<n>"), the host's mirror of the trigger book's
// capacity bound, the runs a boundary's operations go to the backend in, and the rule that holds an event back
// until its slice is collected. No HIP and no SQLite here: it compiles and is tested on a CPU alone
// (tests/host/stops_service_host_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "me_engine.h"

namespace me {

// "SID-<n>", n >= 1 in decimal with no other byte before or after, n <= UINT64_MAX -> n; else 0.
inline uint64_t parse_sid(const char* s) {
  if (!s || s[0] != 'S' || s[1] != 'I' || s[2] != 'D' || s[3] != '-' || !s[4]) return 0;
  uint64_t v = 0;
  for (const char* p = s + 4; *p; ++p) {
    if (*p < '0' || *p > '9') return 0;
    const uint64_t d = (uint64_t)(*p - '0');
    if (v > (UINT64_MAX - d) / 10) return 0;  // v * 10 + d would wrap
    v = v * 10 + d;
  }
  return v;
}

inline std::string print_sid(uint64_t n) { return "SID-" + std::to_string(n); }

// The host's mirror of me_stops_add's bound. A stop is open from the moment SubmitStop accepts it until its
// cancel is confirmed (found = 1) or its event is PROCESSED; the engine counts it from the add until the cancel
// or until its event is READ. Accepting comes before adding and processing after reading, so open() is never
// below the engine's count: while open() + n <= cap the backend's add cannot be refused. Monotonic, 64 bits.
struct StopLedger {
  uint64_t accepted = 0;
  uint64_t closed = 0;
  uint64_t open() const { return accepted - closed; }
  bool room(uint64_t n, uint64_t cap) const {
    const uint64_t o = open();
    return o <= cap && n <= cap - o;
  }
};

// The operations of one boundary in submission order go to the backend in runs: consecutive adds as one
// stops_add, consecutive cancels as one stops_cancel. [begin, end) indexes the operations.
struct StopRun {
  bool cancel;
  size_t begin, end;
};
inline std::vector<StopRun> stop_runs(const std::vector<uint8_t>& is_cancel) {
  std::vector<StopRun> runs;
  for (size_t i = 0; i < is_cancel.size(); ++i) {
    const bool c = is_cancel[i] != 0;
    if (runs.empty() || runs.back().cancel != c) runs.push_back(StopRun{c, i, i});
    runs.back().end = i + 1;
  }
  return runs;
}

// One run of cancels as stops_cancel wants it: `ids` strictly ascending, each id once. slot[i] is operation
// i's index into ids; first[i] is 0 for an operation that repeats an id named earlier in the run (the earlier
// one takes the backend's answer, the repeat is rejected: the stop is gone by then whatever the answer was).
struct CancelRun {
  std::vector<uint64_t> ids;
  std::vector<size_t> slot;
  std::vector<uint8_t> first;
};
inline CancelRun cancel_run(const uint64_t* op_ids, size_t n) {
  CancelRun r;
  r.ids.assign(op_ids, op_ids + n);
  std::sort(r.ids.begin(), r.ids.end());
  r.ids.erase(std::unique(r.ids.begin(), r.ids.end()), r.ids.end());
  r.slot.resize(n);
  r.first.assign(n, 0);
  std::vector<uint8_t> seen(r.ids.size(), 0);
  for (size_t i = 0; i < n; ++i) {
    const size_t k = (size_t)(std::lower_bound(r.ids.begin(), r.ids.end(), op_ids[i]) - r.ids.begin());
    r.slot[i] = k;
    if (!seen[k]) {
      seen[k] = 1;
      r.first[i] = 1;
    }
  }
  return r;
}

// Events as read from the backend, held until the slice they are stamped with has been collected. The service
// keeps two slices in flight, so a read after collecting slice k may already hold events of slice k + 1; they
// wait, so that what the service does with an event does not depend on how far ahead the device happened to be.
// Stamps never descend along the ring (jobs come in launch order): the events due are a prefix.
struct StopHold {
  std::deque<me_stop_event> q;
  void push(const me_stop_event* ev, size_t n) { q.insert(q.end(), ev, ev + n); }
  // The events stamped <= collected, in ring order; they leave the buffer.
  std::vector<me_stop_event> take_due(uint64_t collected) {
    std::vector<me_stop_event> out;
    while (!q.empty() && q.front().batches <= collected) {
      out.push_back(q.front());
      q.pop_front();
    }
    return out;
  }
  size_t held() const { return q.size(); }
};

}  // namespace me
