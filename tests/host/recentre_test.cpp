// recentre_test.cpp — recentre_base (csrc/me_layout.hpp), the new window base of a re-centre, on the host: no GPU,
// no engine. Built with -fsanitize=address,undefined and run by tests/test_recentre_host.py; exit 0 = pass. A
// signed overflow anywhere in the function ends the run (-fno-sanitize-recover).
//
// The spec below is written in __int128, where nothing can overflow. For every window size, every presence of
// the two best prices and every (target, best_bid < best_ask) from the edge list:
//   R   the result lies in [INT64_MIN, INT64_MAX - L + 1]                 (base + L - 1 is an int64)
//   B   with a bid:  best_bid < nb + L                                     (invariant I: no bid above the window)
//   A   with an ask: best_ask >= nb                                        (invariant I: no ask below the window)
//   C   nb == target - L/2 whenever that value satisfies R, B and A        (centred when it can be)
// and the result equals the spec's: target - L/2 clamped into R, raised to the least base B allows, then
// lowered to the ask (A wins over B only where best_bid >= best_ask + L, which best_bid < best_ask excludes).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "me_layout.hpp"

typedef __int128 i128;

static int g_fail = 0;
static void fail(const char* what, uint32_t L, bool wb, bool wa, long long t, long long bb, long long ba, long long nb) {
  if (++g_fail <= 20)
    printf("FAIL %s: L %u with_bid %d with_ask %d target %lld best_bid %lld best_ask %lld -> %lld\n", what, L, wb, wa,
           t, bb, ba, nb);
}

static i128 spec(i128 t, i128 L, bool wb, i128 bb, bool wa, i128 ba) {
  const i128 lo = INT64_MIN, hi = (i128)INT64_MAX - L + 1;
  i128 nb = t - L / 2;
  if (nb < lo) nb = lo;
  if (nb > hi) nb = hi;
  if (wb) {
    i128 need = bb - L + 1;  // the least base with bb < base + L
    if (need < lo) need = lo;
    if (nb < need) nb = need;
  }
  if (wa && nb > ba) nb = ba;
  return nb;
}

int main() {
  const uint32_t Ls[] = {64, 128, 256, 1024, 2048, 32768};
  unsigned long long cases = 0, centred = 0;
  for (uint32_t L : Ls) {
    const i128 l = L, MIN = INT64_MIN, MAX = INT64_MAX, hi = MAX - l + 1;
    const i128 pts128[] = {MIN, MIN + 1, MIN + l / 2 - 1, MIN + l / 2, MIN + l - 1, MIN + l, -1, 0, 1,
                           hi - 1, hi, hi + 1, MAX - l / 2, MAX - 1, MAX};
    std::vector<long long> pts;
    for (i128 p : pts128) pts.push_back((long long)p);
    for (int wbi = 0; wbi < 2; ++wbi)
      for (int wai = 0; wai < 2; ++wai)
        for (long long t : pts)
          for (long long bb : pts)
            for (long long ba : pts) {
              if (!(bb < ba)) continue;
              const bool wb = wbi != 0, wa = wai != 0;
              const long long nb = me::recentre_base(t, L, wb, bb, wa, ba);
              ++cases;
              const i128 n = nb;
              if (n < MIN || n > hi) fail("R", L, wb, wa, t, bb, ba, nb);
              if (wb && !((i128)bb < n + l)) fail("B", L, wb, wa, t, bb, ba, nb);
              if (wa && !((i128)ba >= n)) fail("A", L, wb, wa, t, bb, ba, nb);
              const i128 c = (i128)t - l / 2;
              const bool c_ok = c >= MIN && c <= hi && (!wb || (i128)bb < c + l) && (!wa || (i128)ba >= c);
              if (c_ok) {
                ++centred;
                if (n != c) fail("C", L, wb, wa, t, bb, ba, nb);
              }
              if (n != spec(t, l, wb, bb, wa, ba)) fail("spec", L, wb, wa, t, bb, ba, nb);
            }
  }
  printf("%llu cases, %llu centred, %d failures\n", cases, centred, g_fail);
  if (g_fail || cases < 6ull * 4 * 15 * 100 || centred == 0) return 1;
  printf("recentre_base: ok\n");
  return 0;
}
