// service_feed_test.cpp — what the service's three change streams share (csrc/me_service_feed.hpp) on its own:
// no engine, no SQLite, no service. Built with -fsanitize=address,undefined and run by
// tests/test_service_feed_host.py; exit 0 = pass. Every expected value below is written out by hand.
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <utility>
#include <vector>

#include "me_service_feed.hpp"

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

struct Item {
  int v;
};
// an update whose symbol field holds 8 chars: names are keyed by their first 7
using Feed = me::ServiceFeed<Item, 7>;
using Out = std::vector<std::pair<std::string, int>>;

static Out take(Feed& f, const char* symbol, size_t cap) {
  Out out;
  const size_t k = f.take(symbol, cap, [&](const std::string& key, const Item& it) { out.emplace_back(key, it.v); });
  CHECK(k == out.size(), "take returned %zu, emitted %zu", k, out.size());
  return out;
}

static std::string name_at(Feed& f, uint32_t sid, uint64_t stamp, std::vector<std::string>* popped = nullptr) {
  const std::string* n = f.owner_at(sid, stamp, [&](const std::string& old) {
    if (popped) popped->push_back(old);
  });
  return n ? *n : "<none>";
}

// A book changes hands at slice 5 while events stamped 3, 5 and 6 are still unread.
static void hand_over() {
  Feed f;
  const std::vector<std::string> names = {"AAA", "BBB"};
  f.reset(true, &names);  // book 0 is AAA's, book 1 BBB's, from slice 0
  f.note(1, 2, "BBB");    // (its own book again)
  f.note(1, 5, "CCC");    // book 1 goes to CCC at slice 5
  f.note(0, 5, "AAA");
  std::vector<std::string> popped;
  CHECK(name_at(f, 1, 3, &popped) == "BBB", "stamp 3 is the old owner's");
  CHECK(popped.empty(), "nothing popped before the hand-over slice");
  CHECK(name_at(f, 1, 5, &popped) == "CCC", "a stamp equal to the hand-over slice is the new owner's");
  CHECK(popped.size() == 1 && popped[0] == "BBB", "the old owner is popped once, by name (%zu popped)", popped.size());
  CHECK(name_at(f, 1, 6, &popped) == "CCC", "stamp 6 is the new owner's");
  CHECK(popped.size() == 1, "the pop callback ran exactly once (%zu)", popped.size());
  CHECK(name_at(f, 0, 6, &popped) == "AAA" && popped.size() == 1, "book 0 never changed hands");
  // two hand-overs passed by one stamp: both old owners are popped, oldest first
  f.note(0, 7, "DDD");
  f.note(0, 9, "EEE");
  popped.clear();
  CHECK(name_at(f, 0, 9, &popped) == "EEE", "two hand-overs behind the stamp");
  CHECK(popped.size() == 2 && popped[0] == "AAA" && popped[1] == "DDD", "both popped, oldest first");
}

// An event for a book no slice ever named, or an id past the history, names nobody.
static void unnamed_book() {
  Feed f;
  f.reset(true, nullptr);
  CHECK(name_at(f, 0, 1) == "<none>", "no history at all");
  f.note(2, 1, "CCC");  // books 0 and 1 now have empty histories
  CHECK(f.owner.size() == 3, "history grown to the noted id (%zu)", f.owner.size());
  CHECK(name_at(f, 0, 1) == "<none>" && name_at(f, 1, 9) == "<none>", "a book no slice ever named");
  CHECK(name_at(f, 3, 1) == "<none>" && name_at(f, 0xFFFFFFFFu, 1) == "<none>", "an id past the history");
  CHECK(name_at(f, 2, 0) == "CCC", "the only owner names every stamp, earlier ones too");
}

// Noting the same symbol again adds no entry.
static void same_symbol_again() {
  Feed f;
  f.note(0, 1, "XXX");
  f.note(0, 2, "XXX");
  f.note(0, 3, "XXX");
  CHECK(f.owner[0].size() == 1 && f.owner[0][0].first == 1, "one entry, from slice 1 (%zu)", f.owner[0].size());
  f.note(0, 4, "YYY");
  f.note(0, 5, "XXX");  // back again: that is a change
  CHECK(f.owner[0].size() == 3 && f.owner[0][2].first == 5, "a return is a new entry (%zu)", f.owner[0].size());
}

// Two changes to one name keep its original place in the queue, with the newer payload.
static void first_change_order() {
  Feed f;
  bool fresh = false;
  f.pending("AAA", &fresh).v = 1;
  CHECK(fresh, "AAA's first change is fresh");
  f.pending("BBB", &fresh).v = 2;
  CHECK(fresh, "BBB's first change is fresh");
  Item& a = f.pending("AAA", &fresh);
  CHECK(!fresh && a.v == 1, "AAA's second change finds its pending item (%d)", a.v);
  a.v = 3;
  CHECK(f.q.size() == 2 && f.at.size() == 2, "two entries (%zu, %zu)", f.q.size(), f.at.size());
  const Out got = take(f, nullptr, 8);
  CHECK(got == (Out{{"AAA", 3}, {"BBB", 2}}), "AAA first with its newer payload, then BBB");
  CHECK(f.q.empty() && f.at.empty(), "drained");
  f.pending("AAA").v = 4;  // handed out and forgotten: the next change queues it anew
  CHECK(take(f, "", 8) == (Out{{"AAA", 4}}), "queued again after it was handed out (an empty name is no name)");
}

// take of one symbol from the middle of the queue, then a drain of the rest in order.
static void take_from_the_middle() {
  Feed f;
  f.pending("AAA").v = 1;
  f.pending("BBB").v = 2;
  f.pending("CCC").v = 3;
  CHECK(take(f, nullptr, 0).empty() && f.q.size() == 3 && f.at.size() == 3, "cap 0 takes and removes nothing");
  CHECK(take(f, "BBB", 0).empty() && f.q.size() == 3 && f.at.size() == 3, "cap 0 with a name: the same");
  CHECK(take(f, "ZZZ", 4).empty() && f.q.size() == 3, "an unknown symbol");
  CHECK(take(f, "BBB", 4) == (Out{{"BBB", 2}}), "one symbol from the middle, whatever the cap");
  CHECK(take(f, "BBB", 4).empty(), "it is gone");
  CHECK(f.q.size() == 2 && f.at.size() == 2, "two left (%zu, %zu)", f.q.size(), f.at.size());
  CHECK(take(f, nullptr, 1) == (Out{{"AAA", 1}}), "the front, cap 1");
  CHECK(take(f, nullptr, 9) == (Out{{"CCC", 3}}), "the rest");
  CHECK(take(f, nullptr, 9).empty() && f.at.empty(), "empty");
}

// Names are keyed as the update carries them: cut to the symbol field.
static void long_names() {
  Feed f;
  f.pending("ABCDEFGH1").v = 1;
  f.pending("QRSTUVW").v = 2;  // exactly the field length minus one: kept whole
  bool fresh = true;
  f.pending("ABCDEFGH2", &fresh).v = 3;  // differs from the first beyond the field only
  CHECK(!fresh, "the two long names share one entry");
  CHECK(f.q.size() == 2 && f.at.size() == 2, "two entries (%zu, %zu)", f.q.size(), f.at.size());
  CHECK(Feed::key_of("ABCDEFGH1") == "ABCDEFG" && Feed::key_of("QRSTUVW") == "QRSTUVW" && Feed::key_of("AB") == "AB",
        "key_of cuts at 7");
  CHECK(take(f, "QRSTUVWXYZ", 1) == (Out{{"QRSTUVW", 2}}), "asked for by a longer name, found under the cut one");
  CHECK(take(f, nullptr, 9) == (Out{{"ABCDEFG", 3}}), "one entry under the cut key, the newer payload");
}

// Reset clears the queue, map and history; a later note starts a fresh history.
static void reset() {
  Feed f;
  const std::vector<std::string> names = {"AAA", "BBB", "CCC"};
  f.reset(true, &names);
  CHECK(f.on.load() && f.owner.size() == 3, "on, three books seeded");
  for (size_t i = 0; i < 3; ++i)
    CHECK(f.owner[i].size() == 1 && f.owner[i][0].first == 0 && f.owner[i][0].second == names[i], "book %zu seeded", i);
  f.note(1, 4, "DDD");
  f.pending("AAA").v = 1;
  f.pending("DDD").v = 2;
  f.reset(false, nullptr);
  CHECK(!f.on.load() && f.q.empty() && f.at.empty() && f.owner.empty(), "off and empty");
  CHECK(name_at(f, 1, 9) == "<none>", "no owner survives");
  f.note(1, 7, "EEE");
  CHECK(f.owner.size() == 2 && f.owner[0].empty() && f.owner[1].size() == 1 && f.owner[1][0].first == 7 &&
            f.owner[1][0].second == "EEE",
        "a fresh history from slice 7");
  CHECK(take(f, nullptr, 9).empty(), "nothing queued");
  f.reset(true, &names);  // subscribe again: seeded anew, the note above is gone
  CHECK(name_at(f, 1, 9) == "BBB" && f.owner[1].size() == 1, "seeded anew");
}

int main() {
  hand_over();
  unnamed_book();
  same_symbol_again();
  first_change_order();
  take_from_the_middle();
  long_names();
  reset();
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("service feed: ok\n");
  return 0;
}
