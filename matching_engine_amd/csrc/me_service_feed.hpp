// me_service_feed.hpp — what the service's change streams (quotes, depth, trades) share: no engine, no SQLite.
//
// A backend's feed event names a book by id and carries the number of the slice it belongs to. The service
// turns it into one pending item per symbol NAME, handed out in first-change order. Two things make that more
// than a map: a book changes hands at submit time, while events of earlier slices for its id may still be
// unread, so each feed keeps, per book, who owned it from which slice on; and each feed is read at its own
// moments, so each pops only what its own stamps have passed. Nothing here locks: the service keeps every
// member but `on` under its md_mu (`on` is atomic because the flusher looks at it without that lock).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <deque>
#include <list>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace me {

// Item: what is pending per name (the update's payload). KeyMax: the longest name the handed-out struct
// carries (its symbol field less the NUL); names are keyed cut to it, as the caller will see them.
template <class Item, size_t KeyMax>
struct ServiceFeed {
  struct Entry {
    std::string key;
    Item item;
  };
  std::atomic<bool> on{false};
  std::list<Entry> q;  // one entry per key, in first-change order
  std::unordered_map<std::string, typename std::list<Entry>::iterator> at;
  // per book: {first slice number, symbol}, oldest first
  std::vector<std::deque<std::pair<uint64_t, std::string>>> owner;

  static std::string key_of(const std::string& name) { return name.substr(0, KeyMax); }

  // Slice number k, accepted by the backend, holds a record of `symbol` on book `sid`: the symbol owns the
  // book from slice k on. An entry is added only when the symbol differs from the last one noted.
  void note(uint32_t sid, uint64_t k, const std::string& symbol) {
    if (sid >= owner.size()) owner.resize((size_t)sid + 1);
    auto& h = owner[sid];
    if (h.empty() || h.back().second != symbol) h.emplace_back(k, symbol);
  }

  // The symbol that owned book `sid` at slice `stamp` (a stamp equal to a hand-over's slice names the new
  // owner); NULL for a book no slice ever named. Stamps never decrease, so the owners the stamp has passed
  // are dropped on the way, `popped(name)` run on each.
  template <class Popped>
  const std::string* owner_at(uint32_t sid, uint64_t stamp, Popped&& popped) {
    if (sid >= owner.size() || owner[sid].empty()) return nullptr;
    auto& h = owner[sid];
    while (h.size() > 1 && h[1].first <= stamp) {
      popped(h.front().second);
      h.pop_front();
    }
    return &h.front().second;
  }

  // Empty the feed and switch it; `names` (book id -> symbol, or NULL) own their books from slice 0 on.
  void reset(bool v, const std::vector<std::string>* names) {
    on = v;
    q.clear();
    at.clear();
    owner.clear();
    if (!names) return;
    owner.resize(names->size());
    for (size_t i = 0; i < names->size(); ++i) owner[i].emplace_back(0, (*names)[i]);
  }

  // `name`'s pending item: the one it has, which keeps its place, else a new one at the end of the queue.
  Item& pending(const std::string& name, bool* fresh = nullptr) {
    std::string key = key_of(name);
    auto it = at.find(key);
    if (fresh) *fresh = it == at.end();
    if (it != at.end()) return it->second->item;
    q.push_back(Entry{key, Item{}});
    at.emplace(std::move(key), std::prev(q.end()));
    return q.back().item;
  }

  // Hand out and forget: `symbol`'s entry when one is named (and cap is not 0), else up to `cap` from the
  // front of the queue. emit(key, item) per entry; returns how many.
  template <class Emit>
  size_t take(const char* symbol, size_t cap, Emit&& emit) {
    size_t k = 0;
    if (symbol && *symbol) {
      auto it = at.find(key_of(symbol));
      if (it != at.end() && cap) {
        emit(it->second->key, it->second->item);
        ++k;
        q.erase(it->second);
        at.erase(it);
      }
    } else {
      for (; k < cap && !q.empty(); ++k) {
        emit(q.front().key, q.front().item);
        at.erase(q.front().key);
        q.pop_front();
      }
    }
    return k;
  }
};

}  // namespace me
