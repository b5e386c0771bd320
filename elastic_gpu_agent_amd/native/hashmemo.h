// hashmemo.h — HashMemo: the bounded fragment -> hash table through which
// Allocate hands PreStart the hash of a device set both of them digest.
// Header-only, standard library only; wirecore.h's digest_field_put and
// digest_field_runs are its users.
//
// Allocate and PreStart hash the same device set moments apart. For a set
// that qualifies as runs (idruns.h), the runs fragment is an exact name of the
// sorted list (expand_runs rebuilds it byte for byte), so equal fragments mean
// equal joined bytes and equal hashes: Allocate leaves fragment -> hash here
// and PreStart takes it instead of hashing again. A hit removes the entry, so
// every skipped hash stands for one hash Allocate really computed.
//
// Bounds: at most `cap` entries (kMemoEntries by default, 0 = off), keys of
// at most kMemoMaxKey bytes (a longer fragment is not stored and its PreStart
// hashes), so the memo holds about 1 MiB of keys at the most. At the cap the
// oldest entry goes. One mutex guards it: digests run without the GIL on
// several server threads, and the critical sections are a lookup and a copy
// of ~100 bytes.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <list>
#include <mutex>
#include <string>
#include <string_view>
#include <unordered_map>

namespace wirecore {

constexpr size_t kMemoEntries = 256;
constexpr size_t kMemoMaxKey = 4096;

struct HashMemoStats {
  uint64_t puts = 0, hits = 0, misses = 0, evictions = 0;
  size_t entries = 0, cap = 0;
};

class HashMemo {
 public:
  // 0 turns the memo off and empties it; a smaller cap drops the oldest
  void configure(size_t entries) {
    std::lock_guard<std::mutex> g(mu_);
    cap_ = entries;
    while (order_.size() > cap_) drop_oldest();
  }

  // unlocked peek for the callers' fast path; put and take check again
  bool enabled() const { return cap_.load(std::memory_order_relaxed) != 0; }

  void put(std::string_view key, const char hex[8]) {
    if (key.size() > kMemoMaxKey) return;
    std::lock_guard<std::mutex> g(mu_);
    if (!cap_) return;
    ++stats_.puts;
    auto it = index_.find(key);
    if (it != index_.end()) {
      // the same set again: one entry, now the newest
      memcpy(it->second->hex, hex, 8);
      order_.splice(order_.end(), order_, it->second);
      return;
    }
    if (order_.size() >= cap_) {
      drop_oldest();
      ++stats_.evictions;
    }
    order_.emplace_back();
    Entry& e = order_.back();
    e.key.assign(key.data(), key.size());
    memcpy(e.hex, hex, 8);
    index_.emplace(std::string_view(e.key), std::prev(order_.end()));
  }

  // on a hit copies the hash (NUL-terminated) and removes the entry
  bool take(std::string_view key, char hex[9]) {
    std::lock_guard<std::mutex> g(mu_);
    if (!cap_) return false;
    auto it = key.size() <= kMemoMaxKey ? index_.find(key) : index_.end();
    if (it == index_.end()) {
      ++stats_.misses;
      return false;
    }
    ++stats_.hits;
    memcpy(hex, it->second->hex, 8);
    hex[8] = 0;
    auto node = it->second;
    index_.erase(it);  // before the node that owns the key's bytes
    order_.erase(node);
    return true;
  }

  HashMemoStats stats() {
    std::lock_guard<std::mutex> g(mu_);
    HashMemoStats s = stats_;
    s.entries = order_.size();
    s.cap = cap_;
    return s;
  }

 private:
  struct Entry {
    std::string key;
    char hex[8];
  };

  void drop_oldest() {
    index_.erase(std::string_view(order_.front().key));
    order_.pop_front();
  }

  std::mutex mu_;
  std::atomic<size_t> cap_{kMemoEntries};
  std::list<Entry> order_;  // oldest first; the index's keys view these nodes
  std::unordered_map<std::string_view, std::list<Entry>::iterator> index_;
  HashMemoStats stats_;
};

}  // namespace wirecore
