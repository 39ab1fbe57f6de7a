// What points.cpp (the read by coordinates) and cache.cpp (the decoded-chunk cache) share: the cache's
// half of zgpu_cache_retrieve_elements. Not part of the C ABI.
#pragma once
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/zgpu.h"

namespace zgpu {

#pragma GCC visibility push(hidden)
// One read's hold on a cache: the cache's lock for the read's duration (a slot handed out here must not
// be evicted before the gather has read it), the misses to decode and the slots taken for them.
struct CachePoints {
  zgpu_cache *cache = nullptr;  // set once slots were taken
  bool committed = false;
  // a read that ends before cache_points_commit (an exception on the way to the decode) gives its slots
  // back, under the lock it still holds
  ~CachePoints();
  std::unique_lock<std::mutex> lock;
  bool direct = false;             // the read touches more chunks than the cache holds: nothing is cached
  std::vector<size_t> need;        // positions in lins of the misses whose key is present
  std::vector<int64_t> need_slot;  // their slots
  uint8_t *pool = nullptr;         // slot k at pool + k * slot_bytes
  uint64_t slot_bytes = 0, n_slots = 0;
};
// lins: the distinct chunks the read touches. Counts each as a hit or a miss, caches missing keys as "no
// chunk", and takes a slot for every other miss. direct: the lock is released and nothing else was done.
int cache_points_begin(zgpu_cache *K, zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape,
                       const std::vector<uint64_t> &lins, const void *const *chunk_ptrs, CachePoints &P);
// st: the misses' statuses in the order of P.need (a miss is cached only with status 0).
void cache_points_commit(zgpu_cache *K, CachePoints &P, const std::vector<uint64_t> &lins, const int32_t *st);
// slot[k] of lins[k]: its slot, -1 ("no chunk": the fill value), -2 (not cached: its decode failed)
void cache_points_slots(zgpu_cache *K, const std::vector<uint64_t> &lins, std::vector<int64_t> &slot);
zgpu_ctx *cache_ctx(const zgpu_cache *K);
#pragma GCC visibility pop

}  // namespace zgpu
