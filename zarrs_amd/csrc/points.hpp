// What points.cpp (the read by coordinates) shares: with cache.cpp (the decoded-chunk cache) the cache's
// half of zgpu_cache_retrieve_elements, and with store.cpp (the store by coordinates) its front -- the
// geometry, the mark kernel, the bitmap read back and a slot per touched leaf. Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/zgpu.h"
#include "ctx.hpp"
#include "kernels/launch.hpp"
#include "points_layout.hpp"

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

// ---- the front of a call by coordinates: zgpu_retrieve_elements and zgpu_store_elements ----
// A touched leaf: a set bit of the bitmap, in key order.
struct PointSlot {
  uint64_t lin, j;           // its chunk (C-order linear grid index), its index among the chunk's leaves
  uint64_t origin[ZG_MAXD];  // the leaf's origin inside the chunk
  size_t chunk;              // position of lin among the call's distinct chunks
};
struct PointsFront {
  PointsGeom G;
  ZgPoints P{};
  uint64_t words = 0;               // of the bitmap
  const uint64_t *d_idx = nullptr;  // the indices on the device
  uint32_t *d_bitmap = nullptr;
  const uint32_t *bitmap = nullptr;  // read back (pinned, the call's Scratch's)
};
// No device: the leaf grid (points_geom), the bitmap limit, the kernels' arguments. `what` leads the
// messages ("retrieve_elements"). ZGPU_OK, or the status with the message set.
int points_plan(const char *what, uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                const uint64_t *leaf_shape, const uint8_t *fill, const void *indices, uint64_t n, PointsFront &F);
// Host indices uploaded, k_points_mark, the bitmap and the out-of-bounds word read back (synchronises s).
// An out-of-bounds point: ZGPU_INVALID_ARGUMENT, the message naming the smallest such point and its axis.
int points_mark(Scratch &sc, hipStream_t s, const void *indices, bool idx_dev, PointsFront &F);
// A slot per set bit in key order, prefix[w] = the slots before word w, lins = the distinct chunks ascending.
void points_slots(const PointsFront &F, std::vector<uint32_t> &prefix, std::vector<PointSlot> &slots,
                  std::vector<uint64_t> &lins);
#pragma GCC visibility pop

}  // namespace zgpu
