// The host's view of one store_array_subset before anything touches the device: which chunks of the
// regular grid the subset meets and, for each leaf chunk of them (the chunk, or the inner chunk of a
// shard), whether the subset covers it, meets it partly or leaves it alone. store_classify() is a pure
// function of its arguments: no HIP call, no environment read (this header compiles without the ROCm
// headers), so it runs and is tested on a CPU (tests/test_store_model.py, through zgpu_store_classify).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/zgpu.h"
#include "common.hpp"

namespace zgpu {

#pragma GCC visibility push(hidden)
struct StoreChunk {
  uint64_t lin;              // C-order linear chunk-grid index
  uint64_t origin[ZG_MAXD];  // the chunk's first element in the array
  uint64_t first_leaf;       // index of its first leaf in StoreLayout::leaf_class
  bool covered;              // its whole chunk_shape box lies inside the subset
};
struct StoreLayout {
  uint32_t nd = 0;
  uint64_t leaves_per_chunk = 1;
  uint64_t lpc[ZG_MAXD] = {};      // leaf grid of one chunk
  std::vector<StoreChunk> chunks;  // the chunks the subset meets, in C order of the chunk grid
  std::vector<uint8_t> leaf_class;  // chunks.size() * leaves_per_chunk: ZGPU_LEAF_*, C order of the leaf grid
};
// ZGPU_OK (no chunks for a zero-volume subset), or ZGPU_INVALID_ARGUMENT with a message in err.
int store_classify(uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape, const uint64_t *leaf_shape,
                   const uint64_t *sel_start, const uint64_t *sel_shape, StoreLayout &out, std::string &err);
// Origin (in the array) of leaf j of a chunk.
void store_leaf_origin(const StoreLayout &L, const StoreChunk &c, const uint64_t *leaf_shape, uint64_t j,
                       uint64_t *origin);
#pragma GCC visibility pop

}  // namespace zgpu
