// The host's view of a read by coordinates (zgpu_retrieve_elements, points.cpp) before anything touches
// the device: the geometry of the array-wide leaf grid the kernels key their bitmap by, and which chunks
// of the regular grid a list of points touches. Both are pure functions of their arguments: no HIP call,
// no environment read (this header compiles without the ROCm headers), so they run and are tested on a
// CPU (tests/test_points_layout.py, through zgpu_points_chunks).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/zgpu.h"
#include "common.hpp"

namespace zgpu {

#pragma GCC visibility push(hidden)
// The leaf is the decode granule of a read by coordinates: a box of leaf_shape, chunk_shape a multiple of
// it. The array-wide leaf grid is the chunk grid with every chunk cut into its leaves (edge chunks reach
// past the array, and so does the grid); a leaf's key is its C-order linear index in that grid.
struct PointsGeom {
  uint32_t nd = 0;
  bool wide = false;  // some extent (of the array or of the leaf), or the number of keys, needs more than 32 bits
  uint64_t n_keys = 1;
  uint64_t array_shape[ZG_MAXD] = {}, chunk_shape[ZG_MAXD] = {}, leaf_shape[ZG_MAXD] = {};
  uint64_t chunk_grid[ZG_MAXD] = {};  // ceil(array_shape / chunk_shape)
  uint64_t lpc[ZG_MAXD] = {};         // leaves per chunk along each axis
  uint64_t leaf_grid[ZG_MAXD] = {};   // chunk_grid * lpc
};
// ZGPU_OK, or ZGPU_INVALID_ARGUMENT with a message in err (rank, a zero extent, a chunk that is no
// multiple of the leaf, a grid of 2^64 leaves or more). leaf_shape NULL: the chunk is the leaf.
int points_geom(uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape, const uint64_t *leaf_shape,
                PointsGeom &out, std::string &err);
// A key taken apart: the C-order linear index of its chunk in the chunk grid, the leaf's origin inside
// that chunk (elements), and its C-order index among the chunk's leaves.
void points_key_chunk(const PointsGeom &G, uint64_t key, uint64_t *chunk_lin, uint64_t *origin, uint64_t *leaf_in_chunk);
// The distinct C-order linear chunk-grid indices the n points ([n][nd], row-major) touch, ascending.
// A coordinate >= array_shape[d] (IndexerError::OutOfBounds): ZGPU_INVALID_ARGUMENT, err naming the
// first such point and its first offending axis.
int points_chunks(uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape, const uint64_t *indices,
                  uint64_t n, std::vector<uint64_t> &out, std::string &err);
// The message of an out-of-bounds point (one wording for the host and the device check).
std::string points_oob_message(uint64_t point, uint32_t axis, uint64_t coord, uint64_t extent);
#pragma GCC visibility pop

}  // namespace zgpu
