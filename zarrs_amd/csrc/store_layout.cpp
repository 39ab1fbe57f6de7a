// store_classify: the host classification of a store_array_subset (store_layout.hpp). Pure: no HIP.
#include "store_layout.hpp"

#include <algorithm>

namespace zgpu {

// class of the box [org, org + ext) against the subset [s0, s0 + sn)
static uint8_t box_class(uint32_t nd, const uint64_t *org, const uint64_t *ext, const uint64_t *s0,
                         const uint64_t *sn) {
  bool inside = true;
  for (uint32_t d = 0; d < nd; d++) {
    const uint64_t lo = std::max(org[d], s0[d]), hi = std::min(org[d] + ext[d], s0[d] + sn[d]);
    if (lo >= hi) return ZGPU_LEAF_UNTOUCHED;
    inside = inside && lo == org[d] && hi == org[d] + ext[d];
  }
  return inside ? ZGPU_LEAF_COVERED : ZGPU_LEAF_PARTIAL;
}

void store_leaf_origin(const StoreLayout &L, const StoreChunk &c, const uint64_t *leaf_shape, uint64_t j,
                       uint64_t *origin) {
  for (int d = (int)L.nd - 1; d >= 0; d--) {
    origin[d] = c.origin[d] + (j % L.lpc[d]) * leaf_shape[d];
    j /= L.lpc[d];
  }
}

int store_classify(uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape, const uint64_t *leaf_shape,
                   const uint64_t *sel_start, const uint64_t *sel_shape, StoreLayout &out, std::string &err) {
  out = StoreLayout{};
  if (nd == 0 || nd > ZG_MAXD) return err = "ndim out of range", ZGPU_INVALID_ARGUMENT;
  if (!leaf_shape) leaf_shape = chunk_shape;
  out.nd = nd;
  uint64_t grid[ZG_MAXD], lo[ZG_MAXD], hi[ZG_MAXD], idx[ZG_MAXD];
  bool empty = false;
  for (uint32_t d = 0; d < nd; d++) {
    if (chunk_shape[d] == 0 || leaf_shape[d] == 0) return err = "zero chunk extent", ZGPU_INVALID_ARGUMENT;
    if (chunk_shape[d] % leaf_shape[d]) return err = "shard shape not a multiple of chunk_shape", ZGPU_INVALID_ARGUMENT;
    if (sel_start[d] > array_shape[d] || sel_shape[d] > array_shape[d] - sel_start[d])
      return err = "array subset out of bounds", ZGPU_INVALID_ARGUMENT;
    out.lpc[d] = chunk_shape[d] / leaf_shape[d];
    out.leaves_per_chunk *= out.lpc[d];
    grid[d] = (array_shape[d] + chunk_shape[d] - 1) / chunk_shape[d];
    if (sel_shape[d] == 0) {
      empty = true;
      continue;
    }
    lo[d] = idx[d] = sel_start[d] / chunk_shape[d];
    hi[d] = (sel_start[d] + sel_shape[d] - 1) / chunk_shape[d] + 1;
  }
  if (empty) return ZGPU_OK;
  for (;;) {
    StoreChunk c{};
    for (uint32_t d = 0; d < nd; d++) {
      c.lin = c.lin * grid[d] + idx[d];
      c.origin[d] = idx[d] * chunk_shape[d];
    }
    c.first_leaf = out.leaf_class.size();
    c.covered = box_class(nd, c.origin, chunk_shape, sel_start, sel_shape) == ZGPU_LEAF_COVERED;
    for (uint64_t j = 0; j < out.leaves_per_chunk; j++) {
      uint64_t org[ZG_MAXD];
      store_leaf_origin(out, c, leaf_shape, j, org);
      out.leaf_class.push_back(box_class(nd, org, leaf_shape, sel_start, sel_shape));
    }
    out.chunks.push_back(c);
    int d = (int)nd - 1;
    for (; d >= 0; d--) {
      if (++idx[d] < hi[d]) break;
      idx[d] = lo[d];
    }
    if (d < 0) break;
  }
  return ZGPU_OK;
}

}  // namespace zgpu

extern "C" int zgpu_store_classify(uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                                   const uint64_t *leaf_shape, const uint64_t *sel_start, const uint64_t *sel_shape,
                                   uint64_t *chunks, uint8_t *leaf_class, uint64_t cap, uint64_t *n_chunks) {
  if (!array_shape || !chunk_shape || !sel_start || !sel_shape || !n_chunks || (cap && (!chunks || !leaf_class)))
    return ZGPU_INVALID_ARGUMENT;
  zgpu::StoreLayout L;
  std::string err;
  try {
    if (const int rc = zgpu::store_classify(nd, array_shape, chunk_shape, leaf_shape, sel_start, sel_shape, L, err))
      return rc;
  } catch (const std::exception &) {
    return ZGPU_INVALID_ARGUMENT;
  }
  *n_chunks = L.chunks.size();
  for (uint64_t k = 0; k < L.chunks.size() && k < cap; k++) {
    chunks[k] = L.chunks[k].lin;
    std::copy_n(L.leaf_class.begin() + L.chunks[k].first_leaf, L.leaf_class.size() ? L.leaves_per_chunk : 0,
                leaf_class + k * L.leaves_per_chunk);
  }
  return ZGPU_OK;
}
