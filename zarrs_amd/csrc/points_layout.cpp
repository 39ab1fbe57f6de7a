// points_geom / points_chunks: the host geometry of a read by coordinates (points_layout.hpp). Pure: no HIP.
#include "points_layout.hpp"

#include <algorithm>

namespace zgpu {

// (zgpu.cpp; declared here, not through internal.hpp, which pulls in the HIP headers)
int set_last_error(int status, const std::string &msg);

std::string points_oob_message(uint64_t point, uint32_t axis, uint64_t coord, uint64_t extent) {
  return "point " + std::to_string(point) + " is out of bounds on axis " + std::to_string(axis) + ": " +
         std::to_string(coord) + " >= " + std::to_string(extent);
}

int points_geom(uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape, const uint64_t *leaf_shape,
                PointsGeom &G, std::string &err) {
  G = PointsGeom{};
  if (nd == 0 || nd > ZG_MAXD) return err = "ndim out of range", ZGPU_INVALID_ARGUMENT;
  if (!leaf_shape) leaf_shape = chunk_shape;
  G.nd = nd;
  for (uint32_t d = 0; d < nd; d++) {
    if (chunk_shape[d] == 0 || leaf_shape[d] == 0) return err = "zero chunk extent", ZGPU_INVALID_ARGUMENT;
    if (chunk_shape[d] % leaf_shape[d]) return err = "shard shape not a multiple of chunk_shape", ZGPU_INVALID_ARGUMENT;
    G.array_shape[d] = array_shape[d];
    G.chunk_shape[d] = chunk_shape[d];
    G.leaf_shape[d] = leaf_shape[d];
    G.chunk_grid[d] = array_shape[d] / chunk_shape[d] + (array_shape[d] % chunk_shape[d] ? 1 : 0);
    G.lpc[d] = chunk_shape[d] / leaf_shape[d];
    // (chunk_grid * lpc <= array_shape + chunk_shape, which may wrap for extents near 2^64)
    if (G.chunk_grid[d] && G.lpc[d] > UINT64_MAX / G.chunk_grid[d])
      return err = "leaf grid too large", ZGPU_INVALID_ARGUMENT;
    G.leaf_grid[d] = G.chunk_grid[d] * G.lpc[d];
    if (G.leaf_grid[d] && G.n_keys > UINT64_MAX / G.leaf_grid[d])
      return err = "leaf grid too large", ZGPU_INVALID_ARGUMENT;
    G.n_keys *= G.leaf_grid[d];
    // (the kernels divide a coordinate by leaf_shape[d]: both operands must fit the narrow type)
    G.wide = G.wide || array_shape[d] > UINT32_MAX || leaf_shape[d] > UINT32_MAX;
  }
  G.wide = G.wide || G.n_keys > UINT32_MAX;
  return ZGPU_OK;
}

void points_key_chunk(const PointsGeom &G, uint64_t key, uint64_t *chunk_lin, uint64_t *origin, uint64_t *leaf_in_chunk) {
  uint64_t ci[ZG_MAXD], li[ZG_MAXD];
  for (int d = (int)G.nd - 1; d >= 0; d--) {
    const uint64_t l = key % G.leaf_grid[d];
    key /= G.leaf_grid[d];
    ci[d] = l / G.lpc[d];
    li[d] = l % G.lpc[d];
  }
  uint64_t lin = 0, j = 0;
  for (uint32_t d = 0; d < G.nd; d++) {
    lin = lin * G.chunk_grid[d] + ci[d];
    j = j * G.lpc[d] + li[d];
    if (origin) origin[d] = li[d] * G.leaf_shape[d];
  }
  *chunk_lin = lin;
  if (leaf_in_chunk) *leaf_in_chunk = j;
}

int points_chunks(uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape, const uint64_t *indices,
                  uint64_t n, std::vector<uint64_t> &out, std::string &err) {
  out.clear();
  PointsGeom G;
  if (const int rc = points_geom(nd, array_shape, chunk_shape, nullptr, G, err)) return rc;
  out.reserve(n);
  uint64_t last = UINT64_MAX;  // runs of points in one chunk (sorted or clustered samples) are pushed once
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t *p = indices + i * nd;
    uint64_t lin = 0;
    for (uint32_t d = 0; d < nd; d++) {
      if (p[d] >= array_shape[d]) {
        out.clear();
        return err = points_oob_message(i, d, p[d], array_shape[d]), ZGPU_INVALID_ARGUMENT;
      }
      lin = lin * G.chunk_grid[d] + p[d] / chunk_shape[d];
    }
    if (lin != last) out.push_back(last = lin);
  }
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
  return ZGPU_OK;
}

}  // namespace zgpu

extern "C" int zgpu_points_chunks(uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                                  const uint64_t *indices, uint64_t n, uint64_t *chunks, uint64_t cap,
                                  uint64_t *n_chunks) {
  if (!array_shape || !chunk_shape || !n_chunks || (n && !indices) || (cap && !chunks))
    return zgpu::set_last_error(ZGPU_INVALID_ARGUMENT, "NULL argument");
  std::vector<uint64_t> out;
  std::string err;
  try {
    if (const int rc = zgpu::points_chunks(nd, array_shape, chunk_shape, indices, n, out, err))
      return zgpu::set_last_error(rc, err);
  } catch (const std::exception &e) {
    return zgpu::set_last_error(ZGPU_INVALID_ARGUMENT, e.what());
  }
  *n_chunks = out.size();
  std::copy_n(out.begin(), std::min<uint64_t>(out.size(), cap), chunks);
  return ZGPU_OK;
}

extern "C" int zgpu_points_geometry(uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                                    const uint64_t *leaf_shape, uint64_t *n_leaves, uint32_t *wide) {
  if (!array_shape || !chunk_shape) return zgpu::set_last_error(ZGPU_INVALID_ARGUMENT, "NULL argument");
  zgpu::PointsGeom G;
  std::string err;
  if (const int rc = zgpu::points_geom(nd, array_shape, chunk_shape, leaf_shape, G, err))
    return zgpu::set_last_error(rc, err);
  if (n_leaves) *n_leaves = G.n_keys;
  if (wide) *wide = G.wide ? 1 : 0;
  return ZGPU_OK;
}
