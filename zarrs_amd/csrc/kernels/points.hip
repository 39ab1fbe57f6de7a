// The kernels of a read and of a store by coordinates (points.cpp, store.cpp): Indexer for a list of
// ArrayIndices (zarrs_chunk_grid/src/indexer.rs:285-392) served as partial_decode_fixed_indexer serves it
// (sharding/sharding_partial_decoder_sync.rs:492-560) -- every touched leaf decoded once, the elements
// picked out of the decoded leaves -- with the picking done in HBM; and update_array_bytes_indexer
// (zarrs_codec/src/array_bytes.rs:685-726) -- the update elements copied into the decoded leaves in indexer
// order, so the last of several points on one coordinate wins -- with the copying done in HBM.
//
// A leaf is the decode granule (a chunk, or an inner chunk of a shard); its key is its C-order linear
// index in the array-wide leaf grid (ZgPoints::key_stride). One thread per point in every kernel, a
// grid-stride loop over the points; a point is nd u64 coordinates, row-major.
//   k_points_mark    bounds-checks the point (the smallest offending point index is kept with an atomic
//                    min) and sets its leaf's bit in a bitmap of one bit per key.
//   k_points_gather  key -> slot (the rank of the key's bit: prefix[word] + popcount of the bits below
//                    it) -> source address of the decoded leaf (src[slot]; ZG_POINTS_FILL: the fill
//                    value; ZG_POINTS_SKIP: not staged in this round, out[i] is left alone), plus the
//                    element's C-order offset inside the leaf.
//   k_points_claim   key -> slot -> winner[slot * leaf_n + offset] = max(itself, i + 1): of the points on
//                    one element the one with the highest index i owns it (0: nobody wrote the element).
//   k_points_scatter key -> slot -> the staged leaf (dst[slot]; ZG_POINTS_SKIP: the chunk's entry already
//                    failed, the point is dropped); data[i] is stored iff winner[...] == i + 1, so each
//                    element has one writer and the result does not depend on the schedule. The store has
//                    the element's own width (a byte for ES 1, a halfword for ES 2; a 16-byte element as
//                    two 8-byte halves by its one winner), never a read-modify-write of a wider word:
//                    the neighbouring elements belong to other threads.
// The divisions run in 32 bits (WIDE = false) only when every operand fits: the array's extents (a checked
// coordinate is below them), the leaf's extents (the divisors) and the number of keys; points_geom decides
// it (points_layout.cpp). A 64-bit division is a long software sequence on this hardware. Offsets inside a
// leaf are products and stay 64-bit.
//
// Invariant: a coordinate is used to form an address only after it compared below array_shape[d], in the
// same thread. k_points_mark writes no bit for an out-of-bounds point, the host launches no gather, claim
// or scatter while the out-of-bounds word holds a point, and those three repeat the comparison and skip
// such a point themselves: they read prefix, bitmap and src / dst only at indices derived from in-bounds
// coordinates (key < n_keys, slot < the number of set bits), and winner and the staged leaf only at
// slot * leaf_n + offset with offset < leaf_n (every coordinate's remainder is below the leaf's extent). A
// point whose leaf has no bit has no slot and is skipped. Out-of-bounds coordinates are rejected, never
// dereferenced.
// Plain vector loads and stores; the only atomics are the bitmap's OR, the out-of-bounds min and the
// winner table's max.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "../common.hpp"
#include "launch.hpp"

namespace zgpu {

// The point's key and its element offset inside its leaf; false: out of bounds on axis *bad.
template <typename I>
__device__ __forceinline__ bool point_key(const uint64_t *__restrict__ p, const ZgPoints &P, uint64_t &key,
                                          uint64_t &off, uint32_t &bad) {
  I k = 0;
  uint64_t o = 0;
  for (uint32_t d = 0; d < P.nd; d++) {
    const uint64_t c = p[d];
    if (c >= P.array_shape[d]) {
      bad = d;
      return false;
    }
    const I ci = (I)c, ls = (I)P.leaf_shape[d], l = ci / ls;
    k += l * (I)P.key_stride[d];
    o += (uint64_t)(ci - l * ls) * P.leaf_stride[d];
  }
  key = k;
  off = o;
  return true;
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_points_mark(const uint64_t *__restrict__ idx, ZgPoints P,
                                                     uint32_t *__restrict__ bitmap, unsigned long long *oob) {
  using I = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < P.n; i += step) {
    uint64_t key, off;
    uint32_t bad;
    if (!point_key<I>(idx + i * P.nd, P, key, off, bad)) {
      atomicMin(oob, (unsigned long long)i);
      continue;
    }
    const uint32_t bit = 1u << (key & 31);
    if (!(bitmap[key >> 5] & bit)) atomicOr(&bitmap[key >> 5], bit);  // (clustered points: mostly set already)
  }
}

template <int ES, bool WIDE>
__global__ __launch_bounds__(256) void k_points_gather(const uint64_t *__restrict__ idx, ZgPoints P,
                                                       const uint32_t *__restrict__ bitmap,
                                                       const uint32_t *__restrict__ prefix,
                                                       const uint64_t *__restrict__ src, uint8_t *__restrict__ out) {
  using I = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
  constexpr int U = ES < 8 ? ES : 8;  // a 16-byte element moves as two halves (its natural alignment is 8)
  using T = typename std::conditional<U == 1, uint8_t, typename std::conditional<U == 2, uint16_t,
            typename std::conditional<U == 4, uint32_t, uint64_t>::type>::type>::type;
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < P.n; i += step) {
    uint64_t key, off;
    uint32_t bad;
    if (!point_key<I>(idx + i * P.nd, P, key, off, bad)) continue;
    const uint32_t w = bitmap[key >> 5], below = w & ((1u << (key & 31)) - 1);
    if (!(w >> (key & 31) & 1)) continue;  // (no bit, no slot: the indices changed under the call)
    const uint64_t a = src[(uint64_t)prefix[key >> 5] + __popc(below)];
    if (a == ZG_POINTS_SKIP) continue;
    T v[ES / U];
    if (a == ZG_POINTS_FILL) {
      __builtin_memcpy(v, P.fill, ES);
    } else {
      const T *s = (const T *)a + off * (ES / U);
#pragma unroll
      for (int u = 0; u < ES / U; u++) v[u] = s[u];
    }
    T *o = (T *)(out + i * ES);
#pragma unroll
    for (int u = 0; u < ES / U; u++) o[u] = v[u];
  }
}

// The staged element of point p: false when the point is skipped (out of bounds, no bit, a failed entry).
// cell: the element's index in the winner table; addr: its leaf's staging box.
template <typename I>
__device__ __forceinline__ bool point_cell(const uint64_t *__restrict__ p, const ZgPoints &P, uint64_t leaf_n,
                                           const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ prefix,
                                           const uint64_t *__restrict__ dst, uint64_t &cell, uint64_t &addr,
                                           uint64_t &off) {
  uint64_t key;
  uint32_t bad;
  if (!point_key<I>(p, P, key, off, bad)) return false;
  const uint32_t w = bitmap[key >> 5], below = w & ((1u << (key & 31)) - 1);
  if (!(w >> (key & 31) & 1)) return false;  // (no bit, no slot: the indices changed under the call)
  const uint64_t slot = (uint64_t)prefix[key >> 5] + __popc(below);
  addr = dst[slot];
  cell = slot * leaf_n + off;
  return addr != ZG_POINTS_SKIP;
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_points_claim(const uint64_t *__restrict__ idx, ZgPoints P, uint64_t leaf_n,
                                                      const uint32_t *__restrict__ bitmap,
                                                      const uint32_t *__restrict__ prefix,
                                                      const uint64_t *__restrict__ dst, uint32_t *winner) {
  using I = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < P.n; i += step) {
    uint64_t cell, addr, off;
    if (!point_cell<I>(idx + i * P.nd, P, leaf_n, bitmap, prefix, dst, cell, addr, off)) continue;
    atomicMax(&winner[cell], (uint32_t)i + 1);
  }
}

template <int ES, bool WIDE>
__global__ __launch_bounds__(256) void k_points_scatter(const uint64_t *__restrict__ idx, ZgPoints P, uint64_t leaf_n,
                                                        const uint32_t *__restrict__ bitmap,
                                                        const uint32_t *__restrict__ prefix,
                                                        const uint64_t *__restrict__ dst,
                                                        const uint32_t *__restrict__ winner,
                                                        const uint8_t *__restrict__ data) {
  using I = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
  constexpr int U = ES < 8 ? ES : 8;  // a 16-byte element moves as two halves (its natural alignment is 8)
  using T = typename std::conditional<U == 1, uint8_t, typename std::conditional<U == 2, uint16_t,
            typename std::conditional<U == 4, uint32_t, uint64_t>::type>::type>::type;
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < P.n; i += step) {
    uint64_t cell, addr, off;
    if (!point_cell<I>(idx + i * P.nd, P, leaf_n, bitmap, prefix, dst, cell, addr, off)) continue;
    if (winner[cell] != (uint32_t)i + 1) continue;  // a later point on the same element owns it
    const T *v = (const T *)(data + i * ES);
    T *o = (T *)addr + off * (ES / U);
#pragma unroll
    for (int u = 0; u < ES / U; u++) o[u] = v[u];
  }
}

static uint32_t points_grid(uint64_t n) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)device_cu_count() * 16));
}

hipError_t launch_points_mark(const uint64_t *idx, const ZgPoints &P, bool wide, uint32_t *bitmap, uint64_t *oob,
                              hipStream_t s) {
  if (!P.n) return hipSuccess;
  const dim3 g(points_grid(P.n)), b(256);
  if (wide) hipLaunchKernelGGL(k_points_mark<true>, g, b, 0, s, idx, P, bitmap, (unsigned long long *)oob);
  else hipLaunchKernelGGL(k_points_mark<false>, g, b, 0, s, idx, P, bitmap, (unsigned long long *)oob);
  return hipGetLastError();
}

template <int ES>
static void gather_es(const uint64_t *idx, const ZgPoints &P, bool wide, const uint32_t *bitmap, const uint32_t *prefix,
                      const uint64_t *src, uint8_t *out, hipStream_t s) {
  const dim3 g(points_grid(P.n)), b(256);
  if (wide) hipLaunchKernelGGL((k_points_gather<ES, true>), g, b, 0, s, idx, P, bitmap, prefix, src, out);
  else hipLaunchKernelGGL((k_points_gather<ES, false>), g, b, 0, s, idx, P, bitmap, prefix, src, out);
}

hipError_t launch_points_gather(const uint64_t *idx, const ZgPoints &P, bool wide, uint32_t es, const uint32_t *bitmap,
                                const uint32_t *prefix, const uint64_t *src, uint8_t *out, hipStream_t s) {
  if (!P.n) return hipSuccess;
  switch (es) {
    case 1: gather_es<1>(idx, P, wide, bitmap, prefix, src, out, s); break;
    case 2: gather_es<2>(idx, P, wide, bitmap, prefix, src, out, s); break;
    case 4: gather_es<4>(idx, P, wide, bitmap, prefix, src, out, s); break;
    case 8: gather_es<8>(idx, P, wide, bitmap, prefix, src, out, s); break;
    case 16: gather_es<16>(idx, P, wide, bitmap, prefix, src, out, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_points_claim(const uint64_t *idx, const ZgPoints &P, bool wide, uint64_t leaf_n, const uint32_t *bitmap,
                               const uint32_t *prefix, const uint64_t *dst, uint32_t *winner, hipStream_t s) {
  if (!P.n) return hipSuccess;
  if (P.n >= UINT32_MAX) return hipErrorInvalidValue;  // (winner holds i + 1 in 32 bits)
  const dim3 g(points_grid(P.n)), b(256);
  if (wide) hipLaunchKernelGGL(k_points_claim<true>, g, b, 0, s, idx, P, leaf_n, bitmap, prefix, dst, winner);
  else hipLaunchKernelGGL(k_points_claim<false>, g, b, 0, s, idx, P, leaf_n, bitmap, prefix, dst, winner);
  return hipGetLastError();
}

template <int ES>
static void scatter_es(const uint64_t *idx, const ZgPoints &P, bool wide, uint64_t leaf_n, const uint32_t *bitmap,
                       const uint32_t *prefix, const uint64_t *dst, const uint32_t *winner, const uint8_t *data,
                       hipStream_t s) {
  const dim3 g(points_grid(P.n)), b(256);
  if (wide)
    hipLaunchKernelGGL((k_points_scatter<ES, true>), g, b, 0, s, idx, P, leaf_n, bitmap, prefix, dst, winner, data);
  else
    hipLaunchKernelGGL((k_points_scatter<ES, false>), g, b, 0, s, idx, P, leaf_n, bitmap, prefix, dst, winner, data);
}

hipError_t launch_points_scatter(const uint64_t *idx, const ZgPoints &P, bool wide, uint32_t es, uint64_t leaf_n,
                                 const uint32_t *bitmap, const uint32_t *prefix, const uint64_t *dst,
                                 const uint32_t *winner, const uint8_t *data, hipStream_t s) {
  if (!P.n) return hipSuccess;
  if (P.n >= UINT32_MAX) return hipErrorInvalidValue;
  switch (es) {
    case 1: scatter_es<1>(idx, P, wide, leaf_n, bitmap, prefix, dst, winner, data, s); break;
    case 2: scatter_es<2>(idx, P, wide, leaf_n, bitmap, prefix, dst, winner, data, s); break;
    case 4: scatter_es<4>(idx, P, wide, leaf_n, bitmap, prefix, dst, winner, data, s); break;
    case 8: scatter_es<8>(idx, P, wide, leaf_n, bitmap, prefix, dst, winner, data, s); break;
    case 16: scatter_es<16>(idx, P, wide, leaf_n, bitmap, prefix, dst, winner, data, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace zgpu
