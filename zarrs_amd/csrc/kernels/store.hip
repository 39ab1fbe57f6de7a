// The store path's one kernel of its own (store.cpp): the N-d overlay of a read-modify-write.
//
// Array::store_chunk_subset (zarrs/src/array/array_ops/array_update_ops_array.rs:152-210) decodes the
// chunk, pastes the subset's part of it in and encodes the result. Here every partly covered leaf
// chunk of a store has been decoded into a box of its own in a staging array; k_subset_overlay copies
// the overlap of each with the stored subset from `data` (the subset, C order) into that box, all
// boxes in ONE launch.
//
// Work unit: one innermost run of one box (a "row"), a wave each, grid-stride over all (box, row)
// pairs; rows[b] is the first unit of box b (a prefix sum, rows[n_boxes] = all units), found by
// binary search. Inside a run the lanes follow map_elements (value.hip): where the source and the
// destination address agree modulo 16, the units up to the first 16-byte boundary, then one 16-byte
// vector per lane (consecutive lanes, consecutive vectors: 1 KiB per wave instruction), then the
// units after the last whole vector; otherwise unit by unit. A unit is an element, or half of a
// 16-byte element (whose natural alignment is 8). No LDS. Boxes are disjoint, rows of a box are
// disjoint, and the three parts of a run are disjoint: every destination byte has one writer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "../common.hpp"
#include "launch.hpp"

namespace zgpu {

template <int U>
struct ZgUnit {
  using type = typename std::conditional<U == 1, uint8_t, typename std::conditional<U == 2, uint16_t,
               typename std::conditional<U == 4, uint32_t, uint64_t>::type>::type>::type;
};

template <int ES>
__global__ __launch_bounds__(256) void k_subset_overlay(const ZgOverlayBox *__restrict__ boxes,
                                                        const uint64_t *__restrict__ rows, uint32_t n_boxes,
                                                        uint32_t nd) {
  constexpr int U = ES < 8 ? ES : 8;
  using T = typename ZgUnit<U>::type;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t n_rows = rows[n_boxes];
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / 64, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t r = wave; r < n_rows; r += n_waves) {
    uint32_t lo = 0, hi = n_boxes;  // rows[lo] <= r < rows[hi]
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (rows[mid] <= r) lo = mid;
      else hi = mid;
    }
    const ZgOverlayBox &B = boxes[lo];
    uint64_t rem = r - rows[lo], so = 0, dof = 0;
    for (int d = (int)nd - 2; d >= 0; d--) {
      const uint64_t x = rem % B.ext[d];
      rem /= B.ext[d];
      so += x * B.src_stride[d];
      dof += x * B.dst_stride[d];
    }
    const uint8_t *s = (const uint8_t *)B.src + so * ES;
    uint8_t *d = (uint8_t *)B.dst + dof * ES;
    const uint64_t nb = B.ext[nd - 1] * ES;  // bytes of the run
    uint64_t head = 0, body = 0;
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15) == 0) {
      head = (16 - ((uintptr_t)d & 15)) & 15;
      if (head > nb) head = nb;
      body = (nb - head) / 16;
    }
    for (uint64_t k = lane * U; k < head; k += 64 * U) *(T *)(d + k) = *(const T *)(s + k);
    const uint4 *s16 = (const uint4 *)(s + head);
    uint4 *d16 = (uint4 *)(d + head);
    for (uint64_t k = lane; k < body; k += 64) d16[k] = s16[k];
    for (uint64_t k = head + body * 16 + lane * U; k < nb; k += 64 * U) *(T *)(d + k) = *(const T *)(s + k);
  }
}

hipError_t launch_subset_overlay(const ZgOverlayBox *boxes, const uint64_t *rows, uint32_t n_boxes, uint64_t n_rows,
                                 uint32_t nd, uint32_t es, hipStream_t s) {
  if (!n_boxes || !n_rows) return hipSuccess;
  // a wave per row, four to a workgroup; at most a few workgroups per compute unit, the rest by the loop
  const uint64_t want = (n_rows + 3) / 4, cap = (uint64_t)device_cu_count() * 8;
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
  switch (es) {
    case 1: hipLaunchKernelGGL(k_subset_overlay<1>, dim3(grid), dim3(256), 0, s, boxes, rows, n_boxes, nd); break;
    case 2: hipLaunchKernelGGL(k_subset_overlay<2>, dim3(grid), dim3(256), 0, s, boxes, rows, n_boxes, nd); break;
    case 4: hipLaunchKernelGGL(k_subset_overlay<4>, dim3(grid), dim3(256), 0, s, boxes, rows, n_boxes, nd); break;
    case 8: hipLaunchKernelGGL(k_subset_overlay<8>, dim3(grid), dim3(256), 0, s, boxes, rows, n_boxes, nd); break;
    case 16: hipLaunchKernelGGL(k_subset_overlay<16>, dim3(grid), dim3(256), 0, s, boxes, rows, n_boxes, nd); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace zgpu
