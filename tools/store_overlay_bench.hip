// k_subset_overlay against hipMemcpyAsync (device to device) on the same bytes, in one run (DESIGN.md
// section 4): one box of 256 x 512 x 512 float32 (256 MiB) copied out of a subset array whose rows are
// 520 elements long into a staging box of 512-element rows, with the box at innermost offset 0 (source
// and destination rows 16-byte aligned: the vector path) and at offset 1 (the element path).
// Build (from the repository root, after `make -C zarrs_amd/csrc`):
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/store_overlay_bench.hip -Izarrs_amd/csrc \
//     -Lzarrs_amd/lib -lzgpu -Wl,-rpath,'$ORIGIN/../zarrs_amd/lib' -o tools/store_overlay_bench
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "kernels/launch.hpp"

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));              \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

int main() {
  using namespace zgpu;
  const uint64_t E[3] = {256, 512, 512}, SROW = 520, es = 4;
  const uint64_t box_bytes = E[0] * E[1] * E[2] * es, src_bytes = E[0] * E[1] * SROW * es;
  uint8_t *src, *dst;
  ZgOverlayBox *d_box;
  uint64_t *d_rows;
  CK(hipMalloc(&src, src_bytes));
  CK(hipMalloc(&dst, box_bytes));
  CK(hipMalloc(&d_box, sizeof(ZgOverlayBox)));
  CK(hipMalloc(&d_rows, 16));
  CK(hipMemset(src, 1, src_bytes));
  hipStream_t s;
  CK(hipStreamCreate(&s));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const uint64_t rows[2] = {0, E[0] * E[1]};
  CK(hipMemcpy(d_rows, rows, 16, hipMemcpyHostToDevice));
  auto median = [](std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
  };
  for (uint64_t off = 0; off < 2; off++) {
    ZgOverlayBox B{};
    B.src = (uint64_t)(src + off * es);
    B.dst = (uint64_t)dst;
    for (int d = 0; d < 3; d++) B.ext[d] = E[d];
    B.src_stride[2] = B.dst_stride[2] = 1;
    B.src_stride[1] = SROW;
    B.src_stride[0] = SROW * E[1];
    B.dst_stride[1] = E[2];
    B.dst_stride[0] = E[2] * E[1];
    CK(hipMemcpy(d_box, &B, sizeof(B), hipMemcpyHostToDevice));
    std::vector<float> tk, tm;
    for (int it = 0; it < 25; it++) {  // alternating; the first five of each are warm-up
      float ms = 0;
      CK(hipEventRecord(e0, s));
      CK(launch_subset_overlay(d_box, d_rows, 1, rows[1], 3, (uint32_t)es, s));
      CK(hipEventRecord(e1, s));
      CK(hipEventSynchronize(e1));
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (it >= 5) tk.push_back(ms);
      CK(hipEventRecord(e0, s));
      CK(hipMemcpyAsync(dst, src, box_bytes, hipMemcpyDeviceToDevice, s));
      CK(hipEventRecord(e1, s));
      CK(hipEventSynchronize(e1));
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (it >= 5) tm.push_back(ms);
    }
    const double gib = (double)box_bytes / (1 << 30);
    const float k = median(tk), m = median(tm);
    std::printf("innermost offset %llu: k_subset_overlay %.3f ms (%.0f GiB/s copied, min %.3f max %.3f), "
                "hipMemcpyAsync d2d %.3f ms (%.0f GiB/s), ratio %.2f\n",
                (unsigned long long)off, k, gib / (k * 1e-3), *std::min_element(tk.begin(), tk.end()),
                *std::max_element(tk.begin(), tk.end()), m, gib / (m * 1e-3), m / k);
  }
  return 0;
}
