// Adler-32 and Fletcher-32: the two checksums that are linear in the data.
//
//   Adler-32 (RFC 1950; numcodecs.adler32, zarrs/src/array/codec/bytes_to_bytes/adler32/adler32_codec.rs;
//   the zlib trailer): over n bytes, A = sum b_j, B = sum (n - j) b_j, s1 = 1 + A, s2 = n + B (mod 65521),
//   value s2 << 16 | s1.
//   Fletcher-32 (numcodecs.fletcher32, fletcher32_codec.rs:63-96 h5_checksum_fletcher32): over the
//   N = len / 2 big-endian 16-bit words w_k, S1 = sum w_k, S2 = sum (N - k) w_k, folded with end-around
//   carry: r(x) = 0 if x == 0 else ((x - 1) mod 65535) + 1, value r(S2) << 16 | r(S1). As the reference
//   is written a trailing odd byte is never summed (HDF5 and numcodecs do sum it); zarrs is followed.
//
// Both are sums of unit * weight with the weight falling by one per unit (unit = byte / word), so an
// item is cut into ranges of CK_RANGE bytes that are summed as if each stood alone,
// (A_r, B_r) = (sum u, sum (n_r - k) u), and combined with B = sum_r (B_r + tail_r * A_r), tail_r the
// units after range r. tail_r is reduced modulo M before the multiplication, and inside a range the
// weight is at most CK_RANGE, so nothing depends on an upper bound for the item's length.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"  // CK_ADLER32 / CK_FLETCHER32

namespace zgpu {

constexpr uint32_t CK_THREADS = 256;
constexpr uint64_t CK_RANGE = 256u << 10;  // bytes per range (tuning; even, a multiple of 16)
constexpr uint32_t CK_MAX_Y = 256;         // most workgroups per item
static_assert(CK_RANGE % 16 == 0, "ranges are whole 16-byte vectors (and whole Fletcher words)");
// a thread's sums over one range, unreduced: at most CK_RANGE / 16 / 64 + 1 vectors (one wave; fewer in
// a workgroup), each adding at most weight * 8 * 65535 < 2^18 * 2^19 to B
static_assert((CK_RANGE / 16 / 64 + 1) < (1u << 20), "a thread's range sums stay below 2^57");

__host__ __device__ constexpr uint32_t ck_mod(uint32_t kind) { return kind == CK_ADLER32 ? 65521u : 65535u; }

// partial sums of one (item, y) workgroup; done: block y = 0 finished the item itself
struct CkPart {
  uint32_t a, b, nz, done;
};

struct CkSum {
  uint32_t a, b, nz;  // A mod M, B mod M, any unit non-zero
};

// (A, B) of p[0..n) standing alone, n <= CK_RANGE (Fletcher: n even). Every thread takes 16-byte
// vectors at stride 16 * THREADS (any byte alignment: gfx950 runs in unaligned access mode), reduces
// its two 64-bit sums once, and the workgroup adds the residues. The result is valid in thread 0.
// s_red: 3 * THREADS / 64 u32 of LDS; THREADS = 64 (a workgroup of one wave, k_gzip's) needs none and
// takes no workgroup barrier.
template <uint32_t KIND, uint32_t THREADS = CK_THREADS>
__device__ inline CkSum wg_linsum(const uint8_t *p, uint32_t n, uint32_t *s_red) {
  constexpr uint32_t M = ck_mod(KIND);
  const uint32_t t = threadIdx.x;
  uint64_t A = 0, B = 0;
  for (uint32_t j0 = 16u * t; j0 < n; j0 += 16u * THREADS) {
    uint32_t d[4];
    if (j0 + 16 <= n) {
      __builtin_memcpy(d, p + j0, 16);
    } else {  // the last vector: bytes past n are 0 and add nothing
      uint64_t lo = 0, hi = 0;  // (no indexed array: it would live in scratch)
      for (uint32_t k = 0; j0 + k < n; k++) {
        const uint64_t b = p[j0 + k];
        if (k < 8) lo |= b << (8 * k);
        else hi |= b << (8 * (k - 8));
      }
      d[0] = (uint32_t)lo;
      d[1] = (uint32_t)(lo >> 32);
      d[2] = (uint32_t)hi;
      d[3] = (uint32_t)(hi >> 32);
    }
    uint32_t su = 0, sk = 0;  // sum of the vector's units, sum of (index in the vector) * unit
    if (KIND == CK_ADLER32) {
#pragma unroll
      for (uint32_t i = 0; i < 4; i++) {
        const uint32_t b0 = d[i] & 0xffu, b1 = (d[i] >> 8) & 0xffu, b2 = (d[i] >> 16) & 0xffu, b3 = d[i] >> 24;
        const uint32_t s = b0 + b1 + b2 + b3;
        su += s;
        sk += b1 + 2 * b2 + 3 * b3 + 4 * i * s;
      }
      B += (uint64_t)(n - j0) * su - sk;  // sum (n - j0 - k) b_k; k < n - j0 wherever b_k != 0
    } else {
#pragma unroll
      for (uint32_t i = 0; i < 4; i++) {
        const uint32_t w = __builtin_bswap32(d[i]);  // two big-endian words: w >> 16 first
        const uint32_t w0 = w >> 16, w1 = w & 0xffffu;
        su += w0 + w1;
        sk += w1 + 2 * i * (w0 + w1);
      }
      B += (uint64_t)((n - j0) >> 1) * su - sk;
    }
    A += su;
  }
  uint32_t a = (uint32_t)(A % M), b = (uint32_t)(B % M), nz = A != 0;
  for (int off = 32; off; off >>= 1) {  // 64 residues below 2^16: no overflow
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
    nz |= __shfl_down(nz, off, 64);
  }
  if constexpr (THREADS == 64) {
    return CkSum{a % M, b % M, nz};
  }
  constexpr uint32_t NW = THREADS / 64;
  if ((t & 63) == 0) {
    s_red[t / 64] = a;
    s_red[NW + t / 64] = b;
    s_red[2 * NW + t / 64] = nz;
  }
  __syncthreads();
  CkSum r{0, 0, 0};
  if (t == 0) {
    for (uint32_t w = 0; w < NW; w++) {
      r.a += s_red[w];
      r.b += s_red[NW + w];
      r.nz |= s_red[2 * NW + w];
    }
    r.a %= M;
    r.b %= M;
  }
  __syncthreads();
  return r;
}

// bytes of an item of len data bytes that the checksum covers
template <uint32_t KIND>
__host__ __device__ inline uint64_t ck_covered(uint64_t len) {
  return KIND == CK_ADLER32 ? len : len & ~1ull;
}

// range r's share of the item's sums: (A_r, B_r + tail_r * A_r), tail_r units after the range
template <uint32_t KIND>
__device__ inline void ck_accumulate(CkSum &acc, const CkSum &r, uint64_t tail_bytes) {
  constexpr uint32_t M = ck_mod(KIND);
  const uint64_t tail = (KIND == CK_ADLER32 ? tail_bytes : tail_bytes >> 1) % M;  // reduced before the product
  acc.a = (acc.a + r.a) % M;
  acc.b = (uint32_t)((acc.b + r.b + tail * r.a) % M);
  acc.nz |= r.nz;
}

// the checksum value from the item's sums; len: the data bytes
template <uint32_t KIND>
__device__ inline uint32_t ck_value(const CkSum &s, uint64_t len) {
  constexpr uint32_t M = ck_mod(KIND);
  if (KIND == CK_ADLER32) {
    const uint32_t s1 = (1u + s.a) % M, s2 = (uint32_t)((len % M + s.b) % M);
    return (s2 << 16) | s1;
  }
  // x != 0 iff some word is non-zero (every weight is >= 1); then a residue of 0 stands for 0xFFFF
  const uint32_t r1 = !s.nz ? 0u : (s.a ? s.a : 65535u), r2 = !s.nz ? 0u : (s.b ? s.b : 65535u);
  return (r2 << 16) | r1;
}

// Workgroup-wide checksum of p[0..len), ranges taken in turn (the write path, the zlib trailer): valid
// in thread 0.
template <uint32_t KIND, uint32_t THREADS = CK_THREADS>
__device__ inline uint32_t wg_checksum(const uint8_t *p, uint64_t len, uint32_t *s_red) {
  const uint64_t n = ck_covered<KIND>(len);
  CkSum acc{0, 0, 0};
  for (uint64_t off = 0; off < n; off += CK_RANGE) {
    const uint32_t m = (uint32_t)(n - off < CK_RANGE ? n - off : CK_RANGE);
    const CkSum r = wg_linsum<KIND, THREADS>(p + off, m, s_red);
    ck_accumulate<KIND>(acc, r, n - off - m);
  }
  return ck_value<KIND>(acc, len);
}

}  // namespace zgpu
