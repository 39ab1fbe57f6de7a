// Checksums and shard-index resolution for gfx950.
//
//   crc32c stage   zarrs/src/array/codec/bytes_to_bytes/crc32c/crc32c_codec.rs:108-158
//                  (4-byte LE checksum at End/Start; verify only on the full-decode path and when
//                  validate_checksums; the partial path strips: strip_suffix_partial_decoder.rs:39-62)
//   shard index    zarrs/src/array/codec/array_to_bytes/sharding.rs:156-235 and
//                  sharding/sharding_codec.rs:1262-1298 (index chain bytes{endian}+crc32c, decoded
//                  and verified on both paths), :617-707 (empty entry = (u64::MAX, u64::MAX) -> fill;
//                  offset+size > shard length -> "out-of-bounds" error)
//
// Parallel CRC (crc.hpp): one workgroup per byte range, slice-by-4 segments merged by crc32_combine.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../common.hpp"
#include "crc.hpp"
#include "launch.hpp"
#include "linsum.hpp"

namespace zgpu {

__global__ __launch_bounds__(CRC_THREADS) void k_crc32c_strip(ZgItem *items, uint32_t *status, int at_start,
                                                              int verify) {
  __shared__ CrcTables T;
  __shared__ uint64_t s_len[CRC_THREADS / 64];
  __shared__ uint32_t s_crc[CRC_THREADS / 64];
  const uint32_t i = blockIdx.x;
  ZgItem it = items[i];
  if (status[i] || (it.flags & ZG_ITEM_FILL)) return;
  if (it.len < 4) {
    if (threadIdx.x == 0) status[i] = ZG_CRC_INPUT_TOO_SHORT;
    return;
  }
  const uint8_t *base = (const uint8_t *)it.src;
  const uint8_t *data = at_start ? base + 4 : base;
  const uint8_t *stored = at_start ? base : base + it.len - 4;
  const uint64_t n = it.len - 4;
  if (verify && !(it.flags & ZG_ITEM_PARTIAL)) {
    build_tables(T, POLY_CRC32C);
    const uint32_t c = wg_crc(data, n, T, POLY_CRC32C, s_len, s_crc);
    if (threadIdx.x == 0) {
      const uint32_t s = stored[0] | stored[1] << 8 | stored[2] << 16 | (uint32_t)stored[3] << 24;
      if (s != c) {
        status[i] = ZG_INVALID_CHECKSUM;
        return;
      }
    }
  }
  if (threadIdx.x == 0) {
    items[i].src = (uint64_t)data;
    items[i].len = n;
  }
}

// The trailing crc32c of C3's inner chain verified beside the one-wave k_gzip (which strips the 4 bytes
// itself, crc_tail 3) on a side stream: reads a snapshot of the items and statuses taken before the
// fork (k_gzip rewrites both), writes only bad[i]. k_crc32c_merge, after the join, makes a failed
// checksum the item's status whatever k_gzip reported (the chain decodes crc32c first,
// crc32c_codec.rs:108-141).
__global__ __launch_bounds__(CRC_THREADS) void k_crc32c_check(const ZgItem *items, const uint32_t *status,
                                                              uint32_t *bad) {
  __shared__ CrcTables T;
  __shared__ uint64_t s_len[CRC_THREADS / 64];
  __shared__ uint32_t s_crc[CRC_THREADS / 64];
  const uint32_t i = blockIdx.x;
  const ZgItem it = items[i];
  if (threadIdx.x == 0) bad[i] = 0;
  if (status[i] || (it.flags & (ZG_ITEM_FILL | ZG_ITEM_PARTIAL)) || it.len < 4) return;
  const uint8_t *data = (const uint8_t *)it.src;
  const uint8_t *stored = data + it.len - 4;
  build_tables(T, POLY_CRC32C);
  const uint32_t c = wg_crc(data, it.len - 4, T, POLY_CRC32C, s_len, s_crc);
  if (threadIdx.x == 0) {
    const uint32_t st = stored[0] | stored[1] << 8 | stored[2] << 16 | (uint32_t)stored[3] << 24;
    bad[i] = st != c;
  }
}

__global__ void k_crc32c_merge(uint32_t *status, const uint32_t *bad, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && bad[i]) status[i] = ZG_INVALID_CHECKSUM;
}

hipError_t launch_crc32c_check(const ZgItem *items, const uint32_t *status, uint32_t *bad, uint32_t n_items,
                               hipStream_t s) {
  if (!n_items) return hipSuccess;
  hipLaunchKernelGGL(k_crc32c_check, dim3(n_items), dim3(CRC_THREADS), 0, s, items, status, bad);
  return hipGetLastError();
}

hipError_t launch_crc32c_merge(uint32_t *status, const uint32_t *bad, uint32_t n_items, hipStream_t s) {
  if (!n_items) return hipSuccess;
  hipLaunchKernelGGL(k_crc32c_merge, dim3((n_items + 255) / 256), dim3(256), 0, s, status, bad, n_items);
  return hipGetLastError();
}

hipError_t launch_crc32c_strip(ZgItem *items, uint32_t *status, uint32_t n_items, int at_start, int verify,
                               hipStream_t s) {
  if (!n_items) return hipSuccess;
  hipLaunchKernelGGL(k_crc32c_strip, dim3(n_items), dim3(CRC_THREADS), 0, s, items, status, at_start, verify);
  return hipGetLastError();
}

// ------------------------------- Adler-32 (zlib trailer) ---------------------------------------
// The decoded stream's Adler-32 (linsum.hpp) against the trailer k_gzip<true> left in aux[i].x, for
// the zlib streams of a blosc stream table (a plan's zlib stage checks it inside k_gzip).
__global__ __launch_bounds__(CK_THREADS) void k_adler32_check(const ZgItem *items, uint32_t *status,
                                                              const uint32_t *kind, const uint2 *aux) {
  __shared__ uint32_t s_red[3 * CK_THREADS / 64];
  const uint32_t i = blockIdx.x;
  if (kind[i] != BL_KIND_ZLIB || status[i] != 0) return;
  const ZgItem it = items[i];
  const uint32_t adler = wg_checksum<CK_ADLER32>((const uint8_t *)it.src, it.len, s_red);
  if (threadIdx.x == 0 && adler != aux[i].x) status[i] = ZG_CORRUPT_STREAM;
}

hipError_t launch_adler32_check(const ZgItem *subs, uint32_t *sub_status, const uint32_t *sub_kind, uint32_t n_sub,
                                const uint2 *aux, hipStream_t s) {
  if (!n_sub) return hipSuccess;
  hipLaunchKernelGGL(k_adler32_check, dim3(n_sub), dim3(CK_THREADS), 0, s, subs, sub_status, sub_kind, aux);
  return hipGetLastError();
}

// ------------------------------- adler32 / fletcher32 stages ----------------------------------
// numcodecs.adler32 (adler32_codec.rs: 4-byte LE value at Start (the default) or End) and
// numcodecs.fletcher32 (fletcher32_codec.rs: 4-byte LE value at the end), with k_crc32c_strip's
// semantics: an item below 4 bytes is CRC_INPUT_TOO_SHORT, verified only when the plan validates and
// the item is not on the partial path, INVALID_CHECKSUM on a mismatch, then stripped.
// Grid (items, Y): workgroup (i, y) sums ranges y, y + Y, ... of item i (linsum.hpp) into
// parts[i * Y + y]; k_linsum_finish adds an item's Y parts, compares and strips. An item of at most
// one range (and every item that is skipped or only stripped) is finished by its workgroup y = 0,
// which says so in parts[i * Y].done. With Y = 1 the one workgroup of an item holds all its sums, so
// it finishes the item whatever its length and there is no second launch. Y comes from the host's
// guess at the items' lengths (an inner chunk's length is only known on the device): it decides how
// many workgroups share an item, never the result.
__device__ __forceinline__ uint32_t ck_le32(const uint8_t *p) {
  return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24;
}

template <uint32_t KIND>
__global__ __launch_bounds__(CK_THREADS) void k_linsum_strip(ZgItem *items, uint32_t *status, CkPart *parts,
                                                             int at_start, int verify) {
  __shared__ uint32_t s_red[3 * CK_THREADS / 64];
  const uint32_t i = blockIdx.x, y = blockIdx.y, Y = gridDim.y, t = threadIdx.x;
  const ZgItem it = items[i];
  CkPart *part = parts + (uint64_t)i * Y + y;
  const bool lead = y == 0 && t == 0;
  if (status[i] || (it.flags & ZG_ITEM_FILL)) {
    if (lead) part->done = 1;
    return;
  }
  if (it.len < 4) {
    if (lead) {
      status[i] = ZG_CRC_INPUT_TOO_SHORT;
      part->done = 1;
    }
    return;
  }
  const uint8_t *base = (const uint8_t *)it.src;
  const uint8_t *data = at_start ? base + 4 : base;
  const uint8_t *stored = at_start ? base : base + it.len - 4;
  const uint64_t len = it.len - 4, n = ck_covered<KIND>(len);
  if (!verify || (it.flags & ZG_ITEM_PARTIAL)) {
    if (lead) {
      items[i].src = (uint64_t)data;
      items[i].len = len;
      part->done = 1;
    }
    return;
  }
  const bool alone = n <= CK_RANGE || Y == 1;  // this item's sums all belong to workgroup y = 0
  if (alone && y) return;
  CkSum acc{0, 0, 0};
  for (uint64_t off = (uint64_t)y * CK_RANGE; off < n; off += (uint64_t)Y * CK_RANGE) {
    const uint32_t m = (uint32_t)(n - off < CK_RANGE ? n - off : CK_RANGE);
    const CkSum r = wg_linsum<KIND>(data + off, m, s_red);
    ck_accumulate<KIND>(acc, r, n - off - m);
  }
  if (t) return;
  if (!alone) {
    *part = CkPart{acc.a, acc.b, acc.nz, 0};
    return;
  }
  if (ck_value<KIND>(acc, len) != ck_le32(stored)) {
    status[i] = ZG_INVALID_CHECKSUM;
  } else {
    items[i].src = (uint64_t)data;
    items[i].len = len;
  }
  part->done = 1;
}

template <uint32_t KIND>
__global__ void k_linsum_finish(ZgItem *items, uint32_t *status, const CkPart *parts, uint32_t n_items, uint32_t Y,
                                int at_start) {
  constexpr uint32_t M = ck_mod(KIND);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const CkPart *part = parts + (uint64_t)i * Y;
  if (part[0].done) return;
  uint64_t a = 0, b = 0;  // Y <= CK_MAX_Y residues below 2^16
  uint32_t nz = 0;
  for (uint32_t y = 0; y < Y; y++) {
    a += part[y].a;
    b += part[y].b;
    nz |= part[y].nz;
  }
  const ZgItem it = items[i];
  const uint8_t *base = (const uint8_t *)it.src;
  const uint8_t *data = at_start ? base + 4 : base;
  const uint8_t *stored = at_start ? base : base + it.len - 4;
  const CkSum sum{(uint32_t)(a % M), (uint32_t)(b % M), nz};
  if (ck_value<KIND>(sum, it.len - 4) != ck_le32(stored)) {
    status[i] = ZG_INVALID_CHECKSUM;
    return;
  }
  items[i].src = (uint64_t)data;
  items[i].len = it.len - 4;
}

uint32_t linsum_grid_y(uint64_t len_hint) {
  const uint64_t y = (len_hint + CK_RANGE - 1) / CK_RANGE;
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(y, 1), CK_MAX_Y);
}

uint64_t linsum_scratch_bytes(uint32_t n_items, uint64_t len_hint) {
  return (uint64_t)n_items * linsum_grid_y(len_hint) * sizeof(CkPart);
}

template <uint32_t KIND>
static hipError_t linsum_strip(ZgItem *items, uint32_t *status, uint32_t n_items, int at_start, int verify,
                               uint64_t len_hint, void *scratch, hipStream_t s) {
  const uint32_t Y = linsum_grid_y(len_hint);
  // the y axis of a grid is limited to 65535 blocks, the x axis is not
  hipLaunchKernelGGL(k_linsum_strip<KIND>, dim3(n_items, Y), dim3(CK_THREADS), 0, s, items, status, (CkPart *)scratch,
                     at_start, verify);
  if (Y > 1)
    hipLaunchKernelGGL(k_linsum_finish<KIND>, dim3((n_items + 255) / 256), dim3(256), 0, s, items, status,
                       (const CkPart *)scratch, n_items, Y, at_start);
  return hipGetLastError();
}

hipError_t launch_linsum_strip(uint32_t kind, ZgItem *items, uint32_t *status, uint32_t n_items, int at_start,
                               int verify, uint64_t len_hint, void *scratch, hipStream_t s) {
  if (!n_items) return hipSuccess;
  return kind == CK_ADLER32 ? linsum_strip<CK_ADLER32>(items, status, n_items, at_start, verify, len_hint, scratch, s)
                            : linsum_strip<CK_FLETCHER32>(items, status, n_items, at_start, verify, len_hint, scratch, s);
}

// write path: the value of chunk c's bytes dsts[c] + [lo, lo + len), 4 bytes LE after or before them
// (launch_crc32c_encode's pattern)
template <uint32_t KIND>
__global__ __launch_bounds__(CK_THREADS) void k_linsum_encode(const uint64_t *dsts, uint64_t lo, uint64_t len,
                                                              int at_start) {
  __shared__ uint32_t s_red[3 * CK_THREADS / 64];
  if (!dsts[blockIdx.x]) return;
  uint8_t *p = (uint8_t *)dsts[blockIdx.x] + lo;
  const uint32_t c = wg_checksum<KIND>(p, len, s_red);
  if (threadIdx.x == 0) {
    uint8_t *w = at_start ? p - 4 : p + len;
    for (int k = 0; k < 4; k++) w[k] = (uint8_t)(c >> (8 * k));
  }
}

hipError_t launch_linsum_encode(uint32_t kind, const uint64_t *dsts, uint32_t n, uint64_t lo, uint64_t len,
                                int at_start, hipStream_t s) {
  if (!n) return hipSuccess;
  if (kind == CK_ADLER32)
    hipLaunchKernelGGL(k_linsum_encode<CK_ADLER32>, dim3(n), dim3(CK_THREADS), 0, s, dsts, lo, len, at_start);
  else
    hipLaunchKernelGGL(k_linsum_encode<CK_FLETCHER32>, dim3(n), dim3(CK_THREADS), 0, s, dsts, lo, len, at_start);
  return hipGetLastError();
}

// write path, items: every item's value written after its bytes (or before them: src moves back 4)
template <uint32_t KIND>
__global__ __launch_bounds__(CK_THREADS) void k_linsum_items(ZgItem *items, const uint32_t *status, int at_start) {
  __shared__ uint32_t s_red[3 * CK_THREADS / 64];
  const uint32_t i = blockIdx.x;
  if (status[i]) return;
  const ZgItem it = items[i];
  uint8_t *p = (uint8_t *)it.src;
  const uint32_t c = wg_checksum<KIND>(p, it.len, s_red);
  if (threadIdx.x == 0) {
    uint8_t *w = at_start ? p - 4 : p + it.len;
    for (int k = 0; k < 4; k++) w[k] = (uint8_t)(c >> (8 * k));
    items[i].src = at_start ? it.src - 4 : it.src;
    items[i].len = it.len + 4;
  }
}

hipError_t launch_linsum_items(uint32_t kind, ZgItem *items, const uint32_t *status, uint32_t n, int at_start,
                               hipStream_t s) {
  if (!n) return hipSuccess;
  if (kind == CK_ADLER32)
    hipLaunchKernelGGL(k_linsum_items<CK_ADLER32>, dim3(n), dim3(CK_THREADS), 0, s, items, status, at_start);
  else
    hipLaunchKernelGGL(k_linsum_items<CK_FLETCHER32>, dim3(n), dim3(CK_THREADS), 0, s, items, status, at_start);
  return hipGetLastError();
}

// ------------------------------- shard index --------------------------------------------------
__global__ __launch_bounds__(CRC_THREADS) void k_shard_index(const ZgShard *shards, ZgIndexSpec spec,
                                                             uint64_t *index, uint32_t *shard_status, int keep_err) {
  __shared__ CrcTables T;
  __shared__ uint64_t s_len[CRC_THREADS / 64];
  __shared__ uint32_t s_crc[CRC_THREADS / 64];
  const uint32_t sh = blockIdx.x;
  if (keep_err && shard_status[sh]) return;
  const ZgShard S = shards[sh];
  uint64_t *dst = index + (uint64_t)sh * spec.n_inner * 2;
  if (S.ptr == 0) {  // missing shard: every inner chunk is empty (fill)
    for (uint64_t k = threadIdx.x; k < spec.n_inner * 2; k += blockDim.x) dst[k] = ~0ull;
    if (threadIdx.x == 0) shard_status[sh] = 0;
    return;
  }
  if (S.len < spec.index_bytes) {
    if (threadIdx.x == 0) shard_status[sh] = ZG_SHARD_TOO_SMALL;
    return;
  }
  const uint8_t *p = (const uint8_t *)S.ptr + (spec.at_start ? 0 : S.len - spec.index_bytes);
  uint64_t n = spec.index_bytes;
  if (spec.n_crc && spec.verify) build_tables(T, POLY_CRC32C);
  for (int k = (int)spec.n_crc - 1; k >= 0; k--) {  // b2b decode in reverse
    const uint8_t *data = spec.crc_at_start[k] ? p + 4 : p;
    const uint8_t *stored = spec.crc_at_start[k] ? p : p + n - 4;
    if (spec.verify) {
      const uint32_t c = wg_crc(data, n - 4, T, POLY_CRC32C, s_len, s_crc);
      const uint32_t sv = stored[0] | stored[1] << 8 | stored[2] << 16 | (uint32_t)stored[3] << 24;
      if (c != sv) {
        if (threadIdx.x == 0) shard_status[sh] = ZG_INVALID_CHECKSUM;
        return;
      }
    }
    p = data;
    n -= 4;
  }
  for (uint64_t k = threadIdx.x; k < spec.n_inner * 2; k += blockDim.x) {
    const uint8_t *q = p + k * 8;
    uint64_t v = 0;
    for (int b = 0; b < 8; b++) v |= (uint64_t)q[b] << (8 * (spec.big_endian ? 7 - b : b));
    dst[k] = v;
  }
  if (threadIdx.x == 0) shard_status[sh] = 0;
}

hipError_t launch_shard_index(const ZgShard *shards, uint32_t n_shards, const ZgIndexSpec &spec,
                              uint64_t *index, uint32_t *shard_status, int keep_err, hipStream_t s) {
  if (!n_shards) return hipSuccess;
  hipLaunchKernelGGL(k_shard_index, dim3(n_shards), dim3(CRC_THREADS), 0, s, shards, spec, index, shard_status,
                     keep_err);
  return hipGetLastError();
}

__global__ void k_mid_shards(const ZgItem *mids, const uint32_t *mid_status, uint32_t n, ZgShard *shards,
                             uint32_t *shard_status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ZgItem m = mids[i];
  const uint32_t st = mid_status[i];
  shard_status[i] = st;
  shards[i] = (st || (m.flags & ZG_ITEM_FILL)) ? ZgShard{0, 0} : ZgShard{m.src, m.len};
}

hipError_t launch_mid_shards(const ZgItem *mids, const uint32_t *mid_status, uint32_t n, ZgShard *shards,
                             uint32_t *shard_status, hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_mid_shards, dim3((n + 255) / 256), dim3(256), 0, s, mids, mid_status, n, shards, shard_status);
  return hipGetLastError();
}

__global__ void k_item_resolve(ZgItem *items, uint32_t *status, uint32_t n_items, const ZgShard *shards,
                               const uint64_t *index, const uint32_t *shard_status, uint64_t n_inner,
                               unsigned long long *enc_bytes) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  ZgItem it = items[i];
  if (!(it.flags & ZG_ITEM_SHARDED)) return;
  const uint32_t ss = shard_status[it.shard];
  if (ss) {
    status[i] = ss;
    return;
  }
  const ZgShard S = shards[it.shard];
  const uint64_t off = index[((uint64_t)it.shard * n_inner + it.inner) * 2];
  const uint64_t size = index[((uint64_t)it.shard * n_inner + it.inner) * 2 + 1];
  if (off == ~0ull && size == ~0ull) {
    items[i].flags = it.flags | ZG_ITEM_FILL;
    return;
  }
  if (off > S.len || size > S.len - off) {
    status[i] = ZG_SHARD_INDEX_OOB;
    return;
  }
  items[i].src = S.ptr + off;
  items[i].len = size;
  atomicAdd(enc_bytes, (unsigned long long)size);
}

hipError_t launch_item_resolve(ZgItem *items, uint32_t *status, uint32_t n_items, const ZgShard *shards,
                               const uint64_t *index, const uint32_t *shard_status, uint64_t n_inner,
                               unsigned long long *enc_bytes, hipStream_t s) {
  if (!n_items) return hipSuccess;
  hipLaunchKernelGGL(k_item_resolve, dim3((n_items + 255) / 256), dim3(256), 0, s, items, status, n_items,
                     shards, index, shard_status, n_inner, enc_bytes);
  return hipGetLastError();
}


// ------------------------------- crc32c encode (write path) -----------------------------------
// CodecChain::encode of a crc32c codec (crc32c_codec.rs:88-106): checksum of the bytes so far,
// 4 bytes LE appended (End) or prepended (Start). Chunk c's bytes are dsts[c] + [lo, lo + len).
__global__ __launch_bounds__(CRC_THREADS) void k_crc32c_encode(const uint64_t *dsts, uint64_t lo, uint64_t len,
                                                               int at_start) {
  __shared__ CrcTables T;
  __shared__ uint64_t s_len[CRC_THREADS / 64];
  __shared__ uint32_t s_crc[CRC_THREADS / 64];
  if (!dsts[blockIdx.x]) return;  // a shard whose layout failed (variable-length encode)
  uint8_t *p = (uint8_t *)dsts[blockIdx.x] + lo;
  build_tables(T, POLY_CRC32C);
  const uint32_t c = wg_crc(p, len, T, POLY_CRC32C, s_len, s_crc);
  if (threadIdx.x < 4) {
    uint8_t *w = at_start ? p - 4 : p + len;
    w[threadIdx.x] = (uint8_t)(c >> (8 * threadIdx.x));
  }
}

hipError_t launch_crc32c_encode(const uint64_t *dsts, uint32_t n, uint64_t lo, uint64_t len, int at_start,
                                hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_crc32c_encode, dim3(n), dim3(CRC_THREADS), 0, s, dsts, lo, len, at_start);
  return hipGetLastError();
}

}  // namespace zgpu
