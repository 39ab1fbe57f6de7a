// libzgpu: the read by coordinates (zgpu_retrieve_elements, zgpu_cache_retrieve_elements; zgpu.h).
//
// zarrs reads a list of coordinates through Indexer for &[ArrayIndices] (zarrs_chunk_grid/src/indexer.rs:
// 285-392) and serves it, in a shard, by partial_decode_fixed_indexer (sharding/
// sharding_partial_decoder_sync.rs:492-560): every touched inner chunk decoded once, the elements picked
// out. Here the touched set is found, and the elements are picked, on the device; one path for host and
// device indices (host indices are uploaded first):
//   1. k_points_mark (kernels/points.hip): bounds check of every point, one bit per touched leaf in a
//      bitmap over the array-wide leaf grid (points_layout.hpp). The LEAF is the decode granule: the chunk,
//      or for a chain whose array->bytes codec is sharding_indexed the outermost sharding's inner chunk,
//      carried back through the transposes in front of it into the chunk's frame (value codecs in front of
//      it keep every element in its place, so the rule is the same with them); for the cache, the chunk.
//   2. the bitmap and the out-of-bounds word come back (bytes bounded by the leaf grid, never by n); the
//      host gives every set bit a slot in key order and uploads the per-word prefix counts, so that the
//      device finds a key's slot as prefix[word] + popcount(bits below);
//   3. the touched leaves whose chunk key is present are decoded: ONE decode_general call per round over
//      one descriptor per leaf (selection = the leaf's box, so an unsharded chunk takes the full decode
//      path and an inner chunk the partial-decoder path), into a staging array of leaf boxes stacked along
//      axis 0, as store.cpp's step 3; ZGPU_POINTS_SCRATCH_MB bounds the staging, more leaves take more
//      rounds. The cache decodes its misses into their slots instead and stages nothing;
//   4. k_points_gather per round: key -> slot -> source address (a staged leaf, a cache slot, "fill value"
//      or "not in this round"), one thread per point.
// Every temporary is the call's Scratch's. Steps 1 and 2 (points_plan, points_mark, points_slots; points.hpp)
// are also the front of the store by coordinates (zgpu_store_elements, store.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zgpu.h"
#include "chain.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "kernels/launch.hpp"
#include "plan.hpp"
#include "points.hpp"
#include "points_layout.hpp"

using namespace zgpu;

namespace {

// Bytes of decoded leaves staged at once (ZGPU_POINTS_SCRATCH_MB, read per call). The default is a policy
// choice, not a measurement: large enough that an ordinary sampler's read is one round, small next to HBM.
uint64_t staging_budget() {
  uint64_t mb = 1024;
  if (const char *e = std::getenv("ZGPU_POINTS_SCRATCH_MB"))
    if (*e) mb = std::strtoull(e, nullptr, 10);
  return mb << 20;
}

constexpr int POINTS_DIRECT = -1;  // points_call with a cache: the read does not fit it, take the direct path

using Slot = PointSlot;

int points_call(zgpu_cache *K, zgpu_chain *ch, uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                const void *const *chunk_ptrs, const uint64_t *chunk_lens, const void *indices, uint64_t n, void *out,
                uint32_t flags, void *stream) {
  zgpu_ctx *C = ch->ctx;
  const Chain &top = *ch->chain;
  const uint32_t es = top.es;
  if (es != 1 && es != 2 && es != 4 && es != 8 && es != 16)
    return set_err(ZGPU_UNSUPPORTED, "retrieve_elements: element size " + std::to_string(es));
  // the decode granule
  uint64_t leaf_shape[ZG_MAXD];
  std::copy_n(chunk_shape, nd, leaf_shape);
  if (!K && top.a2b.kind == CodecKind::Sharding) {
    if (top.a2b.inner_shape.size() != nd) return set_err(ZGPU_INVALID_ARGUMENT, "sharding chunk_shape rank");
    for (const Codec &k : top.a2a)
      if (k.kind == CodecKind::Transpose && k.order.size() != nd)
        return set_err(ZGPU_INVALID_ARGUMENT, "transpose order rank != array rank");
    uint32_t m[ZG_MAXD];
    composed_axes(top, nd, m);  // encoded axis a <-> decoded axis m[a]
    for (uint32_t a = 0; a < nd; a++) leaf_shape[m[a]] = top.a2b.inner_shape[a];
  }
  PointsFront F;
  if (const int rc = points_plan("retrieve_elements", nd, array_shape, chunk_shape, leaf_shape, top.fill, indices, n, F))
    return rc;
  const PointsGeom &G = F.G;
  const ZgPoints &P = F.P;
  const uint64_t words = F.words;
  const bool enc_dev = flags & ZGPU_ENC_DEVICE, out_dev = flags & ZGPU_OUT_DEVICE, idx_dev = flags & ZGPU_IDX_DEVICE;
  const bool validate = ch->validate && !(flags & ZGPU_NO_VALIDATE);
  if (n && out_dev && (uintptr_t)out % std::min<uint32_t>(es, 8))
    return set_err(ZGPU_INVALID_ARGUMENT, "retrieve_elements: out is not aligned to its element size");

  HIPCHK(hipSetDevice(C->device));
  uint64_t *ctr = call_counters();
  std::fill(ctr, ctr + CTR_N, 0);
  size_detail() = SizeDetail{};
  if (!n) return ZGPU_OK;

  // host tables the queued copies read: declared before the scratch, whose destructor waits for them
  std::vector<uint64_t> src_tab;
  std::vector<uint32_t> prefix;
  std::vector<zgpu_chunk_desc> descs;
  std::vector<Slot> slots;
  LaneScope ls(C);
  hipStream_t s = pick_stream(ls.L, stream);
  Scratch sc(C, s);

  // 1. mark; 2. a slot per touched leaf, in key order; the read's distinct chunks
  if (const int rc = points_mark(sc, s, indices, idx_dev, F)) return rc;
  const uint64_t *d_idx = F.d_idx;
  const uint32_t *d_bitmap = F.d_bitmap;
  std::vector<uint64_t> lins;
  points_slots(F, prefix, slots, lins);
  const uint64_t n_slots = slots.size();

  CachePoints CP;
  if (K) {
    if (const int rc = cache_points_begin(K, ch, nd, chunk_shape, lins, chunk_ptrs, CP)) return rc;
    if (CP.direct) return POINTS_DIRECT;
  }

  // the encoded chunks to decode from, on the device
  std::vector<const uint8_t *> enc(lins.size(), nullptr);
  {
    std::vector<size_t> want;
    if (K) want = CP.need;
    else
      for (size_t k = 0; k < lins.size(); k++)
        if (chunk_ptrs[lins[k]]) want.push_back(k);
    constexpr uint64_t HR = 64;  // readable bytes either side of a chunk (launch_unpackbits)
    uint64_t total = 0;
    std::vector<uint64_t> off(lins.size(), 0);
    if (!enc_dev)
      for (size_t k : want) {
        off[k] = total + HR;
        total += (HR + chunk_lens[lins[k]] + HR + 255) / 256 * 256;
      }
    uint8_t *pack = total ? sc.dev<uint8_t>(total) : nullptr;
    for (size_t k : want) {
      if (enc_dev) {
        enc[k] = (const uint8_t *)chunk_ptrs[lins[k]];
        continue;
      }
      enc[k] = pack + off[k];
      if (chunk_lens[lins[k]])
        HIPCHK(hipMemcpyAsync(pack + off[k], chunk_ptrs[lins[k]], chunk_lens[lins[k]], hipMemcpyHostToDevice, s));
    }
  }

  uint64_t *d_src = sc.dev<uint64_t>(n_slots);
  uint32_t *d_prefix = sc.dev<uint32_t>(words);
  HIPCHK(hipMemcpyAsync(d_prefix, prefix.data(), words * 4, hipMemcpyHostToDevice, s));
  uint8_t *d_out = out_dev ? (uint8_t *)out : sc.dev<uint8_t>(n * es);
  std::vector<int32_t> slot_status(n_slots, 0);
  uint64_t rounds = 0;
  auto whole_desc = [&](zgpu_chunk_desc &D, size_t k) {
    D.enc = enc[k];
    D.enc_len = chunk_lens[lins[k]];
    for (uint32_t d = 0; d < nd; d++) D.chunk_shape[d] = D.sel_shape[d] = chunk_shape[d];
  };
  auto gather = [&]() {
    HIPCHK(hipMemcpyAsync(d_src, src_tab.data(), n_slots * 8, hipMemcpyHostToDevice, s));
    HIPCHK(launch_points_gather(d_idx, P, G.wide, es, d_bitmap, d_prefix, d_src, d_out, s));
    HIPCHK(hipStreamSynchronize(s));  // (src_tab is rewritten by the next round)
    rounds++;
  };

  if (K) {
    // 3. the misses, whole chunks, into their slots in one batch: the pool is an array [n_slots * c0, c1, ...].
    // Entries hold verified chunks: a caller's ZGPU_NO_VALIDATE does not reach the miss decode.
    if (!CP.need.empty()) {
      std::vector<uint64_t> pshape(chunk_shape, chunk_shape + nd);
      pshape[0] *= CP.n_slots;
      for (size_t q = 0; q < CP.need.size(); q++) {
        zgpu_chunk_desc D{};
        whole_desc(D, CP.need[q]);
        D.out_start[0] = (uint64_t)CP.need_slot[q] * chunk_shape[0];
        descs.push_back(D);
      }
      std::vector<int32_t> st(descs.size(), 0);
      // (an exception up to here or in the decode: ~CachePoints gives the slots back)
      GeneralCall GC{C, ch->validate, nd, CP.pool, pshape.data(), ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE, s, {}};
      decode_general(GC, ch->chain, descs.data(), descs.size(), st.data());
      HIPCHK(hipStreamSynchronize(s));
      cache_points_commit(K, CP, lins, st.data());
      std::vector<int32_t> chunk_status(lins.size(), 0);
      for (size_t q = 0; q < CP.need.size(); q++) chunk_status[CP.need[q]] = st[q];
      for (uint64_t i = 0; i < n_slots; i++) slot_status[i] = chunk_status[slots[i].chunk];
    }
    // 4. the slot table points straight at the pool
    std::vector<int64_t> cslot;
    cache_points_slots(K, lins, cslot);
    src_tab.assign(n_slots, ZG_POINTS_SKIP);
    for (uint64_t i = 0; i < n_slots; i++) {
      const int64_t c = cslot[slots[i].chunk];
      if (c >= 0) src_tab[i] = (uint64_t)(CP.pool + (uint64_t)c * CP.slot_bytes);
      else if (c == -1) src_tab[i] = ZG_POINTS_FILL;
    }
    gather();
  } else {
    const uint64_t leaf_bytes = volume(leaf_shape, nd) * es;
    std::vector<uint64_t> dec;  // the slots to decode; the others read as the fill value
    for (uint64_t i = 0; i < n_slots; i++)
      if (chunk_ptrs[slots[i].lin]) dec.push_back(i);
    const uint64_t per_round = std::max<uint64_t>(1, staging_budget() / std::max<uint64_t>(leaf_bytes, 1));
    const uint64_t n_stage = std::min<uint64_t>(dec.size(), per_round);
    uint8_t *staging = n_stage ? sc.dev<uint8_t>(std::max<uint64_t>(n_stage * leaf_bytes, 1)) : nullptr;
    for (uint64_t lo = 0; lo == 0 || lo < dec.size(); lo += per_round) {
      const uint64_t m = std::min<uint64_t>(dec.size() - std::min<uint64_t>(lo, dec.size()), per_round);
      src_tab.assign(n_slots, ZG_POINTS_SKIP);
      if (lo == 0)
        for (uint64_t i = 0; i < n_slots; i++)
          if (!chunk_ptrs[slots[i].lin]) src_tab[i] = ZG_POINTS_FILL;
      descs.clear();
      for (uint64_t q = 0; q < m; q++) {
        const Slot &S = slots[dec[lo + q]];
        zgpu_chunk_desc D{};
        whole_desc(D, S.chunk);
        for (uint32_t d = 0; d < nd; d++) {
          D.sel_start[d] = S.origin[d];
          D.sel_shape[d] = leaf_shape[d];
        }
        D.out_start[0] = q * leaf_shape[0];
        descs.push_back(D);
        src_tab[dec[lo + q]] = (uint64_t)(staging + q * leaf_bytes);
      }
      if (m) {
        uint64_t stage_shape[ZG_MAXD];
        std::copy_n(leaf_shape, nd, stage_shape);
        stage_shape[0] *= m;
        std::vector<int32_t> st(m, 0);
        GeneralCall GC{C, validate, nd, staging, stage_shape, (flags & ZGPU_NO_VALIDATE) | ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE,
                       s, {}};
        decode_general(GC, ch->chain, descs.data(), m, st.data());
        HIPCHK(hipStreamSynchronize(s));
        for (uint64_t q = 0; q < m; q++) slot_status[dec[lo + q]] = st[q];
      }
      gather();
    }
  }
  if (!out_dev) {
    HIPCHK(hipMemcpyAsync(out, d_out, n * es, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  ctr[CTR_POINT_LEAVES] = n_slots;
  ctr[CTR_POINT_ROUNDS] = rounds;
  // the first failing leaf in ascending (chunk, leaf) order
  int rc = 0;
  uint64_t best[2] = {UINT64_MAX, UINT64_MAX};
  for (uint64_t i = 0; i < n_slots; i++)
    if (slot_status[i] && (slots[i].lin < best[0] || (slots[i].lin == best[0] && slots[i].j < best[1]))) {
      best[0] = slots[i].lin;
      best[1] = slots[i].j;
      rc = slot_status[i];
    }
  if (rc)
    set_err(rc, std::string("retrieve_elements: ") + zgpu_status_name(rc) + " in leaf " + std::to_string(best[1]) +
                    " of chunk " + std::to_string(best[0]));
  return rc;
}

int check_args(zgpu_chain *ch, uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
               const void *const *chunk_ptrs, const uint64_t *chunk_lens, const void *indices, uint64_t n, void *out) {
  if (!ch || !array_shape || !chunk_shape || !chunk_ptrs || !chunk_lens || (n && (!indices || !out)))
    return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  return ZGPU_OK;
}

}  // namespace

int zgpu::points_plan(const char *what, uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                      const uint64_t *leaf_shape, const uint8_t *fill, const void *indices, uint64_t n, PointsFront &F) {
  PointsGeom &G = F.G;
  {
    std::string err;
    if (const int rc = points_geom(nd, array_shape, chunk_shape, leaf_shape, G, err)) return set_err(rc, err);
  }
  F.words = G.n_keys / 32 + (G.n_keys % 32 ? 1 : 0);
  if (F.words > ZGPU_POINTS_BITMAP_MAX_BYTES / 4)
    return set_err(ZGPU_UNSUPPORTED, std::string(what) + ": the array has " + std::to_string(G.n_keys) +
                                         " leaves; the dense bitmap over them is limited to " +
                                         std::to_string(ZGPU_POINTS_BITMAP_MAX_BYTES) + " bytes");
  if (n > (1ull << 56) / nd) return set_err(ZGPU_INVALID_ARGUMENT, std::string(what) + ": too many points");
  if (n && (uintptr_t)indices % 8)
    return set_err(ZGPU_INVALID_ARGUMENT, std::string(what) + ": indices are not 8-byte aligned");
  ZgPoints &P = F.P;
  P.n = n;
  P.nd = nd;
  std::memcpy(P.fill, fill, sizeof(P.fill));
  for (int d = (int)nd - 1; d >= 0; d--) {
    P.array_shape[d] = array_shape[d];
    P.leaf_shape[d] = leaf_shape[d];
    P.key_stride[d] = d == (int)nd - 1 ? 1 : P.key_stride[d + 1] * G.leaf_grid[d + 1];
    P.leaf_stride[d] = d == (int)nd - 1 ? 1 : P.leaf_stride[d + 1] * leaf_shape[d + 1];
  }
  return ZGPU_OK;
}

int zgpu::points_mark(Scratch &sc, hipStream_t s, const void *indices, bool idx_dev, PointsFront &F) {
  const uint64_t n = F.P.n, words = F.words;
  const uint32_t nd = F.P.nd;
  F.d_idx = (const uint64_t *)indices;
  if (!idx_dev) {
    uint64_t *d = sc.dev<uint64_t>(n * nd);
    HIPCHK(hipMemcpyAsync(d, indices, n * nd * 8, hipMemcpyHostToDevice, s));
    F.d_idx = d;
  }
  // [out-of-bounds word | bitmap], cleared and read back together
  const uint64_t mark_words = 1 + (words + 1) / 2;
  uint64_t *d_mark = sc.dev<uint64_t>(mark_words), *h_mark = sc.pinned<uint64_t>(mark_words);
  F.d_bitmap = (uint32_t *)(d_mark + 1);
  HIPCHK(hipMemsetAsync(d_mark, 0xff, 8, s));
  HIPCHK(hipMemsetAsync(F.d_bitmap, 0, (mark_words - 1) * 8, s));
  HIPCHK(launch_points_mark(F.d_idx, F.P, F.G.wide, F.d_bitmap, d_mark, s));
  HIPCHK(hipMemcpyAsync(h_mark, d_mark, mark_words * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  F.bitmap = (const uint32_t *)(h_mark + 1);
  if (h_mark[0] != UINT64_MAX) {  // IndexerError::OutOfBounds: nothing was decoded, nothing written
    const uint64_t i = h_mark[0];
    uint64_t p[ZG_MAXD] = {};
    if (i < n) {
      if (idx_dev) {
        HIPCHK(hipMemcpyAsync(p, F.d_idx + i * nd, nd * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
      } else {
        std::memcpy(p, (const uint64_t *)indices + i * nd, nd * 8);
      }
    }
    for (uint32_t d = 0; d < nd; d++)
      if (p[d] >= F.P.array_shape[d])
        return set_err(ZGPU_INVALID_ARGUMENT, points_oob_message(i, d, p[d], F.P.array_shape[d]));
    return set_err(ZGPU_INVALID_ARGUMENT, "point " + std::to_string(i) + " is out of bounds");
  }
  return ZGPU_OK;
}

void zgpu::points_slots(const PointsFront &F, std::vector<uint32_t> &prefix, std::vector<PointSlot> &slots,
                        std::vector<uint64_t> &lins) {
  prefix.assign(F.words, 0);
  for (uint64_t w = 0; w < F.words; w++) {
    prefix[w] = (uint32_t)slots.size();
    for (uint32_t v = F.bitmap[w]; v; v &= v - 1) {
      PointSlot S{};
      points_key_chunk(F.G, w * 32 + (uint64_t)__builtin_ctz(v), &S.lin, S.origin, &S.j);
      slots.push_back(S);
      if (lins.empty() || lins.back() != S.lin) lins.push_back(S.lin);
    }
  }
  std::sort(lins.begin(), lins.end());
  lins.erase(std::unique(lins.begin(), lins.end()), lins.end());
  for (PointSlot &S : slots) S.chunk = (size_t)(std::lower_bound(lins.begin(), lins.end(), S.lin) - lins.begin());
}

extern "C" int zgpu_retrieve_elements(zgpu_chain *ch, uint32_t nd, const uint64_t *array_shape,
                                      const uint64_t *chunk_shape, const void *const *chunk_ptrs,
                                      const uint64_t *chunk_lens, const void *indices, uint64_t n, void *out,
                                      uint32_t flags, void *stream) {
  ABI_GUARD_BEGIN
  if (const int rc = check_args(ch, nd, array_shape, chunk_shape, chunk_ptrs, chunk_lens, indices, n, out)) return rc;
  return points_call(nullptr, ch, nd, array_shape, chunk_shape, chunk_ptrs, chunk_lens, indices, n, out, flags, stream);
  ABI_GUARD_END
}

extern "C" int zgpu_cache_retrieve_elements(zgpu_cache *K, zgpu_chain *ch, uint32_t nd, const uint64_t *array_shape,
                                            const uint64_t *chunk_shape, const void *const *chunk_ptrs,
                                            const uint64_t *chunk_lens, const void *indices, uint64_t n, void *out,
                                            uint32_t flags, void *stream) {
  ABI_GUARD_BEGIN
  if (!K) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (const int rc = check_args(ch, nd, array_shape, chunk_shape, chunk_ptrs, chunk_lens, indices, n, out)) return rc;
  if (ch->ctx != cache_ctx(K)) return set_err(ZGPU_INVALID_ARGUMENT, "zgpu_cache: chain of another context");
  const int rc = points_call(K, ch, nd, array_shape, chunk_shape, chunk_ptrs, chunk_lens, indices, n, out, flags, stream);
  if (rc != POINTS_DIRECT) return rc;
  // the read touches more chunks than the cache holds: decoded directly, nothing new cached
  return points_call(nullptr, ch, nd, array_shape, chunk_shape, chunk_ptrs, chunk_lens, indices, n, out, flags, stream);
  ABI_GUARD_END
}
