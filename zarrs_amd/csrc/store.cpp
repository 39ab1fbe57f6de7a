// libzgpu: the store path -- Array::store_array_subset on the GPU (zgpu_store_array_subset, zgpu.h).
//
// zarrs stores a subset chunk by chunk (array_write_ops_array.rs:183-208 for a covered chunk,
// array_update_ops_array.rs:152-210 for a partly covered one: decode, paste, encode) and, in a shard,
// inner chunk by inner chunk (sharding/sharding_partial_encoder.rs). Here the unit of read-modify-write
// is the leaf chunk throughout, and one call does every chunk the subset meets:
//   1. store_classify (store_layout.cpp, no device): the chunks met, each leaf covered / partly
//      covered / untouched;
//   2. the old shard indexes (small) are decoded on the host: every entry is range-checked here, so an
//      untouched inner chunk is never copied from outside its shard;
//   3. ONE decode batch of all partly covered leaves (decode_general over the leaf chain, full decode
//      path, checksums verified) into a staging array of one leaf box per leaf, stacked along axis 0;
//   4. ONE k_subset_overlay launch pastes every overlap box from the data into its staging box;
//   5. k_fill_check of the staged and of the covered leaves (the latter straight in the data);
//   6. the leaves that are not all fill go through the write path's encoder (encode_chunks_on):
//      the staged ones with the staging array as the array, the covered ones straight from the data
//      (array_shape = sel_shape, origins relative to sel_start);
//   7. a shard is laid out by k_shard_layout_var / k_shard_copy_var over one item per inner chunk: the
//      newly encoded ones, and the untouched ones pointing into the old shard; then the index crc32c.
// Every temporary is Scratch's; the encoded chunks leave in the result (pooled pinned or device memory).
//
// The store by coordinates (zgpu_store_elements) is ArrayPartialEncoderTraits::partial_encode for a list of
// ArrayIndices: CodecPartialDefault (zarrs_codec/src/codec_partial_default.rs:324-380: decode,
// update_array_bytes, encode) with update_array_bytes_indexer (zarrs_codec/src/array_bytes.rs:685-726)
// copying the elements in indexer order, so the last of several points on one coordinate wins. It shares
// everything but steps 1 and 4 with the store of a box:
//   1'. the front of the read by coordinates (points.hpp): k_points_mark, the bitmap back, a slot per
//       touched leaf in key order; the entries are the chunks that hold a touched leaf;
//   2, 3 as above, with EVERY touched leaf treated as partly covered and staged in its slot;
//   4'. k_points_claim (per staged element the highest point index) and k_points_scatter (the winners
//       write) instead of the overlay; a u32 per staged element is the winner table;
//   5-7 as above (store_tail), nothing read straight from the data.
// All touched leaves are staged at once: no rounds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/zgpu.h"
#include "chain.hpp"
#include "common.hpp"
#include "ctx.hpp"
#include "kernels/launch.hpp"
#include "plan.hpp"
#include "points.hpp"
#include "store_layout.hpp"

using namespace zgpu;

namespace {

// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) of the few bytes of a shard index
uint32_t crc32c_host(const uint8_t *p, size_t n) {
  static const std::vector<uint32_t> T = [] {
    std::vector<uint32_t> t(256);
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1)));
      t[i] = c;
    }
    return t;
  }();
  uint32_t c = ~0u;
  for (size_t i = 0; i < n; i++) c = T[(c ^ p[i]) & 0xFF] ^ (c >> 8);
  return ~c;
}

uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// An encoded shard index (X bytes: bytes{endian} + crc32c codecs) decoded on the host into n_inner
// (offset, nbytes) pairs, every present entry checked against the shard's length.
int parse_index(const uint8_t *enc, uint64_t X, const Chain &xc, uint64_t n_inner, bool validate, uint64_t shard_len,
                uint64_t *out) {
  const uint8_t *p = enc;
  uint64_t len = X;
  for (size_t i = xc.b2b.size(); i-- > 0;) {
    if (len < 4) return ZGPU_CRC_INPUT_TOO_SHORT;
    const Codec &k = xc.b2b[i];
    const uint8_t *c = k.at_start ? p : p + len - 4, *payload = k.at_start ? p + 4 : p;
    len -= 4;
    const uint32_t stored = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)c[3] << 24;
    if (validate && crc32c_host(payload, len) != stored) return ZGPU_INVALID_CHECKSUM;
    p = payload;
  }
  if (len != n_inner * 16) return ZGPU_SHARD_TOO_SMALL;
  for (uint64_t q = 0; q < 2 * n_inner; q++) {
    uint64_t v = 0;
    for (int b = 0; b < 8; b++) v |= (uint64_t)p[q * 8 + b] << (8 * (xc.a2b.big_endian ? 7 - b : b));
    out[q] = v;
  }
  for (uint64_t k = 0; k < n_inner; k++) {
    const uint64_t off = out[2 * k], nb = out[2 * k + 1];
    if (off == ~0ull && nb == ~0ull) continue;
    if (off > shard_len || nb > shard_len - off) return ZGPU_SHARD_INDEX_OOB;
  }
  return ZGPU_OK;
}

struct Leaf {
  uint64_t entry, j;         // its chunk's entry, its index in the chunk's leaf grid
  uint64_t origin[ZG_MAXD];  // in the array
  bool partial;              // partly covered: staged (else covered: read straight from the data)
  uint64_t stage = 0;        // partial: its staging box
  const uint8_t *old = nullptr;  // partial: the old leaf's encoded bytes on the device (null: missing)
  uint64_t old_len = 0;
  uint32_t nonfill = 0;
  bool encode = false;
  uint64_t slot = 0, enc_len = 0;  // encode: its slot and encoded length
};

// What a store call is made of once its chain is accepted, and its entries.
struct StoreCall {
  zgpu_chain *ch = nullptr;
  zgpu_ctx *C = nullptr;
  const Chain *top = nullptr;
  bool sharded = false, enc_dev = false, validate = false, store_empty = false;
  uint32_t nd = 0, es = 0, flags = 0;
  EncodeLayout EL;
  const EncodeLayout *leaf_layout = nullptr;
  const uint64_t *leaf_shape = nullptr;
  std::shared_ptr<Chain> leaf_chain;
  uint64_t lpc = 1, leaf_n = 0, leaf_bytes = 0, leaf_bound = 0, pitch = 0, X = 0;
  // per entry (a chunk the store meets), C order of the chunk grid
  uint64_t nE = 0;
  std::vector<const uint8_t *> old;  // its old bytes on the device (null: missing, or not read)
  std::vector<uint64_t> old_len;
  std::unique_ptr<zgpu_result> R;
  std::vector<zgpu_store_entry> &E() { return R->store_entries; }
};

// Host tables the queued copies read: declared before the scratch, whose destructor waits for them.
struct StoreTables {
  std::vector<uint64_t> index, rows, starts, hsh, dst;
  std::vector<uint32_t> nf, prefix;
  std::vector<Leaf> leaves;
  std::vector<zgpu_chunk_desc> descs;
  std::vector<ZgOverlayBox> boxes;
  std::vector<ZgItem> items;
  std::vector<PointSlot> slots;
};

// The chain's refusals (ZGPU_UNSUPPORTED, or ChainError thrown by encode_layout: before any device work)
// and the leaf's layout.
int store_accept(zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape, uint32_t flags, StoreCall &S) {
  S.ch = ch;
  S.C = ch->ctx;
  S.top = ch->chain.get();
  const Chain &top = *S.top;
  S.sharded = top.a2b.kind == CodecKind::Sharding;
  // what the store path does not take on top of the write path's own refusals (encode_layout throws
  // them, ChainError, before any device work): read-modify-write goes one level deep, in one data type
  if (S.sharded && top.a2b.inner->a2b.kind == CodecKind::Sharding)
    return set_err(ZGPU_UNSUPPORTED, "store: nested sharding_indexed");
  if (S.sharded && chain_has_value_codec(*top.a2b.inner))
    return set_err(ZGPU_UNSUPPORTED, "store: value codecs inside sharding_indexed");
  S.EL = encode_layout(top, nd, chunk_shape);
  S.leaf_layout = S.sharded ? S.EL.inner.get() : &S.EL;
  S.leaf_shape = S.sharded ? top.a2b.inner_shape.data() : chunk_shape;
  S.nd = nd;
  S.es = top.es;
  S.flags = flags;
  S.enc_dev = flags & ZGPU_ENC_DEVICE;
  S.validate = ch->validate && !(flags & ZGPU_NO_VALIDATE);
  S.store_empty = flags & ZGPU_STORE_EMPTY_CHUNKS;
  S.lpc = 1;
  for (uint32_t d = 0; d < nd; d++) S.lpc *= chunk_shape[d] / S.leaf_shape[d];
  S.leaf_n = volume(S.leaf_shape, nd);
  S.leaf_bytes = S.leaf_n * S.es;
  S.leaf_chain = S.sharded ? top.a2b.inner : ch->chain;
  S.leaf_bound = S.leaf_layout->size;
  S.pitch = std::max<uint64_t>(256, align_up(S.leaf_bound, 256));
  S.X = S.sharded ? S.EL.index->size : 0;
  return ZGPU_OK;
}

// The call's device, its counters cleared, its result with one entry per chunk of lins.
void store_begin(StoreCall &S, const uint64_t *lins, uint64_t nE) {
  HIPCHK(hipSetDevice(S.C->device));
  uint64_t *ctr = call_counters();
  std::fill(ctr, ctr + CTR_N, 0);
  size_detail() = SizeDetail{};
  S.R.reset(new zgpu_result());
  ctx_ref(S.C);
  S.R->ctx = S.C;
  S.nE = nE;
  S.E().assign(nE, zgpu_store_entry{});
  for (uint64_t k = 0; k < nE; k++) S.E()[k].chunk = lins[k];
  S.old.assign(nE, nullptr);
  S.old_len.assign(nE, 0);
}

// The old chunks of the entries with need[k] whose key is present, on the device; the old shards' indexes
// decoded and range-checked on the host into T.index (a failure is the entry's status).
void store_old_chunks(StoreCall &S, StoreTables &T, Scratch &sc, hipStream_t s, const void *const *chunk_ptrs,
                      const uint64_t *chunk_lens, const std::vector<uint8_t> &need) {
  const uint64_t nE = S.nE, X = S.X, lpc = S.lpc;
  const Chain &top = *S.top;
  std::vector<zgpu_store_entry> &E = S.E();
  std::vector<const uint8_t *> &old = S.old;
  std::vector<uint64_t> &old_len = S.old_len;
  T.index.assign(S.sharded ? nE * lpc * 2 : 0, ~0ull);
  {
    constexpr uint64_t HR = 64;  // readable bytes either side of an old chunk (launch_unpackbits)
    uint64_t total = 0;
    std::vector<uint64_t> off(nE, 0);
    for (uint64_t k = 0; k < nE; k++) {
      const uint64_t lin = E[k].chunk;
      if (!need[k] || !chunk_ptrs[lin]) continue;
      old_len[k] = chunk_lens[lin];
      off[k] = total + HR;
      total += align_up(HR + old_len[k] + HR, 256);
    }
    uint8_t *pack = (!S.enc_dev && total) ? sc.dev<uint8_t>(total) : nullptr;
    for (uint64_t k = 0; k < nE; k++) {
      const uint64_t lin = E[k].chunk;
      if (!need[k] || !chunk_ptrs[lin]) continue;
      if (S.enc_dev) {
        old[k] = (const uint8_t *)chunk_ptrs[lin];
      } else {
        old[k] = pack + off[k];
        if (old_len[k]) HIPCHK(hipMemcpyAsync(pack + off[k], chunk_ptrs[lin], old_len[k], hipMemcpyHostToDevice, s));
      }
    }
  }

  // the old shards' indexes, decoded and range-checked on the host
  if (S.sharded) {
    const Chain &xc = *top.a2b.index;
    uint8_t *hx = nullptr;
    if (S.enc_dev) {
      hx = sc.pinned<uint8_t>(std::max<uint64_t>(nE * X, 1));
      for (uint64_t k = 0; k < nE; k++)
        if (old[k] && old_len[k] >= X)
          HIPCHK(hipMemcpyAsync(hx + k * X, old[k] + (top.a2b.at_start ? 0 : old_len[k] - X), X, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
    }
    for (uint64_t k = 0; k < nE; k++) {
      if (!old[k]) continue;
      if (old_len[k] < X) {
        E[k].status = ZGPU_SHARD_TOO_SMALL;
        continue;
      }
      const uint8_t *src = S.enc_dev ? hx + k * X
                                     : (const uint8_t *)chunk_ptrs[E[k].chunk] + (top.a2b.at_start ? 0 : old_len[k] - X);
      E[k].status = parse_index(src, X, xc, lpc, S.validate, old_len[k], T.index.data() + k * lpc * 2);
    }
  }
}

// A staged leaf's old encoded bytes: the chunk's, or the inner chunk's as the old shard's index gives them.
void leaf_old_bytes(const StoreCall &S, const StoreTables &T, Leaf &lf) {
  const uint64_t k = lf.entry, q = (k * S.lpc + lf.j) * 2;
  if (!S.sharded) {
    lf.old = S.old[k];
    lf.old_len = S.old_len[k];
  } else if (S.old[k] && T.index[q] != ~0ull) {
    lf.old = S.old[k] + T.index[q];
    lf.old_len = T.index[q + 1];
  }
}

// Step 3: one decode batch of the staged leaves (T.leaves with partial set) into the staging array; a
// failing leaf gives its entry its status. Synchronises s.
void store_decode_staged(StoreCall &S, StoreTables &T, hipStream_t s, uint8_t *staging, const uint64_t *stage_shape) {
  uint64_t *ctr = call_counters();
  std::vector<zgpu_store_entry> &E = S.E();
  std::vector<uint64_t> owner;
  for (const Leaf &lf : T.leaves) {
    if (!lf.partial) continue;
    zgpu_chunk_desc D{};
    D.enc = lf.old;
    D.enc_len = lf.old ? lf.old_len : 0;
    for (uint32_t d = 0; d < S.nd; d++) {
      D.chunk_shape[d] = D.sel_shape[d] = S.leaf_shape[d];
      D.out_start[d] = d == 0 ? lf.stage * S.leaf_shape[0] : 0;
    }
    T.descs.push_back(D);
    owner.push_back(lf.entry);
    if (lf.old) ctr[CTR_STORE_DECODED]++;
  }
  GeneralCall G{S.C, S.validate, S.nd, staging, stage_shape,
                (S.flags & ZGPU_NO_VALIDATE) | ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE, s, {}};
  std::vector<int32_t> st(T.descs.size(), 0);
  decode_general(G, S.leaf_chain, T.descs.data(), T.descs.size(), st.data());
  HIPCHK(hipStreamSynchronize(s));
  for (size_t i = 0; i < st.size(); i++)
    if (st[i] && !E[owner[i]].status) E[owner[i]].status = st[i];
}

// Where the covered leaves are read from (the store of a box): the data, the subset's box and strides.
struct StoreData {
  const uint8_t *d_data = nullptr;
  const uint64_t *sel_start = nullptr, *sel_shape = nullptr, *sel_stride = nullptr;
};

// Steps 5-7 over the leaves of the entries still in good standing: the fill check, the encode of what is
// not all fill, every entry's action, the shard layout, the copy-out; the result is handed over.
int store_tail(StoreCall &S, StoreTables &T, Scratch &sc, hipStream_t s, uint8_t *staging, const uint64_t *stage_shape,
               const uint64_t *stage_stride, const StoreData &SD, const zgpu_store_entry **entries_out, uint64_t *n_out,
               zgpu_result **result_out) {
  zgpu_ctx *C = S.C;
  const Chain &top = *S.top;
  const EncodeLayout &EL = S.EL;
  const bool sharded = S.sharded, enc_dev = S.enc_dev, store_empty = S.store_empty;
  const uint32_t nd = S.nd, es = S.es;
  const uint64_t nE = S.nE, lpc = S.lpc, leaf_n = S.leaf_n, leaf_bound = S.leaf_bound, pitch = S.pitch, X = S.X;
  const uint64_t *leaf_shape = S.leaf_shape;
  zgpu_chain leafch{C, S.leaf_chain, S.ch->validate};
  std::unique_ptr<zgpu_result> &R = S.R;
  std::vector<zgpu_store_entry> &E = S.E();
  std::vector<const uint8_t *> &old = S.old;
  std::vector<uint64_t> &index = T.index, &starts = T.starts, &hsh = T.hsh;
  std::vector<Leaf> &leaves = T.leaves;
  std::vector<ZgItem> &items = T.items;
  std::vector<uint32_t> &nf = T.nf;
  uint64_t *ctr = call_counters();

  // the leaves to go on with, staged ones first; their origins in the array each group reads
  std::vector<Leaf *> group[2];  // [0] staged (array: the staging array), [1] covered (array: the data)
  for (Leaf &lf : leaves)
    if (!E[lf.entry].status) group[lf.partial ? 0 : 1].push_back(&lf);
  const void *g_array[2] = {staging, SD.d_data};
  const uint64_t *g_shape[2] = {stage_shape, SD.sel_shape};
  auto leaf_start = [&](const Leaf &lf, uint32_t d) {
    return lf.partial ? (d == 0 ? lf.stage * leaf_shape[0] : 0) : lf.origin[d] - SD.sel_start[d];
  };

  // rule 3: which leaves equal the fill value everywhere (bytewise, k_fill_check)
  {
    const uint64_t n_all = group[0].size() + group[1].size();
    starts.resize(std::max<uint64_t>(n_all * nd, 1));
    uint64_t q = 0;
    for (int g = 0; g < 2; g++)
      for (const Leaf *lf : group[g])
        for (uint32_t d = 0; d < nd; d++) starts[q++] = leaf_start(*lf, d);
    uint64_t *d_starts = sc.dev<uint64_t>(starts.size());
    uint32_t *d_nf = sc.dev<uint32_t>(std::max<uint64_t>(n_all, 1));
    uint32_t *h_nf = sc.pinned<uint32_t>(std::max<uint64_t>(n_all, 1));
    HIPCHK(hipMemcpyAsync(d_starts, starts.data(), starts.size() * 8, hipMemcpyHostToDevice, s));
    uint64_t base = 0;
    for (int g = 0; g < 2; g++) {
      if (group[g].empty()) continue;
      ZgEncode P{};
      P.nd = nd;
      P.es = es;
      P.nelem = leaf_n;
      std::memcpy(P.fill, top.fill, sizeof(P.fill));
      for (uint32_t d = 0; d < nd; d++) {
        P.dec_shape[d] = leaf_shape[d];
        P.array_shape[d] = g_shape[g][d];
        P.array_stride[d] = g == 0 ? stage_stride[d] : SD.sel_stride[d];
      }
      HIPCHK(launch_fill_check(d_starts + base * nd, (const uint8_t *)g_array[g], P, (uint32_t)group[g].size(),
                               d_nf + base, s));
      base += group[g].size();
    }
    if (n_all) HIPCHK(hipMemcpyAsync(h_nf, d_nf, n_all * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    q = 0;
    for (int g = 0; g < 2; g++)
      for (Leaf *lf : group[g]) {
        lf->nonfill = h_nf[q++];
        lf->encode = lf->nonfill || (!sharded && store_empty);
      }
  }

  // encode: unsharded chunks straight into the output, inner chunks into slots for the shard layout
  uint64_t n_enc = 0;
  for (Leaf &lf : leaves)
    if (lf.encode) lf.slot = n_enc++;
  uint8_t *out_dev = nullptr;  // the encoded chunks on the device
  uint8_t *slots = nullptr;
  if (!sharded) {
    if (enc_dev && n_enc) out_dev = R->dev = (uint8_t *)C->dev_alloc(n_enc * pitch);
    else if (n_enc) out_dev = sc.dev<uint8_t>(n_enc * pitch);
    slots = out_dev;
  } else if (n_enc) {
    slots = sc.dev<uint8_t>(n_enc * pitch);
  }
  for (int g = 0; g < 2; g++) {
    std::vector<zgpu_encode_desc> ed;
    std::vector<Leaf *> who;
    for (Leaf *lf : group[g]) {
      if (!lf->encode) continue;
      zgpu_encode_desc D{};
      D.dst = slots + lf->slot * pitch;
      D.dst_cap = leaf_bound;
      for (uint32_t d = 0; d < nd; d++) D.chunk_start[d] = leaf_start(*lf, d);
      ed.push_back(D);
      who.push_back(lf);
    }
    if (ed.empty()) continue;
    std::vector<uint64_t> lens(ed.size(), 0);
    if (const int rc = encode_chunks_on(&leafch, nd, leaf_shape, g_array[g], g_shape[g], ed.data(), ed.size(),
                                        lens.data(), s))
      return rc;
    for (size_t i = 0; i < who.size(); i++) who[i]->enc_len = lens[i];
    ctr[CTR_STORE_ENCODED] += ed.size();
  }

  // what every entry becomes; a shard is laid out from one item per inner chunk
  std::vector<uint64_t> e_off(nE, 0);  // the entry's bytes in out_dev
  if (!sharded) {
    for (const Leaf &lf : leaves) {
      if (E[lf.entry].status) continue;
      E[lf.entry].action = lf.encode ? ZGPU_STORE_SET : ZGPU_STORE_ERASE;
      E[lf.entry].enc_len = lf.encode ? lf.enc_len : 0;
      e_off[lf.entry] = lf.slot * pitch;
    }
  } else {
    std::vector<const Leaf *> of(nE * lpc, nullptr);
    for (const Leaf &lf : leaves) of[lf.entry * lpc + lf.j] = &lf;
    std::vector<uint64_t> set;  // the entries that get a new shard
    uint64_t total = 0, cap = 0;
    for (uint64_t k = 0; k < nE; k++) {
      if (E[k].status) continue;
      uint64_t present = 0, bytes = X;
      const size_t first = items.size();
      for (uint64_t j = 0; j < lpc; j++) {
        ZgItem it{};
        uint32_t f = 0;
        if (const Leaf *lf = of[k * lpc + j]) {  // touched: newly encoded, or all fill and omitted
          if (lf->encode) {
            it.src = (uint64_t)(slots + lf->slot * pitch);
            it.len = lf->enc_len;
            f = 1;
          }
        } else if (old[k] && index[(k * lpc + j) * 2] != ~0ull) {  // untouched and present: carried over
          it.src = (uint64_t)(old[k] + index[(k * lpc + j) * 2]);
          it.len = index[(k * lpc + j) * 2 + 1];
          f = 1;
          ctr[CTR_STORE_CARRIED]++;
        }
        items.push_back(it);
        nf.push_back(f);
        present += f;
        bytes += f ? it.len : 0;
      }
      if (!present) {  // no inner chunk left: the shard is erased
        E[k].action = ZGPU_STORE_ERASE;
        items.resize(first);
        nf.resize(first);
        continue;
      }
      E[k].action = ZGPU_STORE_SET;
      E[k].enc_len = bytes;
      e_off[k] = total;
      total += align_up(bytes, 256);
      cap = std::max(cap, bytes);
      set.push_back(k);
    }
    const uint64_t nS = set.size();
    if (nS) {
      out_dev = enc_dev ? (R->dev = (uint8_t *)C->dev_alloc(total)) : sc.dev<uint8_t>(total);
      hsh.resize(nS);
      for (uint64_t i = 0; i < nS; i++) hsh[i] = (uint64_t)(out_dev + e_off[set[i]]);
      ZgItem *d_items = sc.dev<ZgItem>(items.size());
      // (A.E_pitch: the largest shard; the item and shard statuses behind the fill flags)
      const ShardTables ST = shard_tables(sc, EL, hsh.data(), nS, items.size(), nf.size() + items.size() + nS, 0, cap, s);
      uint32_t *d_ist = ST.nf + nf.size(), *d_shst = d_ist + items.size();
      HIPCHK(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(ZgItem), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(ST.nf, nf.data(), nf.size() * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemsetAsync(d_ist, 0, (items.size() + nS) * 4, s));
      HIPCHK(launch_shard_layout_var((uint32_t)items.size(), ST.nf, d_items, d_ist, ST.A, ST.dst, ST.off, ST.index_ptr, ST.len,
                                     d_shst, (uint32_t)nS, s));
      checksums_in_place(ST.index_ptr, (uint32_t)nS, *EL.index, s);
      uint64_t *h_len = sc.pinned<uint64_t>(2 * nS);
      HIPCHK(hipMemcpyAsync(h_len, ST.len, nS * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(h_len + nS, d_shst, nS * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      for (uint64_t i = 0; i < nS; i++)
        if (((const uint32_t *)(h_len + nS))[i] || h_len[i] != E[set[i]].enc_len)
          return set_err(ZGPU_HIP_ERROR, "store: the shard layout disagrees with the host's");
    }
  }

  // the encoded chunks to where the caller reads them
  if (enc_dev) {
    for (uint64_t k = 0; k < nE; k++)
      if (E[k].action == ZGPU_STORE_SET) E[k].enc = out_dev + e_off[k];
  } else {
    uint64_t total = 0;
    std::vector<uint64_t> h_off(nE, 0);
    for (uint64_t k = 0; k < nE; k++)
      if (E[k].action == ZGPU_STORE_SET) {
        h_off[k] = total;
        total += align_up(std::max<uint64_t>(E[k].enc_len, 1), 64);
      }
    R->own = (uint8_t *)C->host_alloc(std::max<uint64_t>(total, 1));
    for (uint64_t k = 0; k < nE; k++)
      if (E[k].action == ZGPU_STORE_SET) {
        if (E[k].enc_len)
          HIPCHK(hipMemcpyAsync(R->own + h_off[k], out_dev + e_off[k], E[k].enc_len, hipMemcpyDeviceToHost, s));
        E[k].enc = R->own + h_off[k];
      }
  }
  HIPCHK(hipStreamSynchronize(s));
  int rc = 0;
  for (uint64_t k = 0; k < nE && !rc; k++) rc = E[k].status;
  *entries_out = E.data();
  *n_out = nE;
  *result_out = R.release();
  if (rc) set_err(rc, std::string("store: ") + zgpu_status_name(rc));
  return rc;
}

int store_subset(zgpu_chain *ch, uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                 const void *const *chunk_ptrs, const uint64_t *chunk_lens, const uint64_t *sel_start,
                 const uint64_t *sel_shape, const void *data, uint32_t flags, const zgpu_store_entry **entries_out,
                 uint64_t *n_out, zgpu_result **result_out, void *stream) {
  StoreCall S;
  if (const int rc = store_accept(ch, nd, chunk_shape, flags, S)) return rc;
  const uint64_t *leaf_shape = S.leaf_shape;
  StoreLayout L;
  {
    std::string err;
    if (const int rc = store_classify(nd, array_shape, chunk_shape, leaf_shape, sel_start, sel_shape, L, err))
      return set_err(rc, err);
  }
  if (L.chunks.empty()) return ZGPU_OK;
  const bool data_dev = flags & ZGPU_OUT_DEVICE;
  const uint32_t es = S.es;
  if (data_dev && (uintptr_t)data % std::min<uint32_t>(es, 8))
    return set_err(ZGPU_INVALID_ARGUMENT, "store: data is not aligned to its element size");
  const uint64_t nE = L.chunks.size(), lpc = L.leaves_per_chunk;
  {
    std::vector<uint64_t> lins(nE);
    for (uint64_t k = 0; k < nE; k++) lins[k] = L.chunks[k].lin;
    store_begin(S, lins.data(), nE);
  }
  std::vector<zgpu_store_entry> &E = S.E();

  StoreTables T;
  std::vector<Leaf> &leaves = T.leaves;
  LaneScope ls(S.C);
  hipStream_t s = pick_stream(ls.L, stream);
  Scratch sc(S.C, s);

  // the data and the old chunks the subset does not cover, on the device
  const uint64_t data_bytes = volume(sel_shape, nd) * es;
  const uint8_t *d_data = (const uint8_t *)data;
  if (!data_dev) {
    uint8_t *d = sc.dev<uint8_t>(data_bytes);
    HIPCHK(hipMemcpyAsync(d, data, data_bytes, hipMemcpyHostToDevice, s));
    d_data = d;
  }
  {
    std::vector<uint8_t> need(nE);
    for (uint64_t k = 0; k < nE; k++) need[k] = !L.chunks[k].covered;
    store_old_chunks(S, T, sc, s, chunk_ptrs, chunk_lens, need);
  }

  // the leaves the subset touches
  uint64_t n_stage = 0;
  for (uint64_t k = 0; k < nE; k++) {
    if (E[k].status) continue;
    for (uint64_t j = 0; j < lpc; j++) {
      const uint8_t cls = L.leaf_class[L.chunks[k].first_leaf + j];
      if (cls == ZGPU_LEAF_UNTOUCHED) continue;
      Leaf lf{};
      lf.entry = k;
      lf.j = j;
      store_leaf_origin(L, L.chunks[k], leaf_shape, j, lf.origin);
      lf.partial = cls == ZGPU_LEAF_PARTIAL;
      if (lf.partial) {
        lf.stage = n_stage++;
        leaf_old_bytes(S, T, lf);
      }
      leaves.push_back(lf);
    }
  }

  // one decode batch of the partly covered leaves into the staging array, one overlay launch
  uint64_t stage_shape[ZG_MAXD], stage_stride[ZG_MAXD], sel_stride[ZG_MAXD];
  for (uint32_t d = 0; d < nd; d++) stage_shape[d] = leaf_shape[d];
  stage_shape[0] = std::max<uint64_t>(n_stage, 1) * leaf_shape[0];
  for (int d = (int)nd - 1; d >= 0; d--) {
    stage_stride[d] = d == (int)nd - 1 ? 1 : stage_stride[d + 1] * stage_shape[d + 1];
    sel_stride[d] = d == (int)nd - 1 ? 1 : sel_stride[d + 1] * sel_shape[d + 1];
  }
  uint8_t *staging = n_stage ? sc.dev<uint8_t>(n_stage * S.leaf_bytes) : nullptr;
  if (n_stage) {
    store_decode_staged(S, T, s, staging, stage_shape);
    // the overlap of every staged leaf of a chunk still in good standing
    std::vector<uint64_t> &rows = T.rows;
    std::vector<ZgOverlayBox> &boxes = T.boxes;
    rows.push_back(0);
    for (const Leaf &lf : leaves) {
      if (!lf.partial || E[lf.entry].status) continue;
      ZgOverlayBox B{};
      uint64_t so = 0, dof = lf.stage * leaf_shape[0] * stage_stride[0], nr = 1;
      for (uint32_t d = 0; d < nd; d++) {
        const uint64_t lo = std::max(lf.origin[d], sel_start[d]);
        const uint64_t hi = std::min(lf.origin[d] + leaf_shape[d], sel_start[d] + sel_shape[d]);
        B.ext[d] = hi - lo;
        B.src_stride[d] = sel_stride[d];
        B.dst_stride[d] = stage_stride[d];
        so += (lo - sel_start[d]) * sel_stride[d];
        dof += (lo - lf.origin[d]) * stage_stride[d];
        if (d + 1 < nd) nr *= B.ext[d];
      }
      B.src = (uint64_t)(d_data + so * es);
      B.dst = (uint64_t)(staging + dof * es);
      boxes.push_back(B);
      rows.push_back(rows.back() + nr);
    }
    if (!boxes.empty()) {
      ZgOverlayBox *d_boxes = sc.dev<ZgOverlayBox>(boxes.size());
      uint64_t *d_rows = sc.dev<uint64_t>(rows.size());
      HIPCHK(hipMemcpyAsync(d_boxes, boxes.data(), boxes.size() * sizeof(ZgOverlayBox), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(d_rows, rows.data(), rows.size() * 8, hipMemcpyHostToDevice, s));
      HIPCHK(launch_subset_overlay(d_boxes, d_rows, (uint32_t)boxes.size(), rows.back(), nd, es, s));
    }
  }
  const StoreData SD{d_data, sel_start, sel_shape, sel_stride};
  return store_tail(S, T, sc, s, staging, stage_shape, stage_stride, SD, entries_out, n_out, result_out);
}

// zgpu_store_elements: see the header of this file and zgpu.h.
int store_points(zgpu_chain *ch, uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                 const void *const *chunk_ptrs, const uint64_t *chunk_lens, const void *indices, uint64_t n,
                 const void *data, uint32_t flags, const zgpu_store_entry **entries_out, uint64_t *n_out,
                 zgpu_result **result_out, void *stream) {
  uint64_t *ctr = call_counters();
  std::fill(ctr, ctr + CTR_N, 0);  // (a refused call reports no work of an earlier one)
  StoreCall S;
  if (const int rc = store_accept(ch, nd, chunk_shape, flags, S)) return rc;
  const uint32_t es = S.es;
  if (es != 1 && es != 2 && es != 4 && es != 8 && es != 16)
    return set_err(ZGPU_UNSUPPORTED, "store_elements: element size " + std::to_string(es));
  if (n >= UINT32_MAX)
    return set_err(ZGPU_UNSUPPORTED, "store_elements: " + std::to_string(n) + " points; the winner table holds a "
                                     "point's index + 1 in 32 bits, so a call takes fewer than 2^32 - 1 points");
  const uint64_t *leaf_shape = S.leaf_shape;
  PointsFront F;
  if (const int rc = points_plan("store_elements", nd, array_shape, chunk_shape, leaf_shape, S.top->fill, indices, n, F))
    return rc;
  const bool data_dev = flags & ZGPU_OUT_DEVICE, idx_dev = flags & ZGPU_IDX_DEVICE;
  if (n && data_dev && (uintptr_t)data % std::min<uint32_t>(es, 8))
    return set_err(ZGPU_INVALID_ARGUMENT, "store_elements: data is not aligned to its element size");
  HIPCHK(hipSetDevice(S.C->device));
  size_detail() = SizeDetail{};
  if (!n) return ZGPU_OK;

  StoreTables T;
  std::vector<uint64_t> lins;
  LaneScope ls(S.C);
  hipStream_t s = pick_stream(ls.L, stream);
  Scratch sc(S.C, s);

  // 1'. the data on the device; mark, the bitmap back; a slot per touched leaf, the chunks that hold one
  const uint8_t *d_data = (const uint8_t *)data;
  if (!data_dev) {
    uint8_t *d = sc.dev<uint8_t>(n * es);
    HIPCHK(hipMemcpyAsync(d, data, n * es, hipMemcpyHostToDevice, s));
    d_data = d;
  }
  if (const int rc = points_mark(sc, s, indices, idx_dev, F)) return rc;
  points_slots(F, T.prefix, T.slots, lins);
  const uint64_t n_slots = T.slots.size(), nE = lins.size();
  store_begin(S, lins.data(), nE);
  ctr[CTR_POINT_LEAVES] = n_slots;
  std::vector<zgpu_store_entry> &E = S.E();

  // 2. only the chunks the points touch are read
  store_old_chunks(S, T, sc, s, chunk_ptrs, chunk_lens, std::vector<uint8_t>(nE, 1));

  // every touched leaf is partly covered and staged in its slot (a failed entry's slots stay unused)
  for (uint64_t i = 0; i < n_slots; i++) {
    const PointSlot &PS = T.slots[i];
    if (E[PS.chunk].status) continue;
    Leaf lf{};
    lf.entry = PS.chunk;
    lf.j = PS.j;
    uint64_t rem = PS.lin;
    for (int d = (int)nd - 1; d >= 0; d--) {
      lf.origin[d] = rem % F.G.chunk_grid[d] * chunk_shape[d] + PS.origin[d];
      rem /= F.G.chunk_grid[d];
    }
    lf.partial = true;
    lf.stage = i;
    leaf_old_bytes(S, T, lf);
    T.leaves.push_back(lf);
  }
  uint64_t stage_shape[ZG_MAXD], stage_stride[ZG_MAXD];
  for (uint32_t d = 0; d < nd; d++) stage_shape[d] = leaf_shape[d];
  stage_shape[0] = n_slots * leaf_shape[0];
  for (int d = (int)nd - 1; d >= 0; d--) stage_stride[d] = d == (int)nd - 1 ? 1 : stage_stride[d + 1] * stage_shape[d + 1];
  const uint64_t stage_bytes = n_slots * S.leaf_bytes, winner_bytes = n_slots * S.leaf_n * 4;
  uint8_t *staging = nullptr;
  uint32_t *winner = nullptr;
  try {
    staging = sc.dev<uint8_t>(stage_bytes);
    winner = sc.dev<uint32_t>(n_slots * S.leaf_n);
  } catch (const HipFail &e) {
    return set_err(ZGPU_HIP_ERROR, "store_elements: no memory for " + std::to_string(stage_bytes) +
                                       " staged bytes (all touched leaves at once: no rounds) and " +
                                       std::to_string(winner_bytes) + " bytes of winner table: " + hipGetErrorString(e.e));
  }
  HIPCHK(hipMemsetAsync(winner, 0, winner_bytes, s));

  // 3. one decode batch of the touched leaves
  if (!T.leaves.empty()) store_decode_staged(S, T, s, staging, stage_shape);

  // 4'. claim, then scatter: per slot the staged leaf, or SKIP for an entry that failed
  T.dst.assign(n_slots, ZG_POINTS_SKIP);
  for (uint64_t i = 0; i < n_slots; i++)
    if (!E[T.slots[i].chunk].status) T.dst[i] = (uint64_t)(staging + i * S.leaf_bytes);
  uint64_t *d_dst = sc.dev<uint64_t>(n_slots);
  uint32_t *d_prefix = sc.dev<uint32_t>(F.words);
  HIPCHK(hipMemcpyAsync(d_dst, T.dst.data(), n_slots * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_prefix, T.prefix.data(), F.words * 4, hipMemcpyHostToDevice, s));
  HIPCHK(launch_points_claim(F.d_idx, F.P, F.G.wide, S.leaf_n, F.d_bitmap, d_prefix, d_dst, winner, s));
  HIPCHK(launch_points_scatter(F.d_idx, F.P, F.G.wide, es, S.leaf_n, F.d_bitmap, d_prefix, d_dst, winner, d_data, s));

  return store_tail(S, T, sc, s, staging, stage_shape, stage_stride, StoreData{}, entries_out, n_out, result_out);
}

}  // namespace

extern "C" int zgpu_store_entry_copy(zgpu_chain *ch, const zgpu_store_entry *e, void *dst, void *stream) {
  ABI_GUARD_BEGIN
  if (!ch || !e || (e->enc_len && (!e->enc || !dst))) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (!e->enc_len) return ZGPU_OK;
  HIPCHK(hipSetDevice(ch->ctx->device));
  LaneScope ls(ch->ctx);
  hipStream_t s = pick_stream(ls.L, stream);
  HIPCHK(hipMemcpyAsync(dst, e->enc, e->enc_len, hipMemcpyDefault, s));
  HIPCHK(hipStreamSynchronize(s));
  return ZGPU_OK;
  ABI_GUARD_END
}

extern "C" int zgpu_store_array_subset(zgpu_chain *ch, uint32_t nd, const uint64_t *array_shape,
                                       const uint64_t *chunk_shape, const void *const *chunk_ptrs,
                                       const uint64_t *chunk_lens, const uint64_t *sel_start, const uint64_t *sel_shape,
                                       const void *data, uint32_t flags, const zgpu_store_entry **entries,
                                       uint64_t *n_entries, zgpu_result **result, void *stream) {
  ABI_GUARD_BEGIN
  if (entries) *entries = nullptr;
  if (n_entries) *n_entries = 0;
  if (result) *result = nullptr;
  if (!ch || !array_shape || !chunk_shape || !chunk_ptrs || !chunk_lens || !sel_start || !sel_shape || !entries ||
      !n_entries || !result)
    return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  if (!data && volume(sel_shape, nd)) return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  return store_subset(ch, nd, array_shape, chunk_shape, chunk_ptrs, chunk_lens, sel_start, sel_shape, data, flags,
                      entries, n_entries, result, stream);
  ABI_GUARD_END
}

extern "C" int zgpu_store_elements(zgpu_chain *ch, uint32_t nd, const uint64_t *array_shape, const uint64_t *chunk_shape,
                                   const void *const *chunk_ptrs, const uint64_t *chunk_lens, const void *indices,
                                   uint64_t n, const void *data, uint32_t flags, const zgpu_store_entry **entries,
                                   uint64_t *n_entries, zgpu_result **result, void *stream) {
  ABI_GUARD_BEGIN
  if (entries) *entries = nullptr;
  if (n_entries) *n_entries = 0;
  if (result) *result = nullptr;
  if (!ch || !array_shape || !chunk_shape || !chunk_ptrs || !chunk_lens || !entries || !n_entries || !result ||
      (n && (!indices || !data)))
    return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  return store_points(ch, nd, array_shape, chunk_shape, chunk_ptrs, chunk_lens, indices, n, data, flags, entries,
                      n_entries, result, stream);
  ABI_GUARD_END
}
