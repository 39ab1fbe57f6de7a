// libzgpu: the composed ("general") decode -- the chains and batches one fused plan does not take,
// decoded through several of them (plan.hpp).
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
#include "xfer.hpp"

using namespace zgpu;

// ------------------------------------------------------------------------------------------------
// General decode: the chains and batches one fused plan does not take, composed from fused plans
// (CodecChain composes any chain, codec_chain.rs:192-229, and zarrs decodes every chunk through its
// own chain and shape):
//  * descriptors of more than one chunk (shard) shape: one plan per shape, on one stream;
//  * bytes->bytes codecs after sharding_indexed (a checksum or compressor over the whole shard): the
//    shards go through those codecs first, stage by stage (the leaf-chunk kernels; slots sized from
//    the streams' own size fields), then decode as plain shards;
//  * sharding nested more than two deep, or codecs around a nested sharding_indexed: the outer shard
//    indexes are decoded on the device and read back, and the intersecting middle shards become the
//    descriptors of the inner chain (recursively, sharding.rs:107-126).
// Synchronous (per-stage read-backs); per-descriptor statuses, first failing item of a descriptor.
// ------------------------------------------------------------------------------------------------
bool fused_plannable(const Chain &top) {
  if (chain_has_value_codec(top) || top.a2b.kind == CodecKind::PackBits) return false;
  if (top.a2b.kind != CodecKind::Sharding) return true;
  if (!top.b2b.empty()) return false;
  const Chain &mid = *top.a2b.inner;
  if (mid.a2b.kind != CodecKind::Sharding) return true;
  return mid.a2a.empty() && mid.b2b.empty() && mid.a2b.inner->a2b.kind != CodecKind::Sharding;
}

static bool same_shape(const zgpu_chunk_desc &a, const zgpu_chunk_desc &b, uint32_t nd) {
  for (uint32_t d = 0; d < nd; d++)
    if (a.chunk_shape[d] != b.chunk_shape[d]) return false;
  return true;
}

bool uniform_shapes(const zgpu_chunk_desc *descs, uint64_t n, uint32_t nd) {
  for (uint64_t i = 1; i < n; i++)
    if (!same_shape(descs[0], descs[i], nd)) return false;
  return true;
}

bool desc_geometry_ok(const zgpu_chunk_desc &D, uint32_t nd, const uint64_t *out_shape) {
  for (uint32_t d = 0; d < nd; d++)
    if (D.sel_start[d] + D.sel_shape[d] > D.chunk_shape[d] || D.out_start[d] + D.sel_shape[d] > out_shape[d])
      return false;
  return true;
}

uint64_t sel_volume(const zgpu_chunk_desc &D, uint32_t nd) {
  uint64_t v = 1;
  for (uint32_t d = 0; d < nd; d++) v *= D.sel_shape[d];
  return v;
}

static bool sel_full(const zgpu_chunk_desc &D, uint32_t nd) {
  for (uint32_t d = 0; d < nd; d++)
    if (D.sel_start[d] != 0 || D.sel_shape[d] != D.chunk_shape[d]) return false;
  return true;
}

// The box [org, org + shape) of a device array (C order, array_shape) into dst + dst_off, compact
// (k_box_copy: one wave per contiguous run).
static void pack_box(const uint8_t *src, uint32_t nd, const uint64_t *array_shape, const uint64_t *org,
                     const uint64_t *shape, uint32_t es, uint8_t *dst, uint64_t dst_off, hipStream_t s) {
  const BoxRuns R = box_runs(nd, array_shape, org, shape, es);
  ZgBoxCopy P{};
  P.outer = R.outer;
  uint64_t cs = R.run_bytes;  // compact strides of the outer axes
  for (int d = (int)R.outer - 1; d >= 0; d--) {
    P.shape[d] = R.shape[d];
    P.src_stride[d] = R.stride[d];
    P.dst_stride[d] = cs;
    cs *= R.shape[d];
  }
  P.src_base = R.base;
  P.dst_base = dst_off;
  P.run_bytes = R.run_bytes;
  P.n_runs = R.n_runs;
  HIPCHK(launch_box_copy(src, dst, P, s));
}

// Decode `sub` (sub-descriptor k belongs to caller descriptor owner[k]) and merge: a caller
// descriptor keeps its first error.
static void run_sub(GeneralCall &G, const std::shared_ptr<Chain> &chain, const std::vector<zgpu_chunk_desc> &sub,
                    const std::vector<uint64_t> &owner, int32_t *status) {
  if (sub.empty()) return;
  std::vector<int32_t> st(sub.size(), 0);
  const bool had_detail = size_detail().valid;
  decode_general(G, chain, sub.data(), sub.size(), st.data());
  if (!had_detail && size_detail().valid) size_detail().desc = owner[size_detail().desc];
  for (size_t k = 0; k < sub.size(); k++)
    if (st[k] && !status[owner[k]]) status[owner[k]] = st[k];
}

// One bytes->bytes codec applied to whole shards (items[i] = shard i's current bytes; ist[i] its
// status): decoded by a stages-only plan whose slots hold the decoded shards. Compressors size the
// slots from the streams (kernels/probe.hip); a gzip member longer than its ISIZE hint is re-run
// with larger slots up to DEFLATE's 1032:1 bound, and so is a zlib stream, which carries no size:
// its slots start at four times the encoded shard. A bz2 stream carries no size either and has no
// useful ratio bound (50 bytes decode to 45,899,000 zeros), so only the slot limit ends its regrowing.
static void shard_stage(GeneralCall &G, const Codec &k, std::vector<ZgItem> &items, std::vector<int32_t> &ist) {
  std::vector<uint32_t> todo;
  for (uint32_t i = 0; i < items.size(); i++)
    if (!ist[i]) todo.push_back(i);
  if (todo.empty()) return;
  const std::optional<Stage> known = stage_for(k);
  if (!known) throw ChainError{ZGPU_UNSUPPORTED, "codec '" + k.name + "' after sharding_indexed"};
  const Stage st = *known;
  // the streams that carry their decoded size (a zlib or bz2 stream has none: the regrow loop below finds it)
  const uint32_t hint_kind = st.kind == ST_GZIP ? SIZE_HINT_GZIP : st.kind == ST_ZSTD ? SIZE_HINT_ZSTD
                             : st.kind == ST_BLOSC ? SIZE_HINT_BLOSC : UINT32_MAX;
  uint64_t cap = 0;
  if (st.kind == ST_UNSHUFFLE) {
    for (uint32_t t : todo) cap = std::max(cap, items[t].len);
  } else if (st.kind == ST_ZLIB || st.kind == ST_BZ2) {
    for (uint32_t t : todo) cap = std::max(cap, items[t].len * 4);  // a first guess; regrown 8x on a mismatch
  } else if (hint_kind != UINT32_MAX) {
    const uint32_t nt = (uint32_t)todo.size();
    std::vector<ZgItem> hi(nt);
    for (uint32_t j = 0; j < nt; j++) hi[j] = items[todo[j]];
    Scratch sc(G.C, G.s);
    ZgItem *d_it = sc.dev<ZgItem>(nt);
    uint8_t *d_buf = sc.dev<uint8_t>(nt * 12);
    std::vector<uint64_t> h(nt, 0);
    HIPCHK(hipMemcpyAsync(d_it, hi.data(), nt * sizeof(ZgItem), hipMemcpyHostToDevice, G.s));
    HIPCHK(hipMemsetAsync(d_buf + nt * 8, 0, nt * 4, G.s));
    HIPCHK(launch_size_hint(d_it, (const uint32_t *)(d_buf + nt * 8), nt, hint_kind, (uint64_t *)d_buf, G.s));
    HIPCHK(hipMemcpyAsync(h.data(), d_buf, nt * 8, hipMemcpyDeviceToHost, G.s));
    HIPCHK(hipStreamSynchronize(G.s));
    for (uint64_t v : h) cap = std::max(cap, v);
  }
  cap = std::max<uint64_t>(cap, 256);
  // one stages-only plan over `set` with slots of `c` bytes; statuses in s, decoded items in res
  auto run = [&](const std::vector<uint32_t> &set, uint64_t c, std::vector<int32_t> &s, std::vector<ZgItem> &res) {
    std::vector<ZgItem> sub;
    for (uint32_t t : set) sub.push_back(items[t]);
    auto P = std::make_unique<zgpu_plan>(G.C, stages_only_layout(std::move(sub), st, c));
    P->validate = G.validate;
    P->nd = 1;
    P->n_desc = set.size();
    P->flags = G.flags;
    P->out_shape = {1};
    plan_upload(*P, G.s);
    plan_enqueue(*P, nullptr, G.s);
    s.assign(set.size(), 0);
    const SizeDetail keep_detail = size_detail();
    plan_statuses(*P, s.data(), G.s);
    size_detail() = keep_detail;  // a shard has no expected decoded size
    res.resize(set.size());
    HIPCHK(hipMemcpyAsync(res.data(), P->d_items, set.size() * sizeof(ZgItem), hipMemcpyDeviceToHost, G.s));
    HIPCHK(hipStreamSynchronize(G.s));
    if (std::find(s.begin(), s.end(), 0) != s.end()) G.keep.push_back(std::move(P));  // slots in use
  };
  // gzip's ISIZE is the decoded size modulo 2^32 (RFC 1952), only a hint: a member that outgrows its
  // slot is re-run ALONE with 8x larger slots, up to DEFLATE's 1032:1 bound and the slot limit
  // (ZGPU_SHARD_SLOT_LIMIT, default 64 GiB); past the limit it fails by itself with
  // DECODED_SIZE_MISMATCH instead of sizing every retried shard's slot for the largest
  static const uint64_t slot_limit = [] {
    const char *e = std::getenv("ZGPU_SHARD_SLOT_LIMIT");
    const uint64_t v = e ? std::strtoull(e, nullptr, 10) : 0;
    return v ? v : (64ull << 30);
  }();
  std::vector<int32_t> s;
  std::vector<ZgItem> res;
  run(todo, std::min(cap, slot_limit), s, res);
  auto settle = [&](uint32_t t, int32_t sj, const ZgItem &r) {
    ist[t] = sj;
    if (!sj) {
      items[t].src = r.src;
      items[t].len = r.len;
    }
  };
  std::vector<uint32_t> again;
  auto bound_of = [&](uint32_t t) {
    return st.kind == ST_BZ2 ? slot_limit : std::min(items[t].len * 1032 + 1024, slot_limit);
  };
  for (size_t j = 0; j < todo.size(); j++) {
    const uint32_t t = todo[j];
    const uint64_t bound = bound_of(t);
    if (s[j] == ZGPU_DECODED_SIZE_MISMATCH && (st.kind == ST_GZIP || st.kind == ST_ZLIB || st.kind == ST_BZ2) &&
        cap < bound)
      again.push_back(t);
    else
      settle(t, s[j], res[j]);
  }
  for (uint32_t t : again) {
    const uint64_t bound = bound_of(t);
    for (uint64_t c = std::min(cap * 8, bound);; c = std::min(c * 8, bound)) {
      run({t}, c, s, res);
      if (!(s[0] == ZGPU_DECODED_SIZE_MISMATCH && c < bound)) {
        settle(t, s[0], res[0]);
        break;
      }
    }
  }
}

// bytes->bytes codecs after sharding_indexed: decode every selected shard through them (reverse
// order, codec_chain.rs:612-617), then read the decoded shards through the chain without them.
static void predecode_shards(GeneralCall &G, const std::shared_ptr<Chain> &chain, const zgpu_chunk_desc *descs,
                             uint64_t n, int32_t *status) {
  const Chain &top = *chain;
  const uint32_t nd = G.nd;
  std::vector<ZgItem> items;
  std::vector<uint64_t> owner;
  for (uint64_t i = 0; i < n; i++) {
    const zgpu_chunk_desc &D = descs[i];
    if (!desc_geometry_ok(D, nd, G.out_shape)) {
      status[i] = ZGPU_INVALID_ARGUMENT;
      continue;
    }
    if (!D.enc || sel_volume(D, nd) == 0) continue;
    ZgItem it{};
    it.src = (uint64_t)D.enc;
    it.len = D.enc_len;
    it.desc = (uint32_t)items.size();
    it.flags = sel_full(D, nd) ? 0u : ZG_ITEM_PARTIAL;  // a partial read strips crc32c unverified
    items.push_back(it);
    owner.push_back(i);
  }
  std::vector<int32_t> ist(items.size(), 0);
  for (int k = (int)top.b2b.size() - 1; k >= 0; k--) shard_stage(G, top.b2b[k], items, ist);
  auto bare = std::make_shared<Chain>(top);
  bare->b2b.clear();
  std::vector<zgpu_chunk_desc> sub;
  std::vector<uint64_t> sub_owner;
  size_t j = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (status[i]) continue;
    zgpu_chunk_desc D = descs[i];
    if (j < owner.size() && owner[j] == i) {
      const size_t t = j++;
      if (ist[t]) {
        status[i] = ist[t];
        continue;
      }
      D.enc = (const void *)items[t].src;
      D.enc_len = items[t].len;
    }
    sub.push_back(D);
    sub_owner.push_back(i);
  }
  run_sub(G, bare, sub, sub_owner, status);
}

// A sharded chain whose subchunks are shards the fused plan cannot take (codecs around them, or
// sharding below them again): the outer indexes decode on the device (k_shard_index, checksums
// verified) and come back to the host, and every intersecting middle shard becomes a descriptor of
// the inner chain (sharding_codec.rs:617-707 per subchunk; an empty one decodes to the fill value).
static void nested_host(GeneralCall &G, const std::shared_ptr<Chain> &chain, const zgpu_chunk_desc *descs,
                        uint64_t n, int32_t *status) {
  const Chain &top = *chain;
  const uint32_t nd = G.nd;
  const std::vector<uint64_t> &ms = top.a2b.inner_shape;
  if (ms.size() != nd) throw ChainError{ZGPU_INVALID_ARGUMENT, "sharding chunk_shape rank"};
  uint64_t cps[ZG_MAXD], n_inner = 0;
  std::vector<ZgShard> shards;
  std::vector<uint64_t> shard_of(n, UINT64_MAX);
  for (uint64_t i = 0; i < n; i++) {
    const zgpu_chunk_desc &D = descs[i];
    bool ok = desc_geometry_ok(D, nd, G.out_shape);
    uint64_t ni = 1;
    for (uint32_t d = 0; d < nd && ok; d++) {
      if (!ms[d] || D.chunk_shape[d] % ms[d]) ok = false;  // calculate_chunks_per_shard (sharding.rs:136-154)
      else {
        cps[d] = D.chunk_shape[d] / ms[d];
        ni *= cps[d];
      }
    }
    if (!ok) {
      status[i] = ZGPU_INVALID_ARGUMENT;
      continue;
    }
    n_inner = ni;  // one shard shape per call (decode_general groups by shape)
    if (D.enc && sel_volume(D, nd)) {
      shard_of[i] = shards.size();
      shards.push_back(ZgShard{(uint64_t)D.enc, D.enc_len});
    }
  }
  std::vector<uint64_t> index;
  std::vector<uint32_t> sst;
  if (!shards.empty()) {
    const ZgIndexSpec spec = index_spec(top.a2b, n_inner, G.validate);
    const size_t ns = shards.size();
    index.resize(ns * n_inner * 2);
    sst.resize(ns);
    Scratch sc(G.C, G.s);
    ZgShard *d_sh = sc.dev<ZgShard>(ns);
    uint64_t *d_idx = sc.dev<uint64_t>(index.size());
    uint32_t *d_st = sc.dev<uint32_t>(ns);
    HIPCHK(hipMemcpyAsync(d_sh, shards.data(), ns * sizeof(ZgShard), hipMemcpyHostToDevice, G.s));
    HIPCHK(launch_shard_index(d_sh, (uint32_t)ns, spec, d_idx, d_st, 0, G.s));
    HIPCHK(hipMemcpyAsync(index.data(), d_idx, index.size() * 8, hipMemcpyDeviceToHost, G.s));
    HIPCHK(hipMemcpyAsync(sst.data(), d_st, ns * 4, hipMemcpyDeviceToHost, G.s));
    HIPCHK(hipStreamSynchronize(G.s));
  }
  std::vector<zgpu_chunk_desc> sub;
  std::vector<uint64_t> owner;
  for (uint64_t i = 0; i < n; i++) {
    const zgpu_chunk_desc &D = descs[i];
    if (status[i] || sel_volume(D, nd) == 0) continue;
    const uint64_t sh = shard_of[i];
    if (sh != UINT64_MAX && sst[sh]) {
      status[i] = (int32_t)sst[sh];
      continue;
    }
    uint64_t lo[ZG_MAXD], hi[ZG_MAXD], idx[ZG_MAXD];
    for (uint32_t d = 0; d < nd; d++) {
      cps[d] = D.chunk_shape[d] / ms[d];
      lo[d] = D.sel_start[d] / ms[d];
      hi[d] = (D.sel_start[d] + D.sel_shape[d] - 1) / ms[d] + 1;
      idx[d] = lo[d];
    }
    for (;;) {  // every intersecting middle shard, C order
      zgpu_chunk_desc M{};
      uint64_t lin = 0;
      for (uint32_t d = 0; d < nd; d++) {
        lin = lin * cps[d] + idx[d];
        const uint64_t cs = idx[d] * ms[d], ce = cs + ms[d];
        const uint64_t s0 = std::max(D.sel_start[d], cs), s1 = std::min(D.sel_start[d] + D.sel_shape[d], ce);
        M.chunk_shape[d] = ms[d];
        M.sel_start[d] = s0 - cs;
        M.sel_shape[d] = s1 - s0;
        M.out_start[d] = D.out_start[d] + (s0 - D.sel_start[d]);
      }
      bool oob = false;
      if (sh != UINT64_MAX) {
        const uint64_t off = index[(sh * n_inner + lin) * 2], size = index[(sh * n_inner + lin) * 2 + 1];
        if (!(off == ~0ull && size == ~0ull)) {
          if (off > D.enc_len || size > D.enc_len - off) oob = true;
          M.enc = (const uint8_t *)D.enc + off;
          M.enc_len = size;
        }
      }
      if (oob) {  // sharding_codec.rs: an inner chunk outside the shard
        status[i] = ZGPU_SHARD_INDEX_OOB;
      } else {
        sub.push_back(M);
        owner.push_back(i);
      }
      int d = (int)nd - 1;
      for (; d >= 0; d--) {
        if (++idx[d] < hi[d]) break;
        idx[d] = lo[d];
      }
      if (d < 0 || oob) break;
    }
  }
  run_sub(G, top.a2b.inner, sub, owner, status);
}

// Selections in one frame, each decoded through `chain` into its own box of a scratch buffer (boxes
// stacked along axis 0, the trailing axes as wide as the widest box), and the boxes that decoded packed
// compact, back to back (k_box_copy). enc[k] holds caller descriptor owner[k]'s selection in the
// chain's frame (its out_start is set here); a box that fails gives that descriptor its status.
// leaf[j] describes packed box j as one whole chunk of its caller's selection shape at its caller's
// out_start, for the chain that scatters it.
namespace {
struct PackedBoxes {
  uint8_t *pk = nullptr;  // elems * es bytes (a failed box keeps its room)
  uint64_t elems = 0;
  std::vector<zgpu_chunk_desc> leaf;
  std::vector<uint64_t> owner, elem_off;  // of leaf[j]: its caller descriptor, its first element in pk
};
}  // namespace
static PackedBoxes decode_stacked(GeneralCall &G, Scratch &sc, const std::shared_ptr<Chain> &chain, uint32_t es,
                                  std::vector<zgpu_chunk_desc> &enc, const std::vector<uint64_t> &owner,
                                  const zgpu_chunk_desc *descs, int32_t *status) {
  const uint32_t nd = G.nd;
  PackedBoxes B;
  uint64_t stacked[ZG_MAXD] = {0}, stacked_elems = 1;
  std::vector<uint64_t> off(enc.size());
  for (size_t k = 0; k < enc.size(); k++) {
    zgpu_chunk_desc &E = enc[k];
    for (uint32_t a = 0; a < nd; a++) E.out_start[a] = 0;
    E.out_start[0] = stacked[0];
    stacked[0] += E.sel_shape[0];
    for (uint32_t a = 1; a < nd; a++) stacked[a] = std::max(stacked[a], E.sel_shape[a]);
    off[k] = B.elems;
    B.elems += sel_volume(E, nd);
  }
  for (uint32_t a = 0; a < nd; a++) stacked_elems *= stacked[a];
  uint8_t *T = sc.dev<uint8_t>(stacked_elems * es);
  GeneralCall G1{G.C, G.validate, nd, T, stacked, G.flags, G.s, {}};
  std::vector<int32_t> st(enc.size(), 0);
  const bool had_detail = size_detail().valid;
  decode_general(G1, chain, enc.data(), enc.size(), st.data());
  if (!had_detail && size_detail().valid) size_detail().desc = owner[size_detail().desc];
  B.pk = sc.dev<uint8_t>(std::max<uint64_t>(B.elems * es, 1));
  for (size_t k = 0; k < enc.size(); k++) {
    const uint64_t i = owner[k];
    if (st[k]) {
      status[i] = st[k];
      continue;
    }
    uint64_t org[ZG_MAXD] = {0};
    org[0] = enc[k].out_start[0];
    pack_box(T, nd, stacked, org, enc[k].sel_shape, es, B.pk, off[k] * es, G.s);
    zgpu_chunk_desc L{};
    L.enc = B.pk + off[k] * es;
    L.enc_len = sel_volume(enc[k], nd) * es;
    for (uint32_t a = 0; a < nd; a++) {
      L.chunk_shape[a] = L.sel_shape[a] = descs[i].sel_shape[a];
      L.sel_start[a] = 0;
      L.out_start[a] = descs[i].out_start[a];
    }
    B.leaf.push_back(L);
    B.owner.push_back(i);
    B.elem_off.push_back(off[k]);
  }
  return B;
}

// Transpose codecs before a sharding_indexed the fused plan does not take (bytes->bytes codecs after
// it, or shards with codecs around them / nested deeper below it). zarrs decodes the sharding codec
// on the encoded (transposed) shape, then the transposes (codec_chain.rs:592-646, transpose_codec.rs:
// 264-281), and a partial read asks the sharding partial decoder for the selection's box in the
// encoded frame (transpose_codec_partial.rs). Here every descriptor's selection is decoded by the
// chain without its transposes, in the encoded frame, into its own box of a device buffer (boxes
// stacked along axis 0); the boxes are packed compact (k_box_copy) and then decoded as the leaf chunks
// of [transposes, bytes(native)], which transposes and scatters them into the output in one fused pass.
static void transposed_general(GeneralCall &G, const std::shared_ptr<Chain> &chain, const zgpu_chunk_desc *descs,
                               uint64_t n, int32_t *status) {
  const Chain &top = *chain;
  const uint32_t nd = G.nd, es = top.es;
  uint32_t m[ZG_MAXD];
  composed_axes(top, nd, m);  // encoded axis a <-> decoded axis m[a]
  auto bare = std::make_shared<Chain>(top);
  bare->a2a.clear();
  auto tr = std::make_shared<Chain>(top);
  tr->b2b.clear();
  tr->a2b = Codec{};
  tr->a2b.kind = CodecKind::Bytes;
  tr->a2b.name = "bytes";
  tr->a2b.big_endian = false;  // the decoded elements are native (little-endian) already
  std::vector<zgpu_chunk_desc> enc_descs;
  std::vector<uint64_t> owner;
  for (uint64_t i = 0; i < n; i++) {
    const zgpu_chunk_desc &D = descs[i];
    if (!desc_geometry_ok(D, nd, G.out_shape)) {
      status[i] = ZGPU_INVALID_ARGUMENT;
      continue;
    }
    if (sel_volume(D, nd) == 0) continue;
    zgpu_chunk_desc E = D;
    for (uint32_t a = 0; a < nd; a++) {
      E.chunk_shape[a] = D.chunk_shape[m[a]];
      E.sel_start[a] = D.sel_start[m[a]];
      E.sel_shape[a] = D.sel_shape[m[a]];
    }
    enc_descs.push_back(E);
    owner.push_back(i);
  }
  if (enc_descs.empty()) return;
  Scratch sc(G.C, G.s);
  PackedBoxes B = decode_stacked(G, sc, bare, es, enc_descs, owner, descs, status);
  run_sub(G, tr, B.leaf, B.owner, status);
}

// The chain without its value codecs (numcodecs.fixedscaleoffset, bitround), at every sharding level;
// `steps` receives them in encode order. They work element by element, so they commute with
// chunking, sharding, transposes and selection: what the stripped chain decodes, in the innermost
// encoded data type, is the selection before the value codecs' decode.
std::shared_ptr<Chain> strip_value_codecs(const Chain &c, std::vector<Codec> &steps) {
  auto r = std::make_shared<Chain>(c);
  r->a2a.clear();
  for (const Codec &k : c.a2a) {
    if (is_value_codec(k.kind)) steps.push_back(k);
    else r->a2a.push_back(k);
  }
  if (c.a2b.kind == CodecKind::Sharding) r->a2b.inner = strip_value_codecs(*c.a2b.inner, steps);
  return r;
}

// Every level of a stripped chain bound to the innermost encoded data type and fill value.
void retype_stripped(Chain &c, const Chain &original) {
  const Chain *leaf = &original;
  while (leaf->a2b.kind == CodecKind::Sharding) leaf = leaf->a2b.inner.get();
  for (Chain *l = &c;; l = l->a2b.inner.get()) {
    l->es = l->enc_es = leaf->enc_es;
    l->comp = l->enc_comp = leaf->enc_comp;
    l->data_type = l->enc_data_type = leaf->enc_data_type;
    std::memcpy(l->fill, leaf->enc_fill, 16);
    std::memcpy(l->enc_fill, leaf->enc_fill, 16);
    if (l->a2b.kind != CodecKind::Sharding) break;
  }
}

static uint32_t mantissa_bits_of(uint32_t vt) {
  return vt == VT_F16 ? 10 : vt == VT_BF16 ? 7 : vt == VT_F32 ? 23 : vt == VT_F64 ? 52 : 0;
}

// Whether a value codec's decode changes the elements (bitround's is the identity).
static bool decode_converts(const Codec &k) {
  return k.kind == CodecKind::FixedScaleOffset || k.kind == CodecKind::CastValue;
}

// n elements through the value codecs' decode (`steps` in encode order, run backwards) from `in`, in
// the innermost encoded type, into `out` (must not be `in`), in the decoded type. bitround decodes
// as the identity. A cast_value step lowers *fail (device, preset to ~0; null when no step can fail) to
// the index of an element it cannot cast. Temporaries go to `sc`. Enqueues only.
static void value_decode_elements(const std::vector<Codec> &steps, const uint8_t *in, uint8_t *out, uint64_t n,
                                  uint32_t es_out, Scratch &sc, hipStream_t s, uint64_t *fail) {
  std::vector<const Codec *> conv;
  for (size_t j = steps.size(); j-- > 0;)
    if (decode_converts(steps[j])) conv.push_back(&steps[j]);
  if (conv.empty()) {
    if (n) HIPCHK(hipMemcpyAsync(out, in, n * es_out, hipMemcpyDeviceToDevice, s));
    return;
  }
  const uint8_t *cur = in;
  for (size_t j = 0; j < conv.size(); j++) {
    const Codec &k = *conv[j];
    uint8_t *dst = out;
    if (j + 1 < conv.size()) {
      dst = sc.dev<uint8_t>(std::max<uint64_t>(n * value_type_size(k.vt_dec), 1));
    }
    if (k.kind == CodecKind::CastValue)
      HIPCHK(launch_cast(k.vt_enc, k.vt_dec, cur, dst, n, k.cast_rounding, k.cast_oor, k.cast_dec_map, fail, s));
    else
      HIPCHK(launch_fso_decode(k.vt_enc, k.vt_dec, cur, dst, n, k.fso_offset, k.fso_scale, k.fso_astype ? 1 : 0, s));
    cur = dst;
  }
}

// n elements through the value codecs' encode, `in` (decoded type) to a new device array in the
// innermost encoded type (returned, in `sc`). fail: as for value_decode_elements, for the encode casts.
uint8_t *value_encode_elements(const std::vector<Codec> &steps, const uint8_t *in, uint64_t n, Scratch &sc,
                               hipStream_t s, uint64_t *fail) {
  const uint8_t *cur = in;
  uint8_t *dst = nullptr;
  for (const Codec &k : steps) {
    dst = sc.dev<uint8_t>(std::max<uint64_t>(n * value_type_size(k.vt_enc), 1));
    if (k.kind == CodecKind::FixedScaleOffset)
      HIPCHK(launch_fso_encode(k.vt_dec, k.vt_enc, cur, dst, n, k.fso_offset, k.fso_scale, k.fso_astype ? 1 : 0, s));
    else if (k.kind == CodecKind::CastValue)
      HIPCHK(launch_cast(k.vt_dec, k.vt_enc, cur, dst, n, k.cast_rounding, k.cast_oor, k.cast_enc_map, fail, s));
    else
      HIPCHK(launch_bitround(value_type_size(k.vt_dec), mantissa_bits_of(k.vt_dec), k.keepbits, cur, dst, n, s));
    cur = dst;
  }
  return dst;
}

// Chains with value codecs, before sharding_indexed, inside its inner chains, or both. The chain
// without them, retyped to the innermost encoded data type and fill value, decodes the callers'
// selections into a device buffer of that type (so a missing chunk or inner chunk holds the encoded
// fill value, as in zarrs); k_fso_decode / k_cast then convert the buffer into the output: one extra pass
// over the data when the descriptors cover the output (the converted buffer is the output), and through
// the stacked boxes of transposed_general otherwise. Only bitround: its decode is the identity, so the
// stripped chain writes the output itself.
// A cast_value decode that can meet an element it cannot cast (cast_decode_fallible) always takes the
// stacked boxes, which are contiguous and hold only the selected elements: every box is converted by
// launches of its own with its own failure word, read back once, and a descriptor whose box failed gets
// ZGPU_CAST_NOT_REPRESENTABLE (zarrs' partial decoder casts the selection, so only it counts) while the
// others are scattered as usual. A descriptor that failed in the stripped chain has no box and keeps
// that status.
static void value_general(GeneralCall &G, const std::shared_ptr<Chain> &chain, const zgpu_chunk_desc *descs,
                          uint64_t n, int32_t *status) {
  const Chain &top = *chain;
  const uint32_t nd = G.nd;
  std::vector<Codec> steps;
  auto bare = strip_value_codecs(top, steps);
  retype_stripped(*bare, top);
  bool converts = false, fallible = false;
  for (const Codec &k : steps) {
    converts = converts || decode_converts(k);
    fallible = fallible || (k.kind == CodecKind::CastValue && cast_decode_fallible(k));
  }
  if (!converts) {
    decode_general(G, bare, descs, n, status);
    return;
  }
  const uint32_t es_e = bare->es, es_d = top.es;
  Scratch sc(G.C, G.s);
  bool geometry = true;
  uint64_t covered = 0, out_elems = 1;
  for (uint64_t i = 0; i < n; i++) {
    geometry = geometry && desc_geometry_ok(descs[i], nd, G.out_shape);
    covered += sel_volume(descs[i], nd);
  }
  for (uint32_t d = 0; d < nd; d++) out_elems *= G.out_shape[d];
  if (geometry && covered == out_elems && !fallible) {
    // the (disjoint) selections tile the output: decode into its image in the encoded type, convert
    uint8_t *T = sc.dev<uint8_t>(std::max<uint64_t>(out_elems * es_e, 1));
    GeneralCall G1{G.C, G.validate, nd, T, G.out_shape, G.flags, G.s, {}};
    decode_general(G1, bare, descs, n, status);
    value_decode_elements(steps, T, G.out, out_elems, es_d, sc, G.s, nullptr);
    return;
  }
  // every selection into its own box of a stacked buffer, packed compact, converted, then scattered
  // as the leaf chunks of [bytes(native)] in the decoded type
  auto plain = std::make_shared<Chain>(top);
  plain->a2a.clear();
  plain->b2b.clear();
  plain->a2b = Codec{};
  plain->a2b.kind = CodecKind::Bytes;
  plain->a2b.name = "bytes";
  plain->enc_es = top.es;
  plain->enc_comp = top.comp;
  plain->enc_data_type = top.data_type;
  std::memcpy(plain->enc_fill, top.fill, 16);
  std::vector<zgpu_chunk_desc> enc_descs;
  std::vector<uint64_t> owner;
  for (uint64_t i = 0; i < n; i++) {
    if (!desc_geometry_ok(descs[i], nd, G.out_shape)) {
      status[i] = ZGPU_INVALID_ARGUMENT;
      continue;
    }
    if (sel_volume(descs[i], nd) == 0) continue;
    enc_descs.push_back(descs[i]);
    owner.push_back(i);
  }
  if (enc_descs.empty()) return;
  PackedBoxes B = decode_stacked(G, sc, bare, es_e, enc_descs, owner, descs, status);
  uint8_t *PkD = sc.dev<uint8_t>(B.elems * es_d);
  for (size_t j = 0; j < B.leaf.size(); j++) {  // the leaf chunks are the converted boxes
    B.leaf[j].enc = PkD + B.elem_off[j] * es_d;
    B.leaf[j].enc_len = B.leaf[j].enc_len / es_e * es_d;
  }
  if (!fallible) {
    value_decode_elements(steps, B.pk, PkD, B.elems, es_d, sc, G.s, nullptr);
    run_sub(G, plain, B.leaf, B.owner, status);
    return;
  }
  const size_t nb = B.leaf.size();
  if (!nb) return;
  uint64_t *d_fail = sc.dev<uint64_t>(nb);
  HIPCHK(hipMemsetAsync(d_fail, 0xff, nb * 8, G.s));
  for (size_t j = 0; j < nb; j++)
    value_decode_elements(steps, B.pk + B.elem_off[j] * es_e, PkD + B.elem_off[j] * es_d, B.leaf[j].enc_len / es_d, es_d,
                          sc, G.s, d_fail + j);
  std::vector<uint64_t> failed(nb);
  HIPCHK(hipMemcpyAsync(failed.data(), d_fail, nb * 8, hipMemcpyDeviceToHost, G.s));
  HIPCHK(hipStreamSynchronize(G.s));
  std::vector<zgpu_chunk_desc> cast_leaf;
  std::vector<uint64_t> cast_owner;
  for (size_t j = 0; j < nb; j++) {
    if (failed[j] != UINT64_MAX) {
      status[B.owner[j]] = ZGPU_CAST_NOT_REPRESENTABLE;
      continue;
    }
    cast_leaf.push_back(B.leaf[j]);
    cast_owner.push_back(B.owner[j]);
  }
  run_sub(G, plain, cast_leaf, cast_owner, status);
}

// packbits as the array->bytes codec (unsharded): its chunks are not element-aligned, so whole chunks
// of [bytes(uint8), bytes->bytes codecs...] over the packed length are decoded into a device buffer
// (which checks the packed length: DECODED_SIZE_MISMATCH), k_unpackbits expands them into native
// elements (and checks the padding byte: CORRUPT_STREAM), and those are the leaf chunks of
// [array->array codecs..., bytes(native)] with the callers' selections.
static void packbits_general(GeneralCall &G, const std::shared_ptr<Chain> &chain, const zgpu_chunk_desc *descs,
                             uint64_t n, int32_t *status) {
  const Chain &top = *chain;
  const Codec &pb = top.a2b;
  const uint32_t nd = G.nd, es = top.enc_es;
  uint64_t nelem = 1;
  for (uint32_t d = 0; d < nd; d++) nelem *= descs[0].chunk_shape[d];
  const uint64_t packed = packbits_size(pb, nelem);
  const uint64_t ppitch = ((packed + 15) & ~(uint64_t)15) + 16, upitch = (nelem * es + 15) & ~(uint64_t)15;
  auto packed_chain = std::make_shared<Chain>();
  packed_chain->es = packed_chain->comp = packed_chain->enc_es = packed_chain->enc_comp = 1;
  packed_chain->data_type = packed_chain->enc_data_type = "uint8";
  packed_chain->a2b.kind = CodecKind::Bytes;
  packed_chain->a2b.name = "bytes";
  packed_chain->b2b = top.b2b;
  auto leaf_chain = std::make_shared<Chain>(top);
  leaf_chain->b2b.clear();
  leaf_chain->a2b = Codec{};
  leaf_chain->a2b.kind = CodecKind::Bytes;
  leaf_chain->a2b.name = "bytes";
  std::vector<zgpu_chunk_desc> pk;  // 1-D descriptors of the packed chunks, slot j of the buffer
  std::vector<uint64_t> pk_owner;
  for (uint64_t i = 0; i < n; i++) {
    const zgpu_chunk_desc &D = descs[i];
    if (!desc_geometry_ok(D, nd, G.out_shape)) {
      status[i] = ZGPU_INVALID_ARGUMENT;
      continue;
    }
    if (!D.enc || sel_volume(D, nd) == 0) continue;  // a missing chunk: the leaf chain fills it
    zgpu_chunk_desc E{};
    E.enc = D.enc;
    E.enc_len = D.enc_len;
    E.chunk_shape[0] = E.sel_shape[0] = packed;
    E.out_start[0] = pk.size() * ppitch;
    pk.push_back(E);
    pk_owner.push_back(i);
  }
  const uint64_t m = pk.size();
  Scratch sc(G.C, G.s);
  uint8_t *U = nullptr;
  std::vector<int32_t> st(m, 0);
  std::vector<uint64_t> slot(n, UINT64_MAX);
  if (m) {
    const uint64_t b_shape[1] = {m * ppitch};
    uint8_t *B = sc.dev<uint8_t>(m * ppitch);
    U = sc.dev<uint8_t>(std::max<uint64_t>(m * upitch, 1));
    GeneralCall G1{G.C, G.validate, 1, B, b_shape, G.flags, G.s, {}};
    const bool had_detail = size_detail().valid;
    decode_general(G1, packed_chain, pk.data(), m, st.data());
    if (!had_detail && size_detail().valid) size_detail().desc = pk_owner[size_detail().desc];
    std::vector<uint64_t> tab;
    std::vector<uint64_t> ok;
    for (uint64_t j = 0; j < m; j++)
      if (!st[j]) ok.push_back(j);
    for (uint64_t j : ok) tab.push_back((uint64_t)(B + j * ppitch));
    for (uint64_t j : ok) tab.push_back((uint64_t)(U + j * upitch));
    if (!ok.empty()) {
      uint64_t *d_tab = sc.dev<uint64_t>(tab.size());
      uint32_t *d_st = sc.dev<uint32_t>(ok.size());
      HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, G.s));
      HIPCHK(hipMemsetAsync(d_st, 0, ok.size() * 4, G.s));
      ZgPackBits P{};
      P.nelem = nelem;
      P.packed_len = packed;
      P.ncomp = pb.pb_ncomp;
      P.comp_bytes = es / pb.pb_ncomp;
      P.first = pb.pb_first;
      P.ext = pb.pb_last - pb.pb_first + 1;
      P.sign = pb.pb_signed ? 1 : 0;
      P.padding = (uint32_t)pb.pb_padding;
      HIPCHK(launch_unpackbits(d_tab, d_st, (uint32_t)ok.size(), P, G.s));
      std::vector<uint32_t> ust(ok.size());
      HIPCHK(hipMemcpyAsync(ust.data(), d_st, ok.size() * 4, hipMemcpyDeviceToHost, G.s));
      HIPCHK(hipStreamSynchronize(G.s));
      for (size_t k = 0; k < ok.size(); k++) st[ok[k]] = (int32_t)ust[k];
    }
    for (uint64_t j = 0; j < m; j++) {
      if (st[j]) status[pk_owner[j]] = st[j];
      else slot[pk_owner[j]] = j;
    }
  }
  std::vector<zgpu_chunk_desc> leaf;
  std::vector<uint64_t> leaf_owner;
  for (uint64_t i = 0; i < n; i++) {
    if (status[i] || sel_volume(descs[i], nd) == 0) continue;
    zgpu_chunk_desc L = descs[i];
    if (slot[i] != UINT64_MAX) {
      L.enc = U + slot[i] * upitch;
      L.enc_len = nelem * es;
    } else {
      L.enc = nullptr;
      L.enc_len = 0;
    }
    leaf.push_back(L);
    leaf_owner.push_back(i);
  }
  run_sub(G, leaf_chain, leaf, leaf_owner, status);
}

void decode_general(GeneralCall &G, const std::shared_ptr<Chain> &chain, const zgpu_chunk_desc *descs, uint64_t n,
                    int32_t *status) {
  for (uint64_t i = 0; i < n; i++) status[i] = 0;
  if (!uniform_shapes(descs, n, G.nd)) {  // one plan per chunk shape
    std::vector<char> done(n, 0);
    for (uint64_t i = 0; i < n; i++) {
      if (done[i]) continue;
      std::vector<zgpu_chunk_desc> sub;
      std::vector<uint64_t> owner;
      for (uint64_t j = i; j < n; j++)
        if (!done[j] && same_shape(descs[i], descs[j], G.nd)) {
          sub.push_back(descs[j]);
          owner.push_back(j);
          done[j] = 1;
        }
      run_sub(G, chain, sub, owner, status);
    }
    return;
  }
  const Chain &top = *chain;
  if (chain_has_value_codec(top) || top.a2b.kind == CodecKind::PackBits) {
    if (!n) return;
    if (chain_has_value_codec(top)) value_general(G, chain, descs, n, status);
    else packbits_general(G, chain, descs, n, status);
    return;
  }
  if (fused_plannable(top)) {
    std::unique_ptr<zgpu_plan> P(plan_new(G.C, chain, G.validate, G.nd, descs, n, G.out_shape, G.flags));
    plan_upload(*P, G.s);
    plan_enqueue(*P, G.out, G.s);
    plan_statuses(*P, status, G.s);
    return;
  }
  if (!top.a2a.empty()) transposed_general(G, chain, descs, n, status);
  else if (!top.b2b.empty()) predecode_shards(G, chain, descs, n, status);
  else nested_host(G, chain, descs, n, status);
}
