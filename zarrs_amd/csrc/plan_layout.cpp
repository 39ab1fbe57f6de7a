// libzgpu: the host layout of a fused decode plan (plan_layout.hpp). No HIP call and no environment
// read below layout_knobs_from_env: plan_layout() is a function of its arguments.
#include "plan_layout.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace zgpu {

LayoutKnobs layout_knobs_from_env() {
  LayoutKnobs K;
  if (const char *e = std::getenv("ZGPU_UNSHUFFLE_WIDE")) K.unshuffle_wide = (uint32_t)std::max(0, std::min(2, std::atoi(e)));
  K.blosc_no_direct = std::getenv("ZGPU_BLOSC_NO_DIRECT") != nullptr;
  if (const char *e = std::getenv("ZGPU_GZIP_DIRECT")) K.gzip_direct = std::atoi(e) != 0;
  K.blosc_no_partial = std::getenv("ZGPU_BLOSC_NO_PARTIAL") != nullptr;
  return K;
}

void composed_axes(const Chain &c, uint32_t nd, uint32_t *m) {
  for (uint32_t a = 0; a < nd; a++) m[a] = a;
  for (const Codec &k : c.a2a) {  // E_{k} axis a <-> E_{k-1} axis order[a]
    if (k.kind != CodecKind::Transpose) continue;  // the value codecs keep every element in its place
    uint32_t t[ZG_MAXD];
    for (uint32_t a = 0; a < nd; a++) t[a] = m[k.order[a]];
    std::memcpy(m, t, nd * sizeof(uint32_t));
  }
}

// ShardingIndex decode spec (sharding.rs:136-235, sharding_codec.rs:1262-1298): the index chain
// must be bytes (+ crc32c), the only index_codecs zarrs' sharding writes and the GPU decodes.
ZgIndexSpec index_spec(const Codec &sharding, uint64_t n_inner, bool validate) {
  const Chain &xc = *sharding.index;
  if (xc.a2b.kind != CodecKind::Bytes || !xc.a2a.empty())
    throw ChainError{ZGPU_UNSUPPORTED, "index_codecs must be bytes (+crc32c)"};
  for (const Codec &k : xc.b2b)
    if (k.kind != CodecKind::Crc32c) throw ChainError{ZGPU_UNSUPPORTED, "index_codecs must be bytes (+crc32c)"};
  if (xc.b2b.size() > 4) throw ChainError{ZGPU_UNSUPPORTED, "too many index crc32c codecs"};
  ZgIndexSpec S{};
  S.n_inner = n_inner;
  S.index_bytes = (uint64_t)chain_fixed_encoded_size(xc, n_inner * 2);
  S.at_start = sharding.at_start;
  S.big_endian = xc.a2b.big_endian;
  S.n_crc = (uint32_t)xc.b2b.size();
  for (size_t k = 0; k < xc.b2b.size(); k++) S.crc_at_start[k] = xc.b2b[k].at_start;
  S.verify = validate;
  return S;
}

std::optional<Stage> stage_for(const Codec &k) {
  Stage s{};
  switch (k.kind) {
    case CodecKind::Crc32c:
    case CodecKind::Adler32:
    case CodecKind::Fletcher32: s.kind = checksum_stage(k.kind); s.at_start = k.at_start; break;
    case CodecKind::Gzip: s.kind = ST_GZIP; break;
    case CodecKind::Zlib: s.kind = ST_ZLIB; break;
    case CodecKind::Bz2: s.kind = ST_BZ2; break;
    case CodecKind::Zstd: s.kind = ST_ZSTD; break;
    case CodecKind::Blosc: s.kind = ST_BLOSC; break;
    case CodecKind::Shuffle: s.kind = ST_UNSHUFFLE; s.elementsize = k.elementsize; break;
    default: return std::nullopt;
  }
  return s;
}

PlanLayout stages_only_layout(std::vector<ZgItem> items, Stage st, uint64_t slot_bytes) {
  PlanLayout L;
  L.items = std::move(items);
  for (size_t j = 0; j < L.items.size(); j++) L.items[j].desc = (uint32_t)j;
  L.item_desc_status.assign(L.items.size(), 0);
  st.pool = 0;
  L.stages = {st};
  L.n_pools = strips_only(st.kind) ? 0 : 1;
  L.slot_bytes = (slot_bytes + 255) & ~(uint64_t)255;
  L.no_scatter = true;
  return L;
}

namespace {

// The cells of a regular grid (cells of shape `cell`, grid[d] of them along axis d) that intersect the
// non-empty box [b0, b1), in C order (last axis fastest). f(lin, sel, ext, off): the cell's linear
// index in the grid, the box clipped to the cell as a selection inside the cell (start sel, extent ext)
// and that selection's offset from the box's origin.
template <class F>
void for_each_cell(uint32_t nd, const uint64_t *cell, const uint64_t *grid, const uint64_t *b0, const uint64_t *b1,
                   F &&f) {
  uint64_t lo[ZG_MAXD], hi[ZG_MAXD], idx[ZG_MAXD];
  for (uint32_t d = 0; d < nd; d++) {
    lo[d] = b0[d] / cell[d];
    hi[d] = (b1[d] - 1) / cell[d] + 1;
    idx[d] = lo[d];
  }
  for (;;) {
    uint64_t lin = 0, sel[ZG_MAXD], ext[ZG_MAXD], off[ZG_MAXD];
    for (uint32_t d = 0; d < nd; d++) {
      lin = lin * grid[d] + idx[d];
      const uint64_t cs = idx[d] * cell[d], ce = cs + cell[d];
      const uint64_t s0 = std::max(b0[d], cs), s1 = std::min(b1[d], ce);
      sel[d] = s0 - cs;
      ext[d] = s1 - s0;
      off[d] = s0 - b0[d];
    }
    f(lin, sel, ext, off);
    int d = (int)nd - 1;
    for (; d >= 0; d--) {
      if (++idx[d] < hi[d]) break;
      idx[d] = lo[d];
    }
    if (d < 0) break;
  }
}

// The chain's levels and the shapes they fix. Transpose codecs before sharding_indexed
// (codec_chain.rs:557-646: the sharding codec decodes the transposed array): the shard and its inner
// chunk grid live in the encoded frame, encoded axis a <-> decoded axis mo[a]; descriptors are mapped
// into that frame and the scatter writes through output strides permuted back. Nested sharding
// (sharding.rs:107-126 nested_local_subchunk_grids): the outer shard's subchunks are shards themselves
// ("middle" shards); their indexes are decoded on the device after the outer index resolves them, and
// the leaf chunks resolve through the middle indexes.
struct Levels {
  const Chain *mid = nullptr, *leaf = nullptr;
  bool sharded = false, outer_perm = false;
  uint32_t nd = 0, mo[ZG_MAXD];
  uint64_t leaf_shape[ZG_MAXD], nelem = 1;
  uint64_t sub_shape[ZG_MAXD];               // sharded: the outer shard's subchunks (leaves, or middle shards)
  uint64_t cps2[ZG_MAXD] = {}, n_inner2 = 1;  // nested: leaves per middle shard
};

void check_transposes(const Chain &c, uint32_t nd) {
  for (const Codec &k : c.a2a)
    if (k.kind == CodecKind::Transpose && k.order.size() != nd)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "transpose order rank != array rank"};
}

Levels resolve_levels(const Chain &top, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n) {
  if (chain_has_value_codec(top) || top.a2b.kind == CodecKind::PackBits)
    throw ChainError{ZGPU_UNSUPPORTED, "chains with numcodecs.fixedscaleoffset, bitround or packbits do not take the "
                                       "fused plan (zgpu_plan_create, zgpu_group_create): decode them through "
                                       "zgpu_decode_batch / zgpu_decode_into / zgpu_decode_pinned"};
  Levels V;
  V.nd = nd;
  V.sharded = top.a2b.kind == CodecKind::Sharding;
  for (uint32_t a = 0; a < nd; a++) V.mo[a] = a;
  if (V.sharded) {
    check_transposes(top, nd);
    composed_axes(top, nd, V.mo);
    for (uint32_t a = 0; a < nd; a++) V.outer_perm = V.outer_perm || V.mo[a] != a;
    if (!top.b2b.empty()) throw ChainError{ZGPU_UNSUPPORTED, "bytes->bytes codecs after sharding_indexed"};
    if (top.a2b.inner_shape.size() != nd) throw ChainError{ZGPU_INVALID_ARGUMENT, "sharding chunk_shape rank"};
    if (top.a2b.inner->a2b.kind == CodecKind::Sharding) {
      V.mid = top.a2b.inner.get();
      if (!V.mid->a2a.empty() || !V.mid->b2b.empty())
        throw ChainError{ZGPU_UNSUPPORTED, "codecs around a nested sharding_indexed"};
      if (V.mid->a2b.inner->a2b.kind == CodecKind::Sharding)
        throw ChainError{ZGPU_UNSUPPORTED, "sharding_indexed nested more than two deep"};
      if (V.mid->a2b.inner_shape.size() != nd) throw ChainError{ZGPU_INVALID_ARGUMENT, "sharding chunk_shape rank"};
    }
  }
  V.leaf = V.sharded ? (V.mid ? V.mid->a2b.inner.get() : top.a2b.inner.get()) : &top;
  check_transposes(*V.leaf, nd);
  for (uint32_t d = 0; d < nd; d++) {
    if (V.sharded) {
      V.sub_shape[d] = top.a2b.inner_shape[d];
      V.leaf_shape[d] = V.mid ? V.mid->a2b.inner_shape[d] : V.sub_shape[d];
      if (V.mid) {
        if (!V.leaf_shape[d] || V.sub_shape[d] % V.leaf_shape[d])
          throw ChainError{ZGPU_INVALID_ARGUMENT, "nested sharding: subchunk shape does not divide the shard"};
        V.cps2[d] = V.sub_shape[d] / V.leaf_shape[d];
        V.n_inner2 *= V.cps2[d];
      }
    } else {
      V.leaf_shape[d] = n ? descs[0].chunk_shape[d] : 1;
    }
    V.nelem *= V.leaf_shape[d];
  }
  return V;
}

// A descriptor's own geometry: the selection inside its chunk and inside the output, and (unsharded)
// the batch's one chunk shape. full: the selection is the whole chunk.
bool desc_ok(const Levels &V, const zgpu_chunk_desc &D, const uint64_t *out_shape, bool &full) {
  bool ok = true;
  full = true;
  for (uint32_t d = 0; d < V.nd; d++) {
    if (D.sel_start[d] + D.sel_shape[d] > D.chunk_shape[d] || D.out_start[d] + D.sel_shape[d] > out_shape[d])
      ok = false;
    if (D.sel_start[d] != 0 || D.sel_shape[d] != D.chunk_shape[d]) full = false;
    if (!V.sharded && D.chunk_shape[d] != V.leaf_shape[d]) ok = false;
  }
  return ok;
}

void add_plain_item(PlanLayout &L, uint32_t nd, const zgpu_chunk_desc &D, uint64_t i, bool full) {
  ZgItem it{};
  it.src = (uint64_t)D.enc;
  it.len = D.enc_len;
  it.desc = (uint32_t)i;
  it.flags = (D.enc ? 0u : ZG_ITEM_FILL) | (full ? 0u : ZG_ITEM_PARTIAL);
  if (D.enc) L.alg_bytes_static += D.enc_len;
  L.items.push_back(it);
  L.geom.insert(L.geom.end(), D.sel_start, D.sel_start + nd);
  L.geom.insert(L.geom.end(), D.sel_shape, D.sel_shape + nd);
  L.geom.insert(L.geom.end(), D.out_start, D.out_start + nd);
}

// One leaf item per leaf chunk that intersects the box [b0, b1) of the shard (nested: of the middle
// shard) in index slot `slot`, whose leaf grid is `grid`; out0: the box's origin in the output.
void add_leaves(PlanLayout &L, const Levels &V, const ZgItem &proto, uint32_t slot, const uint64_t *b0, const uint64_t *b1,
                const uint64_t *out0, const uint64_t *grid) {
  const uint32_t nd = V.nd;
  for_each_cell(nd, V.leaf_shape, grid, b0, b1,
                [&](uint64_t lin, const uint64_t *sel, const uint64_t *ext, const uint64_t *off) {
                  ZgItem it = proto;
                  it.shard = slot;
                  it.inner = (uint32_t)lin;
                  L.items.push_back(it);
                  L.geom.insert(L.geom.end(), sel, sel + nd);
                  L.geom.insert(L.geom.end(), ext, ext + nd);
                  for (uint32_t d = 0; d < nd; d++) L.geom.push_back(out0[d] + off[d]);
                });
}

// A sharded descriptor: its shard, (nested) one record per intersecting middle shard, and one item per
// intersecting leaf chunk, all in the sharding codec's (encoded) frame: axis a is decoded axis mo[a].
// Returns the descriptor's plan-time status.
uint32_t add_shard_items(PlanLayout &L, const Levels &V, const zgpu_chunk_desc &D, uint64_t i, bool full) {
  const uint32_t nd = V.nd;
  uint64_t b0[ZG_MAXD], b1[ZG_MAXD], out0[ZG_MAXD], cps[ZG_MAXD], n_inner = 1;
  for (uint32_t a = 0; a < nd; a++) {
    const uint64_t extent = D.chunk_shape[V.mo[a]];
    // calculate_chunks_per_shard error (sharding.rs:136-154)
    if (extent % V.sub_shape[a]) return ZGPU_INVALID_ARGUMENT;
    cps[a] = extent / V.sub_shape[a];
    n_inner *= cps[a];
    b0[a] = D.sel_start[V.mo[a]];
    b1[a] = b0[a] + D.sel_shape[V.mo[a]];
    out0[a] = D.out_start[V.mo[a]];
  }
  if (L.ispec.n_inner && L.ispec.n_inner != n_inner) return ZGPU_UNSUPPORTED;  // mixed shard shapes in one batch
  L.ispec.n_inner = n_inner;
  const uint32_t shard_slot = (uint32_t)L.shards.size();
  L.shards.push_back(ZgShard{(uint64_t)D.enc, D.enc ? D.enc_len : 0});
  ZgItem leaf{}, mid{};
  leaf.desc = mid.desc = (uint32_t)i;
  leaf.flags = D.enc ? (ZG_ITEM_SHARDED | (full ? 0u : ZG_ITEM_PARTIAL)) : ZG_ITEM_FILL;
  mid.flags = D.enc ? ZG_ITEM_SHARDED : ZG_ITEM_FILL;
  if (!V.mid) {
    add_leaves(L, V, leaf, shard_slot, b0, b1, out0, cps);
    return 0;
  }
  // every intersecting middle shard: an index slot, then its leaf chunks
  for_each_cell(nd, V.sub_shape, cps, b0, b1,
                [&](uint64_t lin, const uint64_t *sel, const uint64_t *ext, const uint64_t *off) {
                  uint64_t m1[ZG_MAXD], mout[ZG_MAXD];
                  for (uint32_t d = 0; d < nd; d++) {
                    m1[d] = sel[d] + ext[d];
                    mout[d] = out0[d] + off[d];
                  }
                  const uint32_t mslot = (uint32_t)L.mids.size();
                  mid.shard = shard_slot;
                  mid.inner = (uint32_t)lin;
                  L.mids.push_back(mid);
                  add_leaves(L, V, leaf, mslot, sel, m1, mout, V.cps2);
                });
  return 0;
}

// The leaf chain's bytes->bytes stages in decode order (last codec first), two slot pools alternating
// between the materialising ones; a shuffle directly above the bytes codec is fused into the scatter.
void build_leaf_stages(PlanLayout &L, const Chain &leaf, uint64_t nelem, const LayoutKnobs &knobs) {
  const int nb = (int)leaf.b2b.size();
  int pool = 0;
  uint64_t max_slot = 0;
  bool fused_shuffle = false;
  for (int i = nb - 1; i >= 0; i--) {
    const Codec &k = leaf.b2b[i];
    if (k.kind == CodecKind::Shuffle && i == 0 && k.elementsize == leaf.es) {
      fused_shuffle = true;  // fused into the scatter stage
      continue;
    }
    const std::optional<Stage> known = stage_for(k);
    if (!known) throw ChainError{ZGPU_UNSUPPORTED, "codec '" + k.name + "' among the bytes->bytes codecs"};
    Stage s = *known;
    if (strips_only(s.kind)) {
      L.stages.push_back(s);
      continue;
    }
    // materialising stage: its output is the encoded representation of codecs [bytes, b2b_0..i-1]
    int64_t out_size = (int64_t)(nelem * leaf.es);
    for (int j = 0; j < i; j++) {
      if (is_checksum(leaf.b2b[j].kind)) out_size += 4;
      else if (leaf.b2b[j].kind != CodecKind::Shuffle) out_size = -1;
      if (out_size < 0) break;
    }
    if (out_size < 0) throw ChainError{ZGPU_UNSUPPORTED, "a compressor nested inside another variable-size codec"};
    s.pool = pool;
    pool ^= 1;
    max_slot = std::max<uint64_t>(max_slot, (uint64_t)out_size);
    L.stages.push_back(s);
    L.n_pools = std::min(2, L.n_pools + 1);
  }
  L.slot_bytes = (max_slot + 255) & ~(uint64_t)255;
  L.scatter.shuffle = fused_shuffle;
  L.scatter.pad0 = knobs.unshuffle_wide;
}

// Scatter parameters: the leaf chunk's encoded strides through the leaf chain's transposes, the
// output strides through the transposes before sharding_indexed, and the tiled kernel's two axes.
void scatter_params(PlanLayout &L, const Levels &V, const uint64_t *out_shape) {
  const uint32_t nd = V.nd;
  const Chain &leaf = *V.leaf;
  ZgScatter &S = L.scatter;
  S.nd = nd;
  S.es = leaf.es;
  S.comp = leaf.comp;
  S.swap = leaf.a2b.big_endian && leaf.comp > 1;
  S.nelem = V.nelem;
  std::memcpy(S.fill, leaf.fill, 16);
  uint32_t m[ZG_MAXD];
  composed_axes(leaf, nd, m);
  uint64_t out_strides[ZG_MAXD], s = 1;
  for (int d = (int)nd - 1; d >= 0; d--) {
    out_strides[d] = s;
    s *= out_shape[d];
  }
  s = 1;
  for (int a = (int)nd - 1; a >= 0; a--) {  // the encoded chunk is C order over shape[m[a]]
    S.enc_stride[m[a]] = s;
    s *= V.leaf_shape[m[a]];
  }
  for (uint32_t d = 0; d < nd; d++) {
    S.chunk_shape[d] = V.leaf_shape[d];
    S.out_stride[d] = out_strides[V.mo[d]];
  }
  S.tile_a = m[nd - 1];
  S.tile_b = ZG_MAXD;
  for (uint32_t d = 0; d + 1 < nd; d++) {
    if (d == S.tile_a) continue;
    if (S.tile_b == ZG_MAXD || S.enc_stride[d] <= S.enc_stride[S.tile_b]) S.tile_b = d;
  }
}

// Rows / tiled / generic, the grid units per item, and whether the tiled batch takes the persistent kernel.
void scatter_mode(PlanLayout &L, const Levels &V) {
  const ZgScatter &S = L.scatter;
  const uint32_t nd = V.nd;
  if (V.outer_perm && S.out_stride[nd - 1] != 1) {
    L.scatter_mode = SCATTER_GENERIC;  // the row / tile kernels write unit-stride output rows
  } else if (S.tile_a == nd - 1) {
    L.scatter_mode = SCATTER_ROWS;
  } else if (!S.shuffle && (S.es == 1 || S.es == 2 || S.es == 4 || S.es == 8)) {
    L.scatter_mode = SCATTER_TILED;
  } else {
    L.scatter_mode = SCATTER_GENERIC;
  }
  uint64_t max_sel[ZG_MAXD] = {0};  // the largest selection extent of any item along each axis sizes the grid
  for (size_t i = 0; i < L.items.size(); i++)
    for (uint32_t d = 0; d < nd; d++) max_sel[d] = std::max(max_sel[d], L.geom[(i * 3 + 1) * nd + d]);
  L.scatter_units = L.items.empty() ? 0 : scatter_units_per_item(L.scatter_mode, S, max_sel);
  if (L.scatter_mode == SCATTER_TILED && !L.items.empty()) {
    L.origin.resize(L.items.size());
    L.tiled_p = tiled_persistent_params(S, L.geom.data(), L.items.size(), L.tiled_q, L.origin.data()) &&
                L.tiled_q.upi == L.scatter_units && tiled_persistent_fits(L.items.size(), L.tiled_q.upi);
    if (!L.tiled_p) L.origin.clear();
  }
  L.first_path = L.tiled_p ? ZGPU_SCATTER_TILED_PERSISTENT : L.scatter_mode;
}

bool last_stage_is(const PlanLayout &L, StageKind k) { return !L.stages.empty() && L.stages.back().kind == k; }

// What blosc and gzip share to write whole chunks into the output themselves: the rows scatter would
// copy the decoded bytes unchanged (no swap / shuffle / transpose) into 16-B aligned output rows.
// pow2_mid: the row axes but the outermost and the innermost must have power-of-two extents (gzip).
bool rows_copy_unchanged(const PlanLayout &L, bool pow2_mid) {
  const ZgScatter &S = L.scatter;
  const int nd = (int)S.nd;
  if (L.scatter_mode != SCATTER_ROWS || S.swap || S.shuffle || !S.nelem || S.out_stride[nd - 1] != 1) return false;
  uint64_t st = 1;
  for (int a = nd - 1; a >= 0; a--) {
    if (S.enc_stride[a] != st || (a != nd - 1 && (S.out_stride[a] * S.es) % 16)) return false;
    if (pow2_mid && a != 0 && a != nd - 1 && (S.chunk_shape[a] & (S.chunk_shape[a] - 1))) return false;
    st *= S.chunk_shape[a];
  }
  return true;
}

// blosc as the last stage feeding the rows scatter unchanged, every decoded item a whole chunk on
// 16-B aligned output rows: k_blosc_finish writes the rows itself
bool blosc_direct(const PlanLayout &L, const LayoutKnobs &knobs) {
  const ZgScatter &S = L.scatter;
  const uint32_t nd = S.nd;
  if (!last_stage_is(L, ST_BLOSC) || !rows_copy_unchanged(L, false) || (S.chunk_shape[nd - 1] * S.es) % 16) return false;
  for (size_t i = 0; i < L.items.size(); i++) {
    if (L.items[i].flags & ZG_ITEM_FILL) continue;
    const uint64_t *g = L.geom.data() + i * 3 * nd;
    for (uint32_t d = 0; d < nd; d++)
      if (g[d] != 0 || g[nd + d] != S.chunk_shape[d]) return false;
    if ((g[2 * nd + nd - 1] * S.es) % 16) return false;
  }
  return !knobs.blosc_no_direct;
}

// gzip as the last stage feeding the rows scatter unchanged, rows of a power-of-two multiple of 16
// bytes, the row axes but the outermost of power-of-two extent: k_gzip writes the items whose selection
// is their whole chunk into the output rows itself and the scatter takes only the others (C3: the
// subset's 12,167 interior inner chunks of 15,625).
void gzip_direct(PlanLayout &L, const LayoutKnobs &knobs) {
  const ZgScatter &S = L.scatter;
  const uint32_t nd = S.nd;
  const uint64_t Lb = S.chunk_shape[nd - 1] * S.es;
  L.gz_direct = knobs.gzip_direct && last_stage_is(L, ST_GZIP) && nd <= 3 && Lb >= 16 && (Lb & (Lb - 1)) == 0 &&
                (nd < 2 || S.out_stride[0] * S.es < (1ull << 32)) && S.nelem * S.es < (1ull << 32) &&
                rows_copy_unchanged(L, true);
  if (!L.gz_direct) return;
  L.gz.want = S.nelem * S.es;
  L.gz.nd = nd;
  L.gz.lbs = (uint32_t)__builtin_ctzll(Lb);
  for (uint32_t d = 0; d < nd; d++) {
    L.gz.cshape[d] = S.chunk_shape[d];
    L.gz.ostr[d] = S.out_stride[d] * S.es;
  }
}

// blosc feeding the scatter directly (its decoded bytes are the chunk's encoded-layout elements; a
// fused unshuffle would interleave planes): a partial selection needs only the byte range between
// its first and last element in the encoded layout, so only the blocks that cover it are decoded,
// as the reference's blosc partial decoder does (blosc_partial_decoder.rs:33-60 ->
// blosc_decompress_bytes_partial, c-blosc's blosc_getitem)
void blosc_need(PlanLayout &L, const LayoutKnobs &knobs) {
  const ZgScatter &S = L.scatter;
  const uint32_t nd = S.nd;
  if (!last_stage_is(L, ST_BLOSC) || S.shuffle || knobs.blosc_no_partial) return;
  bool any = false;
  L.bl_need.assign(2 * L.items.size(), 0);
  for (size_t i = 0; i < L.items.size(); i++) {
    L.bl_need[2 * i + 1] = UINT64_MAX;
    if (!(L.items[i].flags & ZG_ITEM_PARTIAL)) continue;
    const uint64_t *g = L.geom.data() + i * 3 * nd;
    uint64_t lo = 0, hi = 0;
    bool empty = false;
    for (uint32_t d = 0; d < nd; d++) {
      if (!g[nd + d]) empty = true;
      lo += g[d] * S.enc_stride[d];
      hi += (g[d] + g[nd + d] - 1) * S.enc_stride[d];
    }
    if (empty) continue;
    L.bl_need[2 * i] = lo * S.es;
    L.bl_need[2 * i + 1] = (hi + 1) * S.es;
    any = true;
  }
  if (!any) L.bl_need.clear();
}

}  // namespace

PlanLayout plan_layout(const Chain &top, bool validate, uint32_t nd, const zgpu_chunk_desc *descs, uint64_t n,
                       const uint64_t *out_shape, const LayoutKnobs &knobs) {
  const Levels V = resolve_levels(top, nd, descs, n);
  PlanLayout L;
  L.item_desc_status.assign(n, 0);
  L.leaf = V.leaf;
  L.sharded = V.sharded;
  L.nested = V.mid != nullptr;
  for (uint64_t i = 0; i < n; i++) {
    const zgpu_chunk_desc &D = descs[i];
    bool full;
    if (!desc_ok(V, D, out_shape, full)) {
      L.item_desc_status[i] = ZGPU_INVALID_ARGUMENT;
      continue;
    }
    uint64_t vol = 1;
    for (uint32_t d = 0; d < nd; d++) vol *= D.sel_shape[d];
    if (vol == 0 && (!full || V.sharded)) continue;  // a zero-extent full chunk still runs its checks
    L.alg_bytes_static += vol * top.es;
    if (V.sharded) L.item_desc_status[i] = add_shard_items(L, V, D, i, full);
    else add_plain_item(L, nd, D, i, full);
  }
  if (V.sharded) {
    L.ispec = index_spec(top.a2b, L.ispec.n_inner, validate);
    for (const ZgShard &sh : L.shards)
      if (sh.ptr) L.alg_bytes_static += L.ispec.index_bytes;
    if (V.mid) {
      L.ispec2 = index_spec(V.mid->a2b, V.n_inner2, validate);
      for (const ZgItem &m : L.mids)
        if (!(m.flags & ZG_ITEM_FILL)) L.alg_bytes_static += L.ispec2.index_bytes;
    }
  }
  build_leaf_stages(L, *V.leaf, V.nelem, knobs);
  scatter_params(L, V, out_shape);
  scatter_mode(L, V);
  L.bl_direct = blosc_direct(L, knobs);
  gzip_direct(L, knobs);
  blosc_need(L, knobs);
  return L;
}

}  // namespace zgpu
