// libzgpu: the write path -- CodecChain::encode on the GPU and the encoded-size queries of the C ABI.
// Every decision is the layout's (encode_layout.hpp: the path, the refusals, the stages with their bounds
// and parameters, the slot geometry, the sharding and packbits geometry); the functions here execute
// one: they check the destinations against its size, allocate, copy and launch.
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
#include "encode_layout.hpp"
#include "kernels/launch.hpp"
#include "plan.hpp"

using namespace zgpu;

extern "C" {

// Encoded size of one chunk for a fixed-size chain (BytesRepresentation::FixedSize), -1 if variable.
int64_t zgpu_chain_encoded_size(const zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape) {
  if (!ch || !chunk_shape || nd == 0 || nd > ZGPU_MAX_DIMS) return -1;
  return chain_fixed_encoded_size(*ch->chain, volume(chunk_shape, nd));
}

// Upper bound of one chunk's encoded size (encoded_bound, encode_layout.hpp); -1 if unbounded.
int64_t zgpu_chain_encoded_bound(const zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape) {
  if (!ch || !chunk_shape || nd == 0 || nd > ZGPU_MAX_DIMS) return -1;
  return encoded_bound(*ch->chain, nd, chunk_shape);
}

}  // extern "C"

// The gather's parameters: the chain's transposes and bytes endianness, the layout's fused shuffle,
// chunk data at its data_off bytes into each destination.
static ZgEncode encode_params(const EncodeLayout &L, uint32_t nd, const uint64_t *chunk_shape,
                              const uint64_t *array_shape) {
  const Chain &c = *L.chain;
  ZgEncode P{};
  P.nd = nd;
  P.es = c.es;
  P.comp = c.comp;
  P.swap = (c.a2b.big_endian && c.comp > 1) ? 1 : 0;
  P.shuffle = L.shuffle;
  P.nelem = L.nelem;
  P.data_off = L.data_off;
  uint32_t m[ZG_MAXD];
  composed_axes(c, nd, m);
  uint64_t stride = 1;
  for (int d = (int)nd - 1; d >= 0; d--) {
    P.array_shape[d] = array_shape[d];
    P.array_stride[d] = stride;
    stride *= array_shape[d];
  }
  for (uint32_t a = 0; a < nd; a++) {
    P.dec_axis[a] = m[a];
    P.enc_shape[a] = chunk_shape[m[a]];
  }
  {
    uint64_t es_ = 1;
    for (int a = (int)nd - 1; a >= 0; a--) {
      P.enc_stride_of_dec[m[a]] = es_;
      es_ *= P.enc_shape[a];
    }
    for (uint32_t d = 0; d < nd; d++) P.dec_shape[d] = chunk_shape[d];
    // tiled encode: the axis (other than the encoded and the array innermost) with the smallest
    // encoded stride, so the TJ slabs of a block are adjacent encoded rows
    P.tile_b = ZG_MAXD;
    for (uint32_t d = 0; d + 1 < nd; d++) {
      if (d == m[nd - 1]) continue;
      if (P.tile_b == ZG_MAXD || P.enc_stride_of_dec[d] < P.enc_stride_of_dec[P.tile_b]) P.tile_b = d;
    }
  }
  std::memcpy(P.fill, c.fill, sizeof(P.fill));
  P.aligned = 0;
  return P;
}

void checksums_in_place(const uint64_t *d_dst, uint32_t n, const EncodeLayout &L, hipStream_t s) {
  for (const EncodeStage &st : L.stages) {
    if (st.kind == ST_CRC32C)
      HIPCHK(launch_crc32c_encode(d_dst, n, st.lo, st.in_bound, st.at_start, s));
    else
      HIPCHK(launch_linsum_encode(st.kind == ST_ADLER32 ? CK_ADLER32 : CK_FLETCHER32, d_dst, n, st.lo, st.in_bound,
                                  st.at_start, s));
  }
}

// An ENC_FIXED layout (CodecChain::encode, codec_chain.rs:528-555, of a fixed-size chain) for n chunks of
// a device array into the device buffers h_tab[0..n) (chunk origins h_tab[n + i*nd..]): one gather
// (transposes + endianness + innermost shuffle, fill past the array edge), then the checksums in place.
// Enqueues only (no synchronisation); *d_tab_out: the device copy of h_tab.
static void encode_fixed(const EncodeLayout &L, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                         const uint64_t *array_shape, const std::vector<uint64_t> &h_tab, uint64_t n, Scratch &sc,
                         hipStream_t s, ZgEncode *out_P = nullptr, const uint64_t **d_tab_out = nullptr) {
  ZgEncode P = encode_params(L, nd, chunk_shape, array_shape);
  bool aligned = (P.data_off % P.es) == 0;
  for (uint64_t i = 0; i < n; i++)
    if (h_tab[i] % 16) aligned = false;
  P.aligned = aligned;
  if (out_P) *out_P = P;
  if (!n) return;
  uint64_t *d = sc.dev<uint64_t>(h_tab.size());
  if (d_tab_out) *d_tab_out = d;
  HIPCHK(hipMemcpyAsync(d, h_tab.data(), h_tab.size() * 8, hipMemcpyHostToDevice, s));
  HIPCHK(launch_encode_gather(d, d + n, (const uint8_t *)array, P, (uint32_t)n, s));
  checksums_in_place(d, (uint32_t)n, L, s);
}

// An ENC_VAR layout (a chain with a compressor) for n chunks whose origins are origins[i*nd..]: the
// gather into pool 0's slots, then the stages in metadata order over the items {src, len}: checksums
// appended / prepended in place, a compressor into the pool the layout names. Enqueues only; on return
// the device item table and statuses describe every chunk's encoded bytes (inside `sc`), and *d_tab_out
// is the device table [n gather destinations | n*nd origins].
static void encode_var(const EncodeLayout &L, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                       const uint64_t *array_shape, const uint64_t *origins, uint64_t n, Scratch &sc, hipStream_t s,
                       ZgItem **d_items_out, uint32_t **d_status_out, uint64_t **d_tab_out, ZgEncode *P_out) {
  const uint64_t HR = L.headroom, pitch = L.pitch;
  uint8_t *pool[2] = {nullptr, nullptr};
  for (int p = 0; p < L.n_pools; p++) pool[p] = sc.dev<uint8_t>(std::max<uint64_t>(n * pitch, 1));
  std::vector<uint64_t> tab(n * (1 + nd));
  for (uint64_t i = 0; i < n; i++) tab[i] = (uint64_t)(pool[0] + i * pitch + HR);
  std::memcpy(tab.data() + n, origins, n * nd * 8);
  uint64_t *d_tab = sc.dev<uint64_t>(std::max<size_t>(tab.size(), 1));
  HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
  ZgEncode P = encode_params(L, nd, chunk_shape, array_shape);
  P.aligned = (P.es <= 16 && (HR % 16) == 0 && (pitch % 16) == 0) ? 1u : 0u;
  if (n) HIPCHK(launch_encode_gather(d_tab, d_tab + n, (const uint8_t *)array, P, (uint32_t)n, s));
  // items over the gathered chunks
  std::vector<ZgItem> items(n);
  for (uint64_t i = 0; i < n; i++) items[i] = ZgItem{tab[i], L.data_bytes, (uint32_t)i, 0, 0, 0};
  ZgItem *d_items = sc.dev<ZgItem>(std::max<uint64_t>(n, 1));
  uint32_t *d_status = sc.dev<uint32_t>(std::max<uint64_t>(n, 1));
  HIPCHK(hipMemcpyAsync(d_items, items.data(), n * sizeof(ZgItem), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(d_status, 0, std::max<uint64_t>(n * 4, 4), s));
  uint32_t *sym = nullptr;
  for (const EncodeStage &st : L.stages) {
    switch (st.kind) {
      case ST_CRC32C: HIPCHK(launch_crc32c_items(d_items, d_status, (uint32_t)n, st.at_start, s)); break;
      case ST_ADLER32:
      case ST_FLETCHER32:
        HIPCHK(launch_linsum_items(st.kind == ST_ADLER32 ? CK_ADLER32 : CK_FLETCHER32, d_items, d_status, (uint32_t)n,
                                   st.at_start, s));
        break;
      case ST_GZIP:
      case ST_ZLIB:
        if (!sym) sym = sc.dev<uint32_t>((uint64_t)gzip_encode_grid((uint32_t)std::max<uint64_t>(n, 1)) * GZE_BLK_SYMS);
        HIPCHK(launch_gzip_encode(d_items, d_status, (uint32_t)n, pool[st.pool], pitch, sym, st.level, s, st.zlib,
                                  st.zlib_bounded));
        break;
      case ST_ZSTD: {
        uint8_t *zscr = sc.dev<uint8_t>(zstd_encode_scratch((uint32_t)n, st.in_bound));
        HIPCHK(launch_zstd_encode(d_items, d_status, (uint32_t)n, st.in_bound, pool[st.pool], pitch, zscr,
                                  st.zstd_checksum ? 1 : 0, s));
        break;
      }
      default: {  // ST_BLOSC: blosclz / lz4 / lz4hc / snappy / zlib / zstd streams on the GPU
        const BloscEnc E = blosc_enc_params(st.bl_comp, st.bl_shuffle, st.bl_typesize, st.in_bound, st.bl_blocksize);
        uint8_t *bscr = sc.dev<uint8_t>(blosc_encode_scratch(E, (uint32_t)n));
        HIPCHK(launch_blosc_encode(d_items, d_status, (uint32_t)n, E, pool[st.pool], pitch, bscr, st.level, s));
      }
    }
  }
  *d_items_out = d_items;
  *d_status_out = d_status;
  if (d_tab_out) *d_tab_out = d_tab;
  if (P_out) *P_out = P;
}

// first non-zero of n device statuses (read back synchronously), 0 if none
static int first_status(const uint32_t *d_status, uint64_t n, hipStream_t s) {
  std::vector<uint32_t> h(n);
  if (n) HIPCHK(hipMemcpyAsync(h.data(), d_status, n * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (uint32_t v : h)
    if (v) return (int)v;
  return 0;
}

static int check_destinations(const zgpu_encode_desc *descs, uint64_t n, uint64_t size) {
  for (uint64_t i = 0; i < n; i++)
    if (!descs[i].dst || descs[i].dst_cap < size)
      return set_err(ZGPU_INVALID_ARGUMENT, "encode: destination missing or smaller than the encoded size or bound");
  return ZGPU_OK;
}

// An ENC_FIXED or ENC_VAR layout to the descriptors' destinations, synchronous; the lengths to enc_lens.
// ENC_VAR: encode_var, then every chunk copied to its destination.
static int encode_plain(const EncodeLayout &L, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                        const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint64_t *enc_lens,
                        Scratch &sc, hipStream_t s) {
  std::vector<uint64_t> tab(n * (1 + nd)), dc(2 * n);  // [destinations | origins], [destinations | capacities]
  for (uint64_t i = 0; i < n; i++) {
    tab[i] = dc[i] = (uint64_t)descs[i].dst;
    dc[n + i] = descs[i].dst_cap;
    for (uint32_t d = 0; d < nd; d++) tab[n + i * nd + d] = descs[i].chunk_start[d];
  }
  if (L.path == ENC_FIXED) {
    encode_fixed(L, nd, chunk_shape, array, array_shape, tab, n, sc, s);
    HIPCHK(hipStreamSynchronize(s));  // the table is read by encode_fixed's copy
    if (enc_lens)
      for (uint64_t i = 0; i < n; i++) enc_lens[i] = L.size;
    return ZGPU_OK;
  }
  ZgItem *items = nullptr;
  uint32_t *st = nullptr;
  encode_var(L, nd, chunk_shape, array, array_shape, tab.data() + n, n, sc, s, &items, &st, nullptr, nullptr);
  uint64_t *d_dc = sc.dev<uint64_t>(3 * n);
  HIPCHK(hipMemcpyAsync(d_dc, dc.data(), 16 * n, hipMemcpyHostToDevice, s));
  HIPCHK(launch_encode_place(items, st, d_dc, d_dc + n, d_dc + 2 * n, (uint32_t)n, s));
  std::vector<uint64_t> lens(n);
  HIPCHK(hipMemcpyAsync(lens.data(), d_dc + 2 * n, 8 * n, hipMemcpyDeviceToHost, s));
  const int rc = first_status(st, n, s);
  if (rc) return set_err(rc, std::string("encode: ") + zgpu_status_name(rc));
  if (enc_lens) std::memcpy(enc_lens, lens.data(), 8 * n);
  return ZGPU_OK;
}

ShardTables shard_tables(Scratch &sc, const EncodeLayout &L, const uint64_t *h_dst, uint64_t n, uint64_t n_chunks,
                         uint64_t nf_words, uint64_t E, uint64_t E_pitch, hipStream_t s) {
  ShardTables T{};
  T.dst = sc.dev<uint64_t>(3 * n + n_chunks);
  T.nf = sc.dev<uint32_t>(nf_words);
  HIPCHK(hipMemcpyAsync(T.dst, h_dst, 8 * n, hipMemcpyHostToDevice, s));
  T.index_ptr = T.dst + n;
  T.len = T.dst + 2 * n;
  T.off = T.dst + 3 * n;
  T.A = ZgShardLayoutArgs{L.n_inner, E, E_pitch, L.index->size, L.index->data_off, L.index_at_start ? 1u : 0u,
                          L.index_big_endian ? 1u : 0u};
  return T;
}

// sharding_indexed (ShardingCodecBound::encode_bounded, sharding_codec.rs:924-1085, SubchunkWriteOrder::
// C): all inner chunks of all shards encoded in one batch (into temporary slots by encode_fixed, or by
// encode_var), all-fill inner chunks omitted, the rest laid out in C order with the encoded index at the
// start or the end, the index checksums; shard lengths to enc_lens.
static int encode_sharded(const EncodeLayout &L, uint32_t nd, const void *array, const uint64_t *array_shape,
                          const zgpu_encode_desc *descs, uint64_t n, uint64_t *enc_lens, Scratch &sc, hipStream_t s) {
  const EncodeLayout &I = *L.inner;
  const uint64_t *inner_shape = L.chain->a2b.inner_shape.data();
  const uint64_t n_chunks = n * L.n_inner;
  // inner chunk k of shard i: its origin in the array
  std::vector<uint64_t> org(n_chunks * nd), hd(n);
  uint64_t cap = UINT64_MAX;
  for (uint64_t i = 0; i < n; i++) {
    hd[i] = (uint64_t)descs[i].dst;
    cap = std::min(cap, descs[i].dst_cap);
    for (uint64_t k = 0; k < L.n_inner; k++) {
      uint64_t rem = k;
      for (int d = (int)nd - 1; d >= 0; d--) {
        org[(i * L.n_inner + k) * nd + d] = descs[i].chunk_start[d] + (rem % L.cps[d]) * inner_shape[d];
        rem /= L.cps[d];
      }
    }
  }
  ZgEncode IP{};
  ShardTables T{};
  ZgItem *items = nullptr;
  uint32_t *st = nullptr, *d_shst = nullptr;
  if (L.path == ENC_SHARD_VAR) {
    uint64_t *d_tab = nullptr;
    encode_var(I, nd, inner_shape, array, array_shape, org.data(), n_chunks, sc, s, &items, &st, &d_tab, &IP);
    // (A.E_pitch: a shard destination's capacity; the shard statuses behind the fill flags)
    T = shard_tables(sc, L, hd.data(), n, n_chunks, std::max<uint64_t>(n_chunks, 1) + n, 0, cap, s);
    d_shst = T.nf + n_chunks;
    HIPCHK(launch_shard_encode_var(d_tab + n_chunks, (const uint8_t *)array, IP, (uint32_t)n_chunks, T.nf, items, st, T.A,
                                   T.dst, T.off, T.index_ptr, T.len, d_shst, (uint32_t)n, s));
  } else {
    uint8_t *tmp = sc.dev<uint8_t>(std::max<uint64_t>(n_chunks * L.pitch, 1));
    std::vector<uint64_t> tab(n_chunks * (1 + nd));  // [dst slots | origins]
    for (uint64_t g = 0; g < n_chunks; g++) tab[g] = (uint64_t)(tmp + g * L.pitch);
    std::memcpy(tab.data() + n_chunks, org.data(), org.size() * 8);
    const uint64_t *d_tab = nullptr;
    encode_fixed(I, nd, inner_shape, array, array_shape, tab, n_chunks, sc, s, &IP, &d_tab);
    T = shard_tables(sc, L, hd.data(), n, n_chunks, std::max<uint64_t>(n_chunks, 1), I.size, L.pitch, s);
    HIPCHK(launch_shard_encode(d_tab + n_chunks, (const uint8_t *)array, IP, (uint32_t)n_chunks, T.nf, tmp, T.A, T.dst,
                               T.off, T.index_ptr, T.len, (uint32_t)n, s));
  }
  checksums_in_place(T.index_ptr, (uint32_t)n, *L.index, s);
  HIPCHK(hipMemcpyAsync(enc_lens, T.len, 8 * n, hipMemcpyDeviceToHost, s));
  if (L.path == ENC_SHARD_FIXED) return ZGPU_OK;
  int rc = first_status(st, n_chunks, s);
  if (!rc) rc = first_status(d_shst, n, s);
  if (rc) return set_err(rc == 1 ? ZGPU_HIP_ERROR : rc, std::string("encode: ") + zgpu_status_name(rc));
  return ZGPU_OK;
}

// packbits as the array->bytes codec (unsharded): the chunks are gathered (and transposed) as native
// elements into temporary slots (L.native), k_packbits packs each slot, and the packed chunks, a 1-D
// uint8 array of one slot per chunk, go through L.packed to their destinations (straight into them
// without bytes->bytes codecs).
static int encode_packbits(const EncodeLayout &L, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                           const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint64_t *enc_lens,
                           Scratch &sc, hipStream_t s) {
  const Codec &pb = L.chain->a2b;
  uint8_t *U = sc.dev<uint8_t>(std::max<uint64_t>(n * L.upitch, 1));
  uint8_t *Pk = L.direct ? nullptr : sc.dev<uint8_t>(std::max<uint64_t>(n * L.ppitch, 1));
  std::vector<uint64_t> tab(n * (1 + nd)), ptab(2 * n);
  for (uint64_t i = 0; i < n; i++) {
    tab[i] = ptab[i] = (uint64_t)(U + i * L.upitch);
    for (uint32_t d = 0; d < nd; d++) tab[n + i * nd + d] = descs[i].chunk_start[d];
    ptab[n + i] = L.direct ? (uint64_t)descs[i].dst : (uint64_t)(Pk + i * L.ppitch);
  }
  encode_fixed(*L.native, nd, chunk_shape, array, array_shape, tab, n, sc, s);
  uint64_t *d_ptab = sc.dev<uint64_t>(ptab.size());
  HIPCHK(hipMemcpyAsync(d_ptab, ptab.data(), ptab.size() * 8, hipMemcpyHostToDevice, s));
  ZgPackBits P{};
  P.nelem = L.nelem;
  P.packed_len = L.packed_len;
  P.ncomp = pb.pb_ncomp;
  P.comp_bytes = L.chain->enc_es / pb.pb_ncomp;
  P.first = pb.pb_first;
  P.ext = pb.pb_last - pb.pb_first + 1;
  P.sign = pb.pb_signed ? 1 : 0;
  P.padding = (uint32_t)pb.pb_padding;
  HIPCHK(launch_packbits(d_ptab, (uint32_t)n, P, s));
  if (L.direct) {
    HIPCHK(hipStreamSynchronize(s));  // ptab is read by the copy above
    for (uint64_t i = 0; i < n; i++) enc_lens[i] = L.packed_len;
    return ZGPU_OK;
  }
  // the packed chunks as chunk i = [i * ppitch, i * ppitch + packed_len) of a 1-D uint8 array
  const uint64_t p_shape[1] = {n * L.ppitch}, p_chunk[1] = {L.packed_len};
  std::vector<zgpu_encode_desc> pd(descs, descs + n);
  for (uint64_t i = 0; i < n; i++) pd[i].chunk_start[0] = i * L.ppitch;
  return encode_plain(*L.packed, 1, p_chunk, Pk, p_shape, pd.data(), n, enc_lens, sc, s);
}

static int check_origins(uint32_t nd, const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    for (uint32_t d = 0; d < nd; d++)
      if (descs[i].chunk_start[d] >= array_shape[d])
        return set_err(ZGPU_INVALID_ARGUMENT, "encode: chunk origin outside the array");
  return ZGPU_OK;
}

// zgpu_encode_chunks (arguments checked) on stream s of the caller's lane: n chunks of the device array to their device
// destinations, synchronous (the temporaries go back when it returns). The chain's refusals (ChainError, from
// encode_layout) leave before any device work; fixed_only: so does a chain whose chunks vary in length.
int encode_chunks_on(zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                     const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint64_t *enc_lens,
                     hipStream_t s, bool fixed_only) {
  if (!n) return ZGPU_OK;
  Scratch sc(ch->ctx, s);
  // value codecs (numcodecs.fixedscaleoffset, bitround) work element by element, so they commute with
  // chunking and sharding: the caller's array is converted once into a device array of the innermost
  // encoded type, which the chain without them, retyped, encodes (strip_value_codecs)
  std::shared_ptr<Chain> stripped;
  std::vector<Codec> steps;
  if (chain_has_value_codec(*ch->chain)) {
    stripped = strip_value_codecs(*ch->chain, steps);
    retype_stripped(*stripped, *ch->chain);
  }
  const EncodeLayout L = encode_layout(stripped ? *stripped : *ch->chain, nd, chunk_shape);
  if (fixed_only && !L.fixed)
    return set_err(ZGPU_INVALID_ARGUMENT, "encode: the chain's chunks have variable lengths: zgpu_encode_chunks");
  if (const int rc = check_destinations(descs, n, L.size)) return rc;
  if (stripped) {
    // the encode entries carry no per-chunk status: an element cast_value cannot cast fails the call
    const Codec *fallible = nullptr;
    for (const Codec &k : steps)
      if (k.kind == CodecKind::CastValue && cast_encode_fallible(k)) fallible = &k;
    uint64_t *d_fail = nullptr;
    if (fallible) {
      d_fail = sc.dev<uint64_t>(1);
      HIPCHK(hipMemsetAsync(d_fail, 0xff, 8, s));
    }
    array = value_encode_elements(steps, (const uint8_t *)array, volume(array_shape, nd), sc, s, d_fail);
    if (fallible) {
      uint64_t first = UINT64_MAX;
      HIPCHK(hipMemcpyAsync(&first, d_fail, 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (first != UINT64_MAX)
        return set_err(ZGPU_CAST_NOT_REPRESENTABLE, "encode: cast_value: element " + std::to_string(first) +
                                                        " of the array is not representable in the encoded data type");
    }
  }
  if (L.path == ENC_FIXED) return encode_plain(L, nd, chunk_shape, array, array_shape, descs, n, enc_lens, sc, s);
  uint64_t *hl = sc.pinned<uint64_t>(n);  // the variable lengths, read back by the callee
  const int rc = L.path == ENC_PACKBITS ? encode_packbits(L, nd, chunk_shape, array, array_shape, descs, n, hl, sc, s)
                 : L.path == ENC_VAR    ? encode_plain(L, nd, chunk_shape, array, array_shape, descs, n, hl, sc, s)
                                        : encode_sharded(L, nd, array, array_shape, descs, n, hl, sc, s);
  HIPCHK(hipStreamSynchronize(s));
  if (!rc && enc_lens) std::memcpy(enc_lens, hl, 8 * n);
  return rc;
}

static int encode_chunks_checked(zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                                 const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint32_t flags,
                                 uint64_t *enc_lens, void *stream, bool fixed_only) {
  ABI_GUARD_BEGIN
  if (!ch || !chunk_shape || !array || !array_shape || (n && !descs))
    return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  if ((flags & (ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE)) != (ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE))
    return set_err(ZGPU_INVALID_ARGUMENT, "encode: array and destinations must be device memory");
  if (const int rc = check_origins(nd, array_shape, descs, n)) return rc;
  HIPCHK(hipSetDevice(ch->ctx->device));
  LaneScope ls(ch->ctx);
  return encode_chunks_on(ch, nd, chunk_shape, array, array_shape, descs, n, enc_lens, pick_stream(ls.L, stream),
                          fixed_only);
  ABI_GUARD_END
}

extern "C" {

int zgpu_encode_chunks(zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                       const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint32_t flags,
                       uint64_t *enc_lens, void *stream) {
  return encode_chunks_checked(ch, nd, chunk_shape, array, array_shape, descs, n, flags, enc_lens, stream, false);
}

// One chunk (or shard) from host bytes, encoded on the GPU, the encoded bytes left in pooled pinned
// memory for the caller to copy (the plugin's CodecChain::encode / ShardingCodecBound::encode).
int zgpu_encode_pinned(zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape, const void *decoded,
                       const void **enc, uint64_t *enc_len, zgpu_result **result) {
  ABI_GUARD_BEGIN
  if (enc) *enc = nullptr;
  if (result) *result = nullptr;
  if (!ch || !chunk_shape || !decoded || !enc || !enc_len || !result)
    return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  zgpu_ctx *C = ch->ctx;
  HIPCHK(hipSetDevice(C->device));
  const int64_t bound = zgpu_chain_encoded_bound(ch, nd, chunk_shape);
  if (bound < 0) return set_err(ZGPU_UNSUPPORTED, "encode: the chain's encoded size is not bounded");
  const uint64_t nbytes = volume(chunk_shape, nd) * ch->chain->es;
  std::unique_ptr<zgpu_result> R(new zgpu_result());
  ctx_ref(C);
  R->ctx = C;
  LaneScope ls(C);  // one lane for the upload, the encode and the read-back
  hipStream_t s = pick_stream(ls.L, nullptr);
  Scratch sc(C, s);
  uint8_t *d_in = sc.dev<uint8_t>(nbytes ? nbytes : 1);
  uint8_t *d_out = sc.dev<uint8_t>(bound ? (uint64_t)bound : 1);
  HIPCHK(hipMemcpyAsync(d_in, decoded, nbytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  zgpu_encode_desc D{};
  D.dst = d_out;
  D.dst_cap = (uint64_t)bound;
  uint64_t len = 0;
  if (const int rc = check_origins(nd, chunk_shape, &D, 1)) return rc;
  const int rc = encode_chunks_on(ch, nd, chunk_shape, d_in, chunk_shape, &D, 1, &len, s);
  if (rc) return rc;
  R->own = (uint8_t *)C->host_alloc(len ? len : 1);
  HIPCHK(hipMemcpyAsync(R->own, d_out, len, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *enc = R->own;
  *enc_len = len;
  *result = R.release();
  return ZGPU_OK;
  ABI_GUARD_END
}

int zgpu_encode_batch(zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                      const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint32_t flags,
                      void *hip_stream) {
  return encode_chunks_checked(ch, nd, chunk_shape, array, array_shape, descs, n, flags, nullptr, hip_stream, true);
}

}  // extern "C"
