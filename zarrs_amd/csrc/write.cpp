// libzgpu: the write path -- CodecChain::encode on the GPU and the encoded-size queries of the C ABI.
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

using namespace zgpu;

extern "C" {

// Encoded size of one chunk for a fixed-size chain (BytesRepresentation::FixedSize), -1 if variable.
int64_t zgpu_chain_encoded_size(const zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape) {
  if (!ch || !chunk_shape || nd == 0 || nd > ZGPU_MAX_DIMS) return -1;
  uint64_t n = 1;
  for (uint32_t d = 0; d < nd; d++) n *= chunk_shape[d];
  return chain_fixed_encoded_size(*ch->chain, n);
}

// Upper bound of one chunk's encoded size: the fixed size, a compressing chain's bounded size
// (chain_encoded_bound), or for sharding_indexed every inner chunk at its bound plus the index
// (ShardingCodec::encoded_shard_bounded_size, sharding_codec.rs:924-945, BytesRepresentation::
// BoundedSize); -1 if unbounded.
int64_t zgpu_chain_encoded_bound(const zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape) {
  if (!ch || !chunk_shape || nd == 0 || nd > ZGPU_MAX_DIMS) return -1;
  const Chain &c = *ch->chain;
  if (c.a2b.kind != CodecKind::Sharding) {
    uint64_t n = 1;
    for (uint32_t d = 0; d < nd; d++) n *= chunk_shape[d];
    return chain_encoded_bound(c, n);
  }
  for (const Codec &k : c.a2a)
    if (!is_value_codec(k.kind)) return -1;  // (value codecs keep the shape; encode strips them)
  if (!c.b2b.empty() || c.a2b.inner_shape.size() != nd) return -1;
  uint64_t n_inner = 1, inner_n = 1;
  for (uint32_t d = 0; d < nd; d++) {
    const uint64_t is = c.a2b.inner_shape[d];
    if (chunk_shape[d] % is) return -1;
    n_inner *= chunk_shape[d] / is;
    inner_n *= is;
  }
  const int64_t E = chain_encoded_bound(*c.a2b.inner, inner_n);
  const int64_t X = chain_fixed_encoded_size(*c.a2b.index, n_inner * 2);
  if (E < 0 || X < 0) return -1;
  return (int64_t)n_inner * E + X;
}

}  // extern "C"

// CodecChain::encode (codec_chain.rs:528-555) of a fixed-size chain for n chunks of a device array
// into device buffers h_dst[i] (chunk origins h_starts[i*nd..]): one gather (transposes + endianness +
// innermost shuffle, fill past the array edge), then one k_crc32c_encode launch per crc32c codec.
// Enqueues only (no synchronisation); *d_tab_out: the device copy of h_tab, n dst pointers + n*nd origins.
// The gather's parameters: the chain's transposes, bytes endianness and (shuffle) an innermost
// numcodecs.shuffle over the data type size, chunk data at data_off bytes into each destination.
static ZgEncode encode_params(const Chain &c, uint32_t nd, const uint64_t *chunk_shape, const uint64_t *array_shape,
                              bool shuffle, uint64_t data_off) {
  ZgEncode P{};
  P.nd = nd;
  P.es = c.es;
  P.comp = c.comp;
  P.swap = (c.a2b.big_endian && c.comp > 1) ? 1 : 0;
  P.shuffle = shuffle;
  P.nelem = 1;
  for (uint32_t d = 0; d < nd; d++) P.nelem *= chunk_shape[d];
  P.data_off = data_off;
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

static int encode_fixed(zgpu_ctx *C, const Chain &c, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                        const uint64_t *array_shape, const std::vector<uint64_t> &h_tab, uint64_t n, Scratch &sc,
                        hipStream_t s, ZgEncode *out_P = nullptr, const uint64_t **d_tab_out = nullptr) {
  if (c.a2b.kind != CodecKind::Bytes) return set_err(ZGPU_UNSUPPORTED, "encode: array->bytes codec must be bytes");
  for (const Codec &k : c.a2a)
    if (k.kind == CodecKind::Transpose && k.order.size() != nd) return set_err(ZGPU_INVALID_ARGUMENT, "transpose order rank != ndim");
  bool shuffle = false;
  int n_start = 0;
  for (size_t i = 0; i < c.b2b.size(); i++) {
    const Codec &k = c.b2b[i];
    if (k.kind == CodecKind::Shuffle && i == 0 && k.elementsize == c.es) shuffle = true;
    else if (is_checksum(k.kind)) n_start += k.at_start ? 1 : 0;
    else return set_err(ZGPU_UNSUPPORTED, "encode: only transpose / bytes / numcodecs.shuffle (innermost, "
                                          "elementsize = data type size) / crc32c / adler32 / fletcher32 / gzip run "
                                          "on the GPU write path");
  }
  ZgEncode P = encode_params(c, nd, chunk_shape, array_shape, shuffle, 4ull * n_start);
  bool aligned = (P.data_off % c.es) == 0;
  for (uint64_t i = 0; i < n; i++)
    if (h_tab[i] % 16) aligned = false;
  P.aligned = aligned;
  if (out_P) *out_P = P;
  if (!n) return ZGPU_OK;
  uint64_t *d = sc.dev<uint64_t>(h_tab.size());
  if (d_tab_out) *d_tab_out = d;
  HIPCHK(hipMemcpyAsync(d, h_tab.data(), h_tab.size() * 8, hipMemcpyHostToDevice, s));
  HIPCHK(launch_encode_gather(d, d + n, (const uint8_t *)array, P, (uint32_t)n, s));
  uint64_t lo = P.data_off, len = P.nelem * c.es;
  for (const Codec &k : c.b2b) {
    if (!is_checksum(k.kind)) continue;
    if (k.kind == CodecKind::Crc32c)
      HIPCHK(launch_crc32c_encode(d, (uint32_t)n, lo, len, k.at_start ? 1 : 0, s));
    else
      HIPCHK(launch_linsum_encode(k.kind == CodecKind::Adler32 ? CK_ADLER32 : CK_FLETCHER32, d, (uint32_t)n, lo, len,
                                  k.at_start ? 1 : 0, s));
    if (k.at_start) lo -= 4;
    len += 4;
  }
  return ZGPU_OK;
}

static bool chain_compresses(const Chain &c) {
  for (const Codec &k : c.b2b)
    if (k.kind == CodecKind::Gzip || k.kind == CodecKind::Zlib || k.kind == CodecKind::Zstd ||
        k.kind == CodecKind::Blosc || k.kind == CodecKind::Bz2)
      return true;
  return false;  // (bz2 is refused by encode_var: it has no encoder on the GPU)
}

// CodecChain::encode (codec_chain.rs:528-555) of a chain with a compressor, for n chunks whose origins
// are origins[i*nd..]: the gather (transposes, endianness, innermost shuffle) into 64 B-headroom
// slots, then the bytes->bytes codecs in metadata order over the items {src, len}: crc32c appended /
// prepended in place, gzip into the other slot pool (k_gzip_encode). Enqueues only; on return the
// device item table and statuses describe every chunk's encoded bytes (inside `sc`), and
// *d_tab_out is the device table [n gather destinations | n*nd origins].
static int encode_var(zgpu_ctx *C, const Chain &c, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                      const uint64_t *array_shape, const uint64_t *origins, uint64_t n, Scratch &sc,
                      hipStream_t s, ZgItem **d_items_out, uint32_t **d_status_out, uint64_t **d_tab_out,
                      ZgEncode *P_out) {
  if (c.a2b.kind != CodecKind::Bytes) return set_err(ZGPU_UNSUPPORTED, "encode: array->bytes codec must be bytes");
  for (const Codec &k : c.a2a)
    if (k.kind == CodecKind::Transpose && k.order.size() != nd) return set_err(ZGPU_INVALID_ARGUMENT, "transpose order rank != ndim");
  uint64_t nelem = 1;
  for (uint32_t d = 0; d < nd; d++) nelem *= chunk_shape[d];
  bool shuffle = false;
  uint64_t size = nelem * c.es, max_size = size;
  uint32_t n_crc = 0;
  for (size_t i = 0; i < c.b2b.size(); i++) {
    const Codec &k = c.b2b[i];
    if (k.kind == CodecKind::Shuffle && i == 0 && k.elementsize == c.es) {
      shuffle = true;
    } else if (is_checksum(k.kind)) {
      size += 4;
      n_crc++;
    } else if (k.kind == CodecKind::Gzip) {
      size = gzip_bound(size);
    } else if (k.kind == CodecKind::Zlib) {
      size = zlib_bound(size);  // k_gzip_encode keeps to it (zlib_bounded)
    } else if (k.kind == CodecKind::Zstd) {
      size = zstd_bound(size);
    } else if (k.kind == CodecKind::Blosc) {
      size += 16;
    } else if (k.kind == CodecKind::Bz2) {
      return set_err(ZGPU_UNSUPPORTED, "encode: numcodecs.bz2 is decode-only on the GPU");
    } else {
      return set_err(ZGPU_UNSUPPORTED, "encode: only transpose / bytes / numcodecs.shuffle (innermost, elementsize = "
                                       "data type size) / crc32c / adler32 / fletcher32 / gzip / zlib / zstd / blosc "
                                       "run on the GPU write path");
    }
    max_size = std::max(max_size, size);
  }
  if (n_crc > 14) return set_err(ZGPU_UNSUPPORTED, "encode: too many checksum codecs");
  constexpr uint64_t HR = 64;  // headroom in front of a slot's bytes (crc32c at the start)
  const uint64_t pitch = (HR + max_size + 4 * n_crc + 16 + 255) & ~(uint64_t)255;
  bool gz = false;  // a compressor: its output goes to the other slot pool
  for (const Codec &k : c.b2b)
    gz = gz || k.kind == CodecKind::Gzip || k.kind == CodecKind::Zlib || k.kind == CodecKind::Zstd ||
         k.kind == CodecKind::Blosc;
  uint8_t *pool[2] = {sc.dev<uint8_t>(std::max<uint64_t>(n * pitch, 1)), nullptr};
  if (gz) pool[1] = sc.dev<uint8_t>(std::max<uint64_t>(n * pitch, 1));
  // gather into pool 0
  std::vector<uint64_t> tab(n * (1 + nd));
  for (uint64_t i = 0; i < n; i++) tab[i] = (uint64_t)(pool[0] + i * pitch + HR);
  std::memcpy(tab.data() + n, origins, n * nd * 8);
  uint64_t *d_tab = sc.dev<uint64_t>(std::max<size_t>(tab.size(), 1));
  HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
  ZgEncode P = encode_params(c, nd, chunk_shape, array_shape, shuffle, 0);
  P.aligned = (c.es <= 16 && (HR % 16) == 0 && (pitch % 16) == 0) ? 1u : 0u;
  if (n) HIPCHK(launch_encode_gather(d_tab, d_tab + n, (const uint8_t *)array, P, (uint32_t)n, s));
  // items over the gathered chunks
  std::vector<ZgItem> items(n);
  for (uint64_t i = 0; i < n; i++) items[i] = ZgItem{tab[i], nelem * c.es, (uint32_t)i, 0, 0, 0};
  ZgItem *d_items = sc.dev<ZgItem>(std::max<uint64_t>(n, 1));
  uint32_t *d_status = sc.dev<uint32_t>(std::max<uint64_t>(n, 1));
  HIPCHK(hipMemcpyAsync(d_items, items.data(), n * sizeof(ZgItem), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(d_status, 0, std::max<uint64_t>(n * 4, 4), s));
  int cur = 0;
  uint32_t *sym = nullptr;
  uint8_t *zscr = nullptr;
  uint64_t in_size = nelem * c.es;  // the current stage's input bound
  bool var_len = false;             // an earlier stage made the lengths variable
  for (size_t i = 0; i < c.b2b.size(); i++) {
    const Codec &k = c.b2b[i];
    const uint64_t stage_in = in_size;
    if (k.kind == CodecKind::Blosc) {
      // BloscCodec::encode (blosc_codec_via_blosc_src.rs:113-128): blosclz / lz4 / lz4hc / zlib / zstd
      // streams on the GPU
      const uint32_t comp = (k.cname == "lz4" || k.cname == "lz4hc") ? (uint32_t)BL_COMP_LZ4
                            : k.cname == "zstd"                       ? (uint32_t)BL_COMP_ZSTD
                            : k.cname == "blosclz"                    ? (uint32_t)BL_COMP_BLOSCLZ
                            : k.cname == "zlib"                       ? (uint32_t)BL_COMP_ZLIB
                            : k.cname == "snappy"                     ? (uint32_t)BL_COMP_SNAPPY
                                                                      : UINT32_MAX;
      if (comp == UINT32_MAX)
        return set_err(ZGPU_UNSUPPORTED, "encode: blosc cname '" + k.cname +
                                             "' (the GPU writes blosclz, lz4, lz4hc, snappy, zlib and zstd)");
      if (var_len) return set_err(ZGPU_UNSUPPORTED, "encode: blosc after a variable-length codec");
      const uint32_t ts = std::max<uint32_t>(1, k.elementsize);
      const int sh = k.shuffle >= 0 ? k.shuffle : (k.elementsize > 0 ? 2 : 0);  // zarrs' default (:119-123)
      const BloscEnc E = blosc_enc_params(comp, (uint32_t)sh, ts, stage_in, k.blocksize);
      uint8_t *bscr = sc.dev<uint8_t>(blosc_encode_scratch(E, (uint32_t)n));
      cur ^= 1;
      HIPCHK(launch_blosc_encode(d_items, d_status, (uint32_t)n, E, pool[cur], pitch, bscr, k.level, s));
      in_size += 16;
      var_len = true;
      continue;
    }
    if (k.kind == CodecKind::Gzip || k.kind == CodecKind::Zlib || k.kind == CodecKind::Zstd) var_len = true;
    in_size = is_checksum(k.kind) ? in_size + 4 : k.kind == CodecKind::Gzip ? gzip_bound(in_size)
              : k.kind == CodecKind::Zlib ? zlib_bound(in_size)
              : k.kind == CodecKind::Zstd ? zstd_bound(in_size) : in_size;
    if (k.kind == CodecKind::Crc32c) {
      HIPCHK(launch_crc32c_items(d_items, d_status, (uint32_t)n, k.at_start ? 1 : 0, s));
    } else if (k.kind == CodecKind::Adler32 || k.kind == CodecKind::Fletcher32) {
      HIPCHK(launch_linsum_items(k.kind == CodecKind::Adler32 ? CK_ADLER32 : CK_FLETCHER32, d_items, d_status,
                                 (uint32_t)n, k.at_start ? 1 : 0, s));
    } else if (k.kind == CodecKind::Gzip || k.kind == CodecKind::Zlib) {
      if (!sym) sym = sc.dev<uint32_t>((uint64_t)gzip_encode_grid((uint32_t)std::max<uint64_t>(n, 1)) * GZE_BLK_SYMS);
      cur ^= 1;
      HIPCHK(launch_gzip_encode(d_items, d_status, (uint32_t)n, pool[cur], pitch, sym, k.level, s,
                                k.kind == CodecKind::Zlib, k.kind == CodecKind::Zlib));
    } else if (k.kind == CodecKind::Zstd) {
      zscr = sc.dev<uint8_t>(zstd_encode_scratch((uint32_t)n, stage_in));
      cur ^= 1;
      HIPCHK(launch_zstd_encode(d_items, d_status, (uint32_t)n, stage_in, pool[cur], pitch, zscr, k.checksum ? 1 : 0,
                                s));
    }
  }
  *d_items_out = d_items;
  *d_status_out = d_status;
  if (d_tab_out) *d_tab_out = d_tab;
  if (P_out) *P_out = P;
  return ZGPU_OK;
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

// a chain with a compressor, unsharded: encode_var, then every chunk copied to its destination
static int encode_compressed(zgpu_ctx *C, const Chain &c, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                             const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint64_t *enc_lens,
                             Scratch &sc, hipStream_t s) {
  uint64_t nelem = 1;
  for (uint32_t d = 0; d < nd; d++) nelem *= chunk_shape[d];
  const int64_t bound = chain_encoded_bound(c, nelem);
  if (bound < 0) return set_err(ZGPU_UNSUPPORTED, "encode: the chain's encoded size is not bounded");
  for (uint64_t i = 0; i < n; i++)
    if (!descs[i].dst || descs[i].dst_cap < (uint64_t)bound)
      return set_err(ZGPU_INVALID_ARGUMENT, "encode: destination missing or smaller than the encoded bound");
  std::vector<uint64_t> org(n * nd), dc(2 * n);
  for (uint64_t i = 0; i < n; i++) {
    for (uint32_t d = 0; d < nd; d++) org[i * nd + d] = descs[i].chunk_start[d];
    dc[i] = (uint64_t)descs[i].dst;
    dc[n + i] = descs[i].dst_cap;
  }
  ZgItem *items = nullptr;
  uint32_t *st = nullptr;
  int rc = encode_var(C, c, nd, chunk_shape, array, array_shape, org.data(), n, sc, s, &items, &st, nullptr, nullptr);
  if (rc) return rc;
  uint64_t *d_dc = sc.dev<uint64_t>(3 * n);
  HIPCHK(hipMemcpyAsync(d_dc, dc.data(), 16 * n, hipMemcpyHostToDevice, s));
  HIPCHK(launch_encode_place(items, st, d_dc, d_dc + n, d_dc + 2 * n, (uint32_t)n, s));
  std::vector<uint64_t> lens(n);
  HIPCHK(hipMemcpyAsync(lens.data(), d_dc + 2 * n, 8 * n, hipMemcpyDeviceToHost, s));
  rc = first_status(st, n, s);
  if (rc) return set_err(rc, std::string("encode: ") + zgpu_status_name(rc));
  if (enc_lens) std::memcpy(enc_lens, lens.data(), 8 * n);
  return ZGPU_OK;
}

// sharding_indexed over a fixed-size inner chain (ShardingCodecBound::encode_bounded,
// sharding_codec.rs:924-1085, SubchunkWriteOrder::C): all inner chunks of all shards encoded into
// temporary slots in one batch, all-fill inner chunks omitted, the rest laid out in C order with the
// encoded index at the start or the end; shard lengths to enc_lens.
static int encode_sharded(zgpu_ctx *C, const Chain &top, uint32_t nd, const uint64_t *shard_shape, const void *array,
                          const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint64_t *enc_lens,
                          Scratch &sc, hipStream_t s) {
  const Chain &inner = *top.a2b.inner, &xc = *top.a2b.index;
  if (!top.a2a.empty() || !top.b2b.empty())
    return set_err(ZGPU_UNSUPPORTED, "encode: codecs around sharding_indexed");
  if (top.a2b.inner_shape.size() != nd) return set_err(ZGPU_INVALID_ARGUMENT, "sharding chunk_shape rank");
  if (xc.a2b.kind != CodecKind::Bytes || !xc.a2a.empty())
    return set_err(ZGPU_UNSUPPORTED, "index_codecs must be bytes (+crc32c)");
  for (const Codec &k : xc.b2b)
    if (k.kind != CodecKind::Crc32c) return set_err(ZGPU_UNSUPPORTED, "index_codecs must be bytes (+crc32c)");
  uint64_t cps[ZG_MAXD], n_inner = 1, inner_n = 1;
  for (uint32_t d = 0; d < nd; d++) {
    const uint64_t is = top.a2b.inner_shape[d];
    if (shard_shape[d] % is) return set_err(ZGPU_INVALID_ARGUMENT, "shard shape not a multiple of chunk_shape");
    cps[d] = shard_shape[d] / is;
    n_inner *= cps[d];
    inner_n *= is;
  }
  const int64_t X = chain_fixed_encoded_size(xc, n_inner * 2);
  if (chain_compresses(inner)) {
    // inner chunks of variable length: encode_var over all inner chunks of all shards, then the
    // variable-length layout (C write order, all-fill inner chunks omitted) and the index crc32c
    const int64_t EB = chain_encoded_bound(inner, inner_n);
    if (EB < 0) return set_err(ZGPU_UNSUPPORTED, "encode: the inner chain's encoded size is not bounded");
    const uint64_t bound = n_inner * (uint64_t)EB + (uint64_t)X;
    uint64_t cap = UINT64_MAX;
    for (uint64_t i = 0; i < n; i++) {
      if (!descs[i].dst || descs[i].dst_cap < bound)
        return set_err(ZGPU_INVALID_ARGUMENT, "encode: destination missing or smaller than the shard's bounded size");
      cap = std::min(cap, descs[i].dst_cap);
    }
    const uint64_t n_chunks = n * n_inner;
    std::vector<uint64_t> org(n_chunks * nd);
    for (uint64_t i = 0; i < n; i++)
      for (uint64_t k = 0; k < n_inner; k++) {
        uint64_t rem = k;
        for (int d = (int)nd - 1; d >= 0; d--) {
          org[(i * n_inner + k) * nd + d] = descs[i].chunk_start[d] + (rem % cps[d]) * top.a2b.inner_shape[d];
          rem /= cps[d];
        }
      }
    ZgItem *items = nullptr;
    uint32_t *st = nullptr;
    uint64_t *d_tab = nullptr;
    ZgEncode IP{};
    int rc = encode_var(C, inner, nd, top.a2b.inner_shape.data(), array, array_shape, org.data(), n_chunks, sc, s,
                        &items, &st, &d_tab, &IP);
    if (rc) return rc;
    uint64_t *d_sh = sc.dev<uint64_t>(3 * n + n_chunks);
    uint32_t *d_nf = sc.dev<uint32_t>(std::max<uint64_t>(n_chunks, 1) + n);
    std::vector<uint64_t> hd(n);
    for (uint64_t i = 0; i < n; i++) hd[i] = (uint64_t)descs[i].dst;
    HIPCHK(hipMemcpyAsync(d_sh, hd.data(), 8 * n, hipMemcpyHostToDevice, s));
    uint64_t *d_index_ptr = d_sh + n, *d_len = d_sh + 2 * n, *d_off = d_sh + 3 * n;
    uint32_t *d_shst = d_nf + n_chunks;
    int n_pre = 0;
    for (const Codec &k : xc.b2b) n_pre += k.at_start ? 1 : 0;
    ZgShardLayoutArgs A{n_inner, 0, cap, (uint64_t)X, 4ull * n_pre, top.a2b.at_start ? 1u : 0u,
                        xc.a2b.big_endian ? 1u : 0u};
    HIPCHK(launch_shard_encode_var(d_tab + n_chunks, (const uint8_t *)array, IP, (uint32_t)n_chunks, d_nf, items, st, A,
                                   d_sh, d_off, d_index_ptr, d_len, d_shst, (uint32_t)n, s));
    uint64_t lo = 4ull * n_pre, len = n_inner * 16;
    for (const Codec &k : xc.b2b) {
      HIPCHK(launch_crc32c_encode(d_index_ptr, (uint32_t)n, lo, len, k.at_start ? 1 : 0, s));
      if (k.at_start) lo -= 4;
      len += 4;
    }
    HIPCHK(hipMemcpyAsync(enc_lens, d_len, 8 * n, hipMemcpyDeviceToHost, s));
    rc = first_status(st, n_chunks, s);
    if (!rc) rc = first_status(d_shst, n, s);
    if (rc) return set_err(rc == 1 ? ZGPU_HIP_ERROR : rc, std::string("encode: ") + zgpu_status_name(rc));
    return ZGPU_OK;
  }
  const int64_t E = chain_fixed_encoded_size(inner, inner_n);
  if (E < 0) return set_err(ZGPU_UNSUPPORTED, "encode: the inner chain of sharding_indexed must be fixed-size or "
                                              "compressed by gzip");
  const uint64_t bound = n_inner * (uint64_t)E + (uint64_t)X;
  for (uint64_t i = 0; i < n; i++)
    if (!descs[i].dst || descs[i].dst_cap < bound)
      return set_err(ZGPU_INVALID_ARGUMENT, "encode: destination missing or smaller than the shard's bounded size");
  const uint64_t pitch = ((uint64_t)E + 255) & ~(uint64_t)255, n_chunks = n * n_inner;
  uint8_t *tmp = sc.dev<uint8_t>(std::max<uint64_t>(n_chunks * pitch, 1));
  // inner chunk k of shard i: dst slot, origin in the array
  std::vector<uint64_t> tab(n_chunks * (1 + nd));
  for (uint64_t i = 0; i < n; i++)
    for (uint64_t k = 0; k < n_inner; k++) {
      const uint64_t g = i * n_inner + k;
      tab[g] = (uint64_t)(tmp + g * pitch);
      uint64_t rem = k;
      for (int d = (int)nd - 1; d >= 0; d--) {
        tab[n_chunks + g * nd + d] = descs[i].chunk_start[d] + (rem % cps[d]) * top.a2b.inner_shape[d];
        rem /= cps[d];
      }
    }
  ZgEncode IP{};
  const uint64_t *d_tab = nullptr;  // [dst slots | origins] on the device
  int rc = encode_fixed(C, inner, nd, top.a2b.inner_shape.data(), array, array_shape, tab, n_chunks, sc, s, &IP,
                        &d_tab);
  if (rc) return rc;
  // per-shard tables: dst pointers, inner offsets, index positions, lengths; fill flags
  uint64_t *d_sh = sc.dev<uint64_t>(3 * n + n_chunks);
  uint32_t *d_nf = sc.dev<uint32_t>(std::max<uint64_t>(n_chunks, 1));
  std::vector<uint64_t> hd(n);
  for (uint64_t i = 0; i < n; i++) hd[i] = (uint64_t)descs[i].dst;
  HIPCHK(hipMemcpyAsync(d_sh, hd.data(), 8 * n, hipMemcpyHostToDevice, s));
  uint64_t *d_index_ptr = d_sh + n, *d_len = d_sh + 2 * n, *d_off = d_sh + 3 * n;
  int n_pre = 0;
  for (const Codec &k : xc.b2b) n_pre += k.at_start ? 1 : 0;
  ZgShardLayoutArgs A{n_inner, (uint64_t)E, pitch, (uint64_t)X, 4ull * n_pre, top.a2b.at_start ? 1u : 0u,
                      xc.a2b.big_endian ? 1u : 0u};
  HIPCHK(launch_shard_encode(d_tab + n_chunks, (const uint8_t *)array, IP, (uint32_t)n_chunks, d_nf, tmp, A, d_sh, d_off,
                             d_index_ptr, d_len, (uint32_t)n, s));
  uint64_t lo = 4ull * n_pre, len = n_inner * 16;
  for (const Codec &k : xc.b2b) {
    HIPCHK(launch_crc32c_encode(d_index_ptr, (uint32_t)n, lo, len, k.at_start ? 1 : 0, s));
    if (k.at_start) lo -= 4;
    len += 4;
  }
  HIPCHK(hipMemcpyAsync(enc_lens, d_len, 8 * n, hipMemcpyDeviceToHost, s));
  return ZGPU_OK;
}

// packbits as the array->bytes codec (unsharded): the chunks are gathered (and transposed) as native
// elements into temporary slots, k_packbits packs each slot, and the packed chunks, a 1-D uint8 array
// of one slot per chunk, go through [bytes(uint8), bytes->bytes codecs...] to their destinations
// (straight into them without bytes->bytes codecs).
static int encode_packbits(zgpu_ctx *C, const Chain &c, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                           const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint64_t *enc_lens,
                           Scratch &sc, hipStream_t s) {
  const Codec &pb = c.a2b;
  const uint32_t es = c.enc_es;
  const uint64_t nelem = volume(chunk_shape, nd), packed = packbits_size(pb, nelem);
  const uint64_t upitch = (nelem * es + 15) & ~(uint64_t)15, ppitch = (packed + 15) & ~(uint64_t)15;
  Chain native = c;  // [array->array codecs..., bytes(native)]
  native.b2b.clear();
  native.a2b = Codec{};
  native.a2b.kind = CodecKind::Bytes;
  native.a2b.name = "bytes";
  Chain packed_chain;  // [bytes(uint8), bytes->bytes codecs...]
  packed_chain.es = packed_chain.comp = packed_chain.enc_es = packed_chain.enc_comp = 1;
  packed_chain.data_type = packed_chain.enc_data_type = "uint8";
  packed_chain.a2b = native.a2b;
  packed_chain.b2b = c.b2b;
  const bool direct = c.b2b.empty();
  const int64_t bound = direct ? (int64_t)packed : chain_encoded_bound(packed_chain, packed);
  if (bound < 0) return set_err(ZGPU_UNSUPPORTED, "encode: the chain's encoded size is not bounded");
  for (uint64_t i = 0; i < n; i++)
    if (!descs[i].dst || descs[i].dst_cap < (uint64_t)bound)
      return set_err(ZGPU_INVALID_ARGUMENT, "encode: destination missing or smaller than the encoded bound");
  uint8_t *U = sc.dev<uint8_t>(std::max<uint64_t>(n * upitch, 1));
  uint8_t *Pk = direct ? nullptr : sc.dev<uint8_t>(std::max<uint64_t>(n * ppitch, 1));
  std::vector<uint64_t> tab(n * (1 + nd)), ptab(2 * n);
  for (uint64_t i = 0; i < n; i++) {
    tab[i] = ptab[i] = (uint64_t)(U + i * upitch);
    for (uint32_t d = 0; d < nd; d++) tab[n + i * nd + d] = descs[i].chunk_start[d];
    ptab[n + i] = direct ? (uint64_t)descs[i].dst : (uint64_t)(Pk + i * ppitch);
  }
  int rc = encode_fixed(C, native, nd, chunk_shape, array, array_shape, tab, n, sc, s);
  if (rc) return rc;
  uint64_t *d_ptab = sc.dev<uint64_t>(ptab.size());
  HIPCHK(hipMemcpyAsync(d_ptab, ptab.data(), ptab.size() * 8, hipMemcpyHostToDevice, s));
  ZgPackBits P{};
  P.nelem = nelem;
  P.packed_len = packed;
  P.ncomp = pb.pb_ncomp;
  P.comp_bytes = es / pb.pb_ncomp;
  P.first = pb.pb_first;
  P.ext = pb.pb_last - pb.pb_first + 1;
  P.sign = pb.pb_signed ? 1 : 0;
  P.padding = (uint32_t)pb.pb_padding;
  HIPCHK(launch_packbits(d_ptab, (uint32_t)n, P, s));
  if (direct) {
    HIPCHK(hipStreamSynchronize(s));  // ptab is read by the copy above
    for (uint64_t i = 0; i < n; i++) enc_lens[i] = packed;
    return ZGPU_OK;
  }
  // the packed chunks as chunk i = [i * ppitch, i * ppitch + packed) of a 1-D uint8 array
  const uint64_t p_shape[1] = {n * ppitch}, p_chunk[1] = {packed};
  std::vector<zgpu_encode_desc> pd(descs, descs + n);
  for (uint64_t i = 0; i < n; i++) pd[i].chunk_start[0] = i * ppitch;
  if (chain_compresses(packed_chain))
    return encode_compressed(C, packed_chain, 1, p_chunk, Pk, p_shape, pd.data(), n, enc_lens, sc, s);
  std::vector<uint64_t> t2(2 * n);
  for (uint64_t i = 0; i < n; i++) {
    t2[i] = (uint64_t)descs[i].dst;
    t2[n + i] = i * ppitch;
  }
  rc = encode_fixed(C, packed_chain, 1, p_chunk, Pk, p_shape, t2, n, sc, s);
  HIPCHK(hipStreamSynchronize(s));  // the tables are read by encode_fixed's copies
  for (uint64_t i = 0; i < n; i++) enc_lens[i] = (uint64_t)bound;
  return rc;
}

static int check_origins(uint32_t nd, const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    for (uint32_t d = 0; d < nd; d++)
      if (descs[i].chunk_start[d] >= array_shape[d])
        return set_err(ZGPU_INVALID_ARGUMENT, "encode: chunk origin outside the array");
  return ZGPU_OK;
}

// zgpu_encode_chunks (arguments checked) on stream s of the caller's lane: n chunks of the device array to their device
// destinations, synchronous (the temporaries go back when it returns).
int encode_chunks_on(zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                     const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint64_t *enc_lens,
                     hipStream_t s) {
  if (!n) return ZGPU_OK;
  zgpu_ctx *C = ch->ctx;
  Scratch sc(C, s);
  int rc = 0;
  // value codecs (numcodecs.fixedscaleoffset, bitround) work element by element, so they commute with
  // chunking and sharding: the caller's array is converted once into a device array of the innermost
  // encoded type, which the chain without them, retyped, encodes (strip_value_codecs)
  std::shared_ptr<Chain> stripped;
  if (chain_has_value_codec(*ch->chain)) {
    std::vector<Codec> steps;
    stripped = strip_value_codecs(*ch->chain, steps);
    retype_stripped(*stripped, *ch->chain);
    array = value_encode_elements(steps, (const uint8_t *)array, volume(array_shape, nd), sc, s);
  }
  const Chain &c = stripped ? *stripped : *ch->chain;
  if (c.a2b.kind == CodecKind::PackBits || c.a2b.kind == CodecKind::Sharding || chain_compresses(c)) {
    uint64_t *hl = sc.pinned<uint64_t>(n);  // the variable lengths, read back by the callee
    rc = c.a2b.kind == CodecKind::PackBits
             ? encode_packbits(C, c, nd, chunk_shape, array, array_shape, descs, n, hl, sc, s)
         : c.a2b.kind == CodecKind::Sharding
             ? encode_sharded(C, c, nd, chunk_shape, array, array_shape, descs, n, hl, sc, s)
             : encode_compressed(C, c, nd, chunk_shape, array, array_shape, descs, n, hl, sc, s);
    HIPCHK(hipStreamSynchronize(s));
    if (!rc && enc_lens) std::memcpy(enc_lens, hl, 8 * n);
    return rc;
  }
  const int64_t enc_size = chain_fixed_encoded_size(c, volume(chunk_shape, nd));
  if (enc_size < 0 && c.a2b.kind == CodecKind::Bytes)
    rc = set_err(ZGPU_UNSUPPORTED, "encode: only transpose / bytes / numcodecs.shuffle (innermost, elementsize = "
                                   "data type size) / crc32c, or sharding_indexed over such a chain, run on "
                                   "the GPU write path");
  for (uint64_t i = 0; i < n && !rc; i++)
    if (!descs[i].dst || descs[i].dst_cap < (uint64_t)std::max<int64_t>(enc_size, 0))
      rc = set_err(ZGPU_INVALID_ARGUMENT, "encode: destination missing or smaller than the encoded size");
  if (rc) return rc;
  std::vector<uint64_t> tab(n * (1 + nd));
  for (uint64_t i = 0; i < n; i++) {
    tab[i] = (uint64_t)descs[i].dst;
    for (uint32_t d = 0; d < nd; d++) tab[n + i * nd + d] = descs[i].chunk_start[d];
  }
  rc = encode_fixed(C, c, nd, chunk_shape, array, array_shape, tab, n, sc, s);
  HIPCHK(hipStreamSynchronize(s));
  if (!rc && enc_lens)
    for (uint64_t i = 0; i < n; i++) enc_lens[i] = (uint64_t)enc_size;
  return rc;
}

extern "C" {

int zgpu_encode_chunks(zgpu_chain *ch, uint32_t nd, const uint64_t *chunk_shape, const void *array,
                       const uint64_t *array_shape, const zgpu_encode_desc *descs, uint64_t n, uint32_t flags,
                       uint64_t *enc_lens, void *stream) {
  ABI_GUARD_BEGIN
  if (!ch || !chunk_shape || !array || !array_shape || (n && !descs))
    return set_err(ZGPU_INVALID_ARGUMENT, "NULL argument");
  if (nd == 0 || nd > ZGPU_MAX_DIMS) return set_err(ZGPU_INVALID_ARGUMENT, "ndim out of range");
  if ((flags & (ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE)) != (ZGPU_ENC_DEVICE | ZGPU_OUT_DEVICE))
    return set_err(ZGPU_INVALID_ARGUMENT, "encode: array and destinations must be device memory");
  if (const int rc = check_origins(nd, array_shape, descs, n)) return rc;
  HIPCHK(hipSetDevice(ch->ctx->device));
  LaneScope ls(ch->ctx);
  return encode_chunks_on(ch, nd, chunk_shape, array, array_shape, descs, n, enc_lens, pick_stream(ls.L, stream));
  ABI_GUARD_END
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
  if (ch && ch->chain->a2b.kind == CodecKind::Sharding)
    return set_err(ZGPU_INVALID_ARGUMENT, "encode: sharding_indexed chunks have variable lengths: zgpu_encode_chunks");
  if (ch && chain_compresses(*ch->chain))
    return set_err(ZGPU_INVALID_ARGUMENT, "encode: compressed chunks have variable lengths: zgpu_encode_chunks");
  return zgpu_encode_chunks(ch, nd, chunk_shape, array, array_shape, descs, n, flags, nullptr, hip_stream);
}

}  // extern "C"
