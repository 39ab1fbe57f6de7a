// libzgpu: the host layout of the write path (encode_layout.hpp). No HIP call and no environment read:
// encode_layout() and encoded_bound() are functions of their arguments.
#include "encode_layout.hpp"

#include <algorithm>

namespace zgpu {

namespace {

uint64_t volume_of(const uint64_t *shape, uint32_t nd) {
  uint64_t n = 1;
  for (uint32_t d = 0; d < nd; d++) n *= shape[d];
  return n;
}

void check_transposes(const Chain &c, uint32_t nd) {
  for (const Codec &k : c.a2a)
    if (k.kind == CodecKind::Transpose && k.order.size() != nd)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "transpose order rank != ndim"};
}

// the streams k_blosc_encode writes (BloscCodec::encode, blosc_codec_via_blosc_src.rs:113-128)
uint32_t blosc_compressor(const std::string &cname) {
  return (cname == "lz4" || cname == "lz4hc") ? (uint32_t)BL_COMP_LZ4
         : cname == "zstd"                    ? (uint32_t)BL_COMP_ZSTD
         : cname == "blosclz"                 ? (uint32_t)BL_COMP_BLOSCLZ
         : cname == "zlib"                    ? (uint32_t)BL_COMP_ZLIB
         : cname == "snappy"                  ? (uint32_t)BL_COMP_SNAPPY
                                              : UINT32_MAX;
}

// CodecChain::encode (codec_chain.rs:528-555) of [array->array codecs, bytes, bytes->bytes codecs]:
// ENC_FIXED when only checksums follow the (fused) shuffle, else ENC_VAR.
EncodeLayout bytes_layout(const Chain &c, uint32_t nd, const uint64_t *chunk_shape) {
  if (c.a2b.kind != CodecKind::Bytes)
    throw ChainError{ZGPU_UNSUPPORTED, "encode: the array->bytes codec must be bytes here (sharding_indexed and packbits "
                                       "are encoded at the top of a chain only)"};
  check_transposes(c, nd);
  EncodeLayout L;
  L.chain = &c;
  L.nelem = volume_of(chunk_shape, nd);
  L.data_bytes = L.nelem * c.enc_es;
  uint64_t size = L.data_bytes, max_size = size;
  uint32_t n_sums = 0, n_start = 0;
  int cur = 0;
  bool var_len = false;  // an earlier stage made the lengths variable
  for (size_t i = 0; i < c.b2b.size(); i++) {
    const Codec &k = c.b2b[i];
    if (k.kind == CodecKind::Shuffle) {
      if (i != 0 || k.elementsize != c.enc_es)
        throw ChainError{ZGPU_UNSUPPORTED, "encode: numcodecs.shuffle is fused into the gather: it must be the first "
                                           "bytes->bytes codec and its elementsize the element size"};
      L.shuffle = true;
      continue;
    }
    EncodeStage st{};
    st.at_start = k.at_start ? 1 : 0;
    st.level = k.level;
    switch (k.kind) {
      case CodecKind::Crc32c:
      case CodecKind::Adler32:
      case CodecKind::Fletcher32:
        st.kind = checksum_stage(k.kind);
        n_sums++;
        n_start += st.at_start;
        break;
      case CodecKind::Gzip: st.kind = ST_GZIP; break;
      case CodecKind::Zlib: st.kind = ST_ZLIB; st.zlib = st.zlib_bounded = true; break;
      case CodecKind::Zstd: st.kind = ST_ZSTD; st.zstd_checksum = k.checksum; break;
      case CodecKind::Blosc:
        st.kind = ST_BLOSC;
        st.bl_comp = blosc_compressor(k.cname);
        if (st.bl_comp == UINT32_MAX)
          throw ChainError{ZGPU_UNSUPPORTED, "encode: blosc cname '" + k.cname +
                                                 "' (the GPU writes blosclz, lz4, lz4hc, snappy, zlib and zstd)"};
        if (var_len)  // (its frame header states one decoded size for every chunk)
          throw ChainError{ZGPU_UNSUPPORTED, "encode: blosc after a variable-length codec"};
        st.bl_typesize = std::max<uint32_t>(1, k.elementsize);
        st.bl_shuffle = k.shuffle >= 0 ? (uint32_t)k.shuffle : (k.elementsize > 0 ? 2u : 0u);  // zarrs' default (:119-123)
        st.bl_blocksize = k.blocksize;
        break;
      case CodecKind::Bz2: throw ChainError{ZGPU_UNSUPPORTED, "encode: numcodecs.bz2 is decode-only on the GPU"};
      default: throw ChainError{ZGPU_UNSUPPORTED, "encode: codec '" + k.name + "' has no encoder on the GPU"};
    }
    st.in_bound = size;
    st.out_bound = size = (uint64_t)codec_encoded_bound(k, size);
    max_size = std::max(max_size, size);
    if (!strips_only(st.kind)) {
      var_len = true;
      st.pool = cur ^= 1;  // into the pool the last compressor did not write
    }
    L.stages.push_back(st);
  }
  L.fixed = !var_len;
  L.size = size;
  if (L.fixed) {
    L.path = ENC_FIXED;
    uint64_t lo = L.data_off = 4ull * n_start;
    for (EncodeStage &st : L.stages) {  // each checksum covers the bytes and the checksums before it
      st.lo = lo;
      if (st.at_start) lo -= 4;
    }
    return L;
  }
  // slots: 64 bytes in front for the checksums located at the start (14 at the most), every stage's
  // bound behind, room for the checksums at the end and the encoders' 16-byte stores
  if (n_sums > 14) throw ChainError{ZGPU_UNSUPPORTED, "encode: more than 14 checksum codecs around a compressor"};
  L.path = ENC_VAR;
  L.headroom = 64;
  L.pitch = (L.headroom + max_size + 4 * n_sums + 16 + 255) & ~(uint64_t)255;
  L.n_pools = 2;
  return L;
}

// Inner chunks per shard along each axis; the refusal's text, or nullptr.
const char *shard_grid(const Codec &sh, uint32_t nd, const uint64_t *shard_shape, uint64_t *cps, uint64_t &n_inner,
                       uint64_t &inner_n) {
  if (sh.inner_shape.size() != nd) return "sharding chunk_shape rank != ndim";
  n_inner = inner_n = 1;
  for (uint32_t d = 0; d < nd; d++) {
    const uint64_t is = sh.inner_shape[d];
    if (!is || shard_shape[d] % is) return "shard shape not a multiple of the sharding chunk_shape";
    cps[d] = shard_shape[d] / is;
    n_inner *= cps[d];
    inner_n *= is;
  }
  return nullptr;
}

// ShardingCodecBound::encode_bounded (sharding_codec.rs:924-1085, SubchunkWriteOrder::C)
EncodeLayout sharded_layout(const Chain &top, uint32_t nd, const uint64_t *shard_shape) {
  if (!top.a2a.empty() || !top.b2b.empty())
    throw ChainError{ZGPU_UNSUPPORTED, "encode: codecs around sharding_indexed"};
  const Chain &xc = *top.a2b.index;
  bool index_ok = xc.a2b.kind == CodecKind::Bytes && xc.a2a.empty();
  for (const Codec &k : xc.b2b) index_ok = index_ok && k.kind == CodecKind::Crc32c;
  if (!index_ok) throw ChainError{ZGPU_UNSUPPORTED, "index_codecs must be bytes (+crc32c)"};
  EncodeLayout L;
  L.chain = &top;
  if (const char *err = shard_grid(top.a2b, nd, shard_shape, L.cps, L.n_inner, L.inner_n))
    throw ChainError{ZGPU_INVALID_ARGUMENT, err};
  L.inner = std::make_shared<EncodeLayout>(bytes_layout(*top.a2b.inner, nd, top.a2b.inner_shape.data()));
  const uint64_t index_shape[1] = {2 * L.n_inner};
  L.index = std::make_shared<EncodeLayout>(bytes_layout(xc, 1, index_shape));
  L.index_at_start = top.a2b.at_start;
  L.index_big_endian = xc.a2b.big_endian;
  L.path = L.inner->fixed ? ENC_SHARD_FIXED : ENC_SHARD_VAR;
  if (L.inner->fixed) L.pitch = (L.inner->size + 255) & ~(uint64_t)255;  // the inner chunks' temporary slots
  L.nelem = volume_of(shard_shape, nd);
  L.size = L.n_inner * L.inner->size + L.index->size;  // (all-fill inner chunks are left out: a bound)
  return L;
}

EncodeLayout packbits_layout(const Chain &c, uint32_t nd, const uint64_t *chunk_shape) {
  check_transposes(c, nd);
  EncodeLayout L;
  L.path = ENC_PACKBITS;
  L.chain = &c;
  L.nelem = volume_of(chunk_shape, nd);
  L.data_bytes = L.nelem * c.enc_es;
  L.packed_len = packbits_size(c.a2b, L.nelem);
  L.upitch = (L.data_bytes + 15) & ~(uint64_t)15;
  L.ppitch = (L.packed_len + 15) & ~(uint64_t)15;
  L.direct = c.b2b.empty();
  auto native = std::make_shared<Chain>(c);  // [array->array codecs..., bytes(native)]
  native->b2b.clear();
  native->a2b = Codec{};
  native->a2b.kind = CodecKind::Bytes;
  native->a2b.name = "bytes";
  auto packed = std::make_shared<Chain>();  // [bytes(uint8), bytes->bytes codecs...] over 1-D chunks of packed_len
  packed->es = packed->comp = packed->enc_es = packed->enc_comp = 1;
  packed->data_type = packed->enc_data_type = "uint8";
  packed->a2b = native->a2b;
  packed->b2b = c.b2b;
  auto sub = [](const std::shared_ptr<Chain> &ch, uint32_t nd, const uint64_t *shape) {
    auto l = std::make_shared<EncodeLayout>(bytes_layout(*ch, nd, shape));
    l->own = ch;
    return l;
  };
  L.native = sub(native, nd, chunk_shape);
  L.packed = sub(packed, 1, &L.packed_len);
  L.fixed = L.packed->fixed;
  L.size = L.packed->size;
  return L;
}

}  // namespace

EncodeLayout encode_layout(const Chain &c, uint32_t nd, const uint64_t *chunk_shape) {
  if (c.a2b.kind == CodecKind::Sharding) return sharded_layout(c, nd, chunk_shape);
  if (c.a2b.kind == CodecKind::PackBits) return packbits_layout(c, nd, chunk_shape);
  return bytes_layout(c, nd, chunk_shape);
}

int64_t encoded_bound(const Chain &c, uint32_t nd, const uint64_t *chunk_shape) {
  if (c.a2b.kind != CodecKind::Sharding) return chain_encoded_bound(c, volume_of(chunk_shape, nd));
  for (const Codec &k : c.a2a)
    if (!is_value_codec(k.kind)) return -1;
  uint64_t cps[ZG_MAXD], n_inner, inner_n;
  if (!c.b2b.empty() || shard_grid(c.a2b, nd, chunk_shape, cps, n_inner, inner_n)) return -1;
  const int64_t E = chain_encoded_bound(*c.a2b.inner, inner_n);
  const int64_t X = chain_fixed_encoded_size(*c.a2b.index, n_inner * 2);
  return E < 0 || X < 0 ? -1 : (int64_t)n_inner * E + X;
}

}  // namespace zgpu
