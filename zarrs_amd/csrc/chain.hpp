// Codec chain model: parse + bind of the Zarr V3 "codecs" metadata list.
// Mirrors CodecChain::from_metadata / with_context
// (zarrs/src/array/codec/array_to_bytes/codec_chain.rs:105-169,192-229): array->array codecs,
// exactly one array->bytes codec, then bytes->bytes codecs; decode runs them in reverse.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "json.hpp"
#include "kernels/cast.hpp"

namespace zgpu {

enum class CodecKind { Transpose, Bytes, Sharding, Crc32c, Gzip, Zstd, Shuffle, Blosc, Zlib, Adler32, Fletcher32, Bz2,
                       PackBits, FixedScaleOffset, BitRound, CastValue };

struct Chain;

struct Codec {
  CodecKind kind;
  std::string name;
  std::vector<uint32_t> order;        // transpose
  bool big_endian = false;            // bytes
  bool at_start = false;              // crc32c / adler32 location, sharding index_location
  int level = 0;                      // gzip / zstd / zlib / bz2
  bool checksum = false;              // zstd
  uint32_t elementsize = 4;           // shuffle; blosc typesize
  std::string cname;                  // blosc compressor (decode reads the compressor from the header)
  int shuffle = -1;                   // blosc: 0 noshuffle, 1 byte shuffle, 2 bitshuffle, -1 absent
  uint64_t blocksize = 0;             // blosc: 0 = automatic
  std::vector<uint64_t> inner_shape;  // sharding
  std::shared_ptr<Chain> inner, index;
  // packbits, bound to the data type it encodes (packbits_codec.rs:152-180)
  uint32_t pb_first = 0, pb_last = 0;      // extracted bit range of a component, inclusive
  uint32_t pb_comp_bits = 0, pb_ncomp = 0; // component width in bits, components per element
  bool pb_signed = false;                  // sign extension (signed integers)
  int pb_padding = 0;                      // padding_encoding: 0 none, 1 first_byte, 2 last_byte
  // numcodecs.fixedscaleoffset: decoded / encoded element types and whether `astype` was given (the
  // cast through f32 happens only then); bitround: keepbits over the element type vt_dec
  float fso_offset = 0, fso_scale = 1;
  uint32_t vt_dec = 0, vt_enc = 0;  // ZgValueType
  bool fso_astype = false;
  uint32_t keepbits = 0;
  // cast_value: vt_dec -> vt_enc on encode and back on decode, both with the same rounding (CastRounding)
  // and out_of_range (CastOutOfRange), each direction through its own scalar map
  uint32_t cast_rounding = 0, cast_oor = 0;
  CastMap cast_enc_map{}, cast_dec_map{};
};

// Element types of the value codecs (the kernels' template parameter).
enum ZgValueType : uint32_t { VT_I8, VT_I16, VT_I32, VT_I64, VT_U8, VT_U16, VT_U32, VT_U64, VT_F32, VT_F64,
                              VT_F16, VT_BF16, VT_NONE };
ZgValueType value_type_of(const std::string &data_type);

inline bool is_value_codec(CodecKind k) {
  return k == CodecKind::FixedScaleOffset || k == CodecKind::BitRound || k == CodecKind::CastValue;
}

struct Chain {
  std::vector<Codec> a2a;
  Codec a2b;
  std::vector<Codec> b2b;
  uint32_t es = 0, comp = 0;
  uint8_t fill[16] = {0};
  std::string data_type;
  // what the array->bytes codec sees: the data type and fill value after the array->array codecs
  // (equal to the above without a value codec)
  uint32_t enc_es = 0, enc_comp = 0;
  uint8_t enc_fill[16] = {0};
  std::string enc_data_type;
};

// Whether the chain, or a sharding inner chain below it, holds a value codec.
bool chain_has_value_codec(const Chain &c);
// Packed byte length of nelem elements under a packbits codec (PackBitsCodecBound::encode).
uint64_t packbits_size(const Codec &k, uint64_t nelem);
// The value codecs' encode of one element on the host (the encoded fill value; the kernels in
// kernels/value.hip compute the same): out receives the encoded element.
void fso_encode_element(const Codec &k, const uint8_t *in, uint8_t *out);
void bitround_element(uint32_t vt, uint32_t keepbits, uint8_t *elem);
// Whether a cast_value codec's decode (encode) can meet an element it cannot cast (cast_infallible).
bool cast_decode_fallible(const Codec &k);
bool cast_encode_fallible(const Codec &k);
uint32_t value_type_size(uint32_t vt);

struct ChainError {
  int status;
  std::string msg;
};

// Data type name -> (element size, endianness component size); false if unsupported.
bool data_type_info(const std::string &name, uint32_t &es, uint32_t &comp);

// Throws ChainError.
std::shared_ptr<Chain> parse_chain(const Json &codecs, const std::string &data_type, const uint8_t *fill);

// A 4-byte checksum codec (crc32c, numcodecs.adler32, numcodecs.fletcher32): fixed size + 4.
inline bool is_checksum(CodecKind k) {
  return k == CodecKind::Crc32c || k == CodecKind::Adler32 || k == CodecKind::Fletcher32;
}

// Encoded byte size of a chain for a fixed decoded element count, or -1 if not fixed-size
// (BytesRepresentation::FixedSize, sharding.rs:163-176): the checksum codecs add 4 each.
int64_t chain_fixed_encoded_size(const Chain &c, uint64_t nelem);

// Upper bound of one chunk's encoded size for an array->bytes `bytes` chain (BytesRepresentation::
// BoundedSize): crc32c / adler32 / fletcher32 +4, gzip as GzipCodec::encoded_representation
// (gzip_codec.rs:122-136, zlib's deflateBound), zlib as ZlibCodec's (zlib/zlib_codec.rs), zstd as
// ZstdCodec's (zstd_codec.rs:132-147), bz2 as Bz2Codec's (bz2_codec.rs: size + size / 8 + 1024); -1 if
// unbounded.
int64_t chain_encoded_bound(const Chain &c, uint64_t nelem);
// One bytes->bytes codec's encoded size for n bytes in, the one statement of the per-stage arithmetic the
// two functions above and the write path's layout (encode_layout.cpp) read: exact for the checksums and
// numcodecs.shuffle, else a bound (*fixed, if given, is cleared); -1 for a codec without one.
int64_t codec_encoded_bound(const Codec &k, uint64_t n, bool *fixed = nullptr);
uint64_t gzip_bound(uint64_t n);
uint64_t zlib_bound(uint64_t n);
uint64_t zstd_bound(uint64_t n);
uint64_t bz2_bound(uint64_t n);

}  // namespace zgpu
