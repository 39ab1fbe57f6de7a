// Codec chain parsing (see chain.hpp). Reference: codec_chain.rs:192-229 (from_metadata: exactly one
// array->bytes codec, error otherwise), zarrs_codec/src/lib.rs:372-449 (name -> codec lookup), and the
// per-codec configurations in zarrs_metadata_ext/src/codec/registered/{transpose,bytes,sharding,
// crc32c,gzip,zstd,shuffle,cast_value}.rs, zarrs_metadata_ext/src/codec/numcodecs/{zlib,adler32,fletcher32,bz2}.rs
// (created by zarrs/src/array/codec/bytes_to_bytes/{zlib,adler32,fletcher32,bz2}.rs).
#include "chain.hpp"

#include <cerrno>
#include <cstring>

#include "../../include/zgpu.h"
#include "kernels/value.hpp"

namespace zgpu {

bool data_type_info(const std::string &n, uint32_t &es, uint32_t &comp) {
  struct E { const char *name; uint32_t es, comp; };
  static const E tab[] = {
      {"bool", 1, 1},    {"int8", 1, 1},    {"uint8", 1, 1},    {"int16", 2, 2},     {"uint16", 2, 2},
      {"float16", 2, 2}, {"bfloat16", 2, 2}, {"int32", 4, 4},   {"uint32", 4, 4},    {"float32", 4, 4},
      {"int64", 8, 8},   {"uint64", 8, 8},  {"float64", 8, 8},  {"complex64", 8, 4}, {"complex128", 16, 8},
  };
  for (const E &e : tab)
    if (n == e.name) {
      es = e.es;
      comp = e.comp;
      return true;
    }
  return false;
}

static std::shared_ptr<Chain> parse(const Json &codecs, const std::string &dt, uint32_t es, uint32_t comp,
                                    const uint8_t *fill);

enum class Role { A2A, A2B, B2B };

// The data type and fill value a codec is bound with (with_context): a value codec replaces them
// with its encoded data type and fill value for every codec after it.
struct TypeCtx {
  std::string dt;
  uint32_t es, comp;
  uint8_t fill[16];
};

ZgValueType value_type_of(const std::string &n) {
  static const char *names[] = {"int8",   "int16",  "int32",   "int64",   "uint8",   "uint16",
                                "uint32", "uint64", "float32", "float64", "float16", "bfloat16"};
  for (uint32_t i = 0; i < 12; i++)
    if (n == names[i]) return (ZgValueType)i;
  return VT_NONE;
}

uint32_t value_type_size(uint32_t vt) {
  static const uint32_t sz[] = {1, 2, 4, 8, 1, 2, 4, 8, 4, 8, 2, 2};
  return vt < 12 ? sz[vt] : 0;
}

// A numpy type string, with or without a byte-order character (fixedscaleoffset_codec.rs:46-54 and
// data_type_metadata_v2_to_v3), as a Zarr V3 data type name; empty if it names none.
static std::string numpy_to_v3(std::string s) {
  if (!s.empty() && (s[0] == '<' || s[0] == '>' || s[0] == '|' || s[0] == '=')) s = s.substr(1);
  static const char *tab[][2] = {{"b1", "bool"},     {"i1", "int8"},      {"i2", "int16"},      {"i4", "int32"},
                                 {"i8", "int64"},    {"u1", "uint8"},     {"u2", "uint16"},     {"u4", "uint32"},
                                 {"u8", "uint64"},   {"f2", "float16"},   {"f4", "float32"},    {"f8", "float64"},
                                 {"c8", "complex64"}, {"c16", "complex128"}};
  for (const auto &e : tab)
    if (s == e[0]) return e[1];
  return "";
}

template <class F>
static void with_value_type(uint32_t vt, F &&f) {
  switch (vt) {
    case VT_I8: f(int8_t{}); break;
    case VT_I16: f(int16_t{}); break;
    case VT_I32: f(int32_t{}); break;
    case VT_I64: f(int64_t{}); break;
    case VT_U8: f(uint8_t{}); break;
    case VT_U16: f(uint16_t{}); break;
    case VT_U32: f(uint32_t{}); break;
    case VT_U64: f(uint64_t{}); break;
    case VT_F32: f(float{}); break;
    default: f(double{}); break;
  }
}

void fso_encode_element(const Codec &k, const uint8_t *in, uint8_t *out) {
  with_value_type(k.vt_dec, [&](auto t) {
    using T = decltype(t);
    T x;
    std::memcpy(&x, in, sizeof(T));
    with_value_type(k.vt_enc, [&](auto e) {
      using E = decltype(e);
      const E y = fso_encode_one<T, E>(x, k.fso_offset, k.fso_scale, k.fso_astype);
      std::memcpy(out, &y, sizeof(E));
    });
  });
}

static uint32_t mantissa_bits(uint32_t vt) {
  return vt == VT_F16 ? 10 : vt == VT_BF16 ? 7 : vt == VT_F32 ? 23 : vt == VT_F64 ? 52 : 0;
}

void bitround_element(uint32_t vt, uint32_t keepbits, uint8_t *elem) {
  const uint32_t mant = mantissa_bits(vt);
  auto go = [&](auto u) {
    using U = decltype(u);
    U x;
    std::memcpy(&x, elem, sizeof(U));
    x = bitround_one<U>(x, keepbits, mant);
    std::memcpy(elem, &x, sizeof(U));
  };
  switch (value_type_size(vt)) {
    case 1: go(uint8_t{}); break;
    case 2: go(uint16_t{}); break;
    case 4: go(uint32_t{}); break;
    default: go(uint64_t{}); break;
  }
}

// ---- cast_value -----------------------------------------------------------------------------------
static_assert((uint32_t)VT_I8 == CT_I8 && (uint32_t)VT_I64 == CT_I64 && (uint32_t)VT_U8 == CT_U8 &&
                  (uint32_t)VT_U64 == CT_U64 && (uint32_t)VT_F32 == CT_F32 && (uint32_t)VT_F64 == CT_F64 &&
                  (uint32_t)VT_F16 == CT_F16 && (uint32_t)VT_BF16 == CT_BF16 && (uint32_t)VT_NONE == CT_COUNT,
              "kernels/cast.hpp numbers the element types as ZgValueType");

bool cast_decode_fallible(const Codec &k) { return !cast_infallible(k.vt_enc, k.vt_dec, k.cast_oor); }
bool cast_encode_fallible(const Codec &k) { return !cast_infallible(k.vt_dec, k.vt_enc, k.cast_oor); }

// One scalar_map key or value as DataType::fill_value_v3 reads it for the 12 cast_value types
// (zarrs/src/array/data_type/macros.rs @fill_value, zarrs_metadata/src/v3/array/fill_value.rs as_*):
// the integers take a JSON integer within the type's range (as_i64 / as_u64, then try_from); the floats a
// JSON number (read as f64, then rounded to nearest even), "NaN" (the canonical pattern), "Infinity",
// "-Infinity", or "0x" and the element's bits as big-endian hex digits. Returns the element's bits.
static uint64_t cast_scalar(const Json &v, uint32_t vt, const std::string &dt) {
  const ChainError bad{ZGPU_INVALID_ARGUMENT, "cast_value: scalar_map entry is not a valid " + dt + " value"};
  const uint32_t size = value_type_size(vt);
  if (!cast_type_is_float(vt)) {
    if (v.kind != Json::Num || !v.is_int) throw bad;
    const char *tok = v.s.c_str();
    char *end = nullptr;
    errno = 0;
    if (cast_type_is_signed(vt)) {
      const long long x = std::strtoll(tok, &end, 10);
      if (errno || *end) throw bad;
      const int64_t lo = size == 8 ? INT64_MIN : -((int64_t)1 << (8 * size - 1));
      if (x < lo || x > -(lo + 1)) throw bad;
      return size == 8 ? (uint64_t)x : (uint64_t)x & (((uint64_t)1 << (8 * size)) - 1);
    }
    if (tok[0] == '-') throw bad;
    const unsigned long long x = std::strtoull(tok, &end, 10);
    if (errno || *end) throw bad;
    if (size < 8 && x >> (8 * size)) throw bad;
    return x;
  }
  uint64_t bits = 0;
  auto from_double = [&](double d) {
    const CastMap none{};
    uint8_t out[8] = {0};
    cast_elements_host(VT_F64, vt, (const uint8_t *)&d, out, 1, none, CAST_NEAREST_EVEN, CAST_OOR_CLAMP);  // overflow: inf
    std::memcpy(&bits, out, size);
  };
  if (v.kind == Json::Num) {
    from_double(v.num);
  } else if (v.kind == Json::Str) {
    if (v.s == "NaN") from_double(std::numeric_limits<double>::quiet_NaN());
    else if (v.s == "Infinity") from_double(std::numeric_limits<double>::infinity());
    else if (v.s == "-Infinity") from_double(-std::numeric_limits<double>::infinity());
    else if (v.s.size() == 2 + 2 * (size_t)size && v.s.compare(0, 2, "0x") == 0) {
      for (size_t i = 2; i < v.s.size(); i++) {
        const char c = v.s[i];
        const int h = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (h < 0) throw bad;
        bits = (bits << 4) | (uint64_t)h;
      }
    } else {
      throw bad;
    }
  } else {
    throw bad;
  }
  return bits;
}

// build_scalar_map (cast_value_codec.rs:353-373): [[key, value], ...] with keys of type `from` and values
// of type `to`. Every entry is kept, in order: the lookup takes the first match, as or_insert does.
static void cast_scalar_map(const Json *list, uint32_t from, const std::string &from_dt, uint32_t to,
                            const std::string &to_dt, CastMap &map) {
  if (!list || list->kind == Json::Null) return;
  if (list->kind != Json::Arr) throw ChainError{ZGPU_INVALID_ARGUMENT, "cast_value: scalar_map lists must be arrays"};
  if (list->arr.size() > CAST_MAP_MAX)
    throw ChainError{ZGPU_UNSUPPORTED, "cast_value: more than " + std::to_string(CAST_MAP_MAX) +
                                           " scalar_map entries in one direction are not supported by the GPU pipeline"};
  for (const Json &e : list->arr) {
    if (e.kind != Json::Arr || e.arr.size() != 2)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "cast_value: a scalar_map entry must be [key, value]"};
    map.key[map.n] = cast_scalar(e.arr[0], from, from_dt);
    map.val[map.n] = cast_scalar(e.arr[1], to, to_dt);
    map.n++;
  }
}

static void cast_encode_element(const Codec &k, const uint8_t *in, uint8_t *out, bool decode, bool &ok) {
  ok = decode ? cast_elements_host(k.vt_enc, k.vt_dec, in, out, 1, k.cast_dec_map, k.cast_rounding, k.cast_oor) == 1
              : cast_elements_host(k.vt_dec, k.vt_enc, in, out, 1, k.cast_enc_map, k.cast_rounding, k.cast_oor) == 1;
}

// CastValueCodecConfigurationV1 (registered/cast_value.rs:22-37, deny_unknown_fields) and with_context
// (cast_value_codec.rs:112-191)
static void create_cast_value(Codec &k, const Json *cfg, TypeCtx &T) {
  k.kind = CodecKind::CastValue;
  const Json *d = cfg && cfg->kind == Json::Obj ? cfg->get("data_type") : nullptr;
  if (!d)  // the only configuration variant is V1, which has data_type (new_with_configuration's wording)
    throw ChainError{ZGPU_UNSUPPORTED, "this cast_value codec configuration variant is unsupported"};
  for (const auto &kv : cfg->obj)
    if (kv.first != "data_type" && kv.first != "rounding" && kv.first != "out_of_range" && kv.first != "scalar_map")
      throw ChainError{ZGPU_INVALID_ARGUMENT, "cast_value: unknown field '" + kv.first + "'"};
  std::string target;
  if (d->kind == Json::Str) target = d->s;
  else if (d->kind == Json::Obj && d->get("name") && d->get("name")->kind == Json::Str) target = d->get("name")->s;
  else throw ChainError{ZGPU_INVALID_ARGUMENT, "cast_value: data_type must be a name or {name, configuration}"};
  auto pick = [&](const char *key, std::initializer_list<const char *> names, uint32_t absent) -> uint32_t {
    const Json *v = cfg->get(key);
    if (!v || v->kind == Json::Null) return absent;
    uint32_t i = 0;
    for (const char *n : names) {
      if (v->kind == Json::Str && v->s == n) return i;
      i++;
    }
    throw ChainError{ZGPU_INVALID_ARGUMENT, std::string("cast_value: bad ") + key};
  };
  k.cast_rounding = pick("rounding", {"nearest-even", "towards-zero", "towards-positive", "towards-negative", "nearest-away"},
                         CAST_NEAREST_EVEN);
  const uint32_t oor = pick("out_of_range", {"clamp", "wrap"}, UINT32_MAX);
  k.cast_oor = oor == UINT32_MAX ? (uint32_t)CAST_OOR_NONE : oor + 1;
  // codec_castvalue(): the data types with the cast_value trait that this pipeline takes
  k.vt_dec = value_type_of(T.dt);
  k.vt_enc = value_type_of(target);
  if (k.vt_enc == VT_NONE) throw ChainError{ZGPU_UNSUPPORTED, "cast_value: data_type " + target};
  if (k.vt_dec == VT_NONE) throw ChainError{ZGPU_UNSUPPORTED, "cast_value: on data type " + T.dt};
  if (k.cast_oor == CAST_OOR_WRAP && cast_type_is_float(k.vt_enc))  // validate_wrap_mode: UnsupportedDataType
    throw ChainError{ZGPU_UNSUPPORTED, "cast_value: out_of_range=wrap needs an integer data_type, not " + target};
  if (const Json *sm = cfg->get("scalar_map")) {
    if (sm->kind != Json::Obj && sm->kind != Json::Null)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "cast_value: scalar_map must be {encode?, decode?}"};
    if (sm->kind == Json::Obj) {
      for (const auto &kv : sm->obj)
        if (kv.first != "encode" && kv.first != "decode")
          throw ChainError{ZGPU_INVALID_ARGUMENT, "cast_value: scalar_map: unknown field '" + kv.first + "'"};
      cast_scalar_map(sm->get("encode"), k.vt_dec, T.dt, k.vt_enc, target, k.cast_enc_map);
      cast_scalar_map(sm->get("decode"), k.vt_enc, target, k.vt_dec, T.dt, k.cast_dec_map);
    }
  }
  uint8_t ef[16] = {0}, back[16] = {0};
  bool ok = true;
  cast_encode_element(k, T.fill, ef, false, ok);
  if (!ok) throw ChainError{ZGPU_INVALID_ARGUMENT, "cast_value: the fill value is not representable in " + target};
  cast_encode_element(k, ef, back, true, ok);
  if (!ok || std::memcmp(back, T.fill, T.es) != 0)
    throw ChainError{ZGPU_INVALID_ARGUMENT, "cast_value fill value does not survive a round-trip cast"};
  std::memcpy(T.fill, ef, 16);
  T.dt = target;
  data_type_info(target, T.es, T.comp);
}

bool chain_has_value_codec(const Chain &c) {
  for (const Codec &k : c.a2a)
    if (is_value_codec(k.kind)) return true;
  return c.a2b.kind == CodecKind::Sharding && c.a2b.inner && chain_has_value_codec(*c.a2b.inner);
}

uint64_t packbits_size(const Codec &k, uint64_t nelem) {
  const uint64_t bits = nelem * (uint64_t)(k.pb_last - k.pb_first + 1) * k.pb_ncomp;
  return (bits + 7) / 8 + (k.pb_padding ? 1 : 0);
}

// The array->array codec names (CodecChain::from_metadata sorts the entries by kind, so these are
// bound before the array->bytes codec wherever they stand in the list).
static bool a2a_name(const std::string &n) {
  return n == "transpose" || n == "numcodecs.fixedscaleoffset" || n == "bitround" || n == "numcodecs.bitround" ||
         n == "https://codec.zarrs.dev/array_to_bytes/bitround" || n == "cast_value";
}

// Codec names zarrs itself creates (zarrs/src/array/codec/**: impl_extension_aliases! v3 names and
// aliases) that this pipeline does not implement. zarrs would create and use such a codec even with
// "must_understand": false, so it is an error here rather than a skip (skipping would decode wrongly).
static bool zarrs_knows(const std::string &n) {
  static const char *names[] = {
      "reshape",    "zarrs.squeeze", "numcodecs.pcodec", "zfp",       "zarrs.zfp",      "numcodecs.zfpy",
      "zarrs.vlen", "zarrs.vlen_v2", "vlen-bytes", "vlen-utf8",        "vlen-array", "zarrs.optional", "zarrs.gdeflate"};
  for (const char *k : names)
    if (n == k) return true;
  return n.rfind("https://codec.zarrs.dev/", 0) == 0;
}

// Codec::from_metadata for one entry (zarrs_codec/src/lib.rs:372-449 with the per-codec
// configurations of zarrs_metadata_ext/src/codec/registered/*.rs). Throws ChainError when the codec
// cannot be created (unknown name or invalid configuration).
static Role create_codec(Codec &k, const Json *cfg, TypeCtx &T) {
  const std::string &dt = T.dt;
  const uint32_t es = T.es, comp = T.comp;
  const uint8_t *fill = T.fill;
  auto cfg_get = [&](const char *key) -> const Json * { return cfg ? cfg->get(key) : nullptr; };
  if (k.name == "transpose") {
    k.kind = CodecKind::Transpose;
    const Json *o = cfg_get("order");
    if (!o || o->kind != Json::Arr) throw ChainError{ZGPU_INVALID_ARGUMENT, "transpose: missing order"};
    uint32_t seen = 0;
    for (const Json &v : o->arr) {
      int64_t a = v.as_int();
      if (a < 0 || a >= (int64_t)o->arr.size() || a >= ZGPU_MAX_DIMS || ((seen >> a) & 1))
        throw ChainError{ZGPU_INVALID_ARGUMENT, "transpose: order is not a permutation"};
      seen |= 1u << a;
      k.order.push_back((uint32_t)a);
    }
    return Role::A2A;
  }
  if (k.name == "numcodecs.fixedscaleoffset") {
    // FixedScaleOffsetCodecConfigurationNumcodecs (numcodecs/fixedscaleoffset.rs:17-33): offset, scale
    // (f32), dtype, astype?; deny_unknown_fields. with_context (fixedscaleoffset_codec.rs:436-471)
    k.kind = CodecKind::FixedScaleOffset;
    if (!cfg || cfg->kind != Json::Obj)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.fixedscaleoffset: missing configuration"};
    for (const auto &kv : cfg->obj)
      if (kv.first != "offset" && kv.first != "scale" && kv.first != "dtype" && kv.first != "astype")
        throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.fixedscaleoffset: unknown field '" + kv.first + "'"};
    const Json *o = cfg_get("offset"), *sc = cfg_get("scale"), *d = cfg_get("dtype"), *as = cfg_get("astype");
    if (!o || o->kind != Json::Num || !sc || sc->kind != Json::Num)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.fixedscaleoffset: offset and scale must be numbers"};
    if (!d || d->kind != Json::Str) throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.fixedscaleoffset: missing dtype"};
    if (as && as->kind != Json::Str && as->kind != Json::Null)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.fixedscaleoffset: astype must be a string"};
    k.fso_offset = (float)o->num;
    k.fso_scale = (float)sc->num;
    k.fso_astype = as && as->kind == Json::Str;
    const std::string dec = numpy_to_v3(d->s), enc = k.fso_astype ? numpy_to_v3(as->s) : dec;
    if (dec.empty() || enc.empty())
      throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.fixedscaleoffset: cannot interpret dtype / astype"};
    k.vt_dec = value_type_of(dt);
    if (k.vt_dec > VT_F64 || dec != dt)
      throw ChainError{ZGPU_UNSUPPORTED, "numcodecs.fixedscaleoffset: dtype " + d->s + " on data type " + dt};
    k.vt_enc = value_type_of(enc);
    if (k.vt_enc > VT_F64) throw ChainError{ZGPU_UNSUPPORTED, "numcodecs.fixedscaleoffset: astype " + enc};
    uint8_t ef[16] = {0};
    fso_encode_element(k, fill, ef);  // encode_fill_value: the fill value through the encoder
    std::memcpy(T.fill, ef, 16);
    T.dt = enc;
    data_type_info(enc, T.es, T.comp);
    return Role::A2A;
  }
  if (k.name == "bitround" || k.name == "numcodecs.bitround" ||
      k.name == "https://codec.zarrs.dev/array_to_bytes/bitround") {
    // BitroundCodecConfigurationV1 (numcodecs/bitround.rs:17-22): keepbits (u32), deny_unknown_fields. The
    // data type stays; the encoded fill value is the rounded fill value (bitround_codec.rs)
    k.kind = CodecKind::BitRound;
    if (!cfg || cfg->kind != Json::Obj) throw ChainError{ZGPU_INVALID_ARGUMENT, "bitround: missing configuration"};
    for (const auto &kv : cfg->obj)
      if (kv.first != "keepbits") throw ChainError{ZGPU_INVALID_ARGUMENT, "bitround: unknown field '" + kv.first + "'"};
    const Json *kb = cfg_get("keepbits");
    if (!kb || kb->kind != Json::Num || !kb->is_int || kb->i < 0 || kb->i > (int64_t)UINT32_MAX)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "bitround: keepbits must be a non-negative integer"};
    k.keepbits = (uint32_t)kb->i;
    k.vt_dec = k.vt_enc = value_type_of(dt);
    if (k.vt_dec == VT_NONE) throw ChainError{ZGPU_UNSUPPORTED, "bitround: data type " + dt};
    bitround_element(k.vt_dec, k.keepbits, T.fill);
    return Role::A2A;
  }
  if (k.name == "cast_value") {
    create_cast_value(k, cfg, T);
    return Role::A2A;
  }
  if (k.name == "packbits") {
    // PackBitsCodecConfigurationV1 (registered/packbits.rs:36-53): padding_encoding?, first_bit?, last_bit?;
    // deny_unknown_fields. with_context (packbits_codec.rs:152-180) binds the bit range to the data type
    k.kind = CodecKind::PackBits;
    if (cfg && cfg->kind != Json::Obj) throw ChainError{ZGPU_INVALID_ARGUMENT, "packbits: bad configuration"};
    if (cfg)
      for (const auto &kv : cfg->obj)
        if (kv.first != "padding_encoding" && kv.first != "first_bit" && kv.first != "last_bit")
          throw ChainError{ZGPU_INVALID_ARGUMENT, "packbits: unknown field '" + kv.first + "'"};
    if (const Json *pe = cfg_get("padding_encoding")) {
      if (pe->kind == Json::Str && pe->s == "first_byte") k.pb_padding = 1;
      else if (pe->kind == Json::Str && pe->s == "last_byte") k.pb_padding = 2;
      else if (!(pe->kind == Json::Null || (pe->kind == Json::Str && pe->s == "none")))
        throw ChainError{ZGPU_INVALID_ARGUMENT, "packbits: padding_encoding must be none, first_byte or last_byte"};
    }
    auto bit = [&](const char *key, int64_t def) -> int64_t {
      const Json *b = cfg_get(key);
      if (!b || b->kind == Json::Null) return def;
      if (b->kind != Json::Num || !b->is_int || b->i < 0)
        throw ChainError{ZGPU_INVALID_ARGUMENT, std::string("packbits: ") + key + " must be a non-negative integer"};
      return b->i;
    };
    // components (zarrs_data_type impl_pack_bits_data_type_traits!): bool is one bit; the complex types
    // are two float components; only the signed integers sign-extend
    k.pb_comp_bits = dt == "bool" ? 1 : 8 * comp;
    k.pb_ncomp = es / comp;
    k.pb_signed = dt == "int8" || dt == "int16" || dt == "int32" || dt == "int64";
    const int64_t first = bit("first_bit", 0), last = bit("last_bit", (int64_t)k.pb_comp_bits - 1);
    if (last < first) throw ChainError{ZGPU_INVALID_ARGUMENT, "packbits: last_bit is less than first_bit"};
    if (last >= (int64_t)k.pb_comp_bits)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "packbits: last_bit is outside the data type component"};
    k.pb_first = (uint32_t)first;
    k.pb_last = (uint32_t)last;
    if (k.pb_comp_bits % 8 == 0 && first == 0 && last == (int64_t)k.pb_comp_bits - 1) {
      // the whole component of a byte-sized type: PackBitsCodecBound encodes and decodes through
      // BytesCodec(little) and writes no padding byte (packbits_codec.rs:230-240,312-319)
      k.kind = CodecKind::Bytes;
      k.big_endian = false;
    }
    return Role::A2B;
  }
  if (k.name == "bytes" || k.name == "endian") {  // "endian": legacy alias (array_to_bytes/bytes.rs:53-55)
    k.kind = CodecKind::Bytes;
    const Json *e = cfg_get("endian");
    if (e && e->kind == Json::Str) {
      if (e->s == "big") k.big_endian = true;
      else if (e->s != "little") throw ChainError{ZGPU_INVALID_ARGUMENT, "bytes: bad endian"};
    } else if (comp > 1) {
      // BytesCodecEndiannessMissingError (zarrs_data_type/src/codec_traits/bytes.rs:109-110)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "bytes: endian required for multi-byte data types"};
    }
    return Role::A2B;
  }
  if (k.name == "sharding_indexed") {
    k.kind = CodecKind::Sharding;
    const Json *cs = cfg_get("chunk_shape");
    if (!cs || cs->kind != Json::Arr) throw ChainError{ZGPU_INVALID_ARGUMENT, "sharding: missing chunk_shape"};
    for (const Json &v : cs->arr) {
      int64_t s = v.as_int();
      if (s <= 0) throw ChainError{ZGPU_INVALID_ARGUMENT, "sharding: chunk_shape must be positive"};
      k.inner_shape.push_back((uint64_t)s);
    }
    const Json *ic = cfg_get("codecs");
    if (!ic) throw ChainError{ZGPU_INVALID_ARGUMENT, "sharding: missing codecs"};
    k.inner = parse(*ic, dt, es, comp, fill);
    if (k.inner->a2b.kind == CodecKind::PackBits)
      throw ChainError{ZGPU_UNSUPPORTED, "packbits as the array->bytes codec inside sharding_indexed is not supported "
                                         "by the GPU pipeline (unsharded packbits chains are)"};
    Json defidx = Json::parse(R"([{"name":"bytes","configuration":{"endian":"little"}},{"name":"crc32c"}])");
    const Json *xc = cfg_get("index_codecs");
    const uint8_t ffill[8] = {0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff};
    k.index = parse(xc ? *xc : defidx, "uint64", 8, 8, ffill);
    const Json *loc = cfg_get("index_location");
    if (loc && loc->kind == Json::Str) {
      if (loc->s == "start") k.at_start = true;
      else if (loc->s != "end") throw ChainError{ZGPU_INVALID_ARGUMENT, "sharding: bad index_location"};
    }
    return Role::A2B;
  }
  if (k.name == "crc32c" || k.name == "numcodecs.crc32c") {
    k.kind = CodecKind::Crc32c;
    const Json *loc = cfg_get("location");
    if (loc && loc->kind == Json::Str && loc->s == "start") k.at_start = true;
  } else if (k.name == "gzip") {
    k.kind = CodecKind::Gzip;
    const Json *l = cfg_get("level");
    k.level = l ? (int)l->as_int() : 5;
  } else if (k.name == "numcodecs.zlib") {
    // ZlibCodecConfigurationV1 (zlib.rs:46-49): level 0..9, required
    k.kind = CodecKind::Zlib;
    const Json *l = cfg_get("level");
    if (!l || l->kind != Json::Num || !l->is_int || l->i < 0 || l->i > 9)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.zlib: level must be an integer 0..9"};
    k.level = (int)l->i;
  } else if (k.name == "numcodecs.bz2" || k.name == "https://codec.zarrs.dev/bytes_to_bytes/bz2") {
    // Bz2CodecConfigurationV1 (bz2.rs): level 0..9, required; deny_unknown_fields. Decode reads the block
    // size from the stream's own header digit
    k.kind = CodecKind::Bz2;
    if (!cfg || cfg->kind != Json::Obj) throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.bz2: missing configuration"};
    for (const auto &kv : cfg->obj)
      if (kv.first != "level") throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.bz2: unknown field '" + kv.first + "'"};
    const Json *l = cfg_get("level");
    if (!l || l->kind != Json::Num || !l->is_int || l->i < 0 || l->i > 9)
      throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.bz2: level must be an integer 0..9"};
    k.level = (int)l->i;
  } else if (k.name == "numcodecs.adler32") {
    // Adler32CodecConfigurationV1 (adler32.rs:47-59): location "start" (the default, unlike crc32c) / "end"
    k.kind = CodecKind::Adler32;
    k.at_start = true;
    if (const Json *loc = cfg_get("location")) {
      if (loc->kind == Json::Str && loc->s == "end") k.at_start = false;
      else if (!(loc->kind == Json::Str && loc->s == "start"))
        throw ChainError{ZGPU_INVALID_ARGUMENT, "numcodecs.adler32: location must be \"start\" or \"end\""};
    }
  } else if (k.name == "numcodecs.fletcher32" || k.name == "https://codec.zarrs.dev/bytes_to_bytes/fletcher32") {
    k.kind = CodecKind::Fletcher32;  // no configuration (fletcher32.rs:47-49); the value sits at the end
  } else if (k.name == "zstd" || k.name == "numcodecs.zstd") {
    k.kind = CodecKind::Zstd;
    const Json *l = cfg_get("level");
    k.level = l ? (int)l->as_int() : 0;
    const Json *cs = cfg_get("checksum");
    k.checksum = cs && cs->kind == Json::Bool && cs->b;
  } else if (k.name == "blosc" || k.name == "numcodecs.blosc") {
    // blosc_codec_via_blosc_src.rs: cname / clevel / shuffle / typesize / blocksize; the decoder
    // reads everything it needs (compressor, shuffle, typesize, block size) from the frame header
    k.kind = CodecKind::Blosc;
    const Json *cn = cfg_get("cname");
    k.cname = cn && cn->kind == Json::Str ? cn->s : "lz4";
    static const char *known[] = {"blosclz", "lz4", "lz4hc", "snappy", "zlib", "zstd"};
    bool ok = false;
    for (const char *n : known) ok = ok || k.cname == n;
    if (!ok) throw ChainError{ZGPU_INVALID_ARGUMENT, "blosc: unknown cname '" + k.cname + "'"};
    const Json *l = cfg_get("clevel");
    k.level = l ? (int)l->as_int() : 5;
    const Json *t = cfg_get("typesize");
    k.elementsize = t && t->kind != Json::Null ? (uint32_t)t->as_int() : 0;
    // shuffle: "noshuffle" / "shuffle" / "bitshuffle" (V3), 0 / 1 / 2 / -1 = auto (numcodecs: bit
    // shuffle for 1-byte items, else byte shuffle)
    if (const Json *sh = cfg_get("shuffle")) {
      if (sh->kind == Json::Str) {
        k.shuffle = sh->s == "noshuffle" ? 0 : sh->s == "shuffle" ? 1 : sh->s == "bitshuffle" ? 2 : -2;
        if (k.shuffle == -2) throw ChainError{ZGPU_INVALID_ARGUMENT, "blosc: unknown shuffle '" + sh->s + "'"};
      } else if (sh->kind != Json::Null) {
        const int v = (int)sh->as_int();
        k.shuffle = v == -1 ? (k.elementsize == 1 ? 2 : 1) : v;
        if (k.shuffle < 0 || k.shuffle > 2) throw ChainError{ZGPU_INVALID_ARGUMENT, "blosc: shuffle out of range"};
      }
    }
    const Json *bsz = cfg_get("blocksize");
    k.blocksize = bsz && bsz->kind != Json::Null ? (uint64_t)bsz->as_int() : 0;
  } else if (k.name == "numcodecs.shuffle" || k.name == "shuffle") {
    k.kind = CodecKind::Shuffle;
    const Json *e = cfg_get("elementsize");
    k.elementsize = e ? (uint32_t)e->as_int() : 4;
    if (k.elementsize == 0) throw ChainError{ZGPU_INVALID_ARGUMENT, "shuffle: elementsize must be > 0"};
  } else {
    throw ChainError{ZGPU_UNSUPPORTED, "codec '" + k.name + "' is not supported by the GPU pipeline"};
  }
  return Role::B2B;
}

// CodecChain::from_metadata (codec_chain.rs:192-229): every entry is created and sorted by its kind
// (array->array, array->bytes, bytes->bytes; metadata order kept within each kind); an entry that
// cannot be created is skipped when it says "must_understand": false (:197-206); exactly one
// array->bytes codec. MetadataV3 accepts "name" or {name, configuration?, must_understand?} and
// nothing else (zarrs_metadata/src/v3/metadata.rs:114-149).
static std::shared_ptr<Chain> parse(const Json &codecs, const std::string &dt, uint32_t es, uint32_t comp,
                                    const uint8_t *fill) {
  if (codecs.kind != Json::Arr) throw ChainError{ZGPU_INVALID_ARGUMENT, "codecs must be a JSON array"};
  auto c = std::make_shared<Chain>();
  c->es = es;
  c->comp = comp;
  c->data_type = dt;
  if (fill) std::memcpy(c->fill, fill, es);
  TypeCtx T{dt, es, comp, {0}};
  std::memcpy(T.fill, c->fill, 16);
  struct Entry {
    Codec k;
    const Json *cfg = nullptr;
    bool must_understand = true;
  };
  std::vector<Entry> entries;
  for (const Json &m : codecs.arr) {
    Entry e;
    if (m.kind == Json::Str) {
      e.k.name = m.s;
    } else if (m.kind == Json::Obj && m.get("name") && m.get("name")->kind == Json::Str) {
      for (const auto &kv : m.obj)
        if (kv.first != "name" && kv.first != "configuration" && kv.first != "must_understand")
          throw ChainError{ZGPU_INVALID_ARGUMENT, "codec metadata: unknown field '" + kv.first + "'"};
      e.k.name = m.get("name")->as_str();
      e.cfg = m.get("configuration");
      if (const Json *mu = m.get("must_understand")) {
        if (mu->kind != Json::Bool) throw ChainError{ZGPU_INVALID_ARGUMENT, "must_understand must be a bool"};
        e.must_understand = mu->b;
      }
    } else {
      throw ChainError{ZGPU_INVALID_ARGUMENT, "codec metadata must be \"name\" or {name, configuration}"};
    }
    entries.push_back(e);
  }
  // the array->array codecs first, in metadata order: each is bound with the data type and fill value
  // the one before it left (with_context, codec_chain.rs:130-160), the others with the last one's
  bool have_a2b = false;
  for (int pass = 0; pass < 2; pass++)
    for (Entry &e : entries) {
      if (a2a_name(e.k.name) != (pass == 0)) continue;
      Codec &k = e.k;
      Role role;
      try {
        role = create_codec(k, e.cfg, T);
      } catch (const ChainError &err) {
        // zarrs skips an optional codec it cannot create (unknown name or invalid configuration); a
        // codec zarrs would create but the GPU pipeline lacks, or cannot bind to this data type, stays
        // an error
        if (e.must_understand || (err.status == ZGPU_UNSUPPORTED && (zarrs_knows(k.name) || a2a_name(k.name) ||
                                                                     k.name == "packbits")))
          throw;
        continue;
      }
      if (role == Role::A2A) {
        c->a2a.push_back(k);
      } else if (role == Role::A2B) {
        if (have_a2b) throw ChainError{ZGPU_INVALID_ARGUMENT, "multiple array to bytes codecs"};
        c->a2b = k;
        have_a2b = true;
      } else {
        c->b2b.push_back(k);
      }
    }
  if (!have_a2b) throw ChainError{ZGPU_INVALID_ARGUMENT, "missing array to bytes codec"};
  c->enc_es = T.es;
  c->enc_comp = T.comp;
  c->enc_data_type = T.dt;
  std::memcpy(c->enc_fill, T.fill, 16);
  return c;
}

std::shared_ptr<Chain> parse_chain(const Json &codecs, const std::string &dt, const uint8_t *fill) {
  uint32_t es, comp;
  if (!data_type_info(dt, es, comp)) throw ChainError{ZGPU_UNSUPPORTED, "data type '" + dt + "'"};
  return parse(codecs, dt, es, comp, fill);
}

uint64_t gzip_bound(uint64_t n) { return n + 10 + 8 + (n + 7) / 8 + (n + 63) / 64 + 5; }

// ZlibCodec::encoded_representation (zlib/zlib_codec.rs): zlib's compressBound
uint64_t zlib_bound(uint64_t n) { return n + (n >> 12) + (n >> 14) + (n >> 25) + 13; }

// ZstdCodec::encoded_representation (zstd_codec.rs:132-147): header/trailer 4 + 14 + 4 bytes and a
// 3-byte block header per 1000 bytes
uint64_t zstd_bound(uint64_t n) { return n + 4 + 14 + 4 + 3 * ((n + 999) / 1000); }

// Bz2Codec::encoded_representation (bz2/bz2_codec.rs)
uint64_t bz2_bound(uint64_t n) { return n + n / 8 + 1024; }

int64_t codec_encoded_bound(const Codec &k, uint64_t n, bool *fixed) {
  if (is_checksum(k.kind)) return (int64_t)(n + 4);
  if (k.kind == CodecKind::Shuffle) return (int64_t)n;
  if (fixed) *fixed = false;
  switch (k.kind) {
    case CodecKind::Gzip: return (int64_t)gzip_bound(n);
    case CodecKind::Zlib: return (int64_t)zlib_bound(n);  // k_gzip_encode keeps to it (zlib_bounded)
    case CodecKind::Zstd: return (int64_t)zstd_bound(n);
    case CodecKind::Bz2: return (int64_t)bz2_bound(n);
    case CodecKind::Blosc: return (int64_t)(n + 16);  // BLOSC_MAX_OVERHEAD (blosc_via_blosc_src.rs:80)
    default: return -1;
  }
}

// the array->bytes codec's bytes through every bytes->bytes codec; -1 if unbounded, or not fixed when asked
static int64_t chain_size(const Chain &c, uint64_t nelem, bool want_fixed) {
  if (c.a2b.kind != CodecKind::Bytes && c.a2b.kind != CodecKind::PackBits) return -1;
  int64_t n = (int64_t)(c.a2b.kind == CodecKind::PackBits ? packbits_size(c.a2b, nelem) : nelem * c.enc_es);
  bool fixed = true;
  for (const Codec &k : c.b2b) {
    n = codec_encoded_bound(k, (uint64_t)n, &fixed);
    if (n < 0 || (want_fixed && !fixed)) return -1;
  }
  return n;
}

int64_t chain_fixed_encoded_size(const Chain &c, uint64_t nelem) { return chain_size(c, nelem, true); }
int64_t chain_encoded_bound(const Chain &c, uint64_t nelem) { return chain_size(c, nelem, false); }

}  // namespace zgpu
