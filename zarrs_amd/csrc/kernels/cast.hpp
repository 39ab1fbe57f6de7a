// Element semantics of the cast_value codec, shared by the kernel (k_cast in kernels/value.hip) and the
// host (the encoded fill value and the bind-time round trip, chain.cpp). Reference: zarrs_data_type/src/
// codec_traits/cast_value.rs (cast_scalar_to_*_integer, float_quantity_from_f64, round_f64_to_*) and
// cast_value/kernels.rs (round_int_to_f64, kernel_float_to_int), zarrs/src/array/codec/array_to_array/
// cast_value/cast_value_codec.rs (the scalar map: exact bytes, before the cast).
//
// Everything is 64-bit integer arithmetic and `double`:
//  * a float of any of the four widths reads as an exact double (float16 / bfloat16 by their bits);
//  * rounding to a float format is one pass over the double's own bits (round_to_format), in the asked
//    mode, subnormals kept -- never through a narrower hardware conversion, so nothing rounds twice;
//  * an integer rounds once from its exact magnitude to the target's precision (the reference's
//    round_int_to_f64), then that double, which the target holds exactly, is packed;
//  * float -> integer is a range test on the rounded double followed by a cast of an in-range value; what
//    lies beyond 2^63 wraps through the double's bits (a multiple of 2^11 there), so no 128-bit integers.
// This header includes nothing of the library and compiles as plain C++ (tests/c/cast_value_harness.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <type_traits>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZG_HD __host__ __device__
#else
#define ZG_HD
#endif

namespace zgpu {

enum CastRounding : uint32_t { CAST_NEAREST_EVEN, CAST_TOWARDS_ZERO, CAST_TOWARDS_POSITIVE, CAST_TOWARDS_NEGATIVE,
                               CAST_NEAREST_AWAY };
enum CastOutOfRange : uint32_t { CAST_OOR_NONE, CAST_OOR_CLAMP, CAST_OOR_WRAP };

// The 12 element types, numbered as ZgValueType (chain.hpp; chain.cpp asserts the match).
enum : uint32_t { CT_I8, CT_I16, CT_I32, CT_I64, CT_U8, CT_U16, CT_U32, CT_U64, CT_F32, CT_F64, CT_F16, CT_BF16, CT_COUNT };

// float16 / bfloat16 elements: their bits, nothing else
struct f16_t { uint16_t bits; };
struct bf16_t { uint16_t bits; };

constexpr uint32_t CAST_MAP_MAX = 32;
// scalar_map of one direction: key[i] is a source element's bits, val[i] the target element's, both
// zero-extended; the first matching entry wins
struct CastMap {
  uint32_t n;
  uint32_t pad_;
  uint64_t key[CAST_MAP_MAX], val[CAST_MAP_MAX];
};

// P: significand digits with the hidden bit; EB: exponent bits
template <class T> struct cast_fmt { static constexpr bool is_float = false; };
template <> struct cast_fmt<f16_t> { static constexpr bool is_float = true; static constexpr int P = 11, EB = 5; using bits_t = uint16_t; };
template <> struct cast_fmt<bf16_t> { static constexpr bool is_float = true; static constexpr int P = 8, EB = 8; using bits_t = uint16_t; };
template <> struct cast_fmt<float> { static constexpr bool is_float = true; static constexpr int P = 24, EB = 8; using bits_t = uint32_t; };
template <> struct cast_fmt<double> { static constexpr bool is_float = true; static constexpr int P = 53, EB = 11; using bits_t = uint64_t; };

ZG_HD inline uint64_t dbl_bits(double d) {
  uint64_t u;
  memcpy(&u, &d, 8);
  return u;
}
ZG_HD inline double dbl_from(uint64_t u) {
  double d;
  memcpy(&d, &u, 8);
  return d;
}
ZG_HD inline uint32_t clz64(uint64_t x) { return (uint32_t)__builtin_clzll((unsigned long long)x); }  // x != 0

// an element's bits, zero-extended (the scalar map compares these)
template <class T>
ZG_HD inline uint64_t cast_bits(T x) {
  typename std::conditional<sizeof(T) == 1, uint8_t, typename std::conditional<sizeof(T) == 2, uint16_t,
      typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type>::type>::type u;
  memcpy(&u, &x, sizeof(T));
  return (uint64_t)u;
}
template <class T>
ZG_HD inline T cast_from_bits(uint64_t b) {
  typename std::conditional<sizeof(T) == 1, uint8_t, typename std::conditional<sizeof(T) == 2, uint16_t,
      typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type>::type>::type u = (decltype(u))b;
  T x;
  memcpy(&x, &u, sizeof(T));
  return x;
}

// bits of a (P, EB) float -> the double of the same value (exact: every such value is a double); NaN of
// any payload becomes a NaN
template <int P, int EB>
ZG_HD inline double format_to_double(uint64_t b) {
  if (P == 53) return dbl_from(b);
  const uint64_t sign = (b >> (P - 1 + EB)) & 1, ef = (b >> (P - 1)) & (((uint64_t)1 << EB) - 1);
  uint64_t m = b & (((uint64_t)1 << (P - 1)) - 1);
  const int bias = (1 << (EB - 1)) - 1;
  uint64_t out;
  if (ef == (((uint64_t)1 << EB) - 1)) {
    out = 0x7ff0000000000000ull | (m ? 0x0008000000000000ull : 0);
  } else if (ef == 0) {
    if (!m) {
      out = 0;
    } else {  // subnormal: m * 2^(1 - bias - (P - 1)); normalise
      const int top = 63 - (int)clz64(m);                          // m's highest set bit
      const int e = top + 1 - bias - (P - 1);                      // the value's exponent
      out = ((uint64_t)(e + 1023) << 52) | ((m << (52 - top)) & 0x000fffffffffffffull);
    }
  } else {
    out = ((uint64_t)((int)ef - bias + 1023) << 52) | (m << (53 - P));
  }
  return dbl_from(out | (sign << 63));
}

template <class F>
ZG_HD inline double cast_to_double(F x) {
  return format_to_double<cast_fmt<F>::P, cast_fmt<F>::EB>(cast_bits(x));
}

// whether rounding magnitude bits (kept | rem) away from zero is asked: rem the discarded bits below
// `half`'s place * 2, `odd` the kept part's last bit
ZG_HD inline bool cast_round_up(uint32_t rounding, bool negative, bool odd, bool rem_nonzero, bool rem_ge_half,
                                bool rem_gt_half) {
  switch (rounding) {
    case CAST_NEAREST_EVEN: return rem_gt_half || (rem_ge_half && odd);
    case CAST_TOWARDS_ZERO: return false;
    case CAST_TOWARDS_POSITIVE: return !negative && rem_nonzero;
    case CAST_TOWARDS_NEGATIVE: return negative && rem_nonzero;
    default: return rem_ge_half;  // nearest, ties away from zero
  }
}

// A finite double, |v| <= the format's largest finite value, rounded once to the (P, EB) format in the
// asked mode; +-inf passes. Returns the format's bits. Subnormal results are kept, -0.0 stays -0.0, and
// a value that rounds below the smallest subnormal becomes a signed zero (or that subnormal, by the mode).
template <int P, int EB>
ZG_HD inline uint64_t round_to_format(double v, uint32_t rounding) {
  const uint64_t b = dbl_bits(v);
  if (P == 53) return b;
  const uint64_t sign = b >> 63;
  const uint64_t sbit = sign << (P - 1 + EB);
  const uint32_t ef = (uint32_t)((b >> 52) & 0x7ff);
  uint64_t m = b & 0x000fffffffffffffull;
  if (ef == 0x7ff) return sbit | ((((uint64_t)1 << EB) - 1) << (P - 1));  // inf
  if (ef == 0 && m == 0) return sbit;
  int e = (int)ef - 1023;
  if (ef == 0) e = -1022;  // a double subnormal: no hidden bit
  else m |= (uint64_t)1 << 52;
  const int bias = (1 << (EB - 1)) - 1, emin = 1 - bias;
  const int et = e > emin ? e : emin;  // the exponent the result is quantised at
  const int sh = et - e + 53 - P;      // > 0: P < 53
  uint64_t kept;
  bool nz, ge, gt;
  if (sh >= 64) {
    kept = 0;
    nz = true;
    ge = gt = false;
  } else {
    kept = m >> sh;
    const uint64_t rem = m & (((uint64_t)1 << sh) - 1), half = (uint64_t)1 << (sh - 1);
    nz = rem != 0;
    ge = rem >= half;
    gt = rem > half;
  }
  if (cast_round_up(rounding, sign != 0, (kept & 1) != 0, nz, ge, gt)) kept++;
  // kept holds the hidden bit for a normal result (adding 1 to the exponent field below), none for a
  // subnormal one; a carry out of the significand moves into the exponent by the same addition
  return sbit | ((((uint64_t)(et + bias - 1)) << (P - 1)) + kept);
}

// the largest finite value of a float format, as a double
template <int P, int EB>
ZG_HD inline double format_max() {
  const int bias = (1 << (EB - 1)) - 1;
  const uint64_t frac = ((((uint64_t)1 << (P - 1)) - 1) << (53 - P));
  return dbl_from(((uint64_t)(bias + 1023) << 52) | frac);
}

// float_quantity_from_f64 for a target with NaN and infinities: v (no NaN) -> the double to round; *ok
// cleared when v is finite, outside [-max, max] and out_of_range is absent
template <int P, int EB>
ZG_HD inline double cast_float_quantity(double v, uint32_t rounding, uint32_t oor, bool &ok) {
  const double mx = format_max<P, EB>(), inf = dbl_from(0x7ff0000000000000ull);
  if (v >= -mx && v <= mx) return v;
  if (v == inf || v == -inf) return v;
  if (oor == CAST_OOR_NONE) {
    ok = false;
    return 0.0;
  }
  const bool neg = v < 0;
  if (oor == CAST_OOR_CLAMP) return neg ? -inf : inf;
  // wrap (decode of an integer-encoded float array only): the overflow by the rounding mode
  const bool to_bound = rounding == CAST_TOWARDS_ZERO ||
                        rounding == (neg ? (uint32_t)CAST_TOWARDS_POSITIVE : (uint32_t)CAST_TOWARDS_NEGATIVE);
  return to_bound ? (neg ? -mx : mx) : (neg ? -inf : inf);
}

// An integer's magnitude rounded once to `digits` significant bits (round_int_to_f64), as the exact
// double of the result.
ZG_HD inline double round_magnitude(uint64_t mag, bool negative, int digits, uint32_t rounding) {
  double r;
  const int sig = mag ? 64 - (int)clz64(mag) : 0;
  if (sig <= digits) {
    r = (double)mag;  // at most 53 significant bits: exact
  } else {
    const int sh = sig - digits;
    const uint64_t unit = (uint64_t)1 << sh, rem = mag & (unit - 1), half = unit >> 1;
    uint64_t t = mag - rem;
    if (cast_round_up(rounding, negative, ((mag >> sh) & 1) != 0, rem != 0, rem >= half, rem > half)) {
      t += unit;
      if (t == 0) return negative ? -18446744073709551616.0 : 18446744073709551616.0;  // carried to 2^64
    }
    r = (double)t;  // `digits` significant bits: exact
  }
  return negative ? -r : r;
}

ZG_HD inline double cast_round_integral(double v, uint32_t rounding) {
  switch (rounding) {
    case CAST_NEAREST_EVEN: return rint(v);  // the default rounding direction is never changed
    case CAST_TOWARDS_ZERO: return trunc(v);
    case CAST_TOWARDS_POSITIVE: return ceil(v);
    case CAST_TOWARDS_NEGATIVE: return floor(v);
    default: return round(v);
  }
}

// the low 64 bits of the two's complement of an integer-valued finite double (exact at any magnitude)
ZG_HD inline uint64_t integral_low64(double r) {
  const uint64_t b = dbl_bits(r);
  const int ef = (int)((b >> 52) & 0x7ff);
  if (ef == 0) return 0;  // integer-valued and below 2^-1022: zero
  const uint64_t m = (b & 0x000fffffffffffffull) | ((uint64_t)1 << 52);
  const int k = ef - 1023 - 52;  // r = m * 2^k
  uint64_t low;
  if (k >= 64) low = 0;
  else if (k >= 0) low = m << k;
  else if (k > -64) low = m >> -k;  // integer-valued: the dropped bits are zero
  else low = 0;
  return (b >> 63) ? (uint64_t)0 - low : low;
}

// a two's complement pattern reduced modulo 2^bits(T)
template <class T>
ZG_HD inline T cast_wrap(uint64_t pattern) {
  using U = typename std::make_unsigned<T>::type;
  const U u = (U)pattern;
  T t;
  memcpy(&t, &u, sizeof(T));
  return t;
}

// One element S -> T. *ok is cleared (and 0 returned) when the value is not representable
// (CastValueError::NotRepresentable); it is never set.
template <class S, class T>
ZG_HD inline T cast_one(S x, uint32_t rounding, uint32_t oor, bool &ok) {
  constexpr bool s_float = cast_fmt<S>::is_float, t_float = cast_fmt<T>::is_float;
  if constexpr (!s_float && !t_float) {
    // integer -> integer: range check, then clamp / wrap
    using L = std::numeric_limits<T>;
    bool below = false, above = false;
    if constexpr (std::is_signed<S>::value) {
      if constexpr (std::is_signed<T>::value) {
        below = (int64_t)x < (int64_t)L::min();
        above = (int64_t)x > (int64_t)L::max();
      } else {
        below = x < 0;
        above = x > 0 && (uint64_t)x > (uint64_t)L::max();
      }
    } else {
      above = (uint64_t)x > (uint64_t)L::max();
    }
    if (!below && !above) return (T)x;
    if (oor == CAST_OOR_CLAMP) return below ? L::min() : L::max();
    if (oor == CAST_OOR_WRAP) return cast_wrap<T>((uint64_t)x);  // sign-extended for a signed source
    ok = false;
    return 0;
  } else if constexpr (s_float && !t_float) {
    using L = std::numeric_limits<T>;
    const double v = cast_to_double(x);
    if (!(v - v == 0.0)) {  // NaN, +-inf: never representable
      ok = false;
      return 0;
    }
    const double r = cast_round_integral(v, rounding);
    const double lo = (double)L::min();                          // 0 or -2^(N-1)
    const double hi_excl = (double)(L::max() / 2 + 1) * 2.0;     // 2^N or 2^(N-1)
    if (r >= lo && r < hi_excl) return (T)r;                     // in range: exact
    if (oor == CAST_OOR_CLAMP) return r < 0 ? L::min() : L::max();
    if (oor == CAST_OOR_WRAP) return cast_wrap<T>(integral_low64(r));
    ok = false;
    return 0;
  } else {
    constexpr int P = cast_fmt<T>::P, EB = cast_fmt<T>::EB;
    double q;
    if constexpr (!s_float) {
      // an integer every bit of which the target holds: exact, never out of range
      if constexpr (std::numeric_limits<S>::digits <= P && (std::is_same<T, float>::value ||
                                                            std::is_same<T, double>::value)) {
        return (T)x;
      } else {
        const bool neg = std::is_signed<S>::value && x < 0;
        const uint64_t mag = neg ? (uint64_t)0 - (uint64_t)(int64_t)x : (uint64_t)x;
        // the range check is on the exact value: only float16 has integers of 64 bits beyond it, and
        // those near its bound are exact doubles
        if (EB == 5 && mag > 65504) q = cast_float_quantity<P, EB>(neg ? -(double)mag : (double)mag, rounding, oor, ok);
        else q = round_magnitude(mag, neg, P, rounding);
      }
    } else {
      const double v = cast_to_double(x);
      if (v != v) {  // the target's canonical NaN: sign and payload are not kept (the reference: f64::NAN)
        return cast_from_bits<T>((((uint64_t)1 << (EB + 1)) - 1) << (P - 2));
      }
      q = cast_float_quantity<P, EB>(v, rounding, oor, ok);
    }
    if (!ok) return cast_from_bits<T>(0);
    return cast_from_bits<T>(round_to_format<P, EB>(q, rounding));
  }
}

// The scalar map, then the cast.
template <class S, class T>
ZG_HD inline T cast_mapped(S x, const CastMap &map, uint32_t rounding, uint32_t oor, bool &ok) {
  if (map.n) {
    const uint64_t b = cast_bits(x);
    for (uint32_t i = 0; i < map.n; i++)
      if (map.key[i] == b) return cast_from_bits<T>(map.val[i]);
  }
  return cast_one<S, T>(x, rounding, oor, ok);
}

// ---- by type number --------------------------------------------------------------------------------

ZG_HD inline bool cast_type_is_float(uint32_t ct) { return ct >= CT_F32 && ct < CT_COUNT; }
ZG_HD inline bool cast_type_is_signed(uint32_t ct) { return ct <= CT_I64; }
ZG_HD inline uint32_t cast_type_size(uint32_t ct) {
  return ct == CT_F32 ? 4 : ct == CT_F64 ? 8 : ct >= CT_F16 ? 2 : 1u << (ct & 3);
}

// Whether no element of type s can fail to cast to type t.
ZG_HD inline bool cast_infallible(uint32_t s, uint32_t t, uint32_t oor) {
  const bool sf = cast_type_is_float(s), tf = cast_type_is_float(t);
  if (sf && !tf) return false;  // NaN and the infinities
  if (oor != CAST_OOR_NONE) return true;
  if (!sf && !tf) {
    const uint32_t sb = 8 * cast_type_size(s), tb = 8 * cast_type_size(t);
    const bool ss = cast_type_is_signed(s), ts = cast_type_is_signed(t);
    if (ss == ts) return tb >= sb;
    return !ss && tb > sb;  // unsigned into a wider signed; signed never fits unsigned
  }
  if (!sf) return t != CT_F16 || s == CT_I8 || s == CT_U8 || s == CT_I16;  // float16: integers past 65504
  auto rank = [](uint32_t f) { return f == CT_F16 ? 0 : f == CT_BF16 ? 1 : f == CT_F32 ? 2 : 3; };  // by largest value
  return rank(t) >= rank(s);
}

template <class F>
inline bool with_cast_type(uint32_t ct, F &&f) {
  switch (ct) {
    case CT_I8: f(int8_t{}); return true;
    case CT_I16: f(int16_t{}); return true;
    case CT_I32: f(int32_t{}); return true;
    case CT_I64: f(int64_t{}); return true;
    case CT_U8: f(uint8_t{}); return true;
    case CT_U16: f(uint16_t{}); return true;
    case CT_U32: f(uint32_t{}); return true;
    case CT_U64: f(uint64_t{}); return true;
    case CT_F32: f(float{}); return true;
    case CT_F64: f(double{}); return true;
    case CT_F16: f(f16_t{}); return true;
    case CT_BF16: f(bf16_t{}); return true;
    default: return false;
  }
}

// n elements on the host, unaligned bytes in and out; returns the index of the first element that cannot
// be cast (its output and the following are not written), or n.
inline uint64_t cast_elements_host(uint32_t s, uint32_t t, const uint8_t *in, uint8_t *out, uint64_t n,
                                   const CastMap &map, uint32_t rounding, uint32_t oor) {
  uint64_t bad = n;
  with_cast_type(s, [&](auto sv) {
    using S = decltype(sv);
    with_cast_type(t, [&](auto tv) {
      using T = decltype(tv);
      for (uint64_t i = 0; i < n; i++) {
        S x;
        memcpy(&x, in + i * sizeof(S), sizeof(S));
        bool ok = true;
        const T y = cast_mapped<S, T>(x, map, rounding, oor, ok);
        if (!ok) {
          bad = i;
          return;
        }
        memcpy(out + i * sizeof(T), &y, sizeof(T));
      }
    });
  });
  return bad;
}

}  // namespace zgpu
