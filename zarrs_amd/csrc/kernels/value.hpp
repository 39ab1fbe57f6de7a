// Element semantics of the value codecs, shared by the kernels (kernels/value.hip) and the host (the
// encoded fill value, chain.cpp). Reference: fixedscaleoffset_codec.rs:159-380 (scale_array,
// unscale_array, cast_array) and zarrs_data_type/src/codec_traits/bitround.rs:3-45 (round_bits*).
//
// Rust's `as` between numbers is what every cast below reproduces: integer -> float rounds to
// nearest even, f64 -> f32 rounds to nearest even, float -> integer truncates toward zero, saturates
// at the integer's bounds and maps NaN to 0. The last is undefined in C++ for out-of-range values, so
// it is written as explicit clamps (sat_cast), never as a bare cast of an unchecked value.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <type_traits>

namespace zgpu {

// float -> integer as Rust's `as`. The bounds are exact in F: lo is 0 or -2^(N-1), hi_excl is 2^N or
// 2^(N-1), both powers of two.
template <class I, class F>
__host__ __device__ inline I sat_cast(F x) {
  static_assert(std::is_integral<I>::value && std::is_floating_point<F>::value, "float -> integer");
  const F lo = (F)std::numeric_limits<I>::min();
  const F hi_excl = (F)(std::numeric_limits<I>::max() / 2 + 1) * (F)2;
  if (x != x) return 0;
  if (x >= hi_excl) return std::numeric_limits<I>::max();
  if (x <= lo) return std::numeric_limits<I>::min();
  return (I)x;  // in range: truncation toward zero
}

// `x as To` for every pair of the fixedscaleoffset element types
template <class To, class From>
__host__ __device__ inline To rust_as(From x) {
  if constexpr (std::is_integral<To>::value && std::is_floating_point<From>::value) return sat_cast<To, From>(x);
  else return (To)x;  // integer -> float, float -> float: IEEE round to nearest even in both languages
}

// FixedScaleOffsetElementType::intermediate_float: f32 for 8- and 16-bit integers and f32, else f64
template <class T>
struct fso_float {
  using type = typename std::conditional<(sizeof(T) <= 2) || std::is_same<T, float>::value, float, double>::type;
};

// round half away from zero (Rust's f32::round / f64::round)
__host__ __device__ inline float round_away(float x) { return roundf(x); }
__host__ __device__ inline double round_away(double x) { return round(x); }

// scale_array then cast_array: T -> E. through_f32: `astype` is present (cast_array runs even for E = T)
template <class T, class E>
__host__ __device__ inline E fso_encode_one(T x, float offset, float scale, bool through_f32) {
#pragma clang fp contract(off)
  using F = typename fso_float<T>::type;
  const F d = (F)x - (F)offset;
  const F p = d * (F)scale;
  const T t = rust_as<T, F>(round_away(p));
  if (!through_f32) return (E)t;  // E == T
  return rust_as<E, float>(rust_as<float, T>(t));
}

// cast_array then unscale_array: E -> T
template <class E, class T>
__host__ __device__ inline T fso_decode_one(E e, float offset, float scale, bool through_f32) {
#pragma clang fp contract(off)
  using F = typename fso_float<T>::type;
  const T t = through_f32 ? rust_as<T, float>(rust_as<float, E>(e)) : (T)e;
  const F q = (F)t / (F)scale;
  const F r = q + (F)offset;
  return rust_as<T, F>(r);
}

// round_bits{8,16,32,64}: keepbits of maxbits stay, round to nearest with ties to even on the raw
// bits, the add saturating. Floats pass their mantissa width; integers pass width - clz (raw bits).
template <class U>
__host__ __device__ inline U round_bits(U x, uint32_t keepbits, uint32_t maxbits) {
  if (keepbits >= maxbits) return x;
  const uint32_t m = maxbits - keepbits;
  // every bit masked (an integer with its top bit set and keepbits = 0): x >> m and the mask are 0 as
  // numbers; a shift by the full width is not defined in C++
  if (m >= 8 * sizeof(U)) return 0;
  const U all = (U)~(U)0;
  const U mask = (U)((U)(all >> m) << m);
  const U add = (U)(((U)(x >> m) & (U)1) + (U)(((U)1 << (m - 1)) - (U)1));
  const U sum = (U)(x + add);
  const U sat = sum < x ? all : sum;  // saturating_add
  return (U)(sat & mask);
}

template <class U>
__host__ __device__ inline uint32_t bit_length(U x) {
  return x ? 64u - (uint32_t)__builtin_clzll((unsigned long long)x) : 0u;
}

// mant: the float's mantissa bits, 0 for an integer (rounded from its most significant set bit)
template <class U>
__host__ __device__ inline U bitround_one(U x, uint32_t keepbits, uint32_t mant) {
  return round_bits<U>(x, keepbits, mant ? mant : bit_length<U>(x));
}

}  // namespace zgpu
