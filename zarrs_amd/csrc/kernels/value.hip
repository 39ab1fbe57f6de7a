// The codecs that change element values or widths: numcodecs.fixedscaleoffset, bitround and cast_value
// (array->array, per element) and packbits (array->bytes, not element-aligned). Element semantics are in
// value.hpp and cast.hpp, shared with the host; the reference is fixedscaleoffset_codec.rs:159-380,
// zarrs_data_type/src/codec_traits/bitround.rs:3-45, codec_traits/cast_value.rs and packbits_codec.rs:216-400.
//
// Floating point in k_fso_decode / k_fso_encode has to match Rust bit for bit. How the build holds
// each property (the Makefile gives this file its own flags on top of the common ones):
//  * correctly rounded division: -fhip-fp32-correctly-rounded-divide-sqrt (hipcc's default, spelled
//    out) makes f32 `/` the IEEE-rounded expansion rather than the 2.5 ulp v_rcp_f32 form; f64 `/` is
//    always the correctly rounded expansion. No fast-math flag is in the build.
//  * denormals kept: -fno-gpu-flush-denormals-to-zero (the default on gfx9, spelled out) leaves the
//    kernel's FP mode at float_denorm_mode_32 = 3; f64 and f16 denormals are never flushed on gfx9.
//  * no contraction: -ffp-contract=off for this file, and `#pragma clang fp contract(off)` inside
//    fso_encode_one / fso_decode_one, whose operations are also written as separate statements. (As
//    written, (x - o) * s and x / s + o hold no a * b + c for a fused multiply-add to replace.)
//  * float -> integer: explicit clamps (sat_cast), saturating with NaN -> 0, never a bare cast.
//
// All three elementwise kernels share map_elements: every thread moves V = 16 / (the wider element
// size) elements at a time, so the wider side is one global_load/store_dwordx4 per lane and the
// narrower side a smaller vector (u8 -> f32: a dword load, a dwordx4 store), while both arrays are
// 16-byte aligned, grid-stride; the last n % V elements, or everything when an array is misaligned, go
// element by element. No LDS. (16 bytes on the narrower side instead, four dwordx4 stores per lane at a
// 64-byte lane stride for u8 -> f32, ran that conversion at 26.0 us against 16.6 us: DESIGN.md section 4.)
#include <hip/hip_runtime.h>

#include "../chain.hpp"
#include "../common.hpp"
#include "cast.hpp"
#include "launch.hpp"
#include "value.hpp"

namespace zgpu {

template <class X, int V>
struct alignas(sizeof(X) * V >= 16 ? 16 : sizeof(X) * V) ZgVec {
  X v[V];
};

template <class In, class Out, class Op>
__device__ __forceinline__ void map_elements(const In *__restrict__ in, Out *__restrict__ out, uint64_t n, int vec,
                                             Op op) {
  constexpr int V = 16 / (sizeof(In) > sizeof(Out) ? sizeof(In) : sizeof(Out));
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (uint64_t)gridDim.x * blockDim.x;
  uint64_t done = 0;
  if (vec) {
    const uint64_t groups = n / V;
    const ZgVec<In, V> *vi = reinterpret_cast<const ZgVec<In, V> *>(in);
    ZgVec<Out, V> *vo = reinterpret_cast<ZgVec<Out, V> *>(out);
    for (uint64_t g = tid; g < groups; g += nth) {
      const ZgVec<In, V> a = vi[g];
      ZgVec<Out, V> r;
#pragma unroll
      for (int k = 0; k < V; k++) r.v[k] = op(a.v[k]);
      vo[g] = r;
    }
    done = groups * V;
  }
  for (uint64_t j = done + tid; j < n; j += nth) out[j] = op(in[j]);
}

// cast_array (through f32, with `astype`) then unscale_array: E -> T
template <class E, class T>
__global__ __launch_bounds__(256) void k_fso_decode(const E *__restrict__ in, T *__restrict__ out, uint64_t n,
                                                    float offset, float scale, int through_f32, int vec) {
  map_elements<E, T>(in, out, n, vec,
                     [=](E e) { return fso_decode_one<E, T>(e, offset, scale, through_f32 != 0); });
}

// scale_array then cast_array: T -> E
template <class T, class E>
__global__ __launch_bounds__(256) void k_fso_encode(const T *__restrict__ in, E *__restrict__ out, uint64_t n,
                                                    float offset, float scale, int through_f32, int vec) {
  map_elements<T, E>(in, out, n, vec,
                     [=](T x) { return fso_encode_one<T, E>(x, offset, scale, through_f32 != 0); });
}

// round_bits on the raw bits; mant = 0: an integer, rounded from its most significant set bit
template <class U>
__global__ __launch_bounds__(256) void k_bitround(const U *__restrict__ in, U *__restrict__ out, uint64_t n,
                                                  uint32_t keepbits, uint32_t mant, int vec) {
  map_elements<U, U>(in, out, n, vec, [=](U x) { return bitround_one<U>(x, keepbits, mant); });
}

// cast_value, S -> T (decode is k_cast<T, S> with the decode map): the scalar map, then cast_one
// (cast.hpp), over the same vector shape as map_elements. rounding, out_of_range and the map are uniform
// kernel arguments. An element that cannot be cast writes 0; every thread keeps the smallest index it
// met and ends with one atomicMin on *fail (the host presets it to ~0), so an infallible pair, whose
// `ok` the compiler sees constant, has neither the compare nor the atomic.
template <class S, class T>
__global__ __launch_bounds__(256) void k_cast(const S *__restrict__ in, T *__restrict__ out, uint64_t n,
                                              uint32_t rounding, uint32_t oor, CastMap map,
                                              unsigned long long *__restrict__ fail, int vec) {
  constexpr int V = 16 / (sizeof(S) > sizeof(T) ? sizeof(S) : sizeof(T));
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long bad = ~0ull;
  auto one = [&](S x, uint64_t idx) {
    bool ok = true;
    const T y = cast_mapped<S, T>(x, map, rounding, oor, ok);
    if (!ok && idx < bad) bad = idx;
    return y;
  };
  uint64_t done = 0;
  if (vec) {
    const uint64_t groups = n / V;
    const ZgVec<S, V> *vi = reinterpret_cast<const ZgVec<S, V> *>(in);
    ZgVec<T, V> *vo = reinterpret_cast<ZgVec<T, V> *>(out);
    for (uint64_t g = tid; g < groups; g += nth) {
      const ZgVec<S, V> a = vi[g];
      ZgVec<T, V> r;
#pragma unroll
      for (int k = 0; k < V; k++) r.v[k] = one(a.v[k], g * V + k);
      vo[g] = r;
    }
    done = groups * V;
  }
  for (uint64_t j = done + tid; j < n; j += nth) out[j] = one(in[j], j);
  if (bad != ~0ull && fail) atomicMin(fail, bad);
}

static uint32_t map_grid(uint64_t n, uint32_t per_thread) {
  const uint64_t want = (n / per_thread + 255) / 256 + 1;
  const uint64_t cap = (uint64_t)device_cu_count() * 8;
  return (uint32_t)(want < cap ? want : cap);
}

static int both_aligned(const void *a, const void *b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

template <class F>
static bool with_fso_type(uint32_t vt, F &&f) {
  switch (vt) {
    case VT_I8: f(int8_t{}); return true;
    case VT_I16: f(int16_t{}); return true;
    case VT_I32: f(int32_t{}); return true;
    case VT_I64: f(int64_t{}); return true;
    case VT_U8: f(uint8_t{}); return true;
    case VT_U16: f(uint16_t{}); return true;
    case VT_U32: f(uint32_t{}); return true;
    case VT_U64: f(uint64_t{}); return true;
    case VT_F32: f(float{}); return true;
    case VT_F64: f(double{}); return true;
    default: return false;
  }
}

hipError_t launch_fso_decode(uint32_t vt_enc, uint32_t vt_dec, const void *in, void *out, uint64_t n, float offset,
                             float scale, int through_f32, hipStream_t s) {
  if (!n) return hipSuccess;
  if (!through_f32 && vt_enc != vt_dec) return hipErrorInvalidValue;
  bool ok = with_fso_type(vt_enc, [&](auto e) {
    using E = decltype(e);
    ok = with_fso_type(vt_dec, [&](auto t) {
      using T = decltype(t);
      constexpr uint32_t V = 16 / (sizeof(E) > sizeof(T) ? sizeof(E) : sizeof(T));
      hipLaunchKernelGGL((k_fso_decode<E, T>), dim3(map_grid(n, V)), dim3(256), 0, s, (const E *)in, (T *)out, n, offset,
                         scale, through_f32, both_aligned(in, out));
    });
  }) && ok;
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_fso_encode(uint32_t vt_dec, uint32_t vt_enc, const void *in, void *out, uint64_t n, float offset,
                             float scale, int through_f32, hipStream_t s) {
  if (!n) return hipSuccess;
  if (!through_f32 && vt_enc != vt_dec) return hipErrorInvalidValue;
  bool ok = with_fso_type(vt_dec, [&](auto t) {
    using T = decltype(t);
    ok = with_fso_type(vt_enc, [&](auto e) {
      using E = decltype(e);
      constexpr uint32_t V = 16 / (sizeof(E) > sizeof(T) ? sizeof(E) : sizeof(T));
      hipLaunchKernelGGL((k_fso_encode<T, E>), dim3(map_grid(n, V)), dim3(256), 0, s, (const T *)in, (E *)out, n, offset,
                         scale, through_f32, both_aligned(in, out));
    });
  }) && ok;
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_cast(uint32_t vt_src, uint32_t vt_dst, const void *in, void *out, uint64_t n, uint32_t rounding,
                       uint32_t oor, const CastMap &map, uint64_t *fail, hipStream_t s) {
  if (!n) return hipSuccess;
  bool ok = with_cast_type(vt_src, [&](auto a) {
    using S = decltype(a);
    ok = with_cast_type(vt_dst, [&](auto b) {
      using T = decltype(b);
      constexpr uint32_t V = 16 / (sizeof(S) > sizeof(T) ? sizeof(S) : sizeof(T));
      hipLaunchKernelGGL((k_cast<S, T>), dim3(map_grid(n, V)), dim3(256), 0, s, (const S *)in, (T *)out, n, rounding, oor,
                         map, (unsigned long long *)fail, both_aligned(in, out));
    });
  }) && ok;
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_bitround(uint32_t width, uint32_t mant, uint32_t keepbits, const void *in, void *out, uint64_t n,
                           hipStream_t s) {
  if (!n) return hipSuccess;
  const int vec = both_aligned(in, out);
  const uint32_t g = map_grid(n, 16 / width);
  switch (width) {
    case 1:
      hipLaunchKernelGGL(k_bitround<uint8_t>, dim3(g), dim3(256), 0, s, (const uint8_t *)in, (uint8_t *)out, n, keepbits,
                         mant, vec);
      break;
    case 2:
      hipLaunchKernelGGL(k_bitround<uint16_t>, dim3(g), dim3(256), 0, s, (const uint16_t *)in, (uint16_t *)out, n,
                         keepbits, mant, vec);
      break;
    case 4:
      hipLaunchKernelGGL(k_bitround<uint32_t>, dim3(g), dim3(256), 0, s, (const uint32_t *)in, (uint32_t *)out, n,
                         keepbits, mant, vec);
      break;
    case 8:
      hipLaunchKernelGGL(k_bitround<uint64_t>, dim3(g), dim3(256), 0, s, (const uint64_t *)in, (uint64_t *)out, n,
                         keepbits, mant, vec);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// packbits
// ------------------------------------------------------------------------------------------------

// `need` (1..64) bits of the packed stream starting at bit `bit` of `base`, from the aligned dwords
// that hold them: at most 3 bytes before `base + bit / 8` and 3 bytes after the last needed byte are
// touched (the host pads its buffers for both).
__device__ __forceinline__ uint64_t pb_window(const uint8_t *base, uint64_t bit, uint32_t need) {
  const uintptr_t a = (uintptr_t)base + (bit >> 3);
  const uint32_t *d = (const uint32_t *)(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3) * 8 + (uint32_t)(bit & 7);  // 0..31
  const uint32_t nd = (sh + need + 31) >> 5;                        // dwords that hold the bits: 1..3
  uint64_t lo = d[0];
  if (nd > 1) lo |= (uint64_t)d[1] << 32;
  uint64_t w = lo >> sh;
  if (nd > 2) w |= (uint64_t)d[2] << (64 - sh);  // nd > 2 implies sh > 0
  return w;
}

// Unpack chunk blockIdx.y: tab[i] = packed bytes (P.packed_len of them), tab[n + i] = 16-byte aligned
// destination of its nelem native elements. Every thread produces 16 bytes of output, a whole number
// of elements (element sizes divide 16), from a 64-bit window it refills as it runs dry; a full
// group is one 16-byte store, the chunk's last partial group is stored component by component. Output
// bytes have one owner. Reproduces PackBitsCodecBound::decode (packbits_codec.rs:362-397) including
// its sign extension, which fills only the rest of the byte that holds the sign bit.
template <class C>
__global__ __launch_bounds__(256) void k_unpackbits(const uint64_t *__restrict__ tab, uint32_t *__restrict__ status,
                                                    uint32_t n_chunks, uint32_t chunk0, ZgPackBits P) {
  constexpr uint32_t NC = 16 / sizeof(C);
  const uint32_t i = chunk0 + blockIdx.y;
  const uint8_t *src = (const uint8_t *)tab[i];
  C *dst = (C *)tab[n_chunks + i];
  const uint64_t ncomp = P.nelem * P.ncomp;
  const uint64_t data_bytes = (ncomp * P.ext + 7) / 8;
  if (P.padding && blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t rem = (uint32_t)((ncomp * P.ext) & 7);
    const uint8_t want = rem ? (uint8_t)(8 - rem) : 0;
    if (src[P.padding == 1 ? 0 : data_bytes] != want) status[i] = ZG_CORRUPT_STREAM;
  }
  const uint8_t *data = src + (P.padding == 1 ? 1 : 0);
  const uint64_t mask = ((uint64_t)1 << P.ext) - 1;  // ext <= 63 (a whole 64-bit component is `bytes`)
  const uint32_t top = P.first + P.ext - 1;          // the sign bit's place in the component
  const uint64_t sign_fill = ((uint64_t)((0xFFu << ((top & 7) + 1)) & 0xFFu)) << (8 * (top >> 3));
  const uint64_t groups = (ncomp + NC - 1) / NC;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups;
       g += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t c0 = g * NC;
    const uint32_t cnt = (uint32_t)(ncomp - c0 < NC ? ncomp - c0 : NC);
    uint64_t bit = c0 * P.ext, left = (uint64_t)cnt * P.ext;
    uint64_t win = pb_window(data, bit, (uint32_t)(left < 64 ? left : 64));
    uint32_t used = 0;
    ZgVec<C, NC> r;
#pragma unroll
    for (uint32_t k = 0; k < NC; k++) {
      C v = 0;
      if (k < cnt) {
        if (used + P.ext > 64) {
          win = pb_window(data, bit, (uint32_t)(left < 64 ? left : 64));
          used = 0;
        }
        uint64_t x = ((win >> used) & mask) << P.first;
        if (P.sign && ((x >> top) & 1)) x |= sign_fill;
        v = (C)x;
        used += P.ext;
        bit += P.ext;
        left -= P.ext;
      }
      r.v[k] = v;
    }
    if (cnt == NC) {
      *reinterpret_cast<ZgVec<C, NC> *>(dst + c0) = r;
    } else {
      for (uint32_t k = 0; k < cnt; k++) dst[c0 + k] = r.v[k];
    }
  }
}

// Pack chunk blockIdx.y: tab[i] = its nelem native elements, tab[n + i] = destination of P.packed_len
// bytes. Every thread owns 8 bytes of the packed elements (and thread 0 the padding byte): it ORs in
// the bit range of each component that reaches into them and stores them bytewise, as destinations
// carry no alignment. PackBitsCodecBound::encode (packbits_codec.rs:262-295).
template <class C>
__global__ __launch_bounds__(256) void k_packbits(const uint64_t *__restrict__ tab, uint32_t n_chunks, uint32_t chunk0,
                                                  ZgPackBits P) {
  const uint32_t i = chunk0 + blockIdx.y;
  const C *src = (const C *)tab[i];
  uint8_t *dst = (uint8_t *)tab[n_chunks + i];
  const uint64_t ncomp = P.nelem * P.ncomp, nbits = ncomp * P.ext;
  const uint64_t data_bytes = (nbits + 7) / 8;
  if (P.padding && blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t rem = (uint32_t)(nbits & 7);
    dst[P.padding == 1 ? 0 : data_bytes] = rem ? (uint8_t)(8 - rem) : 0;
  }
  uint8_t *data = dst + (P.padding == 1 ? 1 : 0);
  const uint64_t mask = ((uint64_t)1 << P.ext) - 1;
  const uint64_t words = (data_bytes + 7) / 8;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words;
       w += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t b0 = w * 64, b1 = b0 + 64 < nbits ? b0 + 64 : nbits;  // this thread's bits [b0, b1)
    uint64_t acc = 0;
    for (uint64_t c = b0 / P.ext; c < ncomp && c * P.ext < b1; c++) {
      const uint64_t x = ((uint64_t)src[c] >> P.first) & mask;
      const uint64_t cb = c * P.ext;
      acc |= cb >= b0 ? x << (cb - b0) : x >> (b0 - cb);  // shifts are 0..63: the ranges overlap
    }
    const uint64_t nb = data_bytes - w * 8 < 8 ? data_bytes - w * 8 : 8;
    for (uint64_t k = 0; k < nb; k++) data[w * 8 + k] = (uint8_t)(acc >> (8 * k));
  }
}

template <class F>
static bool with_comp_type(uint32_t comp_bytes, F &&f) {
  switch (comp_bytes) {
    case 1: f(uint8_t{}); return true;
    case 2: f(uint16_t{}); return true;
    case 4: f(uint32_t{}); return true;
    case 8: f(uint64_t{}); return true;
    default: return false;
  }
}

hipError_t launch_unpackbits(const uint64_t *tab, uint32_t *status, uint32_t n_chunks, const ZgPackBits &P,
                             hipStream_t s) {
  if (!n_chunks || !P.nelem) return hipSuccess;
  if (P.ext == 0 || P.ext > 63) return hipErrorInvalidValue;
  const uint64_t groups = (P.nelem * P.ncomp * P.comp_bytes + 15) / 16;
  const uint64_t want = (groups + 255) / 256;
  const uint32_t gx = (uint32_t)(want < 1024 ? want : 1024);
  bool ok = true;
  for (uint32_t c0 = 0; c0 < n_chunks && ok; c0 += 65535) {
    const uint32_t gy = n_chunks - c0 < 65535 ? n_chunks - c0 : 65535;
    ok = with_comp_type(P.comp_bytes, [&](auto c) {
      using C = decltype(c);
      hipLaunchKernelGGL(k_unpackbits<C>, dim3(gx, gy), dim3(256), 0, s, tab, status, n_chunks, c0, P);
    });
  }
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_packbits(const uint64_t *tab, uint32_t n_chunks, const ZgPackBits &P, hipStream_t s) {
  if (!n_chunks) return hipSuccess;
  if (P.ext == 0 || P.ext > 63) return hipErrorInvalidValue;
  const uint64_t words = ((P.nelem * P.ncomp * P.ext + 7) / 8 + 7) / 8;
  const uint64_t want = (words + 255) / 256 + 1;
  const uint32_t gx = (uint32_t)(want < 1024 ? want : 1024);
  bool ok = true;
  for (uint32_t c0 = 0; c0 < n_chunks && ok; c0 += 65535) {
    const uint32_t gy = n_chunks - c0 < 65535 ? n_chunks - c0 : 65535;
    ok = with_comp_type(P.comp_bytes, [&](auto c) {
      using C = decltype(c);
      hipLaunchKernelGGL(k_packbits<C>, dim3(gx, gy), dim3(256), 0, s, tab, n_chunks, c0, P);
    });
  }
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace zgpu
