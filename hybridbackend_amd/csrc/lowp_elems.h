// The elements of a 16-bit table (include/hbk.h, "Low-precision tables"): the exact upcast of bf16 / fp16 to fp32,
// the two roundings back and the stochastic rounding's noise.  Included by lowp_tables.hip (the forward reads rows
// with load_elems) and by sparse_apply.hip (the 16-bit apply reads a lane chunk with load_w and writes it with
// store_w), so that a row is upcast and rounded by ONE piece of code wherever it is touched.
#ifndef HBK_CSRC_LOWP_ELEMS_H_
#define HBK_CSRC_LOWP_ELEMS_H_

#include "common.h"
#include "lookup_common.h"

namespace hbk {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ inline float up_bf16(uint32_t h) { return __uint_as_float(h << 16); }
__device__ inline float up_fp16(uint32_t h) {
  const uint16_t b = (uint16_t)h;
  _Float16 x;
  __builtin_memcpy(&x, &b, 2);
  return (float)x;
}
__device__ inline float upcast(uint32_t h, bool bf16) { return bf16 ? up_bf16(h) : up_fp16(h); }

// W elements of a row starting at element `off` (W = 4: 8-byte aligned, W = 8: 16-byte aligned), upcast
template <int W>
__device__ inline void load_elems(const uint16_t* table, uint64_t off, bool bf16, float (&v)[W]) {
  if constexpr (W == 1) {
    v[0] = upcast(table[off], bf16);
  } else if constexpr (W == 4) {
    const u32x2 p = *reinterpret_cast<const u32x2*>(table + off);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      v[2 * i] = upcast(p[i] & 0xffffu, bf16);
      v[2 * i + 1] = upcast(p[i] >> 16, bf16);
    }
  } else {
    const u32x4 p = *reinterpret_cast<const u32x4*>(table + off);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = upcast(p[i] & 0xffffu, bf16);
      v[2 * i + 1] = upcast(p[i] >> 16, bf16);
    }
  }
}

// murmur3's finalizer, and the noise of include/hbk.h
__device__ inline uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__device__ inline uint32_t noise_base(uint32_t seed, uint32_t step, int32_t c) {
  return fmix32(seed ^ fmix32(step + 0x9E3779B9u * ((uint32_t)c + 1u)));
}
__device__ inline uint32_t noise_row(uint32_t base, int64_t r) {
  return fmix32(fmix32(base ^ (uint32_t)(uint64_t)r) ^ (uint32_t)((uint64_t)r >> 32));
}
__device__ inline uint32_t noise_elem(uint32_t rowh, int k) {
  return fmix32(rowh + 0x9E3779B9u * ((uint32_t)k + 1u));
}

// fp32 -> bf16, round to nearest even (a NaN stays a NaN: 0x7FC0)
__device__ inline uint32_t bf16_nearest(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// fp32 -> bf16, stochastic: nearest when the exponent field is all ones, else add 16 bits of noise and cut
__device__ inline uint32_t bf16_stochastic(float x, uint32_t noise) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7f800000u) == 0x7f800000u) return bf16_nearest(x);
  return (u + (noise & 0xffffu)) >> 16;
}
__device__ inline uint32_t fp16_nearest(float x) {
  const _Float16 h = (_Float16)x;
  uint16_t b;
  __builtin_memcpy(&b, &h, 2);
  return b;
}

// element k0 + i of row r rounded to the table's type
__device__ inline uint32_t round_elem(float x, bool bf16, bool stochastic, uint32_t rowh, int k) {
  if (!bf16) return fp16_nearest(x);
  return stochastic ? bf16_stochastic(x, noise_elem(rowh, k)) : bf16_nearest(x);
}

// a lane chunk of a row of the table: load + upcast, round + store.  V = f32x4: 4 elements (8 bytes), V = float: one
__device__ inline f32x4 load_w(const uint16_t* p, bool bf16, f32x4) {
  float v[4];
  load_elems<4>(p, 0, bf16, v);
  return f32x4{v[0], v[1], v[2], v[3]};
}
__device__ inline float load_w(const uint16_t* p, bool bf16, float) { return upcast(*p, bf16); }
__device__ inline void store_w(uint16_t* p, f32x4 v, bool bf16, bool stochastic, uint32_t rowh, int k0) {
  u32x2 o;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    o[i] = round_elem(v[2 * i], bf16, stochastic, rowh, k0 + 2 * i) |
           (round_elem(v[2 * i + 1], bf16, stochastic, rowh, k0 + 2 * i + 1) << 16);
  }
  *reinterpret_cast<u32x2*>(p) = o;
}
__device__ inline void store_w(uint16_t* p, float v, bool bf16, bool stochastic, uint32_t rowh, int k0) {
  *p = (uint16_t)round_elem(v, bf16, stochastic, rowh, k0);
}

}  // namespace
}  // namespace hbk

#endif  // HBK_CSRC_LOWP_ELEMS_H_
