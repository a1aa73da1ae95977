// Register-level access to the rows of the optimizer chunk tables (optim.hip, prodigy.hip): N consecutive
// elements of a bf16 or f32 tensor as f32 values, one element per lane or 16 bytes per access.
#pragma once
#include "common.h"
#include "philox.h"

namespace ltx {

// N consecutive elements starting at element i, as f32 (N = 1, or 4 f32 / 8 bf16 as one 16-byte access;
// an f32 column of a bf16 row, the shadow, as two)
template <bool BF16, int N>
__device__ __forceinline__ void ld(const void* base, int64_t i, float (&x)[N]) {
  if constexpr (N == 1) {
    x[0] = BF16 ? bf2f(((const bf16_t*)base)[i]) : ((const float*)base)[i];
  } else if constexpr (BF16) {
    static_assert(N == 8, "bf16 vector width");
    const u32x4 w = *(const u32x4*)((const bf16_t*)base + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = __uint_as_float(w[j] << 16);
      x[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
    }
  } else {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      const f32x4 w = *(const f32x4*)((const float*)base + i + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[4 * q + j] = w[j];
    }
  }
}

// the values are already rounded to the tensor's dtype, so the bf16 conversion is exact
template <bool BF16, int N>
__device__ __forceinline__ void st(void* base, int64_t i, const float (&x)[N]) {
  if constexpr (N == 1) {
    if (BF16) ((bf16_t*)base)[i] = f2bf(x[0]);
    else ((float*)base)[i] = x[0];
  } else if constexpr (BF16) {
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = pack2(x[2 * j], x[2 * j + 1]);
    *(u32x4*)((bf16_t*)base + i) = w;
  } else {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      f32x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = x[4 * q + j];
      *(f32x4*)((float*)base + i + 4 * q) = w;
    }
  }
}

// The stochastically rounded store of N f32 values to the bf16 tensor at element i (N = 1 or 8; for 8,
// i is a multiple of 8 and the tensor 16-byte aligned) with `o`, the generator's call for i's group of 8
// (sr_philox): one call serves the 8 elements, and a single element takes its lane i & 7 of the same
// call, so the bits do not depend on the access width. x becomes the values stored. The caller makes the
// call before it touches what it loaded: the generator needs nothing from memory, so its ~100 integer
// operations run while the loads are in flight.
template <int N>
__device__ __forceinline__ void st_sr(void* base, int64_t i, float (&x)[N], const Philox4& o) {
  if constexpr (N == 1) {
    const bf16_t b = sr_bf16(x[0], mask_lane(o, (int)(i & 7)));
    ((bf16_t*)base)[i] = b;
    x[0] = bf2f(b);
  } else {
    static_assert(N == 8, "bf16 vector width");
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t lo = sr_bf16(x[2 * j], o.v[j] & 0xffffu), hi = sr_bf16(x[2 * j + 1], o.v[j] >> 16);
      w[j] = lo | (hi << 16);
      x[2 * j] = __uint_as_float(lo << 16);
      x[2 * j + 1] = __uint_as_float(hi << 16);
    }
    *(u32x4*)((bf16_t*)base + i) = w;
  }
}

}  // namespace ltx
