// What the kernels over the optimizer chunk tables (optim.hip, prodigy.hip) share: register-level access to
// a row's tensors (N consecutive elements of a bf16 or f32 tensor as f32 values, one element per lane or 16
// bytes per access), the walk of a row's elements, the fixed-order sums behind the f64 partials, and the
// host's choice of a kernel instantiation from run-time flags.
#pragma once
#include <type_traits>

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

// The block's walk of one row, `count` elements from element `start`, calling at(N, i) for N consecutive
// elements at i (N a std::integral_constant). With `vector_ok` (the caller's: every tensor touched 16-byte
// aligned, and whatever else its stores need) count / VEC steps of VEC elements, thread-strided, then the
// row's last count % VEC elements one per lane; otherwise one element per lane throughout.
template <int VEC, class At>
__device__ __forceinline__ void walk_row(int64_t start, int64_t count, bool vector_ok, At&& at) {
  if (vector_ok) {
    const int64_t nvec = count / VEC;
    for (int64_t q = threadIdx.x; q < nvec; q += 256) at(std::integral_constant<int, VEC>{}, start + q * VEC);
    const int64_t i = start + nvec * VEC + threadIdx.x;
    if (i < start + count) at(std::integral_constant<int, 1>{}, i);
  } else {
    for (int64_t i = start + threadIdx.x; i < start + count; i += 256) at(std::integral_constant<int, 1>{}, i);
  }
}

// the block's sum of one f64 per thread: wave butterfly, then the four waves in order; valid in thread 0
__device__ __forceinline__ double block_sum_ordered(double x, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// One block's sums of K interleaved f64 columns of `n` rows (part[K * i + c]), left in red[c][0]: each of
// the 256 threads adds its strided rows in order, then a fixed-shape tree. Eight loads per column are in
// flight at a time, added in the strided order (a row past the end reads as 0): one block walks ~10^4
// partials, and with one load per add it took 11 us against 4.7 us this way.
template <int K>
__device__ __forceinline__ void strided_partials_sum(const double* __restrict__ part, int n, double (&red)[K][256]) {
  double s[K] = {};
  for (int64_t base = threadIdx.x; base < n; base += 8 * 256) {
    double v[K][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t i = base + k * 256;
#pragma unroll
      for (int c = 0; c < K; ++c) v[c][k] = i < n ? part[K * i + c] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
      for (int c = 0; c < K; ++c) s[c] += v[c][k];
    }
  }
#pragma unroll
  for (int c = 0; c < K; ++c) red[c][threadIdx.x] = s[c];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int c = 0; c < K; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + o];
    }
    __syncthreads();
  }
}

// The device record of ltx_grad_guard_record (32 bytes; the host views it as four f64): the clip record's
// three fields in the clip record's places, then the guard's own. A guarded update kernel reads `applied`
// once per workgroup (step_applied: the same address in every lane, a uniform load) and returns before its
// first store when it is 0, so a skipped step writes this record and nothing else.
struct GuardRecord {
  double sumsq;     // sum of squares of every gradient element, f64: finite iff every element is finite
  float norm;       // (float)sqrt(sumsq): the pre-clip global norm
  float coef;       // grad_clip_coef_kernel's coefficient; 1 without a max_norm
  int32_t applied;  // 1 when sumsq is finite (the step runs), 0 when it is skipped
  int32_t pad;
  int64_t skipped;  // steps skipped so far, this one included: the previous record's count carried on
};
static_assert(sizeof(GuardRecord) == 32, "GuardRecord layout");

__device__ __forceinline__ bool step_applied(const GuardRecord* __restrict__ guard) { return guard->applied != 0; }

// host: f(std::true_type) or f(std::false_type) by a run-time flag, nested once per template parameter
template <class F>
static inline void with_flag(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace ltx
