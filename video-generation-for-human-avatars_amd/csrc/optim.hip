// The multi-tensor AdamW step of the LoRA path (ltx_amd/training.py FusedAdamW) and what rides on it. The
// LoRA gradients are hundreds of separate tensors of two dtypes (f32 adapters and DoRA magnitudes, the bf16
// caption projection), so every kernel here walks a chunk table -- int64 rows of (param, grad, exp_avg,
// exp_avg_sq, first element, count <= 2048), two more fields per row for the EMA, the swap and the
// stochastic step -- one block per row:
//   adamw_multi_kernel<BF16, CLIP, EMA>: the AdamW update of a row (ltx_adamw_multi); CLIP on g' = R(g * coef)
//     with coef read from the clip record (ltx_adamw_multi_clip); EMA with the f32 shadow update fused in, on
//     8-field rows (ltx_adamw_multi_ema);
//   the global gradient-norm clip in front of it:
//     1. grad_sumsq_multi_kernel: block b -> part[b], the f64 sum of squares of its row's gradient elements
//        (one launch per bucket, the next bucket's partials behind the previous one's);
//     2. grad_clip_coef_kernel: one block adds all partials and writes the record {sumsq, norm, coef};
//   ema_swap_multi_kernel: installs the averaged weights for an evaluation or an export and puts the live
//     ones back;
//   adamw_multi_sr_kernel: the mixed step of a bf16 parameter with f32 moments and a stochastically rounded
//     store (FusedAdamW(bf16_update="stochastic"), ltx_adamw_multi_sr);
//   the non-finite guard (FusedAdamW(skip_nonfinite=True)): grad_guard_record_kernel in the coefficient
//     kernel's place writes the wider GuardRecord (chunk_io.h) from the same partials, and
//     adamw_multi_guard_kernel / adamw_multi_sr_guard_kernel run the row bodies of the kernels above behind
//     one read of the record's `applied` (ltx_adamw_multi_guard, ltx_adamw_multi_sr_guard).
// Every sum has a fixed order and there are no atomics, so the record is bitwise reproducible; nothing here
// reads a value back to the host.
#include <cmath>

#include "adamw_elem.h"
#include "chunk_io.h"
#include "common.h"
#include "ltx_hip.h"

namespace ltx {

// the device record of ltx_grad_clip_coef (16 bytes; the host views it as one f64 and two f32)
struct ClipRecord {
  double sumsq;  // sum of squares of every gradient element, f64
  float norm;    // (float)sqrt(sumsq): the pre-clip global norm
  float coef;    // min(1, max_norm / (norm + 1e-6f)); 1 when max_norm <= 0
};
static_assert(sizeof(ClipRecord) == 16, "ClipRecord layout");

// Every element converts to f64 and squares exactly (24- or 8-bit significands: the square has at most 48
// bits). Order within the block, as sumsq_kernel (zero.hip): each thread adds its strided elements, the wave's
// shuffle tree, then the four wave sums in order.
template <bool BF16>
__global__ __launch_bounds__(256) void grad_sumsq_multi_kernel(const int64_t* __restrict__ table,
                                                               double* __restrict__ part) {
  const int64_t* e = table + (int64_t)blockIdx.x * 6;
  const void* grad = (const void*)e[1];
  const int64_t start = e[4], end = e[4] + e[5];
  double s = 0.0;
  for (int64_t i = start + threadIdx.x; i < end; i += 256) {
    const double v = BF16 ? (double)bf2f(((const bf16_t*)grad)[i]) : (double)((const float*)grad)[i];
    s += v * v;
  }
  __shared__ double red[4];
  s = block_sum_ordered(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// the record of a sum of squares: the coefficient is clip_coef_kernel's f32 arithmetic with inv_world = 1
__device__ __forceinline__ ClipRecord clip_record(double sumsq, float max_norm) {
  const float norm = (float)sqrt(sumsq);
  float c = 1.0f;
  if (max_norm > 0.f) {
    const float cc = max_norm / (norm + 1e-6f);
    if (cc < 1.0f) c = cc;
  }
  return {sumsq, norm, c};
}

// the sum of all partials (strided_partials_sum, as sumsq_finish_kernel)
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const double* __restrict__ part, int nparts,
                                                             float max_norm, ClipRecord* __restrict__ out) {
  __shared__ double red[1][256];
  strided_partials_sum<1>(part, nparts, red);
  if (threadIdx.x == 0) *out = clip_record(red[0][0], max_norm);
}

// grad_clip_coef_kernel's sum and record, and the guard's decision: a NaN element makes the sum NaN, an
// infinite one +inf (or NaN), and no finite f32 or bf16 gradient set overflows f64, so the sum is finite
// iff every element is. The test is on the exponent bits. `prev` (the last step's record, or null) carries
// the skipped count; it is read before `out` is written, so the two may be one record.
__global__ __launch_bounds__(256) void grad_guard_record_kernel(const double* __restrict__ part, int nparts,
                                                                float max_norm, const GuardRecord* prev,
                                                                GuardRecord* out) {
  __shared__ double red[1][256];
  strided_partials_sum<1>(part, nparts, red);
  if (threadIdx.x == 0) {
    const ClipRecord c = clip_record(red[0][0], max_norm);
    const uint64_t exponent = 0x7ff0000000000000ull;
    const bool finite = ((uint64_t)__double_as_longlong(c.sumsq) & exponent) != exponent;
    const int64_t skipped = (prev ? prev->skipped : 0) + (finite ? 0 : 1);
    out->sumsq = c.sumsq;
    out->norm = c.norm;
    out->coef = c.coef;
    out->applied = finite ? 1 : 0;
    out->pad = 0;
    out->skipped = skipped;
  }
}

// Every trainable tensor of one dtype in one launch: a block per table row, the per-element math of the
// per-tensor adamw_kernel (adamw_elem.h). CLIP: the gradient scaled by *coef on the way in. EMA: rows of 8
// int64, the six fields above, then the row's tensor's f32 shadow and its stash (a buffer of the parameter's
// dtype; 0 where an entry point does not use it); the shadow update rides on the parameter register. Rows
// index the shadow and the stash like the parameter: element i of the tensor, first element .. first element
// + count.
// Accesses are one element per lane (4 or 2 bytes, a wave's 64 lanes contiguous): a row's first element has
// only its tensor's alignment, so 16-byte accesses would need a per-row alignment guard and a peeled tail,
// and this kernel already moves its 28 B per f32 element at 6 TB/s this way (profiles/grad_clip_bench.md).
constexpr int EMA_ROW = 8;

template <bool BF16, bool CLIP, bool EMA>
__device__ __forceinline__ void adamw_multi_row(const int64_t* __restrict__ table, float decay, float w1, float b2,
                                                float w2, float step_size, float bc2_sqrt, float eps,
                                                const float* __restrict__ coef, float omd) {
  const int64_t* e = table + (int64_t)blockIdx.x * (EMA ? EMA_ROW : 6);
  void* param = (void*)e[0];
  const void* grad = (const void*)e[1];
  void* m = (void*)e[2];
  void* v = (void*)e[3];
  const int64_t start = e[4], end = e[4] + e[5];
  float* shadow = EMA ? (float*)e[6] : nullptr;
  const float c = CLIP ? *coef : 1.0f;
  for (int64_t i = start + threadIdx.x; i < end; i += 256)
    adamw_elem<BF16, CLIP, EMA>(param, grad, m, v, i, decay, w1, b2, w2, step_size, bc2_sqrt, eps, c, shadow, omd);
}

template <bool BF16, bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void adamw_multi_kernel(const int64_t* __restrict__ table, float decay, float w1,
                                                          float b2, float w2, float step_size, float bc2_sqrt,
                                                          float eps, const float* __restrict__ coef, float omd) {
  adamw_multi_row<BF16, CLIP, EMA>(table, decay, w1, b2, w2, step_size, bc2_sqrt, eps, coef, omd);
}

// the same row behind the guard: a skipped step returns before the first load
template <bool BF16, bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void adamw_multi_guard_kernel(const int64_t* __restrict__ table, float decay,
                                                                float w1, float b2, float w2, float step_size,
                                                                float bc2_sqrt, float eps,
                                                                const float* __restrict__ coef, float omd,
                                                                const GuardRecord* __restrict__ guard) {
  if (!step_applied(guard)) return;
  adamw_multi_row<BF16, CLIP, EMA>(table, decay, w1, b2, w2, step_size, bc2_sqrt, eps, coef, omd);
}

// LOAD: stash <- param, param <- R(shadow) (R: round to nearest even to bf16 for bf16 parameters);
// otherwise param <- stash
template <bool BF16, bool LOAD>
__global__ __launch_bounds__(256) void ema_swap_multi_kernel(const int64_t* __restrict__ table) {
  const int64_t* e = table + (int64_t)blockIdx.x * EMA_ROW;
  const int64_t start = e[4], end = e[4] + e[5];
  const float* __restrict__ shadow = (const float*)e[6];
  if (BF16) {
    bf16_t* __restrict__ param = (bf16_t*)e[0];
    bf16_t* __restrict__ stash = (bf16_t*)e[7];
    for (int64_t i = start + threadIdx.x; i < end; i += 256) {
      if (LOAD) {
        stash[i] = param[i];
        param[i] = f2bf(shadow[i]);
      } else {
        param[i] = stash[i];
      }
    }
  } else {
    float* __restrict__ param = (float*)e[0];
    float* __restrict__ stash = (float*)e[7];
    for (int64_t i = start + threadIdx.x; i < end; i += 256) {
      if (LOAD) {
        stash[i] = param[i];
        param[i] = shadow[i];
      } else {
        param[i] = stash[i];
      }
    }
  }
}

// ---- bf16 parameters with f32 moments and a stochastically rounded store ----------------------------
// Rows of 8 int64: (param bf16, grad bf16, exp_avg f32, exp_avg_sq f32, first element, count, shadow f32
// or 0, the parameter's ordinal). Per element 2 + 2 + 4 + 4 bytes in and 2 + 4 + 4 out (8 more with the
// shadow), so a row whose tensors are 16-byte aligned is walked 8 elements per lane: one 16-byte load each
// of p and g, two each of m and v, one Philox call for the 8 stores (st_sr). A row's last count % 8
// elements, and rows over a tensor that is not aligned, go one element per lane with that element's lane
// of the same call.
constexpr int SR_ROW = 8;

struct AdamWSr {
  float decay, w1, b2, w2, step_size, bc2_sqrt, eps, coef, omd;
  uint32_t k0, k1, step;
};

template <bool CLIP, bool EMA, int N>
__device__ __forceinline__ void adamw_sr_at(const int64_t* __restrict__ e, int64_t i, const AdamWSr& c) {
  float p[N], g[N], m[N], v[N], sh[N];
  ld<true, N>((const void*)e[0], i, p);
  ld<true, N>((const void*)e[1], i, g);
  ld<false, N>((const void*)e[2], i, m);
  ld<false, N>((const void*)e[3], i, v);
  if (EMA) ld<false, N>((const void*)e[6], i, sh);
  const Philox4 o = sr_philox(i, (uint32_t)e[7], c.step, c.k0, c.k1);  // under the loads
#pragma unroll
  for (int j = 0; j < N; ++j) {
    // the clipped gradient is what grad.mul_(coef) would leave in the bf16 tensor
    const float gj = CLIP ? rbf(g[j] * c.coef) : g[j];
    adamw_update<false, false>(p[j], gj, m[j], v[j], c.decay, c.w1, c.b2, c.w2, c.step_size, c.bc2_sqrt, c.eps,
                               1.0f);
  }
  st_sr<N>((void*)e[0], i, p, o);  // p becomes the value stored
  st<false, N>((void*)e[2], i, m);
  st<false, N>((void*)e[3], i, v);
  if (EMA) {
#pragma unroll
    for (int j = 0; j < N; ++j) sh[j] = ema_update(sh[j], p[j], c.omd);
    st<false, N>((void*)e[6], i, sh);
  }
}

template <bool CLIP, bool EMA>
__device__ __forceinline__ void adamw_multi_sr_row(const int64_t* __restrict__ table, AdamWSr c,
                                                   const float* __restrict__ coef) {
  const int64_t* e = table + (int64_t)blockIdx.x * SR_ROW;
  const int64_t start = e[4], count = e[5];
  if (CLIP) c.coef = *coef;
  uint64_t bits = (uint64_t)e[0] | (uint64_t)e[1] | (uint64_t)e[2] | (uint64_t)e[3];
  if (EMA) bits |= (uint64_t)e[6];
  // st_sr's 8 elements share one generator call: a vector starts at a multiple of 8 in its tensor
  walk_row<8>(start, count, (bits & 15) == 0 && (start & 7) == 0,
              [&](auto n, int64_t i) { adamw_sr_at<CLIP, EMA, decltype(n)::value>(e, i, c); });
}

template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void adamw_multi_sr_kernel(const int64_t* __restrict__ table, AdamWSr c,
                                                             const float* __restrict__ coef) {
  adamw_multi_sr_row<CLIP, EMA>(table, c, coef);
}

template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void adamw_multi_sr_guard_kernel(const int64_t* __restrict__ table, AdamWSr c,
                                                                   const float* __restrict__ coef,
                                                                   const GuardRecord* __restrict__ guard) {
  if (!step_applied(guard)) return;
  adamw_multi_sr_row<CLIP, EMA>(table, c, coef);
}

// the launch of adamw_multi_kernel<is_bf16, CLIP, EMA> behind the three nearest-mode entry points, of
// adamw_multi_guard_kernel behind the guarded one (guard != null)
template <bool CLIP, bool EMA>
static void launch_adamw_multi(const int64_t* table, int64_t nchunks, int is_bf16, float lr, float beta1, float beta2,
                               float eps, float weight_decay, int64_t step, const float* coef, float omd,
                               void* stream, const GuardRecord* guard = nullptr) {
  const AdamWScalars a = adamw_scalars(lr, beta1, beta2, weight_decay, step);
  with_flag(is_bf16, [&](auto bf) {
    if (guard)
      hipLaunchKernelGGL((adamw_multi_guard_kernel<decltype(bf)::value, CLIP, EMA>), dim3((unsigned)nchunks),
                         dim3(256), 0, (hipStream_t)stream, table, a.decay, a.w1, beta2, a.w2, a.step_size,
                         a.bc2_sqrt, eps, coef, omd, guard);
    else
      hipLaunchKernelGGL((adamw_multi_kernel<decltype(bf)::value, CLIP, EMA>), dim3((unsigned)nchunks), dim3(256), 0,
                         (hipStream_t)stream, table, a.decay, a.w1, beta2, a.w2, a.step_size, a.bc2_sqrt, eps, coef,
                         omd);
  });
}

// the launch of adamw_multi_sr_kernel<CLIP, EMA>, behind the guard when one is given
static void launch_adamw_multi_sr(const int64_t* table, int64_t nchunks, float lr, float beta1, float beta2, float eps,
                                  float weight_decay, int64_t step, const float* coef_or_null, int ema,
                                  float one_minus_decay, uint64_t seed, void* stream, const GuardRecord* guard) {
  const AdamWScalars a = adamw_scalars(lr, beta1, beta2, weight_decay, step);
  const AdamWSr c = {a.decay, a.w1, beta2, a.w2, a.step_size, a.bc2_sqrt, eps, 1.0f, ema ? one_minus_decay : 0.f,
                     (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), (uint32_t)((uint64_t)step & 0xffffffffu)};
  with_flag(coef_or_null != nullptr, [&](auto clip) {
    with_flag(ema, [&](auto em) {
      if (guard)
        hipLaunchKernelGGL((adamw_multi_sr_guard_kernel<decltype(clip)::value, decltype(em)::value>),
                           dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, table, c, coef_or_null, guard);
      else
        hipLaunchKernelGGL((adamw_multi_sr_kernel<decltype(clip)::value, decltype(em)::value>), dim3((unsigned)nchunks),
                           dim3(256), 0, (hipStream_t)stream, table, c, coef_or_null);
    });
  });
}

template <bool LOAD>
static void launch_ema_swap(const int64_t* table, int64_t nchunks, int is_bf16, void* stream) {
  with_flag(is_bf16, [&](auto bf) {
    hipLaunchKernelGGL((ema_swap_multi_kernel<decltype(bf)::value, LOAD>), dim3((unsigned)nchunks), dim3(256), 0,
                       (hipStream_t)stream, table);
  });
}

}  // namespace ltx

using namespace ltx;

extern "C" {

int ltx_grad_sumsq_multi(const int64_t* table, int64_t nchunks, int is_bf16, double* part, void* stream) {
  LTX_CHECK_ARG(table && part && nchunks > 0 && nchunks < (1LL << 31), "grad_sumsq_multi: bad args");
  with_flag(is_bf16, [&](auto bf) {
    hipLaunchKernelGGL(grad_sumsq_multi_kernel<decltype(bf)::value>, dim3((unsigned)nchunks), dim3(256), 0,
                       (hipStream_t)stream, table, part);
  });
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_grad_clip_coef(const double* part, int64_t nparts, float max_norm, void* out, void* stream) {
  LTX_CHECK_ARG(part && out && nparts > 0 && nparts < (1LL << 31), "grad_clip_coef: bad args");
  LTX_CHECK_ARG(((uintptr_t)out & 7) == 0, "grad_clip_coef: out must be 8-byte aligned");
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, (int)nparts, max_norm,
                     (ClipRecord*)out);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_adamw_multi(const int64_t* table, int64_t nchunks, int is_bf16, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int64_t step, void* stream) {
  LTX_CHECK_ARG(table && nchunks > 0 && nchunks < (1LL << 31) && step >= 1, "adamw_multi: bad args");
  launch_adamw_multi<false, false>(table, nchunks, is_bf16, lr, beta1, beta2, eps, weight_decay, step, nullptr, 0.f,
                                   stream);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_adamw_multi_clip(const int64_t* table, int64_t nchunks, int is_bf16, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int64_t step, const float* coef, void* stream) {
  LTX_CHECK_ARG(table && coef && nchunks > 0 && nchunks < (1LL << 31) && step >= 1, "adamw_multi_clip: bad args");
  launch_adamw_multi<true, false>(table, nchunks, is_bf16, lr, beta1, beta2, eps, weight_decay, step, coef, 0.f,
                                  stream);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_adamw_multi_ema(const int64_t* table, int64_t nchunks, int is_bf16, float lr, float beta1, float beta2,
                        float eps, float weight_decay, int64_t step, const float* coef_or_null,
                        float one_minus_decay, void* stream) {
  LTX_CHECK_ARG(table && nchunks > 0 && nchunks < (1LL << 31) && step >= 1, "adamw_multi_ema: bad args");
  LTX_CHECK_ARG(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "adamw_multi_ema: one_minus_decay outside [0, 1]");
  with_flag(coef_or_null != nullptr, [&](auto clip) {
    launch_adamw_multi<decltype(clip)::value, true>(table, nchunks, is_bf16, lr, beta1, beta2, eps, weight_decay, step,
                                                    coef_or_null, one_minus_decay, stream);
  });
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_ema_load_multi(const int64_t* table, int64_t nchunks, int is_bf16, void* stream) {
  LTX_CHECK_ARG(table && nchunks > 0 && nchunks < (1LL << 31), "ema_load_multi: bad args");
  launch_ema_swap<true>(table, nchunks, is_bf16, stream);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_ema_restore_multi(const int64_t* table, int64_t nchunks, int is_bf16, void* stream) {
  LTX_CHECK_ARG(table && nchunks > 0 && nchunks < (1LL << 31), "ema_restore_multi: bad args");
  launch_ema_swap<false>(table, nchunks, is_bf16, stream);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_adamw_multi_sr(const int64_t* table, int64_t nchunks, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int64_t step, const float* coef_or_null, int ema, float one_minus_decay,
                       uint64_t seed, void* stream) {
  LTX_CHECK_ARG(table && nchunks > 0 && nchunks < (1LL << 31) && step >= 1, "adamw_multi_sr: bad args");
  LTX_CHECK_ARG(!ema || (one_minus_decay >= 0.f && one_minus_decay <= 1.f),
                "adamw_multi_sr: one_minus_decay outside [0, 1]");
  launch_adamw_multi_sr(table, nchunks, lr, beta1, beta2, eps, weight_decay, step, coef_or_null, ema, one_minus_decay,
                        seed, stream, nullptr);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_grad_guard_record(const double* part, int64_t nparts, float max_norm, const void* prev_or_null, void* out,
                          void* stream) {
  LTX_CHECK_ARG(part && out && nparts > 0 && nparts < (1LL << 31), "grad_guard_record: bad args");
  LTX_CHECK_ARG((((uintptr_t)out | (uintptr_t)prev_or_null) & 7) == 0,
                "grad_guard_record: the records must be 8-byte aligned");
  hipLaunchKernelGGL(grad_guard_record_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, (int)nparts, max_norm,
                     (const GuardRecord*)prev_or_null, (GuardRecord*)out);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_adamw_multi_guard(const int64_t* table, int64_t nchunks, int is_bf16, float lr, float beta1, float beta2,
                          float eps, float weight_decay, int64_t step, const float* coef_or_null, int ema,
                          float one_minus_decay, const void* guard, void* stream) {
  LTX_CHECK_ARG(table && guard && nchunks > 0 && nchunks < (1LL << 31) && step >= 1, "adamw_multi_guard: bad args");
  LTX_CHECK_ARG(((uintptr_t)guard & 7) == 0, "adamw_multi_guard: guard must be 8-byte aligned");
  LTX_CHECK_ARG(!ema || (one_minus_decay >= 0.f && one_minus_decay <= 1.f),
                "adamw_multi_guard: one_minus_decay outside [0, 1]");
  with_flag(coef_or_null != nullptr, [&](auto clip) {
    with_flag(ema, [&](auto em) {
      launch_adamw_multi<decltype(clip)::value, decltype(em)::value>(table, nchunks, is_bf16, lr, beta1, beta2, eps,
                                                                     weight_decay, step, coef_or_null,
                                                                     ema ? one_minus_decay : 0.f, stream,
                                                                     (const GuardRecord*)guard);
    });
  });
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_adamw_multi_sr_guard(const int64_t* table, int64_t nchunks, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int64_t step, const float* coef_or_null, int ema,
                             float one_minus_decay, uint64_t seed, const void* guard, void* stream) {
  LTX_CHECK_ARG(table && guard && nchunks > 0 && nchunks < (1LL << 31) && step >= 1, "adamw_multi_sr_guard: bad args");
  LTX_CHECK_ARG(((uintptr_t)guard & 7) == 0, "adamw_multi_sr_guard: guard must be 8-byte aligned");
  LTX_CHECK_ARG(!ema || (one_minus_decay >= 0.f && one_minus_decay <= 1.f),
                "adamw_multi_sr_guard: one_minus_decay outside [0, 1]");
  launch_adamw_multi_sr(table, nchunks, lr, beta1, beta2, eps, weight_decay, step, coef_or_null, ema, one_minus_decay,
                        seed, stream, (const GuardRecord*)guard);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

}  // extern "C"
