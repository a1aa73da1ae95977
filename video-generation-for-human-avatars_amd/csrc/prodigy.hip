// Prodigy (Mishchenko & Defazio), the learning-rate-free optimizer, for the multi-tensor LoRA step
// (ltx_amd/training.py FusedProdigy). The step-size estimate d lives in a device record and never visits
// the host; a step is three kinds of launches on one stream, ordered by the stream alone:
//   1. prodigy_moments_multi_kernel (pass 1, one launch per dtype): block b walks row b of the chunk
//      table, updates exp_avg / exp_avg_sq / s with the old d and writes two f64 partials, the row's
//      sum of R(p0 - p) g and of |s| (the second dtype's partials behind the first's);
//   2. prodigy_d_update_kernel: one block adds all partials in row order and runs the f64 update of
//      d_numerator, d_hat, d_max, d, k in the record;
//   3. prodigy_apply_multi_kernel (pass 2, one launch per dtype): the parameter step with the new d in
//      the denominator and the old d lr as the step, a no-op when the record says d_denom was 0; with a
//      shadow column the EMA of the value just stored.
// Every sum has a fixed order and there are no atomics, so the record is bitwise reproducible and every
// data-parallel rank computes the same d from the same (all-reduced) gradients.
//
// The table has 10 int64 per row: (param, grad, exp_avg, exp_avg_sq, first element, count <= 2048, s, p0,
// shadow, stash); shadow and stash are 0 without the EMA. A row whose tensors are all 16-byte aligned is
// walked with 16-byte accesses (4 f32 or 8 bf16 per lane, the row's last count % 4 or 8 elements one per
// lane); rows over a tensor that is not (a gradient that is a view into a reducer's bucket) take one
// element per lane throughout. The arithmetic per element is the same (prodigy_elem.h).
//
// The mixed step of a bf16 parameter (FusedProdigy(bf16_update="stochastic")): param, grad and p0 bf16,
// exp_avg, exp_avg_sq and s f32, the f32 arithmetic on the widened values, and pass 2 stores the
// parameter stochastically rounded (chunk_io.h st_sr); the row's last field is the parameter's ordinal.
#include <cmath>

#include "chunk_io.h"
#include "common.h"
#include "ltx_hip.h"
#include "prodigy_elem.h"

namespace ltx {

constexpr int PRODIGY_ROW = 10;

struct ProdigyRow {
  void* param;
  const void* grad;
  void* m;
  void* v;
  void* s;
  const void* p0;
  float* shadow;
  int64_t start, count;
  bool aligned;  // every tensor the entry point touches is 16-byte aligned
};

__device__ __forceinline__ ProdigyRow prodigy_row(const int64_t* __restrict__ table, bool pass1, bool ema) {
  const int64_t* e = table + (int64_t)blockIdx.x * PRODIGY_ROW;
  ProdigyRow r;
  r.param = (void*)e[0];
  r.grad = (const void*)e[1];
  r.m = (void*)e[2];
  r.v = (void*)e[3];
  r.start = e[4];
  r.count = e[5];
  r.s = (void*)e[6];
  r.p0 = (const void*)e[7];
  r.shadow = (float*)e[8];
  uint64_t bits = (uint64_t)e[0] | (uint64_t)e[2] | (uint64_t)e[3];
  if (pass1) bits |= (uint64_t)e[1] | (uint64_t)e[6] | (uint64_t)e[7];
  if (ema) bits |= (uint64_t)e[8];
  r.aligned = (bits & 15) == 0;
  return r;
}

// the block's sum of one f64 per thread: wave butterfly, then the four waves in order; valid in thread 0
__device__ __forceinline__ double block_sum_ordered(double x, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

struct ProdigyHyper {
  double lr, beta1, beta2, beta3, d0, weight_decay;
  int use_bias_correction, safeguard_warmup;
};

template <bool BF16, bool CLIP, bool COUPLED, int N>
__device__ __forceinline__ void moments_at(const ProdigyRow& r, int64_t i, const ProdigyMoments& c, double& num,
                                           double& den) {
  float p[N], g[N], p0[N], m[N], v[N], s[N];
  ld<BF16, N>(r.param, i, p);
  ld<BF16, N>(r.grad, i, g);
  ld<BF16, N>(r.p0, i, p0);
  ld<BF16, N>(r.m, i, m);
  ld<BF16, N>(r.v, i, v);
  ld<BF16, N>(r.s, i, s);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    float tn, td;
    prodigy_moments_elem<BF16, CLIP, COUPLED>(p[j], g[j], p0[j], m[j], v[j], s[j], c, tn, td);
    num += (double)tn;
    den += (double)td;
  }
  st<BF16, N>(r.m, i, m);
  st<BF16, N>(r.v, i, v);
  st<BF16, N>(r.s, i, s);
}

// pass 1 of the mixed step: the f32 instantiation on (float(p), float(g), float(p0)) and the f32 state;
// with a coefficient the gradient is first what grad.mul_(coef) would leave in the bf16 tensor
template <bool CLIP, bool COUPLED, int N>
__device__ __forceinline__ void moments_mixed_at(const ProdigyRow& r, int64_t i, const ProdigyMoments& c,
                                                 double& num, double& den) {
  float p[N], g[N], p0[N], m[N], v[N], s[N];
  ld<true, N>(r.param, i, p);
  ld<true, N>(r.grad, i, g);
  ld<true, N>(r.p0, i, p0);
  ld<false, N>(r.m, i, m);
  ld<false, N>(r.v, i, v);
  ld<false, N>(r.s, i, s);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    float tn, td;
    const float gj = CLIP ? rbf(g[j] * c.coef) : g[j];
    prodigy_moments_elem<false, false, COUPLED>(p[j], gj, p0[j], m[j], v[j], s[j], c, tn, td);
    num += (double)tn;
    den += (double)td;
  }
  st<false, N>(r.m, i, m);
  st<false, N>(r.v, i, v);
  st<false, N>(r.s, i, s);
}

// MIXED: bf16 param / grad / p0 with f32 state (BF16 is then ignored)
template <bool BF16, bool CLIP, bool COUPLED, bool MIXED = false>
__global__ __launch_bounds__(256) void prodigy_moments_multi_kernel(const int64_t* __restrict__ table,
                                                                    const ProdigyRecord* __restrict__ rec,
                                                                    ProdigyHyper h, const float* __restrict__ coef,
                                                                    double* __restrict__ part) {
  constexpr int VEC = (BF16 || MIXED) ? 8 : 4;
  const ProdigyRow r = prodigy_row(table, true, false);
  const double d = rec->d;
  const double dlr = prodigy_dlr(d, rec->k, h.lr, h.beta1, h.beta2, h.use_bias_correction);
  ProdigyMoments c;
  c.b1 = (float)h.beta1;
  c.b2 = (float)h.beta2;
  c.b3 = (float)h.beta3;
  c.a1 = (float)(d * (1.0 - h.beta1));
  c.a2 = (float)(d * d * (1.0 - h.beta2));
  c.a3 = (float)((d / h.d0) * (h.safeguard_warmup ? d : dlr));
  c.wd = (float)h.weight_decay;
  c.coef = CLIP ? *coef : 1.0f;
  double num = 0.0, den = 0.0;
  if constexpr (MIXED) {
    if (r.aligned) {
      const int64_t nvec = r.count / VEC;
      for (int64_t q = threadIdx.x; q < nvec; q += 256)
        moments_mixed_at<CLIP, COUPLED, VEC>(r, r.start + q * VEC, c, num, den);
      const int64_t i = r.start + nvec * VEC + threadIdx.x;
      if (i < r.start + r.count) moments_mixed_at<CLIP, COUPLED, 1>(r, i, c, num, den);
    } else {
      for (int64_t i = r.start + threadIdx.x; i < r.start + r.count; i += 256)
        moments_mixed_at<CLIP, COUPLED, 1>(r, i, c, num, den);
    }
  } else if (r.aligned) {
    const int64_t nvec = r.count / VEC;
    for (int64_t q = threadIdx.x; q < nvec; q += 256)
      moments_at<BF16, CLIP, COUPLED, VEC>(r, r.start + q * VEC, c, num, den);
    const int64_t i = r.start + nvec * VEC + threadIdx.x;
    if (i < r.start + r.count) moments_at<BF16, CLIP, COUPLED, 1>(r, i, c, num, den);
  } else {
    for (int64_t i = r.start + threadIdx.x; i < r.start + r.count; i += 256)
      moments_at<BF16, CLIP, COUPLED, 1>(r, i, c, num, den);
  }
  __shared__ double red[2][4];
  num = block_sum_ordered(num, red[0]);
  den = block_sum_ordered(den, red[1]);
  if (threadIdx.x == 0) {
    part[2 * (int64_t)blockIdx.x] = num;
    part[2 * (int64_t)blockIdx.x + 1] = den;
  }
}

// part holds (num, den) pairs, one per row. 256 threads add strided rows in a fixed order, eight loads in
// flight (as grad_clip_coef_kernel), then a fixed-shape tree; thread 0 runs the update.
__global__ __launch_bounds__(256) void prodigy_d_update_kernel(const double* __restrict__ part, int nrows,
                                                               ProdigyRecord* __restrict__ rec, ProdigyHyper h,
                                                               double d_coef, double growth_rate) {
  double sn = 0.0, sd = 0.0;
  for (int64_t base = threadIdx.x; base < nrows; base += 8 * 256) {
    double vn[8], vd[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t i = base + k * 256;
      vn[k] = i < nrows ? part[2 * i] : 0.0;
      vd[k] = i < nrows ? part[2 * i + 1] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      sn += vn[k];
      sd += vd[k];
    }
  }
  __shared__ double redn[256], redd[256];
  redn[threadIdx.x] = sn;
  redd[threadIdx.x] = sd;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      redn[threadIdx.x] += redn[threadIdx.x + o];
      redd[threadIdx.x] += redd[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double d = rec->d;
    const double dlr = prodigy_dlr(d, rec->k, h.lr, h.beta1, h.beta2, h.use_bias_correction);
    const double d_denom = redd[0];
    rec->dlr = dlr;
    rec->d_denom = d_denom;
    if (d_denom == 0.0) {
      rec->applied = 0.0;
    } else {
      const double d_numerator = h.beta3 * rec->d_numerator + (d / h.d0) * dlr * redn[0];
      const double d_hat = d_coef * d_numerator / d_denom;
      if (d == h.d0) d = d > d_hat ? d : d_hat;
      const double d_max = rec->d_max > d_hat ? rec->d_max : d_hat;
      const double grown = d * growth_rate;
      rec->d = d_max < grown ? d_max : grown;
      rec->d_max = d_max;
      rec->d_numerator = d_numerator;
      rec->d_hat = d_hat;
      rec->k = rec->k + 1.0;
      rec->applied = 1.0;
    }
  }
}

template <bool BF16, bool DECAY, bool EMA, int N>
__device__ __forceinline__ void apply_at(const ProdigyRow& r, int64_t i, const ProdigyApply& c) {
  float p[N], m[N], v[N], sh[N];
  ld<BF16, N>(r.param, i, p);
  ld<BF16, N>(r.m, i, m);
  ld<BF16, N>(r.v, i, v);
  if (EMA) ld<false, N>(r.shadow, i, sh);
#pragma unroll
  for (int j = 0; j < N; ++j) p[j] = prodigy_apply_elem<BF16, DECAY, EMA>(p[j], m[j], v[j], c, sh[j]);
  st<BF16, N>(r.param, i, p);
  if (EMA) st<false, N>(r.shadow, i, sh);
}

template <bool BF16, bool DECAY, bool EMA>
__global__ __launch_bounds__(256) void prodigy_apply_multi_kernel(const int64_t* __restrict__ table,
                                                                  const ProdigyRecord* __restrict__ rec, double eps,
                                                                  double weight_decay, float omd) {
  constexpr int VEC = BF16 ? 8 : 4;
  if (rec->applied == 0.0) return;
  const ProdigyRow r = prodigy_row(table, false, EMA);
  const double dlr = rec->dlr;
  ProdigyApply c;
  c.deps = (float)(rec->d * eps);
  c.decay = (float)(-weight_decay * dlr);
  c.step = (float)(-dlr);
  c.omd = omd;
  if (r.aligned) {
    const int64_t nvec = r.count / VEC;
    for (int64_t q = threadIdx.x; q < nvec; q += 256) apply_at<BF16, DECAY, EMA, VEC>(r, r.start + q * VEC, c);
    const int64_t i = r.start + nvec * VEC + threadIdx.x;
    if (i < r.start + r.count) apply_at<BF16, DECAY, EMA, 1>(r, i, c);
  } else {
    for (int64_t i = r.start + threadIdx.x; i < r.start + r.count; i += 256) apply_at<BF16, DECAY, EMA, 1>(r, i, c);
  }
}

// pass 2 of the mixed step: the f32 instantiation on float(p) and the f32 moments, the stochastically
// rounded store, and the shadow following the value stored
template <bool DECAY, bool EMA, int N>
__device__ __forceinline__ void apply_sr_at(const ProdigyRow& r, int64_t i, const ProdigyApply& c, uint32_t ordinal,
                                            uint32_t step, uint32_t k0, uint32_t k1) {
  float p[N], m[N], v[N], sh[N], unused = 0.f;
  ld<true, N>(r.param, i, p);
  ld<false, N>(r.m, i, m);
  ld<false, N>(r.v, i, v);
  if (EMA) ld<false, N>(r.shadow, i, sh);
  const Philox4 o = sr_philox(i, ordinal, step, k0, k1);  // under the loads
#pragma unroll
  for (int j = 0; j < N; ++j) p[j] = prodigy_apply_elem<false, DECAY, false>(p[j], m[j], v[j], c, unused);
  st_sr<N>(r.param, i, p, o);  // p becomes the value stored
  if (EMA) {
#pragma unroll
    for (int j = 0; j < N; ++j) sh[j] = __fsub_rn(sh[j], __fmul_rn(c.omd, __fsub_rn(sh[j], p[j])));
    st<false, N>(r.shadow, i, sh);
  }
}

template <bool DECAY, bool EMA>
__global__ __launch_bounds__(256) void prodigy_apply_multi_sr_kernel(const int64_t* __restrict__ table,
                                                                     const ProdigyRecord* __restrict__ rec,
                                                                     double eps, double weight_decay, float omd,
                                                                     uint32_t k0, uint32_t k1, uint32_t step) {
  if (rec->applied == 0.0) return;
  const ProdigyRow r = prodigy_row(table, false, EMA);
  const uint32_t ordinal = (uint32_t)table[(int64_t)blockIdx.x * PRODIGY_ROW + 9];
  const double dlr = rec->dlr;
  ProdigyApply c;
  c.deps = (float)(rec->d * eps);
  c.decay = (float)(-weight_decay * dlr);
  c.step = (float)(-dlr);
  c.omd = omd;
  if (r.aligned && (r.start & 7) == 0) {
    const int64_t nvec = r.count / 8;
    for (int64_t q = threadIdx.x; q < nvec; q += 256)
      apply_sr_at<DECAY, EMA, 8>(r, r.start + q * 8, c, ordinal, step, k0, k1);
    const int64_t i = r.start + nvec * 8 + threadIdx.x;
    if (i < r.start + r.count) apply_sr_at<DECAY, EMA, 1>(r, i, c, ordinal, step, k0, k1);
  } else {
    for (int64_t i = r.start + threadIdx.x; i < r.start + r.count; i += 256)
      apply_sr_at<DECAY, EMA, 1>(r, i, c, ordinal, step, k0, k1);
  }
}

}  // namespace ltx

using namespace ltx;

extern "C" {

int ltx_prodigy_moments_multi(const int64_t* table, int64_t nchunks, int is_bf16, const double* record, double lr,
                              double beta1, double beta2, double beta3, double d0, double coupled_weight_decay,
                              int use_bias_correction, int safeguard_warmup, const float* coef_or_null, double* part,
                              void* stream) {
  LTX_CHECK_ARG(table && record && part && nchunks > 0 && nchunks < (1LL << 31), "prodigy_moments_multi: bad args");
  LTX_CHECK_ARG((((uintptr_t)record | (uintptr_t)part) & 7) == 0, "prodigy_moments_multi: record and part must be 8-byte aligned");
  LTX_CHECK_ARG(d0 > 0.0, "prodigy_moments_multi: d0 must be > 0");
  const ProdigyHyper h = {lr, beta1, beta2, beta3, d0, coupled_weight_decay, use_bias_correction, safeguard_warmup};
  const dim3 grid((unsigned)nchunks), block(256);
  hipStream_t st = (hipStream_t)stream;
  const ProdigyRecord* rec = (const ProdigyRecord*)record;
  LTX_CHECK_ARG(is_bf16 >= 0 && is_bf16 <= 2, "prodigy_moments_multi: is_bf16 is 0 (f32), 1 (bf16) or 2 (mixed)");
  const int sel = (is_bf16 == 2 ? 8 : is_bf16 ? 4 : 0) | (coef_or_null ? 2 : 0) | (coupled_weight_decay != 0.0 ? 1 : 0);
#define LTX_PRODIGY_P1(BF, CL, CO)                                                                          \
  hipLaunchKernelGGL((prodigy_moments_multi_kernel<BF, CL, CO>), grid, block, 0, st, table, rec, h, coef_or_null, \
                     part)
  switch (sel) {
    case 0: LTX_PRODIGY_P1(false, false, false); break;
    case 1: LTX_PRODIGY_P1(false, false, true); break;
    case 2: LTX_PRODIGY_P1(false, true, false); break;
    case 3: LTX_PRODIGY_P1(false, true, true); break;
    case 4: LTX_PRODIGY_P1(true, false, false); break;
    case 5: LTX_PRODIGY_P1(true, false, true); break;
    case 6: LTX_PRODIGY_P1(true, true, false); break;
    case 7: LTX_PRODIGY_P1(true, true, true); break;
#define LTX_PRODIGY_P1M(CL, CO)                                                                                  \
  hipLaunchKernelGGL((prodigy_moments_multi_kernel<true, CL, CO, true>), grid, block, 0, st, table, rec, h,     \
                     coef_or_null, part)
    case 8: LTX_PRODIGY_P1M(false, false); break;
    case 9: LTX_PRODIGY_P1M(false, true); break;
    case 10: LTX_PRODIGY_P1M(true, false); break;
    default: LTX_PRODIGY_P1M(true, true); break;
#undef LTX_PRODIGY_P1M
  }
#undef LTX_PRODIGY_P1
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_prodigy_d_update(const double* part, int64_t nrows, double* record, double lr, double beta1, double beta2,
                         double beta3, double d0, double d_coef, double growth_rate, int use_bias_correction,
                         void* stream) {
  LTX_CHECK_ARG(part && record && nrows > 0 && nrows < (1LL << 31), "prodigy_d_update: bad args");
  LTX_CHECK_ARG((((uintptr_t)record | (uintptr_t)part) & 7) == 0, "prodigy_d_update: record and part must be 8-byte aligned");
  LTX_CHECK_ARG(d0 > 0.0, "prodigy_d_update: d0 must be > 0");
  const ProdigyHyper h = {lr, beta1, beta2, beta3, d0, 0.0, use_bias_correction, 0};
  hipLaunchKernelGGL(prodigy_d_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, (int)nrows,
                     (ProdigyRecord*)record, h, d_coef, growth_rate);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_prodigy_apply_multi(const int64_t* table, int64_t nchunks, int is_bf16, const double* record, double eps,
                            double decoupled_weight_decay, int ema, float one_minus_decay, void* stream) {
  LTX_CHECK_ARG(table && record && nchunks > 0 && nchunks < (1LL << 31), "prodigy_apply_multi: bad args");
  LTX_CHECK_ARG(((uintptr_t)record & 7) == 0, "prodigy_apply_multi: record must be 8-byte aligned");
  LTX_CHECK_ARG(!ema || (one_minus_decay >= 0.f && one_minus_decay <= 1.f),
                "prodigy_apply_multi: one_minus_decay outside [0, 1]");
  const dim3 grid((unsigned)nchunks), block(256);
  hipStream_t st = (hipStream_t)stream;
  const ProdigyRecord* rec = (const ProdigyRecord*)record;
  const int sel = (is_bf16 ? 4 : 0) | (decoupled_weight_decay != 0.0 ? 2 : 0) | (ema ? 1 : 0);
#define LTX_PRODIGY_P2(BF, DE, EM)                                                                         \
  hipLaunchKernelGGL((prodigy_apply_multi_kernel<BF, DE, EM>), grid, block, 0, st, table, rec, eps,        \
                     decoupled_weight_decay, one_minus_decay)
  switch (sel) {
    case 0: LTX_PRODIGY_P2(false, false, false); break;
    case 1: LTX_PRODIGY_P2(false, false, true); break;
    case 2: LTX_PRODIGY_P2(false, true, false); break;
    case 3: LTX_PRODIGY_P2(false, true, true); break;
    case 4: LTX_PRODIGY_P2(true, false, false); break;
    case 5: LTX_PRODIGY_P2(true, false, true); break;
    case 6: LTX_PRODIGY_P2(true, true, false); break;
    default: LTX_PRODIGY_P2(true, true, true); break;
  }
#undef LTX_PRODIGY_P2
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_prodigy_apply_multi_sr(const int64_t* table, int64_t nchunks, const double* record, double eps,
                               double decoupled_weight_decay, int ema, float one_minus_decay, uint64_t seed,
                               int64_t step, void* stream) {
  LTX_CHECK_ARG(table && record && nchunks > 0 && nchunks < (1LL << 31) && step >= 1, "prodigy_apply_multi_sr: bad args");
  LTX_CHECK_ARG(((uintptr_t)record & 7) == 0, "prodigy_apply_multi_sr: record must be 8-byte aligned");
  LTX_CHECK_ARG(!ema || (one_minus_decay >= 0.f && one_minus_decay <= 1.f),
                "prodigy_apply_multi_sr: one_minus_decay outside [0, 1]");
  const dim3 grid((unsigned)nchunks), block(256);
  hipStream_t st = (hipStream_t)stream;
  const ProdigyRecord* rec = (const ProdigyRecord*)record;
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  const uint32_t step32 = (uint32_t)((uint64_t)step & 0xffffffffu);
#define LTX_PRODIGY_P2S(DE, EM)                                                                            \
  hipLaunchKernelGGL((prodigy_apply_multi_sr_kernel<DE, EM>), grid, block, 0, st, table, rec, eps,         \
                     decoupled_weight_decay, one_minus_decay, k0, k1, step32)
  if (decoupled_weight_decay != 0.0) {
    if (ema) LTX_PRODIGY_P2S(true, true);
    else LTX_PRODIGY_P2S(true, false);
  } else {
    if (ema) LTX_PRODIGY_P2S(false, true);
    else LTX_PRODIGY_P2S(false, false);
  }
#undef LTX_PRODIGY_P2S
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

}  // extern "C"
