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
// Behind the non-finite guard (FusedProdigy(skip_nonfinite=True); GuardRecord, chunk_io.h) pass 1 and the d
// update run as prodigy_moments_multi_guard_kernel and prodigy_d_update_guard_kernel, the same bodies
// behind one read of the guard's `applied`: a skipped step's pass 1 returns before its first load (its row
// partials stay unwritten and unread), its d update sets the record's applied to 0 and leaves the other
// seven fields, and pass 2 is then the no-op it already is under applied == 0.
//
// The table has 10 int64 per row: (param, grad, exp_avg, exp_avg_sq, first element, count <= 2048, s, p0,
// shadow, ordinal); the shadow is 0 without the EMA, the ordinal 0 outside the stochastic step. A row whose
// tensors are all 16-byte aligned is walked with 16-byte accesses (4 f32 or 8 bf16 per lane, the row's last
// count % 4 or 8 elements one per lane); rows over a tensor that is not (a gradient that is a view into a
// reducer's bucket) take one element per lane throughout (chunk_io.h walk_row). The arithmetic per element
// is the same (prodigy_elem.h).
//
// Both passes are templated on two storage types: PBF, bf16 param / grad / p0, and SBF, bf16 exp_avg /
// exp_avg_sq / s, whose dtype the arithmetic is rounded to. f32 / f32 and bf16 / bf16 are the nearest-mode
// steps. bf16 storage with f32 state is the mixed step of FusedProdigy(bf16_update="stochastic"): the f32
// arithmetic on the widened values, and pass 2 stores the parameter stochastically rounded (chunk_io.h
// st_sr) under the row's ordinal.
#include <cmath>

#include "adamw_elem.h"
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

struct ProdigyHyper {
  double lr, beta1, beta2, beta3, d0, weight_decay;
  int use_bias_correction, safeguard_warmup;
};

// with a coefficient the gradient is first what grad.mul_(coef) would leave in its tensor
template <bool PBF, bool SBF, bool CLIP, bool COUPLED, int N>
__device__ __forceinline__ void moments_at(const ProdigyRow& r, int64_t i, const ProdigyMoments& c, double& num,
                                           double& den) {
  float p[N], g[N], p0[N], m[N], v[N], s[N];
  ld<PBF, N>(r.param, i, p);
  ld<PBF, N>(r.grad, i, g);
  ld<PBF, N>(r.p0, i, p0);
  ld<SBF, N>(r.m, i, m);
  ld<SBF, N>(r.v, i, v);
  ld<SBF, N>(r.s, i, s);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    float tn, td;
    const float gj = !CLIP ? g[j] : PBF ? rbf(g[j] * c.coef) : g[j] * c.coef;
    prodigy_moments_elem<SBF, COUPLED>(p[j], gj, p0[j], m[j], v[j], s[j], c, tn, td);
    num += (double)tn;
    den += (double)td;
  }
  st<SBF, N>(r.m, i, m);
  st<SBF, N>(r.v, i, v);
  st<SBF, N>(r.s, i, s);
}

template <bool PBF, bool SBF, bool CLIP, bool COUPLED>
__device__ __forceinline__ void prodigy_moments_row(const int64_t* __restrict__ table,
                                                    const ProdigyRecord* __restrict__ rec, const ProdigyHyper& h,
                                                    const float* __restrict__ coef, double* __restrict__ part) {
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
  walk_row<PBF ? 8 : 4>(r.start, r.count, r.aligned, [&](auto n, int64_t i) {
    moments_at<PBF, SBF, CLIP, COUPLED, decltype(n)::value>(r, i, c, num, den);
  });
  __shared__ double red[2][4];
  num = block_sum_ordered(num, red[0]);
  den = block_sum_ordered(den, red[1]);
  if (threadIdx.x == 0) {
    part[2 * (int64_t)blockIdx.x] = num;
    part[2 * (int64_t)blockIdx.x + 1] = den;
  }
}

template <bool PBF, bool SBF, bool CLIP, bool COUPLED>
__global__ __launch_bounds__(256) void prodigy_moments_multi_kernel(const int64_t* __restrict__ table,
                                                                    const ProdigyRecord* __restrict__ rec,
                                                                    ProdigyHyper h, const float* __restrict__ coef,
                                                                    double* __restrict__ part) {
  prodigy_moments_row<PBF, SBF, CLIP, COUPLED>(table, rec, h, coef, part);
}

template <bool PBF, bool SBF, bool CLIP, bool COUPLED>
__global__ __launch_bounds__(256) void prodigy_moments_multi_guard_kernel(const int64_t* __restrict__ table,
                                                                          const ProdigyRecord* __restrict__ rec,
                                                                          ProdigyHyper h,
                                                                          const float* __restrict__ coef,
                                                                          double* __restrict__ part,
                                                                          const GuardRecord* __restrict__ guard) {
  if (!step_applied(guard)) return;
  prodigy_moments_row<PBF, SBF, CLIP, COUPLED>(table, rec, h, coef, part);
}

// part holds (num, den) pairs, one per row, summed in a fixed order (strided_partials_sum, as
// grad_clip_coef_kernel); thread 0 runs the update.
__device__ __forceinline__ void prodigy_d_update_block(const double* __restrict__ part, int nrows,
                                                       ProdigyRecord* __restrict__ rec, const ProdigyHyper& h,
                                                       double d_coef, double growth_rate) {
  __shared__ double red[2][256];
  strided_partials_sum<2>(part, nrows, red);
  if (threadIdx.x == 0) {
    double d = rec->d;
    const double dlr = prodigy_dlr(d, rec->k, h.lr, h.beta1, h.beta2, h.use_bias_correction);
    const double d_denom = red[1][0];
    rec->dlr = dlr;
    rec->d_denom = d_denom;
    if (d_denom == 0.0) {
      rec->applied = 0.0;
    } else {
      const double d_numerator = h.beta3 * rec->d_numerator + (d / h.d0) * dlr * red[0][0];
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

__global__ __launch_bounds__(256) void prodigy_d_update_kernel(const double* __restrict__ part, int nrows,
                                                               ProdigyRecord* __restrict__ rec, ProdigyHyper h,
                                                               double d_coef, double growth_rate) {
  prodigy_d_update_block(part, nrows, rec, h, d_coef, growth_rate);
}

// a skipped step: applied = 0, which makes pass 2 a no-op; d, d_max, d_numerator, d_denom, d_hat, dlr and k stay
__global__ __launch_bounds__(256) void prodigy_d_update_guard_kernel(const double* __restrict__ part, int nrows,
                                                                     ProdigyRecord* __restrict__ rec, ProdigyHyper h,
                                                                     double d_coef, double growth_rate,
                                                                     const GuardRecord* __restrict__ guard) {
  if (!step_applied(guard)) {
    if (threadIdx.x == 0) rec->applied = 0.0;
    return;
  }
  prodigy_d_update_block(part, nrows, rec, h, d_coef, growth_rate);
}

// the stream of a row's stochastic rounding (the mixed step only)
struct SrStream {
  uint32_t ordinal, step, k0, k1;
};

// the mixed step (PBF and not SBF) stores stochastically rounded; the shadow follows the value stored
template <bool PBF, bool SBF, bool DECAY, bool EMA, int N>
__device__ __forceinline__ void apply_at(const ProdigyRow& r, int64_t i, const ProdigyApply& c, const SrStream& z) {
  constexpr bool SR = PBF && !SBF;
  float p[N], m[N], v[N], sh[N];
  ld<PBF, N>(r.param, i, p);
  ld<SBF, N>(r.m, i, m);
  ld<SBF, N>(r.v, i, v);
  if (EMA) ld<false, N>(r.shadow, i, sh);
  Philox4 o;
  if constexpr (SR) o = sr_philox(i, z.ordinal, z.step, z.k0, z.k1);  // under the loads
#pragma unroll
  for (int j = 0; j < N; ++j) p[j] = prodigy_apply_elem<SBF, DECAY>(p[j], m[j], v[j], c);
  if constexpr (SR) st_sr<N>(r.param, i, p, o);  // p becomes the value stored
  else st<PBF, N>(r.param, i, p);
  if (EMA) {
#pragma unroll
    for (int j = 0; j < N; ++j) sh[j] = ema_update(sh[j], p[j], c.omd);
    st<false, N>(r.shadow, i, sh);
  }
}

// k0, k1 (the seed's words) and step serve the mixed step only
template <bool PBF, bool SBF, bool DECAY, bool EMA>
__global__ __launch_bounds__(256) void prodigy_apply_multi_kernel(const int64_t* __restrict__ table,
                                                                  const ProdigyRecord* __restrict__ rec, double eps,
                                                                  double weight_decay, float omd, uint32_t k0,
                                                                  uint32_t k1, uint32_t step) {
  constexpr bool SR = PBF && !SBF;
  if (rec->applied == 0.0) return;
  const ProdigyRow r = prodigy_row(table, false, EMA);
  const SrStream z = {SR ? (uint32_t)table[(int64_t)blockIdx.x * PRODIGY_ROW + 9] : 0u, step, k0, k1};
  const double dlr = rec->dlr;
  ProdigyApply c;
  c.deps = (float)(rec->d * eps);
  c.decay = (float)(-weight_decay * dlr);
  c.step = (float)(-dlr);
  c.omd = omd;
  // st_sr's 8 elements share one generator call: a vector starts at a multiple of 8 in its tensor
  walk_row<PBF ? 8 : 4>(r.start, r.count, r.aligned && (!SR || (r.start & 7) == 0), [&](auto n, int64_t i) {
    apply_at<PBF, SBF, DECAY, EMA, decltype(n)::value>(r, i, c, z);
  });
}

// the launch of pass 2 in the storage types (PBF, SBF) behind its two entry points
template <bool PBF, bool SBF>
static void launch_prodigy_apply(const int64_t* table, int64_t nchunks, const double* record, double eps,
                                 double decoupled_weight_decay, int ema, float one_minus_decay, uint64_t seed,
                                 int64_t step, void* stream) {
  with_flag(decoupled_weight_decay != 0.0, [&](auto decay) {
    with_flag(ema, [&](auto em) {
      hipLaunchKernelGGL((prodigy_apply_multi_kernel<PBF, SBF, decltype(decay)::value, decltype(em)::value>),
                         dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, table,
                         (const ProdigyRecord*)record, eps, decoupled_weight_decay, one_minus_decay,
                         (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32),
                         (uint32_t)((uint64_t)step & 0xffffffffu));
    });
  });
}

// pass 1 in the storage types of is_bf16 (0 f32, 1 bf16, 2 mixed), behind the guard when one is given
static int launch_prodigy_moments(const int64_t* table, int64_t nchunks, int is_bf16,
                                  const double* record, double lr, double beta1, double beta2, double beta3, double d0,
                                  double coupled_weight_decay, int use_bias_correction, int safeguard_warmup,
                                  const float* coef_or_null, double* part, const GuardRecord* guard, void* stream) {
  LTX_CHECK_ARG(table && record && part && nchunks > 0 && nchunks < (1LL << 31), "prodigy_moments_multi: bad args");
  LTX_CHECK_ARG((((uintptr_t)record | (uintptr_t)part | (uintptr_t)guard) & 7) == 0,
                "prodigy_moments_multi: record, part and guard must be 8-byte aligned");
  LTX_CHECK_ARG(d0 > 0.0, "prodigy_moments_multi: d0 must be > 0");
  const ProdigyHyper h = {lr, beta1, beta2, beta3, d0, coupled_weight_decay, use_bias_correction, safeguard_warmup};
  LTX_CHECK_ARG(is_bf16 >= 0 && is_bf16 <= 2, "prodigy_moments_multi: is_bf16 is 0 (f32), 1 (bf16) or 2 (mixed)");
  auto launch = [&](auto pbf, auto sbf) {
    with_flag(coef_or_null != nullptr, [&](auto clip) {
      with_flag(coupled_weight_decay != 0.0, [&](auto coupled) {
        if (guard)
          hipLaunchKernelGGL((prodigy_moments_multi_guard_kernel<decltype(pbf)::value, decltype(sbf)::value,
                                                                 decltype(clip)::value, decltype(coupled)::value>),
                             dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, table,
                             (const ProdigyRecord*)record, h, coef_or_null, part, guard);
        else
          hipLaunchKernelGGL((prodigy_moments_multi_kernel<decltype(pbf)::value, decltype(sbf)::value,
                                                           decltype(clip)::value, decltype(coupled)::value>),
                             dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, table,
                             (const ProdigyRecord*)record, h, coef_or_null, part);
      });
    });
  };
  if (is_bf16 == 2) launch(std::true_type{}, std::false_type{});
  else if (is_bf16) launch(std::true_type{}, std::true_type{});
  else launch(std::false_type{}, std::false_type{});
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

// the d update, behind the guard when one is given
static int launch_prodigy_d_update(const double* part, int64_t nrows, double* record, double lr, double beta1,
                                   double beta2, double beta3, double d0, double d_coef, double growth_rate,
                                   int use_bias_correction, const GuardRecord* guard, void* stream) {
  LTX_CHECK_ARG(part && record && nrows > 0 && nrows < (1LL << 31), "prodigy_d_update: bad args");
  LTX_CHECK_ARG((((uintptr_t)record | (uintptr_t)part | (uintptr_t)guard) & 7) == 0,
                "prodigy_d_update: record, part and guard must be 8-byte aligned");
  LTX_CHECK_ARG(d0 > 0.0, "prodigy_d_update: d0 must be > 0");
  const ProdigyHyper h = {lr, beta1, beta2, beta3, d0, 0.0, use_bias_correction, 0};
  if (guard)
    hipLaunchKernelGGL(prodigy_d_update_guard_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, (int)nrows,
                       (ProdigyRecord*)record, h, d_coef, growth_rate, guard);
  else
    hipLaunchKernelGGL(prodigy_d_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, (int)nrows,
                       (ProdigyRecord*)record, h, d_coef, growth_rate);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

}  // namespace ltx

using namespace ltx;

extern "C" {

int ltx_prodigy_moments_multi(const int64_t* table, int64_t nchunks, int is_bf16, const double* record, double lr,
                              double beta1, double beta2, double beta3, double d0, double coupled_weight_decay,
                              int use_bias_correction, int safeguard_warmup, const float* coef_or_null, double* part,
                              void* stream) {
  return launch_prodigy_moments(table, nchunks, is_bf16, record, lr, beta1, beta2, beta3, d0,
                                coupled_weight_decay, use_bias_correction, safeguard_warmup, coef_or_null, part,
                                nullptr, stream);
}

int ltx_prodigy_moments_multi_guard(const int64_t* table, int64_t nchunks, int is_bf16, const double* record,
                                    double lr, double beta1, double beta2, double beta3, double d0,
                                    double coupled_weight_decay, int use_bias_correction, int safeguard_warmup,
                                    const float* coef_or_null, double* part, const void* guard, void* stream) {
  LTX_CHECK_ARG(guard, "prodigy_moments_multi_guard: guard is null");
  return launch_prodigy_moments(table, nchunks, is_bf16, record, lr, beta1, beta2,
                                beta3, d0, coupled_weight_decay, use_bias_correction, safeguard_warmup, coef_or_null,
                                part, (const GuardRecord*)guard, stream);
}

int ltx_prodigy_d_update(const double* part, int64_t nrows, double* record, double lr, double beta1, double beta2,
                         double beta3, double d0, double d_coef, double growth_rate, int use_bias_correction,
                         void* stream) {
  return launch_prodigy_d_update(part, nrows, record, lr, beta1, beta2, beta3, d0, d_coef, growth_rate,
                                 use_bias_correction, nullptr, stream);
}

int ltx_prodigy_d_update_guard(const double* part, int64_t nrows, double* record, double lr, double beta1,
                               double beta2, double beta3, double d0, double d_coef, double growth_rate,
                               int use_bias_correction, const void* guard, void* stream) {
  LTX_CHECK_ARG(guard, "prodigy_d_update_guard: guard is null");
  return launch_prodigy_d_update(part, nrows, record, lr, beta1, beta2, beta3, d0, d_coef, growth_rate,
                                 use_bias_correction, (const GuardRecord*)guard, stream);
}

int ltx_prodigy_apply_multi(const int64_t* table, int64_t nchunks, int is_bf16, const double* record, double eps,
                            double decoupled_weight_decay, int ema, float one_minus_decay, void* stream) {
  LTX_CHECK_ARG(table && record && nchunks > 0 && nchunks < (1LL << 31), "prodigy_apply_multi: bad args");
  LTX_CHECK_ARG(((uintptr_t)record & 7) == 0, "prodigy_apply_multi: record must be 8-byte aligned");
  LTX_CHECK_ARG(!ema || (one_minus_decay >= 0.f && one_minus_decay <= 1.f),
                "prodigy_apply_multi: one_minus_decay outside [0, 1]");
  if (is_bf16)
    launch_prodigy_apply<true, true>(table, nchunks, record, eps, decoupled_weight_decay, ema, one_minus_decay, 0, 0,
                                     stream);
  else
    launch_prodigy_apply<false, false>(table, nchunks, record, eps, decoupled_weight_decay, ema, one_minus_decay, 0, 0,
                                       stream);
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
  launch_prodigy_apply<true, false>(table, nchunks, record, eps, decoupled_weight_decay, ema, one_minus_decay, seed,
                                    step, stream);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

}  // extern "C"
