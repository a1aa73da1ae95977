// The per-element AdamW update shared by the optimizer kernels (elementwise.hip: ltx_adamw_step; optim.hip:
// ltx_adamw_multi / ltx_adamw_multi_clip / ltx_adamw_multi_ema / ltx_adamw_multi_sr), so every entry point
// runs one arithmetic; the shadow's step (ema_update) serves prodigy.hip too.
#pragma once
#include <cmath>

#include "common.h"

namespace ltx {

// torch.lerp's two-sided form (ATen lerp: w < 0.5 ? self + w (end - self) : end - (end - self)(1 - w))
__device__ __forceinline__ float torch_lerp(float self, float end, float w) {
  const float d = end - self;
  return fabsf(w) < 0.5f ? fmaf(w, d, self) : fmaf(-d, 1.0f - w, end);
}

// The arithmetic described below on register values: p, m, v in and out, g the gradient as loaded. R rounds
// to bf16 for BF16 and is the identity for f32.
template <bool BF16, bool CLIP>
__device__ __forceinline__ void adamw_update(float& p, float g, float& m, float& v, float decay, float w1, float b2,
                                             float w2, float step_size, float bc2_sqrt, float eps, float coef) {
  auto R = [](float x) { return BF16 ? rbf(x) : x; };
  if (CLIP) g = R(g * coef);
  p = R(p * decay);
  m = R(torch_lerp(m, g, w1));
  v = R(v * b2);
  v = R(v + w2 * g * g);
  float den = R(sqrtf(v));
  den = R(den / bc2_sqrt);
  den = R(den + eps);
  p = R(p + step_size * (m / den));
}

// the shadow's step: s - omd (s - p') as three separately rounded f32 operations
__device__ __forceinline__ float ema_update(float s, float p, float omd) {
  return __fsub_rn(s, __fmul_rn(omd, __fsub_rn(s, p)));
}

// torch.optim.AdamW, foreach implementation order (weight decay, lerp m, v*b2 + (1-b2) g g,
// sqrt, / sqrt(bc2), + eps, p += step_size * m / den), rounding every op for bf16 tensors.
// CLIP: the gradient is first scaled by `coef` and rounded to its dtype, which is what an in-place
// grad.mul_(coef) would leave in memory (the global-norm clip; grad itself is not written).
// EMA: the f32 shadow of the parameter follows the value this step stores, p' (for bf16 the value just
// rounded to bf16): s <- s - omd (s - float(p')), diffusers' EMAModel.step
// s_param.sub_(one_minus_decay * (s_param - param)) as three separately rounded f32 operations (no FMA).
// The shadow only observes the step: p', m and v are those of EMA = false.
template <bool BF16, bool CLIP = false, bool EMA = false>
__device__ __forceinline__ void adamw_elem(void* __restrict__ param, const void* __restrict__ grad,
                                           void* __restrict__ m_, void* __restrict__ v_, int64_t i, float decay,
                                           float w1, float b2, float w2, float step_size, float bc2_sqrt, float eps,
                                           float coef = 1.0f, float* __restrict__ shadow = nullptr,
                                           float omd = 0.0f) {
  float p, g, m, v;
  if (BF16) {
    p = bf2f(((bf16_t*)param)[i]); g = bf2f(((const bf16_t*)grad)[i]);
    m = bf2f(((bf16_t*)m_)[i]); v = bf2f(((bf16_t*)v_)[i]);
  } else {
    p = ((float*)param)[i]; g = ((const float*)grad)[i]; m = ((float*)m_)[i]; v = ((float*)v_)[i];
  }
  adamw_update<BF16, CLIP>(p, g, m, v, decay, w1, b2, w2, step_size, bc2_sqrt, eps, coef);
  if (EMA) shadow[i] = ema_update(shadow[i], p, omd);
  if (BF16) {
    ((bf16_t*)param)[i] = f2bf(p); ((bf16_t*)m_)[i] = f2bf(m); ((bf16_t*)v_)[i] = f2bf(v);
  } else {
    ((float*)param)[i] = p; ((float*)m_)[i] = m; ((float*)v_)[i] = v;
  }
}

// the host half: the step's scalars from the hyper-parameters, in double as torch computes them
struct AdamWScalars {
  float decay, w1, w2, step_size, bc2_sqrt;
};
static inline AdamWScalars adamw_scalars(float lr, float beta1, float beta2, float weight_decay, int64_t step) {
  const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
  const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
  AdamWScalars s;
  s.decay = (float)(1.0 - (double)lr * (double)weight_decay);
  s.step_size = (float)(-((double)lr / bc1));
  s.bc2_sqrt = (float)std::sqrt(bc2);
  s.w1 = (float)(1.0 - (double)beta1);
  s.w2 = (float)(1.0 - (double)beta2);
  return s;
}

}  // namespace ltx
