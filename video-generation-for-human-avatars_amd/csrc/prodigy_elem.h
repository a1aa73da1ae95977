// The per-element Prodigy arithmetic shared by the kernels of prodigy.hip, on register values, so every
// entry point and both access widths run one arithmetic. It is the published optimizer's sequence of torch
// ops (prodigyopt, one parameter group, fsdp_in_use = False), each evaluated the way torch's device
// kernels evaluate it and rounded to the tensor's dtype (R) after each op:
//   x.mul_(c)                       R(x * c)                 one f32 multiply
//   x.add_(y, alpha=a)              R(fma(a, y, x))          the add kernel's a * y + x is one fused op
//   x.addcmul_(y, z, value=a)       R(fma(a, y * z, x))      y * z rounded to f32 (not to bf16), then one fused op
//   x.addcdiv_(y, z, value=a)       R(fma(a, y / z, x))      y / z correctly rounded to f32, then one fused op
//   x.sqrt(), x - y, x.add_(c)      one correctly rounded f32 op each
// The library is built with -ffp-contract=off, so only the fmaf calls written here fuse; sqrtf and / are hipcc's
// correctly rounded ones (its default; the __fsqrt_rn intrinsic is the native approximation here).
#pragma once
#include <cmath>

#include "common.h"

namespace ltx {

// the device record of the optimizer (8 f64; the host holds it as one float64 tensor)
struct ProdigyRecord {
  double d;            // the step-size estimate
  double d_max;        // its running maximum
  double d_numerator;  // beta3-averaged sum of dlr (d / d0) <g, p0 - p>
  double d_denom;      // the last step's sum of |s|
  double d_hat;        // the last applied step's d_coef d_numerator / d_denom
  double dlr;          // d lr bc of the last step, with the d that step started from
  double k;            // applied steps (an integer value)
  double applied;      // 1 when the last step's d_denom was not 0 (pass 2 ran), else 0
};
static_assert(sizeof(ProdigyRecord) == 64, "ProdigyRecord layout");

// bc = sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) or 1; dlr = d lr bc, in f64 from the record. Passes 1
// and the d update both call this on the same record, so they see the same bits.
__device__ __forceinline__ double prodigy_dlr(double d, double k, double lr, double beta1, double beta2,
                                              int use_bias_correction) {
  double bc = 1.0;
  if (use_bias_correction) bc = sqrt(1.0 - pow(beta2, k + 1.0)) / (1.0 - pow(beta1, k + 1.0));
  return d * lr * bc;
}

// pass 1's scalars: f32 where torch casts a Python float to the tensor's compute type
struct ProdigyMoments {
  float b1, b2, b3;  // (float)beta
  float a1;          // (float)(d (1 - beta1))
  float a2;          // (float)(d d (1 - beta2))
  float a3;          // (float)((d / d0) (safeguard_warmup ? d : dlr))
  float wd;          // (float)weight_decay of the coupled form (COUPLED only)
  float coef;        // the clip coefficient, applied by the caller in the gradient's dtype
};

// One element of pass 1, all with the step's old d. g is the gradient as loaded (under the clip, scaled
// and rounded to its dtype); m, v, s are updated in place; num and den are the element's terms of the two
// sums, R(p0 - p) * g as an f32 product and the stored |s|. BF16: the dtype of the state, whose arithmetic
// this is.
template <bool BF16, bool COUPLED>
__device__ __forceinline__ void prodigy_moments_elem(float p, float g, float p0, float& m, float& v, float& s,
                                                     const ProdigyMoments& c, float& num, float& den) {
  auto R = [](float x) { return BF16 ? rbf(x) : x; };
  if (COUPLED) g = R(fmaf(c.wd, p, g));
  num = R(p0 - p) * g;
  m = R(fmaf(c.a1, g, R(m * c.b1)));
  v = R(fmaf(c.a2, g * g, R(v * c.b2)));
  s = R(fmaf(c.a3, g, R(s * c.b3)));
  den = fabsf(s);
}

// pass 2's scalars
struct ProdigyApply {
  float deps;   // (float)(d_new eps)
  float decay;  // (float)(-weight_decay dlr) of the decoupled form (DECAY only)
  float step;   // (float)(-dlr)
  float omd;    // (float)(1 - EMA decay) of the caller's shadow update (adamw_elem.h ema_update)
};

// One element of pass 2: returns the new parameter, before the store
template <bool BF16, bool DECAY>
__device__ __forceinline__ float prodigy_apply_elem(float p, float m, float v, const ProdigyApply& c) {
  auto R = [](float x) { return BF16 ? rbf(x) : x; };
  const float den = R(R(sqrtf(v)) + c.deps);
  if (DECAY) p = R(fmaf(c.decay, p, p));
  return R(fmaf(c.step, m / den, p));
}

}  // namespace ltx
