// Weighted velocity loss of the LTX-Video training step: per-token loss weights built on the device
// (face box coverage x frame weight x per-sample timestep factor x caller weights, normalised so each
// sample's weights average to its timestep factor) and the weighted form of mse_kernel
// (elementwise.hip) that consumes them: the same flat traversal, roundings and fixed-order partial
// sums, one multiply and one rounding more per element. ltx_mse_fwd_bwd itself is untouched: with
// nothing configured the step never comes here. And the robust (pseudo-Huber) loss that takes either's
// place under loss_type huber / smooth_l1: the same traversal and sums, the loss term evaluated in f32
// against a threshold per sample.
#include "common.h"
#include "ltx_hip.h"

namespace ltx {

// ---------------------------------------------------------------------------------------------
// Token weights. One 256-thread workgroup per sample: pass 1 writes raw[b, n] into wt and sums it
// (each thread its strided elements in order, the wave butterfly, four waves in order: no atomics,
// bitwise run to run), pass 2 rescales what the same thread wrote. All arithmetic f32.
//   box      = the sample's (x0, y0, x1, y1), padded by face_pad x its width / height on each side,
//              clipped to [0, 1]; a NaN coordinate or an empty clipped box: coverage 0 everywhere
//   ox       = min(1, max(0, min(x1, (w + 1) / W) - max(x0, w / W)) * W), oy likewise with h, H
//   raw[n]   = frame_w[f] * (1 + (face_weight - 1) * ox * oy) * user_w[b, n]
//   wt[b, n] = raw[n] * (sample_w[b] * N / raw_sum[b]), 0 where raw_sum[b] == 0
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void loss_token_weights_kernel(
    const float* __restrict__ bbox, const float* __restrict__ frame_w, const float* __restrict__ sample_w,
    const float* __restrict__ user_w, float face_weight, float face_pad, float* __restrict__ wt,
    float* __restrict__ raw_sum, int64_t F, int64_t H, int64_t W) {
  const int64_t b = blockIdx.x;
  const int64_t HW = H * W, N = F * HW;
  float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
  bool face = false;
  if (bbox) {
    x0 = bbox[4 * b + 0];
    y0 = bbox[4 * b + 1];
    x1 = bbox[4 * b + 2];
    y1 = bbox[4 * b + 3];
    // the NaN test comes before the clip: fminf / fmaxf drop a NaN operand
    face = !(x0 != x0 || y0 != y0 || x1 != x1 || y1 != y1);
    const float px = face_pad * (x1 - x0), py = face_pad * (y1 - y0);
    x0 = fminf(fmaxf(x0 - px, 0.f), 1.f);
    x1 = fminf(fmaxf(x1 + px, 0.f), 1.f);
    y0 = fminf(fmaxf(y0 - py, 0.f), 1.f);
    y1 = fminf(fmaxf(y1 + py, 0.f), 1.f);
    face = face && x1 > x0 && y1 > y0;
  }
  const float gain = face_weight - 1.0f, fW = (float)W, fH = (float)H;
  float* wrow = wt + b * N;
  const float* urow = user_w ? user_w + b * N : nullptr;
  float s = 0.f;
  for (int64_t n = threadIdx.x; n < N; n += 256) {
    const int64_t f = n / HW, hw = n - f * HW;
    const int64_t h = hw / W, w = hw - h * W;
    float cov = 0.f;
    if (face) {
      const float ox = fminf(fmaxf(fminf(x1, (float)(w + 1) / fW) - fmaxf(x0, (float)w / fW), 0.f) * fW, 1.f);
      const float oy = fminf(fmaxf(fminf(y1, (float)(h + 1) / fH) - fmaxf(y0, (float)h / fH), 0.f) * fH, 1.f);
      cov = ox * oy;
    }
    float raw = (frame_w ? frame_w[f] : 1.0f) * (1.0f + gain * cov);
    if (urow) raw = raw * urow[n];
    wrow[n] = raw;
    s += raw;
  }
  s = wave_sum(s);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const float total = red[0] + red[1] + red[2] + red[3];
  if (threadIdx.x == 0) raw_sum[b] = total;
  const float scale = total != 0.f ? (sample_w ? sample_w[b] : 1.0f) * (float)N / total : 0.f;
  // each thread rescales the elements it wrote itself: no other thread's store is read
  for (int64_t n = threadIdx.x; n < N; n += 256) wrow[n] = total != 0.f ? wrow[n] * scale : 0.f;
}

// ---------------------------------------------------------------------------------------------
// Weighted loss forward statistics + backward seed. mse_kernel's arithmetic per element
//   d = bf16(o - v), q = bf16(d * d), g = bf16(bf16(d * 2 / n) * gscale)
// then dout = bf16(g * wt[token]) (round to nearest even), token = element / C, and
//   s0 = sum wt * q, s1 = sum v, s2 = sum v^2, s3 = sum q
// over mse_kernel's flat order (16-B vectors over n / 8, then the scalar tail) on its fixed grid, so
// with wt == 1 every output is bitwise ltx_mse_fwd_bwd's, and s1..s3 are for any wt. VEC_TOKEN
// (C % 8 == 0): a vector lies inside one token and loads one weight; otherwise the token is taken
// per element. Partials: stats[4 + c * WMSE_BLOCKS + block], c < 4.
// ---------------------------------------------------------------------------------------------
constexpr int WMSE_BLOCKS = 256;
template <bool VEC_TOKEN>
__global__ __launch_bounds__(256) void wmse_kernel(const bf16_t* __restrict__ o, const bf16_t* __restrict__ v,
                                                   const float* __restrict__ wt, bf16_t* __restrict__ dout,
                                                   float* __restrict__ stats, int64_t n, int64_t C, float norm,
                                                   float gscale) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const int64_t n8 = n / 8;
  const int64_t C8 = VEC_TOKEN ? C / 8 : 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const u32x4 ow = *(const u32x4*)(o + 8 * i), vw = *(const u32x4*)(v + 8 * i);
    const float wv = VEC_TOKEN ? wt[i / C8] : 0.f;
    u32x4 dw;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      float d2[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float ov = bf2f((bf16_t)(ow[h] >> (16 * e))), vv = bf2f((bf16_t)(vw[h] >> (16 * e)));
        const float wk = VEC_TOKEN ? wv : wt[(8 * i + 2 * h + e) / C];
        const float diff = rbf(ov - vv);
        const float q = rbf(diff * diff);
        s0 += wk * q;
        s1 += vv;
        s2 += vv * vv;
        s3 += q;
        d2[e] = rbf(rbf(diff * norm) * gscale) * wk;
      }
      dw[h] = pack2(d2[0], d2[1]);
    }
    if (dout) *(u32x4*)(dout + 8 * i) = dw;
  }
  for (int64_t i = 8 * n8 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float ov = bf2f(o[i]), vv = bf2f(v[i]);
    const float wk = wt[i / C];
    const float diff = rbf(ov - vv);
    const float q = rbf(diff * diff);
    s0 += wk * q;
    s1 += vv;
    s2 += vv * vv;
    s3 += q;
    if (dout) dout[i] = f2bf(rbf(rbf(diff * norm) * gscale) * wk);
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  s3 = wave_sum(s3);
  __shared__ float red[4][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][w] = s0;
    red[1][w] = s1;
    red[2][w] = s2;
    red[3][w] = s3;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int c = threadIdx.x;
    stats[4 + c * WMSE_BLOCKS + blockIdx.x] = red[c][0] + red[c][1] + red[c][2] + red[c][3];
  }
}

// mse_finish_kernel's fixed-order sum of the per-block partials, over four sums
__global__ __launch_bounds__(256) void wmse_finish_kernel(float* __restrict__ stats) {
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float s = 0.f;
  for (int b = lane; b < WMSE_BLOCKS; b += 64) s += stats[4 + c * WMSE_BLOCKS + b];
  s = wave_sum(s);
  if (lane == 0) stats[c] = s;
}

// ---------------------------------------------------------------------------------------------
// Robust (pseudo-Huber) loss forward statistics + backward seed. Per element, in f32 from the bf16 o, v:
//   e = o - v, r = sqrt(e * e + c * c), l = k * (e * e) / (r + c), g = k * e / r
//   k = 2 c (KIND 1, huber) | 2 (KIND 2, smooth_l1), c = c[sample] > 0, sample = element / per_sample
// (l == k (r - c), in the form that does not cancel for |e| << c) and dout = bf16((wt[token] * g) * gsn),
// gsn = grad_scale / n, rounded once; wt == null: every weight 1. r is kept >= c, which it is before
// rounding: a c whose square underflows then still gives l == 0 and g == 0 at e == 0. The square root and
// the two reciprocals are the hardware's 1-ulp instructions. Sums:
//   s0 = sum wt * l, s4 = sum l, and mse_kernel's s1 = sum v, s2 = sum v^2, s3 = sum bf16(d * d),
//   d = bf16(o - v), in its arithmetic
// over mse_kernel's flat order on its fixed grid, so s1..s3 are bitwise ltx_mse_fwd_bwd's. VEC (C % 8 == 0,
// hence per_sample % 8 == 0): a 16-B vector lies inside one token and one sample and loads one weight
// and one threshold; otherwise token and sample are taken per element. Partials:
// stats[8 + c * ROBUST_BLOCKS + block], c < 5.
// ---------------------------------------------------------------------------------------------
constexpr int ROBUST_BLOCKS = 256;

struct RobustSums {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
};

// one element: adds its terms to acc, returns the f32 seed before the one bf16 rounding
__device__ __forceinline__ float robust_elem(float ov, float vv, float wk, float cb, int kind, float gsn,
                                             RobustSums& acc) {
  const float diff = rbf(ov - vv);
  acc.s1 += vv;
  acc.s2 += vv * vv;
  acc.s3 += rbf(diff * diff);
  const float e = ov - vv;
  const float e2 = e * e;
  // v_sqrt_f32 and v_rcp_f32 (1 ulp each) for the correctly rounded sqrt and two divisions, which at one
  // wave per SIMD on the fixed grid cost more than the memory traffic. r >= the smallest normal keeps both
  // reciprocals finite, so e == 0 gives 0 * rcp == 0 for every c > 0; an infinite e gives inf * 0 = NaN
  const float r = fmaxf(fmaxf(__builtin_amdgcn_sqrtf(e2 + cb * cb), cb), 1.17549435e-38f);
  const float kb = kind == 1 ? 2.0f * cb : 2.0f;
  const float l = (kb * e2) * __builtin_amdgcn_rcpf(r + cb);
  acc.s0 += wk * l;
  acc.s4 += l;
  return (wk * ((kb * e) * __builtin_amdgcn_rcpf(r))) * gsn;
}

template <bool VEC>
__global__ __launch_bounds__(256) void robust_loss_kernel(const bf16_t* __restrict__ o, const bf16_t* __restrict__ v,
                                                          const float* __restrict__ wt, const float* __restrict__ cs,
                                                          bf16_t* __restrict__ dout, float* __restrict__ stats,
                                                          int64_t n, int64_t C, int64_t per_sample, int kind,
                                                          float gsn) {
  RobustSums acc;
  const int64_t n8 = n / 8;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const u32x4 ow = *(const u32x4*)(o + 8 * i), vw = *(const u32x4*)(v + 8 * i);
    float wv = 1.0f, cv = 0.f;
    if (VEC) {
      if (wt) wv = wt[8 * i / C];
      cv = cs[8 * i / per_sample];
    }
    u32x4 dw;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      float d2[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float ov = bf2f((bf16_t)(ow[h] >> (16 * e))), vv = bf2f((bf16_t)(vw[h] >> (16 * e)));
        const int64_t idx = 8 * i + 2 * h + e;
        const float wk = VEC ? wv : (wt ? wt[idx / C] : 1.0f);
        const float cb = VEC ? cv : cs[idx / per_sample];
        d2[e] = robust_elem(ov, vv, wk, cb, kind, gsn, acc);
      }
      dw[h] = pack2(d2[0], d2[1]);
    }
    if (dout) *(u32x4*)(dout + 8 * i) = dw;
  }
  for (int64_t i = 8 * n8 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = robust_elem(bf2f(o[i]), bf2f(v[i]), wt ? wt[i / C] : 1.0f, cs[i / per_sample], kind, gsn, acc);
    if (dout) dout[i] = f2bf(d);
  }
  const float s[5] = {wave_sum(acc.s0), wave_sum(acc.s1), wave_sum(acc.s2), wave_sum(acc.s3), wave_sum(acc.s4)};
  __shared__ float red[5][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 5; ++c) red[c][w] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const int c = threadIdx.x;
    stats[8 + c * ROBUST_BLOCKS + blockIdx.x] = red[c][0] + red[c][1] + red[c][2] + red[c][3];
  }
}

// mse_finish_kernel's fixed-order sum of the per-block partials, over five sums: wave w takes sums w, w + 4
__global__ __launch_bounds__(256) void robust_loss_finish_kernel(float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  for (int c = threadIdx.x >> 6; c < 5; c += 4) {
    float s = 0.f;
    for (int b = lane; b < ROBUST_BLOCKS; b += 64) s += stats[8 + c * ROBUST_BLOCKS + b];
    s = wave_sum(s);
    if (lane == 0) stats[c] = s;
  }
}

}  // namespace ltx

using namespace ltx;

extern "C" {

int ltx_loss_token_weights(const float* bbox, const float* frame_w, const float* sample_w, const float* user_w,
                           float face_weight, float face_pad, float* wt, float* raw_sum, int64_t B, int64_t F,
                           int64_t H, int64_t W, void* stream) {
  LTX_CHECK_ARG(wt && raw_sum && B > 0 && F > 0 && H > 0 && W > 0, "loss_token_weights: bad args");
  // one workgroup per sample; F * H * W stays far inside int64, and (float)(w + 1) exact
  LTX_CHECK_ARG(B <= 0x7fffffff && F <= (1 << 20) && H <= (1 << 20) && W <= (1 << 20),
                "loss_token_weights: shape out of range");
  LTX_CHECK_ARG(face_weight > 0.f && face_pad >= 0.f, "loss_token_weights: face_weight must be > 0, face_pad >= 0");
  hipLaunchKernelGGL(loss_token_weights_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, bbox, frame_w,
                     sample_w, user_w, face_weight, face_pad, wt, raw_sum, F, H, W);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_wmse_fwd_bwd(const void* out, const void* v, const float* wt, void* dout, float* stats, int64_t rows,
                     int64_t C, float grad_scale, void* stream) {
  LTX_CHECK_ARG(out && v && wt && stats && rows > 0 && C > 0, "wmse: bad args");
  LTX_CHECK_ARG(rows <= ((int64_t)1 << 62) / C, "wmse: rows * C out of range");
  LTX_CHECK_ARG(((uintptr_t)out | (uintptr_t)v | (uintptr_t)dout) % 16 == 0, "wmse: operands must be 16-B aligned");
  const int64_t n = rows * C;
  const float norm = (float)(2.0 / (double)n);
  hipStream_t s = (hipStream_t)stream;
  if (C % 8 == 0)
    hipLaunchKernelGGL(wmse_kernel<true>, dim3(WMSE_BLOCKS), dim3(256), 0, s, (const bf16_t*)out, (const bf16_t*)v, wt,
                       (bf16_t*)dout, stats, n, C, norm, grad_scale);
  else
    hipLaunchKernelGGL(wmse_kernel<false>, dim3(WMSE_BLOCKS), dim3(256), 0, s, (const bf16_t*)out, (const bf16_t*)v,
                       wt, (bf16_t*)dout, stats, n, C, norm, grad_scale);
  hipLaunchKernelGGL(wmse_finish_kernel, dim3(1), dim3(256), 0, s, stats);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_robust_loss_fwd_bwd(const void* out, const void* v, const float* wt, const float* c, int kind, void* dout,
                            float* stats, int64_t B, int64_t rows_per_sample, int64_t C, float grad_scale,
                            void* stream) {
  LTX_CHECK_ARG(out && v && c && stats, "robust_loss: out, v, c and stats must not be null");
  LTX_CHECK_ARG(kind == LTX_ROBUST_HUBER || kind == LTX_ROBUST_SMOOTH_L1,
                "robust_loss: kind must be 1 (huber) or 2 (smooth_l1)");
  LTX_CHECK_ARG(B > 0 && rows_per_sample > 0 && C > 0, "robust_loss: B, rows_per_sample and C must be positive");
  LTX_CHECK_ARG(rows_per_sample <= ((int64_t)1 << 62) / C && B <= ((int64_t)1 << 62) / (rows_per_sample * C),
                "robust_loss: B * rows_per_sample * C out of range");
  LTX_CHECK_ARG(((uintptr_t)out | (uintptr_t)v | (uintptr_t)dout) % 16 == 0,
                "robust_loss: operands must be 16-B aligned");
  const int64_t per_sample = rows_per_sample * C, n = B * per_sample;
  const float gsn = (float)((double)grad_scale / (double)n);
  hipStream_t s = (hipStream_t)stream;
  if (C % 8 == 0)
    hipLaunchKernelGGL(robust_loss_kernel<true>, dim3(ROBUST_BLOCKS), dim3(256), 0, s, (const bf16_t*)out,
                       (const bf16_t*)v, wt, c, (bf16_t*)dout, stats, n, C, per_sample, kind, gsn);
  else
    hipLaunchKernelGGL(robust_loss_kernel<false>, dim3(ROBUST_BLOCKS), dim3(256), 0, s, (const bf16_t*)out,
                       (const bf16_t*)v, wt, c, (bf16_t*)dout, stats, n, C, per_sample, kind, gsn);
  hipLaunchKernelGGL(robust_loss_finish_kernel, dim3(1), dim3(256), 0, s, stats);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

}  // extern "C"
