// DoRA (peft use_dora, weight-decomposed LoRA; DESIGN.md "DoRA (use_dora)"): the device code behind
//   y = c (.) (x W^T + s (x A^T) B^T) + b,   c_j = m_j / ||W[j,:] + s (B A)[j,:]||_2   (norm detached)
// with the column scale folded into the GEMM operands, so every forward / dgrad GEMM stays the kernel
// it is for plain LoRA:
//   * dora_fold_kernel: per output row the norm of V = W + s B A (f32, never stored), c, the effective
//     base weight W_eff = bf16(c W) and the effective up-projection c (.) s B (f32), once per adapter
//     and weight version;
//   * dora_mag_grad_kernel + dora_mag_finish_kernel: the magnitude gradient
//     dm_j = (1 / m_j) sum_rows dY (Y - b), a two-level deterministic column reduction;
//   * dora_rowscale_add_kernel: dB[j,:] += alpha c_j scratch[j,:], the row scale of the plain dB
//     kernels' result.
// f32 throughout, fixed summation orders, no atomics.
#include "common.h"
#include "lora_plan.h"
#include "ltx_hip.h"

namespace ltx {

__device__ __forceinline__ void dora_ld8(const bf16_t* p, float* v) {
  const u32x4 w = *(const u32x4*)p;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = bf2f((bf16_t)(w[j >> 1] >> ((j & 1) * 16)));
}

// A workgroup owns DF_ROWS output rows for the whole K, so a column chunk of A (r x 8 floats per lane)
// is read once for the DF_ROWS rows. Pass 1 forms V = W + sum_j sB[row, j] A[j, :] eight columns per
// lane (the j sum an fma chain in j order) and adds V^2 into the lane's row sums (chunk order); the row
// sums meet by a wave butterfly and, over the four waves, in wave order. Pass 2 re-reads W (L2-hot:
// DF_ROWS x K bf16) and writes bf16(c W).
constexpr int DF_ROWS = 8, DF_THREADS = 256, DF_MAXR = 128;

__global__ __launch_bounds__(DF_THREADS) void dora_fold_kernel(
    const bf16_t* __restrict__ W, int64_t ldw, const float* __restrict__ A, int64_t lda,
    const float* __restrict__ B, int64_t brs, int64_t bcs, const float* __restrict__ mag, float s, int N, int K,
    int r, float* __restrict__ norm, float* __restrict__ cvec, bf16_t* __restrict__ weff, int64_t ldo,
    float* __restrict__ sbeff) {
  __shared__ float sB[DF_ROWS][DF_MAXR];
  __shared__ float red[DF_THREADS / 64][DF_ROWS];
  __shared__ float cs[DF_ROWS];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * DF_ROWS;
  for (int i = tid; i < DF_ROWS * r; i += DF_THREADS) {
    const int rr = i / r, j = i % r;
    const int row = row0 + rr;
    sB[rr][j] = row < N ? s * B[(int64_t)row * brs + (int64_t)j * bcs] : 0.f;
  }
  __syncthreads();
  float ss[DF_ROWS];
#pragma unroll
  for (int rr = 0; rr < DF_ROWS; ++rr) ss[rr] = 0.f;
  for (int k = tid * 8; k < K; k += DF_THREADS * 8) {
    float acc[DF_ROWS][8];
#pragma unroll
    for (int rr = 0; rr < DF_ROWS; ++rr) {
      if (row0 + rr < N) {
        dora_ld8(W + (int64_t)(row0 + rr) * ldw + k, acc[rr]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[rr][e] = 0.f;
      }
    }
    // the adapter term: up[rr][e] = sum_j sB[rr][j] A[j][k + e], then V = W + up
    float up[DF_ROWS][8];
#pragma unroll
    for (int rr = 0; rr < DF_ROWS; ++rr)
#pragma unroll
      for (int e = 0; e < 8; ++e) up[rr][e] = 0.f;
    for (int j = 0; j < r; ++j) {
      const f32x4 a0 = *(const f32x4*)(A + (int64_t)j * lda + k);
      const f32x4 a1 = *(const f32x4*)(A + (int64_t)j * lda + k + 4);
#pragma unroll
      for (int rr = 0; rr < DF_ROWS; ++rr) {
        const float b = sB[rr][j];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          up[rr][e] = __builtin_fmaf(b, a0[e], up[rr][e]);
          up[rr][e + 4] = __builtin_fmaf(b, a1[e], up[rr][e + 4]);
        }
      }
    }
#pragma unroll
    for (int rr = 0; rr < DF_ROWS; ++rr)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = acc[rr][e] + up[rr][e];
        ss[rr] = __builtin_fmaf(v, v, ss[rr]);
      }
  }
#pragma unroll
  for (int rr = 0; rr < DF_ROWS; ++rr) {
    const float t = wave_sum(ss[rr]);
    if ((tid & 63) == 0) red[tid >> 6][rr] = t;
  }
  __syncthreads();
  if (tid < DF_ROWS) {
    const int row = row0 + tid;
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < DF_THREADS / 64; ++w) t += red[w][tid];
    const float nv = sqrtf(t);
    const float c = (row < N && nv != 0.f) ? mag[row] / nv : 0.f;
    cs[tid] = c;
    if (row < N) {
      norm[row] = nv;
      cvec[row] = c;
    }
  }
  __syncthreads();
  for (int i = tid; i < DF_ROWS * r; i += DF_THREADS) {
    const int rr = i / r, j = i % r;
    if (row0 + rr < N) sbeff[(int64_t)(row0 + rr) * r + j] = cs[rr] * sB[rr][j];
  }
  for (int k = tid * 8; k < K; k += DF_THREADS * 8) {
#pragma unroll
    for (int rr = 0; rr < DF_ROWS; ++rr) {
      if (row0 + rr >= N) continue;
      float w[8];
      dora_ld8(W + (int64_t)(row0 + rr) * ldw + k, w);
      const float c = cs[rr];
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack2(c * w[2 * e], c * w[2 * e + 1]);
      *(u32x4*)(weff + (int64_t)(row0 + rr) * ldo + k) = o;
    }
  }
}

// part[split][n] = sum over the split's rows of f32(dY[m,n]) * (f32(Y[m,n]) - f32(b[n])). A workgroup
// owns 256 columns (32 lanes x 8) of one row split; its 8 row lanes (tid / 32) take every 8th row and
// meet in LDS in lane order.
constexpr int MG_COLS = 256, MG_RLANES = 8, MG_UNROLL = 4;

__global__ __launch_bounds__(256) void dora_mag_grad_kernel(const bf16_t* __restrict__ dY, int64_t lddy,
                                                            const bf16_t* __restrict__ Y, int64_t ldy,
                                                            const bf16_t* __restrict__ bias, int64_t M, int N, int S,
                                                            float* __restrict__ part) {
  __shared__ float red[MG_RLANES][MG_COLS];
  const int cl = threadIdx.x % 32, rl = threadIdx.x / 32;
  const int c0 = blockIdx.x * MG_COLS + cl * 8;
  const int split = blockIdx.y;
  const int64_t r0 = (int64_t)split * M / S, r1 = (int64_t)(split + 1) * M / S;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < N) {
    float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (bias) dora_ld8(bias + c0, bv);
    // four of the lane's rows per iteration: their eight 16-byte loads are issued before the first
    // product (the rows are still added in row order)
    int64_t m = r0 + rl;
    for (; m + (MG_UNROLL - 1) * MG_RLANES < r1; m += MG_UNROLL * MG_RLANES) {
      u32x4 gw[MG_UNROLL], yw[MG_UNROLL];
#pragma unroll
      for (int i = 0; i < MG_UNROLL; ++i) {
        gw[i] = *(const u32x4*)(dY + (m + i * MG_RLANES) * lddy + c0);
        yw[i] = *(const u32x4*)(Y + (m + i * MG_RLANES) * ldy + c0);
      }
#pragma unroll
      for (int i = 0; i < MG_UNROLL; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float g = bf2f((bf16_t)(gw[i][e >> 1] >> ((e & 1) * 16)));
          const float y = bf2f((bf16_t)(yw[i][e >> 1] >> ((e & 1) * 16)));
          acc[e] = __builtin_fmaf(g, y - bv[e], acc[e]);
        }
    }
    for (; m < r1; m += MG_RLANES) {
      float g[8], y[8];
      dora_ld8(dY + m * lddy + c0, g);
      dora_ld8(Y + m * ldy + c0, y);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(g[e], y[e] - bv[e], acc[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][cl * 8 + e] = acc[e];
  __syncthreads();
  const int n = blockIdx.x * MG_COLS + threadIdx.x;
  if (n < N) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < MG_RLANES; ++j) t += red[j][threadIdx.x];
    part[(int64_t)split * N + n] = t;
  }
}

// dm[n] (+)= m[n] != 0 ? (1 / m[n]) * sum_s part[s][n] : 0. A workgroup owns 16 columns: its 16 rows of
// 16 lanes (tid / 16) each sum every 16th split in order, the 16 sums meet in LDS in lane order.
constexpr int MF_COLS = 16, MF_LANES = 16;
__global__ __launch_bounds__(256) void dora_mag_finish_kernel(const float* __restrict__ part, int S, int N,
                                                              const float* __restrict__ mag, int accumulate,
                                                              float* __restrict__ out) {
  __shared__ float red[MF_LANES][MF_COLS];
  const int cl = threadIdx.x % MF_COLS, ls = threadIdx.x / MF_COLS;
  const int n = blockIdx.x * MF_COLS + cl;
  float t = 0.f;
  if (n < N)
    for (int s = ls; s < S; s += MF_LANES) t += part[(int64_t)s * N + n];
  red[ls][cl] = t;
  __syncthreads();
  if (ls != 0 || n >= N) return;
  float tot = 0.f;
#pragma unroll
  for (int j = 0; j < MF_LANES; ++j) tot += red[j][cl];
  const float mv = mag[n];
  const float v = mv != 0.f ? (1.0f / mv) * tot : 0.f;
  out[n] = accumulate ? out[n] + v : v;
}

// out[j*on + i*oj] += (alpha * c[j]) * src[j*r + i]
__global__ __launch_bounds__(256) void dora_rowscale_add_kernel(const float* __restrict__ src,
                                                                const float* __restrict__ c, float alpha, int64_t n,
                                                                int r, float* __restrict__ out, int64_t on,
                                                                int64_t oj) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n) return;
  const int64_t j = i / r, q = i % r;
  float* o = out + j * on + q * oj;
  *o = *o + (alpha * c[j]) * src[i];
}

}  // namespace ltx

using namespace ltx;

extern "C" {

int ltx_dora_fold(const void* W, int64_t ldw, const float* A, int64_t lda, const float* B, int64_t brs, int64_t bcs,
                  const float* m, float s, int64_t N, int64_t K, int64_t r, float* norm, float* c, void* w_eff,
                  int64_t ldo, float* sb_eff, void* stream) {
  LTX_CHECK_ARG(W && A && B && m && norm && c && w_eff && sb_eff && N > 0 && K > 0, "dora_fold: bad args");
  LTX_CHECK_ARG(lora_rank_ok(r), "dora_fold: rank must be " LTX_LORA_RANK_TEXT);
  LTX_CHECK_ARG(K % 8 == 0 && ldw % 8 == 0 && ldo % 8 == 0 && lda % 4 == 0 && ldw >= K && ldo >= K && lda >= K,
                "dora_fold: K and the bf16 strides must be %8, lda %4, every stride >= K");
  LTX_CHECK_ARG(((uintptr_t)W | (uintptr_t)w_eff | (uintptr_t)A) % 16 == 0, "dora_fold: operands must be 16-B aligned");
  LTX_CHECK_ARG(N < (1 << 30) && K < (1 << 30), "dora_fold: shape too large");
  const dim3 grid((unsigned)((N + DF_ROWS - 1) / DF_ROWS));
  hipLaunchKernelGGL(dora_fold_kernel, grid, dim3(DF_THREADS), 0, (hipStream_t)stream, (const bf16_t*)W, ldw, A, lda,
                     B, brs, bcs, m, s, (int)N, (int)K, (int)r, norm, c, (bf16_t*)w_eff, ldo, sb_eff);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_dora_mag_grad_workspace(int64_t M, int64_t N, int64_t* splits, int64_t* floats) {
  LTX_CHECK_ARG(M > 0 && N > 0 && splits && floats, "dora_mag_grad_workspace: bad args");
  // 64 rows per split (8 per row lane), at most 256 splits: 224 x 8 workgroups at M = 14336, N = 2048
  int64_t S = (M + 63) / 64;
  if (S > 256) S = 256;
  *splits = S;
  *floats = S * N;
  return LTX_OK;
}

int ltx_dora_mag_grad(const void* dY, int64_t lddy, const void* Y, int64_t ldy, const void* bias, const float* m,
                      int64_t M, int64_t N, float* out, int accumulate, float* workspace, void* stream) {
  LTX_CHECK_ARG(dY && Y && m && out && workspace && M > 0 && N > 0, "dora_mag_grad: bad args");
  LTX_CHECK_ARG(N % 8 == 0 && lddy % 8 == 0 && ldy % 8 == 0 && lddy >= N && ldy >= N,
                "dora_mag_grad: N and the strides must be %8, strides >= N");
  LTX_CHECK_ARG(((uintptr_t)dY | (uintptr_t)Y | (uintptr_t)bias) % 16 == 0, "dora_mag_grad: operands must be 16-B aligned");
  LTX_CHECK_ARG(N < (1 << 30), "dora_mag_grad: N too large");
  int64_t S = 0, fl = 0;
  ltx_dora_mag_grad_workspace(M, N, &S, &fl);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + MG_COLS - 1) / MG_COLS), (unsigned)S);
  hipLaunchKernelGGL(dora_mag_grad_kernel, grid, dim3(256), 0, st, (const bf16_t*)dY, lddy, (const bf16_t*)Y, ldy,
                     (const bf16_t*)bias, M, (int)N, (int)S, workspace);
  LTX_LAUNCH_CHECK();
  hipLaunchKernelGGL(dora_mag_finish_kernel, dim3((unsigned)((N + MF_COLS - 1) / MF_COLS)), dim3(256), 0, st, workspace, (int)S,
                     (int)N, m, accumulate, out);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_dora_rowscale_add(const float* src, const float* c, float alpha, int64_t N, int64_t r, float* out, int64_t on,
                          int64_t oj, void* stream) {
  LTX_CHECK_ARG(src && c && out && N > 0 && r > 0, "dora_rowscale_add: bad args");
  const int64_t n = N * r;
  hipLaunchKernelGGL(dora_rowscale_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     src, c, alpha, n, (int)r, out, on, oj);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

}  // extern "C"
