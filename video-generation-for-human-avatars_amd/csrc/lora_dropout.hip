// LoRA dropout (peft lora_dropout): the counter-based keep mask and the two kernels that use it.
// The mask of adapter stream sid under the 64-bit key is a pure function of (row, column), so the
// forward, a checkpoint recompute and the backward regenerate it instead of storing it:
// Philox4x32-10, counter (m, k / 8, sid, 0), key (key lo, key hi); one call covers 8 columns as eight
// 16-bit lanes, element k kept iff its lane >= T (ltx_hip.h, DESIGN.md "LoRA dropout").
//   ltx_lora_dropout_apply   xd = keep ? x : 0, the bf16 operand every adapter kernel then consumes
//   ltx_lora_up_masked_add   dx += g * c * sum_g keep_g * (w_g . A_g), the adapter's input-gradient
//                            term that cannot ride the dgrad GEMM's K extension under a mask
#include "common.h"
#include "lora_plan.h"
#include "ltx_hip.h"
#include "philox.h"

namespace ltx {

// one 16-B vector (8 columns) per thread and step, grid-stride over the M * K / 8 vectors
__global__ __launch_bounds__(256) void lora_dropout_apply_kernel(const bf16_t* __restrict__ x, int64_t ldx,
                                                                 bf16_t* __restrict__ out, int64_t ldo, int M, int K8,
                                                                 uint32_t k0, uint32_t k1, uint32_t sid, uint32_t T) {
  const int64_t total = (int64_t)M * K8;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t m = (uint32_t)(i / K8), kg = (uint32_t)(i % K8);
    u32x4 v = *(const u32x4*)(x + (int64_t)m * ldx + (int64_t)kg * 8);
    const Philox4 o = philox4x32_10(m, kg, sid, 0u, k0, k1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t lo = o.v[q] & 0xffffu, hi = o.v[q] >> 16;
      v[q] &= (lo >= T ? 0x0000ffffu : 0u) | (hi >= T ? 0xffff0000u : 0u);
    }
    *(u32x4*)(out + (int64_t)m * ldo + (int64_t)kg * 8) = v;
  }
}

struct MaskedAddGroups {
  const float* A[3];
  uint32_t sid[3];
};

// Block = 4 waves on 64 rows x 128 columns, one 16 x 128 tile per wave on v_mfma_f32_16x16x4_f32
// (an exact f32 fma chain): per 4 ranks a lane loads w[m0 + (lane & 15)][j0 + (lane >> 4)] and the 8
// consecutive columns k0 + 8 (lane & 15) .. of A's row j0 + (lane >> 4) (two 16-B loads), and MFMA t
// (t = 0..7) takes element t, so its output column c stands for k0 + 8c + t. A lane then holds rows
// m0 + 4 (lane >> 4) + rr (rr = 0..3) x the 8 consecutive columns of its column group: one Philox
// call, one 16-B load and one 16-B store of dx per row. A (r x K f32 per adapter) is read by every
// row tile and stays in L2.
template <int R>
__global__ __launch_bounds__(256) void lora_up_masked_add_kernel(bf16_t* __restrict__ dx, int64_t lddx,
                                                                 const float* __restrict__ w, int64_t ldw,
                                                                 MaskedAddGroups gr, int64_t lda, int G, int M, int K,
                                                                 uint32_t k0, uint32_t k1, uint32_t T, float c,
                                                                 const int16_t* __restrict__ gq, int64_t ldg) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.y * 64 + wave * 16;
  if (m0 >= M) return;  // wave-uniform
  const int c8 = blockIdx.x * 128 + 8 * (lane & 15);  // this lane's 8 columns
  const bool colok = c8 < K;                          // K % 8 == 0: all 8 in or all out
  const int jq = lane >> 4;
  const int mw = m0 + (lane & 15);  // the row whose w this lane feeds
  const bool wok = mw < M;
  // this lane's four rows of dx (and of the GELU factor). From rank 32 on they are loaded ahead of
  // the products (measured at config A: 219 vs 273 us at r = 32 with the GELU factor, 2 - 3 % without);
  // at r <= 16 after them (35.5 vs 41 us at r = 16, G = 1: profiles/lora_dropout_bench.md)
  constexpr bool EARLY = R >= 32;
  u32x4 dv[4], qv[4];
  auto load_rows = [&]() {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int m = m0 + 4 * jq + rr;
      dv[rr] = qv[rr] = (u32x4){0, 0, 0, 0};
      if (colok && m < M) {
        dv[rr] = *(const u32x4*)(dx + (int64_t)m * lddx + c8);
        if (gq != nullptr) qv[rr] = *(const u32x4*)(gq + (int64_t)m * ldg + c8);
      }
    }
  };
  if constexpr (EARLY) load_rows();
  float tot[4][8];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int t = 0; t < 8; ++t) tot[rr][t] = 0.f;
  for (int g = 0; g < G; ++g) {
    const float* __restrict__ Ag = g == 0 ? gr.A[0] : (g == 1 ? gr.A[1] : gr.A[2]);
    const uint32_t sid = g == 0 ? gr.sid[0] : (g == 1 ? gr.sid[1] : gr.sid[2]);
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* wp = w + (int64_t)(wok ? mw : 0) * ldw + g * R + jq;
    const float* ap = Ag + (int64_t)jq * lda + (colok ? c8 : 0);
#pragma unroll 4
    for (int j0 = 0; j0 < R; j0 += 4) {
      const float wv = wok ? wp[j0] : 0.f;
      f32x4 a0 = (f32x4){0.f, 0.f, 0.f, 0.f}, a1 = a0;
      if (colok) {
        a0 = *(const f32x4*)(ap + (int64_t)j0 * lda);
        a1 = *(const f32x4*)(ap + (int64_t)j0 * lda + 4);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, a0[t], acc[t], 0, 0, 0);
        acc[4 + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, a1[t], acc[4 + t], 0, 0, 0);
      }
    }
    // C layout: col = lane & 15 (the column group), row = 4 (lane >> 4) + rr
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const uint32_t m = (uint32_t)(m0 + 4 * jq + rr);
      const Philox4 o = philox4x32_10(m, (uint32_t)(c8 >> 3), sid, 0u, k0, k1);
#pragma unroll
      for (int t = 0; t < 8; ++t) tot[rr][t] += mask_lane(o, t) >= T ? acc[t][rr] : 0.f;
    }
  }
  if constexpr (!EARLY) load_rows();
  if (!colok) return;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int m = m0 + 4 * jq + rr;
    if (m >= M) continue;
    bf16_t* p = dx + (int64_t)m * lddx + c8;
    const u32x4 d = dv[rr], q = qv[rr];
    u32x4 o;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      float t0 = tot[rr][2 * h] * c, t1 = tot[rr][2 * h + 1] * c;
      if (gq != nullptr) {
        t0 = (t0 * gelu_qlo(q[h])) * GELU_DQ;
        t1 = (t1 * gelu_qhi(q[h])) * GELU_DQ;
      }
      o[h] = pack2(bf2f((bf16_t)(d[h] & 0xffffu)) + t0, bf2f((bf16_t)(d[h] >> 16)) + t1);
    }
    *(u32x4*)p = o;
  }
}

}  // namespace ltx

using namespace ltx;

extern "C" int ltx_lora_dropout_apply(const void* x, int64_t ldx, void* out, int64_t ldo, int64_t M, int64_t K,
                                      uint64_t key, int64_t sid, int64_t T, void* stream) {
  LTX_CHECK_ARG(x && out && M > 0 && K > 0 && M < ((int64_t)1 << 31), "lora_dropout_apply: bad args");
  LTX_CHECK_ARG(K % 8 == 0 && ldx % 8 == 0 && ldo % 8 == 0 && ldx >= K && ldo >= K && ((uintptr_t)x % 16) == 0 &&
                    ((uintptr_t)out % 16) == 0,
                "lora_dropout_apply: K % 8, 16-B aligned rows");
  LTX_CHECK_ARG(T >= 1 && T <= 65535 && sid >= 0 && sid < ((int64_t)1 << 32),
                "lora_dropout_apply: T in [1, 65535], sid in [0, 2^32)");
  const int64_t total = M * (K / 8);
  int64_t g = (total + 255) / 256;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(lora_dropout_apply_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, ldx, (bf16_t*)out, ldo, (int)M, (int)(K / 8), (uint32_t)(key & 0xffffffffu),
                     (uint32_t)(key >> 32), (uint32_t)sid, (uint32_t)T);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

extern "C" int ltx_lora_up_masked_add(void* dx, int64_t lddx, const float* w, int64_t ldw, const float* const* A,
                                      int64_t lda, const int64_t* sids, int64_t groups, int64_t M, int64_t K,
                                      int64_t r, uint64_t key, int64_t T, float c, const void* gq, int64_t ldg,
                                      void* stream) {
  LTX_CHECK_ARG(dx && w && A && sids && M > 0 && K > 0 && M < ((int64_t)1 << 31) - 64 && K < ((int64_t)1 << 31) - 128,
                "lora_up_masked_add: bad args");
  LTX_CHECK_ARG(groups >= 1 && groups <= 3 && ldw >= groups * r, "lora_up_masked_add: 1..3 groups, w is [M, groups*r]");
  LTX_CHECK_ARG(K % 8 == 0 && lddx % 8 == 0 && lddx >= K && ((uintptr_t)dx % 16) == 0,
                "lora_up_masked_add: K % 8, 16-B aligned dx rows");
  LTX_CHECK_ARG(lda % 4 == 0 && lda >= K, "lora_up_masked_add: A rows must be 16-B aligned");
  LTX_CHECK_ARG(!gq || (ldg % 8 == 0 && ldg >= K && ((uintptr_t)gq % 16) == 0),
                "lora_up_masked_add: 16-B aligned g rows");
  LTX_CHECK_ARG(T >= 1 && T <= 65535, "lora_up_masked_add: T in [1, 65535]");
  MaskedAddGroups gr = {};
  for (int g = 0; g < groups; ++g) {
    LTX_CHECK_ARG(A[g] && ((uintptr_t)A[g] % 16) == 0 && sids[g] >= 0 && sids[g] < ((int64_t)1 << 32),
                  "lora_up_masked_add: A[g] 16-B aligned, sid in [0, 2^32)");
    gr.A[g] = A[g];
    gr.sid[g] = (uint32_t)sids[g];
  }
  const dim3 grid((unsigned)((K + 127) / 128), (unsigned)((M + 63) / 64));
  LTX_CHECK_ARG(grid.y <= 65535, "lora_up_masked_add: M <= 64 * 65535");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t k0 = (uint32_t)(key & 0xffffffffu), k1 = (uint32_t)(key >> 32);
  LTX_CHECK_ARG(lora_rank_ok(r), "lora_up_masked_add: rank must be " LTX_LORA_RANK_TEXT);
  with_rank(r, [&](auto rank) {
    hipLaunchKernelGGL(lora_up_masked_add_kernel<decltype(rank)::value>, grid, dim3(256), 0, s, (bf16_t*)dx, lddx, w, ldw,
                       gr, lda, (int)groups, (int)M, (int)K, k0, k1, (uint32_t)T, c, (const int16_t*)gq, ldg);
  });
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}
