// One pass over dY for a token-sized LoRA adapter's backward (peft's f32 lora_B, training.py:50-68):
//   w  = alpha * dY . B        [M, r]  (the input-gradient term, consumed as the dgrad GEMM's
//                                       K-extension after the hi / lo split)
//   dB (+)= alpha * dY^T . u   [N, r]  (u = x . A^T, saved by the forward)
// Until now these were two kernels that each streamed dY from HBM (ltx_lora_rows and
// ltx_lora_wgrad, ~18.5 us each at M = 14336, N = 2048); here one LDS-DMA stream of dY feeds both
// products on the bf16 matrix core, and a small second kernel finishes the sums.
//
// Block = 8 waves over 512 columns x G row groups of 32 rows x one rank slice of SW <= 32 adapter
// columns (grid: N / 512 column splits x r / SW rank slices in x, ceil(M / 32G) row splits in y;
// G = 7, SW = 16 up to r = 16; G = 4, SW = 32 from r = 32 on: see dy_g / dy_sw below). Wave w owns columns c0 = 512 bx + 64 w .. +64 and streams its 32 x 64
// slot of every row group (4 KiB, the attention tiles' chunk swizzle swz<64>) through a private
// 4-slot ring, so no barrier is needed in the loop. Per slot:
//   * w:  [32 rows x SW j] += slot . (B^T pieces)^T: 12 v_mfma_f32_16x16x32_bf16 per 16 j (2 row
//         halves x 2 k halves x 3 pieces), the slice's B^T pieces (ltx_lora_pieces) in registers for
//         the whole block;
//   * dB: [SW j x 64 cols] += (u pieces)^T . slot: 12 MFMAs per 16 j (4 column blocks x 3 pieces), the
//         slot read transposed (ds_read_b64_tr_b16, the attention dQ product's k-slot order), u
//         split into exact hi / mid / lo bf16 pieces from an LDS copy of the block's u rows.
// Exact bf16 products summed in f32, as ltx_lora_rows; the sums run in a different order than
// ltx_lora_rows / ltx_lora_wgrad (f32 rounding differences only).
// Partials (deterministic, no atomics): w over the 4 column splits [CS][RP][M], dB over the row
// splits [RS][N][RP] (a rank slice writes its own j range of both); lora_dy_finish_kernel sums them in a fixed order, applies alpha, writes w,
// its [hi | hi | lo | 0..] split operand, and adds dB into the gradient buffer.
//
// Grouped launches (ltx_lora_rows_grouped, ltx_lora_dy_dA_grouped): up to 4 adapters of one rank that
// share an input (the q / k / v adapters of a LoRA-wrapped self-attention) in one launch per kernel.
// The block programs live in lora_dy_bodies.h and are included into the one-adapter kernels and
// into their grouped twins, which only map a group's block index and operands: every output keeps
// the one-adapter kernel's summation order (bitwise the separate calls).
#include <cstdlib>

#include "attention_common.h"
#include "lora_plan.h"
#include "ltx_hip.h"

namespace ltx {

namespace {
constexpr int DY_NR = 4;  // ring slots per wave
// DY_COLS columns per block, DY_MAXCS column splits a MODE-6 pass sums its u from, dy_g / dy_nsl: lora_plan.h.
// A block works on one rank slice of DY_SW(r) <= 32 columns of the adapter: the whole rank up to
// r = 32, so dY is streamed from HBM once; ranks 64 / 128 run 2 / 4 slices per dY tile as
// consecutive blockIdx.x of the same launch, each streaming the tile again (at 6r FLOP/B those
// ranks sit at or past the matrix-core ridge, and the slice's B^T pieces (24 VGPRs per 16 columns),
// accumulators and the 8 waves' w partials keep the r = 32 budget). Row groups of 32 per block:
// 7 for 16-wide slices (14336 = 64 x 7 x 32), 4 for 32-wide ones -- the 8 waves' w partials,
// 8 . 32 . (32 G + 4) . 4 B, must fit the ring plus the u^T area they overlay (147,968 B at G = 4;
// G = 7 would need 236,544 B), and 4 divides config A's 448 row groups where 3 would not.
constexpr int dy_sw(int r) { return r <= 16 ? 16 : 32; }
}  // namespace

// MODE: bit 0 the w product, bit 1 the dB product. MODE 2 is ltx_lora_wgrad's token-sized path
// (dw = alpha . Y^T . u on the bf16 matrix core with u's exact three-piece split, where
// lora_wgrad_kernel runs f32 MFMAs); MODE 1 is ltx_lora_rows' (u = x . A^T from A's pieces).
// Bit 2 (with bit 1, round 6): u is not read but summed from another pass's column-split w partials
// part_u[c][j][m] (c < CSu, in c order) times alpha_u -- bitwise the w lora_dy_finish_kernel writes
// from them -- so the dA pass of an adapter (dA = w^T . x) need not wait for that finish launch.
// Bit 3 (with bits 2 and 1, MODE 14): the same from any number of partials (N > 2048, the feed-forward's
// d_f [M, 8192]): a loop over groups of DY_MAXCS partials, one running sum in c order.
template <int R, int MODE>
__global__ __launch_bounds__(512) void lora_dy_kernel(const bf16_t* __restrict__ y, int64_t ldy,
                                                      const float* __restrict__ u, int64_t ldu,
                                                      const bf16_t* __restrict__ w3, int64_t ldw,
                                                      float* __restrict__ part_w, float* __restrict__ part_b,
                                                      int M, int N, const float* __restrict__ part_u, int CSu,
                                                      float alpha_u) {
#define DY_BX blockIdx.x
#define DY_BY blockIdx.y
#define LTX_DY_BODY 1
#include "lora_dy_bodies.h"
#undef LTX_DY_BODY
#undef DY_BX
#undef DY_BY
}

// Per-group operands of the grouped launches (kernel arguments by value; G <= LORA_MAX_GROUPS)
struct DyGroupPtrs {
  const float* u[LORA_MAX_GROUPS];
  const bf16_t* w3[LORA_MAX_GROUPS];
  float* dw[LORA_MAX_GROUPS];
  float* dwa[LORA_MAX_GROUPS];
};

// lora_dy_kernel for G adapters on the column blocks of one packed dY [M, G N] (the fused QKV
// gradient) that share the input x. Every group runs the one-adapter block program on its own
// operands, so each output is bitwise the one-adapter launch's.
// MODE 3 (the dY pass): group = blockIdx.z; dY columns from g*gy, the partials of group g at
// part_w + g*gpw / part_b + g*gpb.
// MODE 6 (the x pass): the G * NSL (group, rank slice) pairs of one 512-column tile of x are
// consecutive blockIdx.x, so the tile is fetched from HBM once and serves all G r columns of w
// (the later slices hit L2 / MALL, as the rank slices of one adapter do); w of group g is summed
// from part_u + g*gpu, its dA partials go to part_b + g*gpb.
template <int R, int MODE>
__global__ __launch_bounds__(512) void lora_dy_grouped_kernel(const bf16_t* __restrict__ y0, int64_t ldy,
                                                              DyGroupPtrs gp, int64_t ldu, int64_t ldw,
                                                              float* __restrict__ part_w0,
                                                              float* __restrict__ part_b0, int M, int N,
                                                              const float* __restrict__ part_u0, int CSu,
                                                              float alpha_u, int G, int64_t gy, int64_t gpw,
                                                              int64_t gpb, int64_t gpu) {
  unsigned g, gbx;
  if constexpr ((MODE & 4) != 0) {
    constexpr unsigned NSLG = dy_nsl(R);
    g = (blockIdx.x / NSLG) % (unsigned)G;
    gbx = (blockIdx.x / (NSLG * (unsigned)G)) * NSLG + blockIdx.x % NSLG;
  } else {
    g = blockIdx.z;
    gbx = blockIdx.x;
  }
  const bf16_t* __restrict__ y = y0 + g * gy;
  const float* __restrict__ u = (MODE & 4) ? nullptr : gp.u[g];
  const bf16_t* __restrict__ w3 = (MODE & 1) ? gp.w3[g] : nullptr;
  float* __restrict__ part_w = (MODE & 1) ? part_w0 + g * gpw : nullptr;
  float* __restrict__ part_b = part_b0 + g * gpb;
  const float* __restrict__ part_u = (MODE & 4) ? part_u0 + g * gpu : nullptr;
#define DY_BX gbx
#define DY_BY blockIdx.y
#define LTX_DY_BODY 1
#include "lora_dy_bodies.h"
#undef LTX_DY_BODY
#undef DY_BX
#undef DY_BY
}

// Blocks [0, nwb): w[m,j] = alpha * sum_c part_w[c][m][j] and the [hi | hi | lo | 0..] split row,
// one thread per split element. Blocks [nwb, ..): dw[n*on + j*oj] (+)= alpha * sum_s part_b[s][n][j]
// for 64 (n, j) pairs per block, the row splits dealt to 4 thread groups (strided, independent
// loads in flight) and the 4 group sums added in a fixed order (deterministic).
// Blocks [nwb + nbb, ..) (round 6): a second row-split sum of the same kind, dwa (+)= alpha_a *
// sum_s part_a[s][n][j] over Na columns (the adapter's dA from the pass that ran after its dY pass).
template <int R>
__device__ __forceinline__ void finish_rows(const float* __restrict__ part, int RS, int N, float alpha,
                                            float* __restrict__ dw, int64_t on, int64_t oj, int accumulate, int blk,
                                            float (*red)[64]) {
  constexpr int RP = R >= 16 ? R : 16;
  const int pr = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t e = (int64_t)blk * 64 + pr;  // pair (n, j), j fastest
  const bool ok = e < (int64_t)N * R;
  const int n = ok ? (int)(e / R) : 0, j = ok ? (int)(e % R) : 0;
  float sum = 0.f;
#pragma unroll 8
  for (int s = grp; s < RS; s += 4) sum += part[((int64_t)s * N + n) * RP + j];
  red[grp][pr] = sum;
  __syncthreads();
  if (grp == 0 && ok) {
    const float v = (((red[0][pr] + red[1][pr]) + red[2][pr]) + red[3][pr]) * alpha;
    float* o = dw + (int64_t)n * on + (int64_t)j * oj;
    *o = accumulate ? *o + v : v;
  }
}

template <int R>
__global__ __launch_bounds__(256) void lora_dy_finish_kernel(const float* __restrict__ part_w, int CS,
                                                             const float* __restrict__ part_b, int RS, int M, int N,
                                                             float alpha, float* __restrict__ w, int64_t ldw_out,
                                                             bf16_t* __restrict__ split, int64_t lds, int K2,
                                                             float* __restrict__ dw, int64_t on, int64_t oj,
                                                             int accumulate, int nwb, int nbb,
                                                             const float* __restrict__ part_a, int Na, float alpha_a,
                                                             float* __restrict__ dwa, int64_t ona, int64_t oja,
                                                             int acc_a) {
#define DY_BX blockIdx.x
#define DY_BY blockIdx.y
#define LTX_DY_BODY 2
#include "lora_dy_bodies.h"
#undef LTX_DY_BODY
#undef DY_BX
#undef DY_BY
}

// the finish of G adapters in one launch: group = blockIdx.y, its partials at g*gpw / g*gpb / g*gpa,
// its w and split columns at g*gwo / g*gso of the shared [M, .] outputs, its dB / dA from gp
template <int R>
__global__ __launch_bounds__(256) void lora_dy_finish_grouped_kernel(
    const float* __restrict__ part_w0, int CS, const float* __restrict__ part_b0, int RS, int M, int N, float alpha,
    float* __restrict__ w0, int64_t ldw_out, bf16_t* __restrict__ split0, int64_t lds, int K2, DyGroupPtrs gp,
    int64_t on, int64_t oj, int accumulate, int nwb, int nbb, const float* __restrict__ part_a0, int Na,
    float alpha_a, int64_t ona, int64_t oja, int acc_a, int64_t gpw, int64_t gpb, int64_t gpa, int64_t gwo,
    int64_t gso) {
  const unsigned g = blockIdx.y;
  const float* __restrict__ part_w = part_w0 + g * gpw;
  const float* __restrict__ part_b = part_b0 + g * gpb;
  const float* __restrict__ part_a = part_a0 + g * gpa;
  float* __restrict__ w = w0 + g * gwo;
  bf16_t* __restrict__ split = split0 + g * gso;
  float* __restrict__ dw = gp.dw[g];
  float* __restrict__ dwa = gp.dwa[g];
#define DY_BX blockIdx.x
#define DY_BY blockIdx.y
#define LTX_DY_BODY 2
#include "lora_dy_bodies.h"
#undef LTX_DY_BODY
#undef DY_BX
#undef DY_BY
}

// u = alpha * x . A^T for token-sized M with the whole contraction inside one block (round 6):
// block = 8 waves on RG row groups of 32 rows, wave w owns the K / 8 = 64 CH contiguous columns
// from 64 CH w, so the block's rows are complete after its cross-wave sum and u and the split
// operand leave the kernel directly (the column-split MODE 1 pass needed lora_dy_finish_kernel
// for the 4 column partials: one more launch and 3.7 MB of partials per call). The wave's A^T
// pieces (3 x 16 j x 64 CH columns) stay in registers for its RG x CH slots, which stream through
// the same private 4-slot LDS-DMA ring as lora_dy_kernel (slot = 32 rows x 64 columns, order
// (group, chunk)). Same exact bf16 products summed in f32; the sum order is per-slot MFMA
// accumulation, then the 8 wave partials in wave order.
template <int R, int RG, int CH, int NR>
__global__ __launch_bounds__(512) void lora_rows_full_kernel(const bf16_t* __restrict__ x, int64_t ldx,
                                                             const bf16_t* __restrict__ w3, int64_t ldw,
                                                             float* __restrict__ out, int64_t ldo, int M, float alpha,
                                                             bf16_t* __restrict__ split, int64_t lds, int K2) {
#define DY_BX blockIdx.x
#define DY_BY blockIdx.y
#define LTX_DY_BODY 3
#include "lora_dy_bodies.h"
#undef LTX_DY_BODY
#undef DY_BX
#undef DY_BY
}

// lora_rows_full_kernel for G adapters that share x (the q / k / v adapters on the modulated norm
// output): blockIdx.y = (group, rank slice), so a row tile is fetched from HBM once and every
// further slice of every group reads it through L2 / MALL, as the rank slices of one adapter do.
// Group g takes its pieces from w3[g] and writes out + g*go, split + g*gs; the block program and so
// each output's summation order are the one-adapter kernel's.
struct RowsGroupPtrs {
  const bf16_t* w3[LORA_MAX_GROUPS];
};
template <int R, int RG, int CH, int NR>
__global__ __launch_bounds__(512) void lora_rows_full_grouped_kernel(const bf16_t* __restrict__ x, int64_t ldx,
                                                                     RowsGroupPtrs gp, int64_t ldw,
                                                                     float* __restrict__ out0, int64_t ldo, int M,
                                                                     float alpha, bf16_t* __restrict__ split0,
                                                                     int64_t lds, int K2, int nsl, int64_t go,
                                                                     int64_t gs) {
  const unsigned g = blockIdx.y / (unsigned)nsl, gsl = blockIdx.y % (unsigned)nsl;
  const bf16_t* __restrict__ w3 = gp.w3[g];
  float* __restrict__ out = out0 + g * go;
  bf16_t* __restrict__ split = split0 ? split0 + g * gs : nullptr;
#define DY_BX blockIdx.x
#define DY_BY gsl
#define LTX_DY_BODY 3
#include "lora_dy_bodies.h"
#undef LTX_DY_BODY
#undef DY_BX
#undef DY_BY
}

// ---- launchers: every route, grid and offset below comes from the call's LoraPlan (lora_plan.h)

// lora_dy_finish_kernel over the partials of pl.dy in pl.ws (N, K: the columns of its dB / dA blocks): w and
// its split operand, dB, dA, each null where the route has none
template <int R>
static void launch_dy_finish(const LoraPlan& pl, hipStream_t s, int64_t M, int64_t N, int64_t K, float alpha, float* w,
                             int64_t ldw, bf16_t* split, int64_t lds, int64_t K2, float* dw = nullptr, int64_t on = 0,
                             int64_t oj = 0, int acc = 0, float alpha_a = 1.f, float* dwa = nullptr, int64_t ona = 0,
                             int64_t oja = 0, int acc_a = 0) {
  const DyLayout& d = pl.dy;
  const LoraLaunch& l = pl.l[pl.n - 1];
  hipLaunchKernelGGL((lora_dy_finish_kernel<R>), grid_of(l), dim3(l.threads), 0, s, d.gpw ? pl.ws + d.pw : nullptr,
                     d.gpw ? d.CS : 0, d.gpb ? pl.ws + d.pb : nullptr, d.gpb ? d.RS : 0, (int)M, (int)N, alpha, w, ldw,
                     split, lds, (int)K2, dw, on, oj, acc, d.nwb, d.finish_nbb(),
                     (const float*)(d.gpa ? pl.ws + d.pa : nullptr), (int)K, alpha_a, dwa, ona, oja, acc_a);
}

// ltx_lora_wgrad's token-sized route (called from lora.hip): dw (+)= alpha . Y^T . u through the dB
// product of lora_dy_kernel (bf16 matrix core, u split into exact hi / mid / lo pieces) and the dB
// half of the finish kernel, the row-split partials in the stream's workspace.
void lora_wgrad_rows(const LoraPlan& pl, const bf16_t* y, int64_t ldy, const float* u, int64_t ldu, float* dw,
                     int64_t on, int64_t oj, int64_t M, int64_t N, int64_t r, float alpha, int accumulate, hipStream_t s) {
  with_rank(r, [&](auto rank) {
    constexpr int R = decltype(rank)::value;
    hipLaunchKernelGGL((lora_dy_kernel<R, 2>), grid_of(pl.l[0]), dim3(pl.l[0].threads), 0, s, y, ldy, u, ldu, nullptr,
                       (int64_t)0, nullptr, pl.ws + pl.dy.pb, (int)M, (int)N, (const float*)nullptr, 0, 1.f);
    launch_dy_finish<R>(pl, s, M, N, 0, alpha, nullptr, 0, nullptr, 0, 0, dw, on, oj, accumulate);
  });
}

// ltx_lora_rows' token-sized routes (called from lora.hip): out = alpha . x . A^T and its split
// operand, either with the whole contraction inside one block (lora_rows_full_kernel) or through the
// w product of lora_dy_kernel (MODE 1: eight waves x 64 columns per block, column-split partials in
// the stream's workspace) and the w half of the finish kernel.
void lora_rows_dy(const LoraPlan& pl, const bf16_t* x, int64_t ldx, const bf16_t* w3, int64_t ldw, float* out,
                  int64_t ldo, int64_t M, int64_t K, int64_t r, float alpha, bf16_t* split, int64_t ld_split, int64_t K2,
                  hipStream_t s) {
  const LoraLaunch& l = pl.l[0];
  with_rank(r, [&](auto rank) {
    constexpr int R = decltype(rank)::value;
    if (l.k == LK_ROWS_FULL) {
      with_value<1, 2, 4>(l.a[1], [&](auto ch) {
        hipLaunchKernelGGL((lora_rows_full_kernel<R, RF_RG, decltype(ch)::value, LTX_RF_NR>), grid_of(l), dim3(l.threads),
                           0, s, x, ldx, w3, ldw, out, ldo, (int)M, alpha, split, ld_split, (int)K2);
      });
      return;
    }
    hipLaunchKernelGGL((lora_dy_kernel<R, 1>), grid_of(l), dim3(l.threads), 0, s, x, ldx, nullptr, (int64_t)0, w3, ldw,
                       pl.ws + pl.dy.pw, nullptr, (int)M, (int)K, (const float*)nullptr, 0, 1.f);
    launch_dy_finish<R>(pl, s, M, K, 0, alpha, out, ldo, split, ld_split, K2);
  });
}

static int dy_workspace(const char* who, int64_t M, int64_t N, int64_t K, int64_t r, int64_t groups, bool ok,
                        int64_t* floats) {
  if (!(ok && floats && M > 0 && N > 0 && lora_rank_ok(r)))
    return fail(LTX_ERR_BAD_ARG, std::string(who) + ": bad args (rank " LTX_LORA_RANK_TEXT ")");
  *floats = dy_layout(M, N, K, r, groups).total;
  return LTX_OK;
}
extern "C" int ltx_lora_dy_workspace(int64_t M, int64_t N, int64_t r, int64_t* floats) {
  return dy_workspace("lora_dy_workspace", M, N, 0, r, 1, true, floats);
}
extern "C" int ltx_lora_dy_dA_workspace(int64_t M, int64_t N, int64_t K, int64_t r, int64_t* floats) {
  return dy_workspace("lora_dy_dA_workspace", M, N, K, r, 1, K > 0, floats);
}
extern "C" int ltx_lora_dy_dA_grouped_workspace(int64_t M, int64_t N, int64_t K, int64_t r, int64_t groups,
                                                int64_t* floats) {
  LTX_CHECK_ARG(groups >= 1 && groups <= LORA_MAX_GROUPS, "lora_dy_dA_grouped_workspace: 1 to 4 groups");
  return dy_workspace("lora_dy_dA_workspace", M, N, K, r, groups, K > 0, floats);
}

// ltx_lora_dy_dA: the dY pass (w and dB partials), the x pass reading w from those partials, and one finish
// for w / split, dB and dA. Every output is bitwise what ltx_lora_dy followed by ltx_lora_wgrad(x, w, alpha_a)
// produces (dA: where that takes its token-sized route, M >= LORA_TOKEN_ROWS). ltx_lora_dy is the same
// without x (K = 0): the dY pass and the finish.
static int lora_dy_entry(const char* who, bool dA, const void* y, int64_t ldy, const float* u, int64_t ldu,
                         const void* w3, int64_t ldw3, const void* x, int64_t ldx, int64_t M, int64_t N, int64_t K,
                         int64_t r, float alpha, float* w, int64_t ldw_out, void* split, int64_t ld_split, int64_t K2,
                         float* dw, int64_t on, int64_t oj, int accumulate, float alpha_a, float* dwa, int64_t ona,
                         int64_t oja, int acc_a, float* workspace, void* stream) {
  if (!(y && u && w3 && w && split && dw && workspace && (!dA || (x && dwa && K > 0))))
    return fail(LTX_ERR_BAD_ARG, std::string(who) + ": null operand");
  const DyCall c{M, N, K, r, 0, ldy, ldu, ldw3, ldx, ldw_out, r, ld_split, K2, K2, on, oj, ona, oja,
                 (uintptr_t)y, (uintptr_t)w3, (uintptr_t)x, (uintptr_t)w, (uintptr_t)split};
  if (const char* err = lora_dy_check(c)) return fail(LTX_ERR_BAD_ARG, std::string(who) + ": " + err);
  LoraPlan pl = plan_lora_dy(M, N, K, r, 0);
  pl.ws = workspace;
  const DyLayout& d = pl.dy;
  hipStream_t s = (hipStream_t)stream;
  with_rank(r, [&](auto rank) {
    constexpr int R = decltype(rank)::value;
    hipLaunchKernelGGL((lora_dy_kernel<R, 3>), grid_of(pl.l[0]), dim3(pl.l[0].threads), 0, s, (const bf16_t*)y, ldy, u,
                       ldu, (const bf16_t*)w3, ldw3, pl.ws + d.pw, pl.ws + d.pb, (int)M, (int)N, (const float*)nullptr, 0,
                       1.f);
    if (dA) {
      with_value<6, 14>(pl.l[1].a[0], [&](auto mode) {
        hipLaunchKernelGGL((lora_dy_kernel<R, decltype(mode)::value>), grid_of(pl.l[1]), dim3(pl.l[1].threads), 0, s,
                           (const bf16_t*)x, ldx, (const float*)nullptr, (int64_t)0, (const bf16_t*)nullptr, (int64_t)0,
                           (float*)nullptr, pl.ws + d.pa, (int)M, (int)K, (const float*)(pl.ws + d.pw), d.CS, alpha);
      });
    }
    launch_dy_finish<R>(pl, s, M, N, K, alpha, w, ldw_out, (bf16_t*)split, ld_split, K2, dw, on, oj, accumulate, alpha_a,
                        dwa, ona, oja, acc_a);
  });
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}
extern "C" int ltx_lora_dy(const void* y, int64_t ldy, const float* u, int64_t ldu, const void* w3, int64_t ldw3,
                           int64_t M, int64_t N, int64_t r, float alpha, float* w, int64_t ldw_out, void* split,
                           int64_t ld_split, int64_t K2, float* dw, int64_t on, int64_t oj, int accumulate,
                           float* workspace, void* stream) {
  return lora_dy_entry("lora_dy", false, y, ldy, u, ldu, w3, ldw3, nullptr, 0, M, N, 0, r, alpha, w, ldw_out, split,
                       ld_split, K2, dw, on, oj, accumulate, 1.f, nullptr, 0, 0, 0, workspace, stream);
}
extern "C" int ltx_lora_dy_dA(const void* y, int64_t ldy, const float* u, int64_t ldu, const void* w3, int64_t ldw3,
                              const void* x, int64_t ldx, int64_t M, int64_t N, int64_t K, int64_t r, float alpha,
                              float* w, int64_t ldw_out, void* split, int64_t ld_split, int64_t K2, float* dw,
                              int64_t on, int64_t oj, int accumulate, float alpha_a, float* dwa, int64_t ona,
                              int64_t oja, int acc_a, float* workspace, void* stream) {
  return lora_dy_entry("lora_dy_dA", true, y, ldy, u, ldu, w3, ldw3, x, ldx, M, N, K, r, alpha, w, ldw_out, split,
                       ld_split, K2, dw, on, oj, accumulate, alpha_a, dwa, ona, oja, acc_a, workspace, stream);
}

// ltx_lora_dy_dA for `groups` adapters on the column blocks of one packed dY [M, groups * N] that
// share x: the dY pass with the groups in grid z, one x pass whose blocks cover every group's rank
// slices per 512-column tile, one finish with the groups in grid y. Three launches; every output
// bitwise the one-adapter call on the column slice (the same block program on the same operands).
extern "C" int ltx_lora_dy_dA_grouped(const void* y, int64_t ldy, const float* const* u, int64_t ldu,
                                      const void* const* w3, int64_t ldw3, const void* x, int64_t ldx, int64_t M,
                                      int64_t N, int64_t K, int64_t r, int64_t groups, float alpha, float* w,
                                      int64_t ldw_out, int64_t gw, void* split, int64_t ld_split, int64_t K2,
                                      int64_t gs, float* const* dw, int64_t on, int64_t oj, int accumulate,
                                      float alpha_a, float* const* dwa, int64_t ona, int64_t oja, int acc_a,
                                      float* workspace, void* stream) {
  LTX_CHECK_ARG(y && u && w3 && x && w && split && dw && dwa && workspace && K > 0, "lora_dy_dA_grouped: null operand");
  LTX_CHECK_ARG(groups >= 1 && groups <= LORA_MAX_GROUPS, "lora_dy_dA_grouped: 1 to 4 groups");
  DyGroupPtrs gp{};
  for (int g = 0; g < (int)groups; ++g) {
    LTX_CHECK_ARG(u[g] && w3[g] && dw[g] && dwa[g] && ((uintptr_t)w3[g] % 16) == 0,
                  "lora_dy_dA_grouped: null or misaligned group operand");
    gp.u[g] = u[g];
    gp.w3[g] = (const bf16_t*)w3[g];
    gp.dw[g] = dw[g];
    gp.dwa[g] = dwa[g];
  }
  const DyCall c{M, N, K, r, groups, ldy, ldu, ldw3, ldx, ldw_out, gw, ld_split, K2, gs, on, oj, ona, oja,
                 (uintptr_t)y, (uintptr_t)w3[0], (uintptr_t)x, (uintptr_t)w, (uintptr_t)split};
  if (const char* err = lora_dy_check(c)) return fail(LTX_ERR_BAD_ARG, std::string("lora_dy_dA_grouped: ") + err);
  const LoraPlan pl = plan_lora_dy(M, N, K, r, groups);
  const DyLayout& d = pl.dy;
  const int G = (int)groups;
  float *pw = workspace + d.pw, *pb = workspace + d.pb, *pa = workspace + d.pa;
  hipStream_t s = (hipStream_t)stream;
  with_rank(r, [&](auto rank) {
    constexpr int R = decltype(rank)::value;
    hipLaunchKernelGGL((lora_dy_grouped_kernel<R, 3>), grid_of(pl.l[0]), dim3(pl.l[0].threads), 0, s, (const bf16_t*)y,
                       ldy, gp, ldu, ldw3, pw, pb, (int)M, (int)N, (const float*)nullptr, 0, 1.f, G, N, d.gpw, d.gpb,
                       (int64_t)0);
    hipLaunchKernelGGL((lora_dy_grouped_kernel<R, 6>), grid_of(pl.l[1]), dim3(pl.l[1].threads), 0, s, (const bf16_t*)x,
                       ldx, gp, (int64_t)0, (int64_t)0, (float*)nullptr, pa, (int)M, (int)K, (const float*)pw, d.CS,
                       alpha, G, (int64_t)0, (int64_t)0, d.gpa, d.gpw);
    hipLaunchKernelGGL((lora_dy_finish_grouped_kernel<R>), grid_of(pl.l[2]), dim3(pl.l[2].threads), 0, s, pw, d.CS, pb,
                       d.RS, (int)M, (int)N, alpha, w, ldw_out, (bf16_t*)split, ld_split, (int)K2, gp, on, oj, accumulate,
                       d.nwb, d.nbb, (const float*)pa, (int)K, alpha_a, ona, oja, acc_a, d.gpw, d.gpb, d.gpa, gw, gs);
  });
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

// ltx_lora_rows for `groups` adapters that share x. Where ltx_lora_rows' whole-contraction route
// holds for every group's operands (rows_full_route, the same function ltx_lora_rows plans from) this
// is ONE launch with (group, rank slice) as grid y; everywhere else it issues the one-adapter calls.
// Either way every output is bitwise ltx_lora_rows' on the same operands.
extern "C" int ltx_lora_rows_grouped(const void* x, int64_t ldx, const void* const* w3, int64_t ldw, float* out,
                                     int64_t ldo, int64_t go, int64_t M, int64_t K, int64_t r, float alpha,
                                     void* split, int64_t ld_split, int64_t K2, int64_t gs, int64_t groups,
                                     void* stream) {
  LTX_CHECK_ARG(x && w3 && out && M > 0 && K > 0, "lora_rows_grouped: bad args");
  LTX_CHECK_ARG(groups >= 1 && groups <= LORA_MAX_GROUPS, "lora_rows_grouped: 1 to 4 groups");
  LTX_CHECK_ARG(go >= r && ldo >= (groups - 1) * go + r, "lora_rows_grouped: every group's out columns inside the row");
  LTX_CHECK_ARG(!split || (K2 >= 3 * r && K2 % 64 == 0 && gs >= K2 && ld_split >= (groups - 1) * gs + K2),
                "lora_rows_grouped: split needs K2 >= 3r, %64, every group's columns inside the row");
  RowsGroupPtrs gp{};
  for (int g = 0; g < (int)groups; ++g) {
    LTX_CHECK_ARG(w3[g] && ((uintptr_t)w3[g] % 16) == 0, "lora_rows_grouped: null or misaligned pieces");
    gp.w3[g] = (const bf16_t*)w3[g];
  }
  const RowsCall c{M, K, r, ldx, ldw, ldo, (uintptr_t)x, (uintptr_t)w3[0], (uintptr_t)out, split != nullptr,
                   (uintptr_t)split, ld_split, K2};
  if (const char* err = lora_rows_check(c)) return fail(LTX_ERR_BAD_ARG, err);
  hipStream_t s = (hipStream_t)stream;
  bf16_t* sp = (bf16_t*)split;
  const LoraPlan pl = plan_lora_rows(c, lora_site(s), groups, go, gs);
  const LoraLaunch* l = &pl.l[0];
  if (l->k != LK_ROWS_FULL_GROUPED) {
    for (int g = 0; g < (int)groups; ++g) {
      const int rc = ltx_lora_rows(x, ldx, w3[g], ldw, out + g * go, ldo, M, K, r, alpha, sp ? sp + g * gs : nullptr,
                                   ld_split, K2, stream);
      if (rc != LTX_OK) return rc;
    }
    return LTX_OK;
  }
  with_rank(r, [&](auto rank) {
    with_value<1, 2, 4>(l->a[1], [&](auto ch) {
      hipLaunchKernelGGL((lora_rows_full_grouped_kernel<decltype(rank)::value, RF_RG, decltype(ch)::value, LTX_RF_NR>),
                         grid_of(*l), dim3(l->threads), 0, s, (const bf16_t*)x, ldx, gp, ldw, out, ldo, (int)M, alpha, sp,
                         ld_split, (int)K2, (int)(l->gy / groups), go, gs);
    });
  });
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

}  // namespace ltx
