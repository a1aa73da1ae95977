// Max-norm regularisation of the LoRA adapters (FusedAdamW / FusedProdigy(scale_weight_norms=c); DESIGN.md
// "Max-norm (scale_weight_norms)"): after the optimizer's update every adapter pair (A f32 [r, K], B f32
// [N, r], s) whose norm = |s| ||B A||_F exceeds the cap c has A and B multiplied by f = f32(sqrt(c / norm)),
// so the product sits on the cap. Everything walks device tables, nothing reads a value back, there are no
// atomics and every sum has a fixed order, so two runs and two ranks agree bit for bit.
//
// The product is never formed: ||B A||_F^2 = sum_ij (B^T B)_ij (A A^T)_ij, two r x r Gram matrices, taken in
// f64 (an f32 element converts exactly and the product of two has 48 bits, so every term is exact and only the
// f64 additions round). The Gram matrices are symmetric: they are cut into T x T tiles, T = min(r, 64), and
// only the tiles on and above the diagonal are computed, the ones above it counted twice.
//   gram_partials_kernel   one workgroup per (pair, A or B, slab of K or N, tile): the tile's sums over the
//                          slab, T^2 f64 into the caller's workspace (ltx_max_norm_sumsq, first launch);
//   gram_contract_kernel   one workgroup per pair: per Gram entry the slabs added in order, then the sum of
//                          the weighted products -> sumsq[pair] (ltx_max_norm_sumsq, second launch);
//   max_norm_finish_kernel one workgroup: per pair norm, ratio and f in f64, factor[pair], and the record
//                          {keys_scaled, mean and maximum of the scaled norms} (ltx_max_norm_finish);
//   max_norm_scale_multi_kernel  a chunk table over the paired tensors, one workgroup per row of at most 2048
//                          elements: p <- p f and, where the row has an EMA shadow, the shadow's correction
//                          (ltx_max_norm_scale_multi).
// The pair table has MN_FIELDS int64 per pair: A, B, N, K, r, the bits of the f64 s, the first f64 of the
// pair's A partials and of its B partials in the workspace, its first workgroup, the slab length, the slabs
// of K and of N (ltx_max_norm_plan gives the last three and the sizes).
#include <cmath>

#include "chunk_io.h"
#include "common.h"
#include "ltx_hip.h"

namespace ltx {

constexpr int MN_FIELDS = 12;
constexpr int MN_ROW = 5;      // the scale table: param, shadow or 0, first element, count, pair
constexpr int MN_STEP = 64;    // elements of the long dimension staged in LDS per step
constexpr int MN_TILE = 64;    // the largest Gram tile

__host__ __device__ inline int mn_tile(int r) { return r < MN_TILE ? r : MN_TILE; }
__host__ __device__ inline int mn_tiles(int r) {
  const int nt = r / mn_tile(r);
  return nt * (nt + 1) / 2;
}
// slabs of 1024 elements up to r = 16, of 2048 above: at r = 16 a 2048 x 2048 pair is four workgroups of 1024
// steps, at r = 128 the partials of a pair (3 tiles of 4096 f64 per slab) stay under half a megabyte
__host__ __device__ inline int64_t mn_slab(int r) { return r <= 16 ? 1024 : 2048; }

static bool mn_rank_ok(int64_t r) { return r == 8 || r == 16 || r == 32 || r == 64 || r == 128; }

// tile number t of the upper triangle, row by row -> (ti, tj), ti <= tj
__device__ __forceinline__ void mn_tile_at(int t, int nt, int& ti, int& tj) {
  ti = 0;
  while (t >= nt - ti) {
    t -= nt - ti;
    ++ti;
  }
  tj = ti + t;
}

// One T x T tile of a Gram matrix over elements [l0, l1) of the long dimension: element (short index i, long
// index l) of the operand is src[i * ss + l * sl] (A: ss = K, sl = 1; B: ss = 1, sl = r). The slab is staged
// MN_STEP long indices at a time as X[l][i0 + .] and Y[l][j0 + .] (zeros past l1: they add nothing); thread
// (ty, tx) keeps the E x E entries (ty E + a, tx E + b) and adds the slab's terms in the order of l.
template <int T, int E>
__device__ __forceinline__ void gram_tile(const float* __restrict__ src, int64_t ss, int64_t sl, int i0, int j0,
                                          int64_t l0, int64_t l1, double* __restrict__ out, float* lds) {
  constexpr int LD = T + 4;  // the rows stay 16-byte aligned; a column walk spreads over 8 banks
  constexpr int TX = T / E;
  float* X = lds;
  float* Y = lds + MN_STEP * LD;
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const bool active = ty < TX;
  double acc[E][E] = {};
  for (int64_t base = l0; base < l1; base += MN_STEP) {
    for (int idx = threadIdx.x; idx < T * MN_STEP; idx += 256) {
      // the lanes walk the operand's contiguous dimension
      const int i = sl == 1 ? idx / MN_STEP : idx % T;
      const int l = sl == 1 ? idx % MN_STEP : idx / T;
      const bool in = base + l < l1;
      const int64_t at = (base + l) * sl;
      X[l * LD + i] = in ? src[(int64_t)(i0 + i) * ss + at] : 0.f;
      Y[l * LD + i] = in ? src[(int64_t)(j0 + i) * ss + at] : 0.f;
    }
    __syncthreads();
    if (active) {
#pragma unroll 4
      for (int l = 0; l < MN_STEP; ++l) {
        double x[E], y[E];
#pragma unroll
        for (int a = 0; a < E; ++a) {
          x[a] = (double)X[l * LD + ty * E + a];
          y[a] = (double)Y[l * LD + tx * E + a];
        }
#pragma unroll
        for (int a = 0; a < E; ++a) {
#pragma unroll
          for (int b = 0; b < E; ++b) acc[a][b] = fma(x[a], y[b], acc[a][b]);  // the product is exact either way
        }
      }
    }
    __syncthreads();
  }
  if (active) {
#pragma unroll
    for (int a = 0; a < E; ++a) {
#pragma unroll
      for (int b = 0; b < E; ++b) out[(ty * E + a) * T + tx * E + b] = acc[a][b];
    }
  }
}

__global__ __launch_bounds__(256) void gram_partials_kernel(const int64_t* __restrict__ table, int npairs,
                                                            double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float lds[2 * MN_STEP * (MN_TILE + 4)];
  // the last pair whose first workgroup is not behind this one
  int lo = 0, hi = npairs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[(int64_t)mid * MN_FIELDS + 8] <= (int64_t)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const int64_t* e = table + (int64_t)lo * MN_FIELDS;
  const int64_t N = e[2], K = e[3];
  const int r = (int)e[4];
  const int64_t slab = e[9], slabs_a = e[10];
  const int T = mn_tile(r), nt = r / T, ntile = nt * (nt + 1) / 2;
  int64_t local = (int64_t)blockIdx.x - e[8];
  const bool of_b = local >= slabs_a * ntile;
  if (of_b) local -= slabs_a * ntile;
  const int64_t s = local / ntile;
  const int t = (int)(local % ntile);
  int ti, tj;
  mn_tile_at(t, nt, ti, tj);
  const float* src = (const float*)(of_b ? e[1] : e[0]);
  const int64_t len = of_b ? N : K, ss = of_b ? 1 : K, sl = of_b ? r : 1;
  const int64_t l0 = s * slab, l1 = l0 + slab < len ? l0 + slab : len;
  double* out = ws + (of_b ? e[7] : e[6]) + (s * ntile + t) * (int64_t)(T * T);
  switch (T) {
    case 8: gram_tile<8, 1>(src, ss, sl, ti * T, tj * T, l0, l1, out, lds); break;
    case 16: gram_tile<16, 1>(src, ss, sl, ti * T, tj * T, l0, l1, out, lds); break;
    case 32: gram_tile<32, 2>(src, ss, sl, ti * T, tj * T, l0, l1, out, lds); break;
    default: gram_tile<64, 4>(src, ss, sl, ti * T, tj * T, l0, l1, out, lds); break;
  }
}

// Per pair: entry by entry the slabs of both Gram matrices in order, the products (doubled above the
// diagonal) added thread-strided, then block_sum_ordered.
__global__ __launch_bounds__(256) void gram_contract_kernel(const int64_t* __restrict__ table,
                                                            const double* __restrict__ ws,
                                                            double* __restrict__ sumsq) {
  const int64_t* e = table + (int64_t)blockIdx.x * MN_FIELDS;
  const int r = (int)e[4];
  const int64_t slabs_a = e[10], slabs_b = e[11];
  const int T = mn_tile(r), nt = r / T, ntile = nt * (nt + 1) / 2, TT = T * T;
  const double* pa = ws + e[6];
  const double* pb = ws + e[7];
  double acc = 0.0;
  for (int idx = threadIdx.x; idx < ntile * TT; idx += 256) {
    const int t = idx / TT;
    int ti, tj;
    mn_tile_at(t, nt, ti, tj);
    double ga = 0.0, gb = 0.0;
    for (int64_t s = 0; s < slabs_a; ++s) ga += pa[s * ntile * TT + idx];
    for (int64_t s = 0; s < slabs_b; ++s) gb += pb[s * ntile * TT + idx];
    const double w = ti == tj ? 1.0 : 2.0;
    acc += w * (ga * gb);
  }
  __shared__ double red[4];
  acc = block_sum_ordered(acc, red);
  if (threadIdx.x == 0) sumsq[blockIdx.x] = acc;
}

// the device record of ltx_max_norm_finish (16 bytes)
struct MaxNormRecord {
  int32_t keys_scaled;  // pairs with ratio != 1
  float avg;            // mean of the scaled norms, the f64 mean rounded once
  float max;            // their maximum
  int32_t pad;
};
static_assert(sizeof(MaxNormRecord) == 16, "MaxNormRecord layout");

// One workgroup: thread-strided over the pairs, then a fixed-shape tree. A step the guard skipped scales
// nothing: every ratio is 1 and the record reports the norms as they stand.
__global__ __launch_bounds__(256) void max_norm_finish_kernel(const int64_t* __restrict__ table,
                                                              const double* __restrict__ sumsq, int npairs,
                                                              double cap, const GuardRecord* __restrict__ guard,
                                                              float* __restrict__ factor,
                                                              MaxNormRecord* __restrict__ rec) {
  const bool applied = guard ? step_applied(guard) : true;
  double sum = 0.0, mx = 0.0;
  int keys = 0;
  for (int p = threadIdx.x; p < npairs; p += 256) {
    const double s = __longlong_as_double(table[(int64_t)p * MN_FIELDS + 5]);
    const double norm = fabs(s) * sqrt(sumsq[p]);
    const double ratio = (!applied || norm <= cap) ? 1.0 : cap / norm;
    factor[p] = (float)sqrt(ratio);
    const double scaled = norm * ratio;
    keys += ratio != 1.0 ? 1 : 0;
    sum += scaled;
    mx = scaled > mx ? scaled : mx;
  }
  __shared__ double rs[256], rm[256];
  __shared__ int rk[256];
  rs[threadIdx.x] = sum;
  rm[threadIdx.x] = mx;
  rk[threadIdx.x] = keys;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      rs[threadIdx.x] += rs[threadIdx.x + o];
      rm[threadIdx.x] = rm[threadIdx.x + o] > rm[threadIdx.x] ? rm[threadIdx.x + o] : rm[threadIdx.x];
      rk[threadIdx.x] += rk[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    rec->keys_scaled = rk[0];
    rec->avg = (float)(rs[0] / (double)npairs);
    rec->max = (float)rm[0];
    rec->pad = 0;
  }
}

// One element per lane, as adamw_multi_kernel: a row's first element has only its tensor's alignment. The
// three operations of the shadow's correction round separately (-ffp-contract=off), as the EMA's own.
__global__ __launch_bounds__(256) void max_norm_scale_multi_kernel(const int64_t* __restrict__ rows,
                                                                   const float* __restrict__ factor, float omd,
                                                                   const GuardRecord* __restrict__ guard) {
  if (guard && !step_applied(guard)) return;
  const int64_t* e = rows + (int64_t)blockIdx.x * MN_ROW;
  const float f = factor[e[4]];
  if (f == 1.0f) return;
  float* __restrict__ param = (float*)e[0];
  float* __restrict__ shadow = (float*)e[1];
  const int64_t start = e[2], end = e[2] + e[3];
  for (int64_t i = start + threadIdx.x; i < end; i += 256) {
    const float before = param[i];
    const float after = before * f;
    param[i] = after;
    if (shadow) {
      const float moved = before - after;
      const float step = omd * moved;
      shadow[i] = shadow[i] - step;
    }
  }
}

}  // namespace ltx

using namespace ltx;

extern "C" {

int ltx_max_norm_plan(int64_t N, int64_t K, int64_t r, int64_t* out) {
  LTX_CHECK_ARG(out && N > 0 && K > 0, "max_norm_plan: bad args");
  LTX_CHECK_ARG(mn_rank_ok(r), "max_norm_plan: the rank is not one of 8, 16, 32, 64, 128");
  LTX_CHECK_ARG(N < (1LL << 31) && K < (1LL << 31), "max_norm_plan: N or K does not fit 31 bits");
  const int T = mn_tile((int)r), ntile = mn_tiles((int)r);
  const int64_t slab = mn_slab((int)r);
  const int64_t sa = (K + slab - 1) / slab, sb = (N + slab - 1) / slab;
  out[0] = slab;
  out[1] = sa;
  out[2] = sb;
  out[3] = (sa + sb) * ntile;          // workgroups of the first launch
  out[4] = sa * ntile * (int64_t)T * T;  // f64 of the A partials
  out[5] = sb * ntile * (int64_t)T * T;  // f64 of the B partials
  return LTX_OK;
}

int ltx_max_norm_sumsq(const int64_t* table, int64_t npairs, int64_t nwg, double* ws, double* sumsq, void* stream) {
  LTX_CHECK_ARG(table && ws && sumsq && npairs > 0 && npairs < (1LL << 31) && nwg >= npairs && nwg < (1LL << 31),
                "max_norm_sumsq: bad args");
  LTX_CHECK_ARG((((uintptr_t)table | (uintptr_t)ws | (uintptr_t)sumsq) & 7) == 0,
                "max_norm_sumsq: the table, the workspace and sumsq must be 8-byte aligned");
  hipLaunchKernelGGL(gram_partials_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, table, (int)npairs,
                     ws);
  hipLaunchKernelGGL(gram_contract_kernel, dim3((unsigned)npairs), dim3(256), 0, (hipStream_t)stream, table,
                     (const double*)ws, sumsq);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_max_norm_finish(const int64_t* table, const double* sumsq, int64_t npairs, double cap,
                        const void* guard_or_null, float* factor, void* record, void* stream) {
  LTX_CHECK_ARG(table && sumsq && factor && record && npairs > 0 && npairs < (1LL << 31),
                "max_norm_finish: bad args");
  LTX_CHECK_ARG(cap > 0.0 && std::isfinite(cap), "max_norm_finish: the cap must be a finite value > 0");
  LTX_CHECK_ARG((((uintptr_t)sumsq | (uintptr_t)guard_or_null) & 7) == 0 &&
                    (((uintptr_t)factor | (uintptr_t)record) & 3) == 0,
                "max_norm_finish: misaligned sumsq, guard, factor or record");
  hipLaunchKernelGGL(max_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, table, sumsq, (int)npairs,
                     cap, (const GuardRecord*)guard_or_null, factor, (MaxNormRecord*)record);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

int ltx_max_norm_scale_multi(const int64_t* rows, int64_t nrows, const float* factor, float one_minus_decay,
                             const void* guard_or_null, void* stream) {
  LTX_CHECK_ARG(rows && factor && nrows > 0 && nrows < (1LL << 31), "max_norm_scale_multi: bad args");
  LTX_CHECK_ARG(one_minus_decay >= 0.f && one_minus_decay <= 1.f,
                "max_norm_scale_multi: one_minus_decay outside [0, 1]");
  LTX_CHECK_ARG(((uintptr_t)guard_or_null & 7) == 0, "max_norm_scale_multi: guard must be 8-byte aligned");
  hipLaunchKernelGGL(max_norm_scale_multi_kernel, dim3((unsigned)nrows), dim3(256), 0, (hipStream_t)stream, rows,
                     factor, one_minus_decay, (const GuardRecord*)guard_or_null);
  LTX_LAUNCH_CHECK();
  return LTX_OK;
}

}  // extern "C"
