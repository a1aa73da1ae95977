// The LoRA adapter dispatch, host only: the rank list, the three library switches, the partials
// layout of the dY family, the shared argument checks and the planners that every ltx_lora_* launcher
// launches from and ltx_lora_describe names (DESIGN "LoRA adapter dispatch plan"). A plan is a
// function of the call, the switch values and the stream's workspace; nothing here touches a device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "common.h"

namespace ltx {

// ---- the ranks every adapter kernel is instantiated for (ops.LORA_RANKS in Python)
#define LTX_LORA_RANK_TEXT "8, 16, 32, 64 or 128"
// f(std::integral_constant<int, V>{}) for the V that equals v; false (and nothing called) when none does
template <int... V, class F>
constexpr bool with_value(int64_t v, F&& f) {
  return ((v == V && (f(std::integral_constant<int, V>{}), true)) || ...);
}
// the list itself, written once; callers reject another rank first, with LTX_ERR_BAD_ARG
template <class F>
constexpr bool with_rank(int64_t r, F&& f) {
  return with_value<8, 16, 32, 64, 128>(r, f);
}
constexpr bool lora_rank_ok(int64_t r) {
  return with_rank(r, [](auto) {});
}

// ---- the gates' numbers (DESIGN section 7 says where each was measured)
constexpr int LORA_DOWN_BIG_ROWS = 8192;  // lora_down_kernel: 32-row blocks from here on
constexpr int LORA_TOKEN_ROWS = 2048;     // the dY-family routes of ltx_lora_rows / ltx_lora_wgrad from here on
constexpr int DY_COLS = 512;              // columns per block of lora_dy_kernel
constexpr int DY_MAXCS = 4;   // column splits a MODE-6 pass sums its u from (N <= 2048; MODE 14: per loop trip)
constexpr int LORA_MAX_GROUPS = 4;  // adapters per grouped launch (their operands are kernel arguments)
#ifndef LTX_RF_NR
#define LTX_RF_NR 5  // ring slots per wave of lora_rows_full_kernel
#endif
constexpr int RF_RG = 2;  // its 32-row groups per block
// row groups of 32 per lora_dy_kernel block and rank slices per dY tile (lora_dy.hip says why)
constexpr int dy_g(int r) { return r <= 16 ? 7 : 4; }
constexpr int dy_nsl(int r) { return r <= 32 ? 1 : r / 32; }

// ---- the library-side switches (atoi, default 1), read once at the first call; a test that needs
// another value starts a child process
inline int lora_env(const char* name) {
  const char* e = getenv(name);
  return e ? atoi(e) : 1;
}
struct LoraSwitches {
  int wgrad_rows = lora_env("LTX_LORA_WGRAD_ROWS");  // 0: lora_wgrad_kernel everywhere
  int rows_dy = lora_env("LTX_LORA_ROWS_DY");        // 0: lora_rows_kernel everywhere
  int rows_full = lora_env("LTX_LORA_ROWS_FULL");    // 0: the column-split pass + finish at K = 512 / 1024 / 2048 too
};
inline const LoraSwitches& lora_switches() {
  static const LoraSwitches sw;
  return sw;
}
// where a call runs: the switches and the stream's workspace (never dereferenced here)
struct LoraSite {
  LoraSwitches sw;
  float* ws;
  size_t ws_bytes;
  bool fits(int64_t floats) const { return ws != nullptr && (size_t)floats * sizeof(float) <= ws_bytes; }
};
inline LoraSite lora_site(hipStream_t s) {
  LoraSite e{lora_switches(), nullptr, 0};
  e.ws = stream_workspace(s, &e.ws_bytes);
  return e;
}

// ---- the partials of the dY family: `groups` adapters, each [CS][M][RP] of w (products & 1),
// [RS][N][RP] of dB (products & 2) and [RS][K][RP] of dA (K > 0), every w block first, then every
// dB block, then every dA block. The *_workspace entries return `total`; the launchers take their
// offsets and grids from here.
struct DyLayout {
  int64_t RP;                // padded rank
  int G, NSL, CS, CSx, RS;   // row groups per block, rank slices, column splits of dY / of x, row splits
  int64_t gpw, gpb, gpa;     // floats per group
  int64_t pw, pb, pa, total;  // float offsets of the three areas, and the sum
  int nwb, nbb, nba;         // finish blocks for w + split, dB, dA
  int finish_nbb() const { return nba ? nbb : 1 << 30; }  // the finish kernel's "dA blocks start here"
  unsigned finish_grid() const { return (unsigned)(nwb + nbb + nba); }
};
inline DyLayout dy_layout(int64_t M, int64_t N, int64_t K, int64_t r, int64_t groups, int products = 3) {
  DyLayout d{};
  d.RP = r >= 16 ? r : 16;
  d.G = dy_g((int)r);
  d.NSL = dy_nsl((int)r);
  d.CS = (int)(N / DY_COLS);
  d.CSx = (int)(K / DY_COLS);
  d.RS = (int)((M + d.G * 32 - 1) / (d.G * 32));
  d.gpw = (products & 1) ? (int64_t)d.CS * M * d.RP : 0;
  d.gpb = (products & 2) ? (int64_t)d.RS * N * d.RP : 0;
  d.gpa = (int64_t)d.RS * K * d.RP;
  d.pb = groups * d.gpw;  // pw = 0
  d.pa = d.pb + groups * d.gpb;
  d.total = d.pa + groups * d.gpa;
  d.nwb = (products & 1) ? (int)((M * (r / 4) + 255) / 256) : 0;
  d.nbb = (products & 2) ? (int)((N * r + 63) / 64) : 0;
  d.nba = (int)((K * r + 63) / 64);
  return d;
}

// ---- kernels and plans
enum LoraKernel {
  LK_DOWN, LK_ROWS, LK_ROWS_FULL, LK_ROWS_FULL_GROUPED, LK_DY, LK_DY_GROUPED, LK_DY_FINISH, LK_DY_FINISH_GROUPED,
  LK_WGRAD, LK_WGRAD_FINISH
};
// name and number of template arguments after the rank (-1: not a template), as rocprof prints them
struct LoraKernelDef {
  const char* name;
  int nargs;
};
constexpr LoraKernelDef LORA_KERNELS[] = {
    {"lora_down_kernel", 2},  // <R, RG, KW>
    {"lora_rows_kernel", 2},  // <R, NW, NR>
    {"lora_rows_full_kernel", 3},  // <R, RG, CH, NR>
    {"lora_rows_full_grouped_kernel", 3},
    {"lora_dy_kernel", 1},  // <R, MODE>
    {"lora_dy_grouped_kernel", 1},
    {"lora_dy_finish_kernel", 0},
    {"lora_dy_finish_grouped_kernel", 0},
    {"lora_wgrad_kernel", 0},
    {"lora_wgrad_finish_kernel", -1},
};
struct LoraLaunch {
  LoraKernel k;
  int a[3];  // the template arguments after the rank
  unsigned gx, gy, gz, threads;
};
struct LoraPlan {
  LoraLaunch l[3];  // in launch order
  int n = 0;
  int times = 1;            // ltx_lora_rows_grouped outside its one-launch route: this plan once per group
  int splits = 1, rps = 0;  // lora_wgrad_kernel's row splits and rows per split
  DyLayout dy{};            // the dY-family routes
  float* ws = nullptr;      // the stream's workspace, where the route keeps partials there
  void add(LoraKernel k, int a0, int a1, int a2, int threads, int64_t gx, int64_t gy = 1, int64_t gz = 1) {
    l[n++] = LoraLaunch{k, {a0, a1, a2}, (unsigned)gx, (unsigned)gy, (unsigned)gz, (unsigned)threads};
  }
};
inline dim3 grid_of(const LoraLaunch& l) { return dim3(l.gx, l.gy, l.gz); }

// ltx_lora_down(_grouped): lora_down_kernel<R, RG, KW>. 32-row blocks (RG = 2) for token-sized M
// (16-row blocks measured 26 vs 21 us at M = 14336); K split 8 ways (512 threads) where K allows:
// 19.7 vs 20.7 us (forward A), 18.6 vs 19.6 us (split B^T dgrad). Ranks above 32: one 32-wide rank
// slice per grid z.
inline LoraPlan plan_lora_down(int64_t M, int64_t K, int64_t r, int64_t groups) {
  LoraPlan pl;
  const bool big = M >= LORA_DOWN_BIG_ROWS;
  const int kw = K % 256 == 0 ? 8 : 4;
  pl.add(LK_DOWN, big ? 2 : 1, kw, 0, 64 * kw, big ? (M + 31) / 32 : (M + 15) / 16, groups, r > 32 ? r / 32 : 1);
  return pl;
}

// what the planners read of an ltx_lora_rows call (pointers as integers: only their alignment counts)
struct RowsCall {
  int64_t M, K, r, ldx, ldw, ldo;
  uintptr_t x, w3, out;
  bool split;
  uintptr_t sp;
  int64_t ld_split, K2;
};
// ltx_lora_rows' argument checks: null, or the text of the first one that fails
inline const char* lora_rows_check(const RowsCall& c) {
  if (!(c.x && c.w3 && c.out && c.M > 0 && c.K > 0 && c.ldo >= c.r)) return "lora_rows: bad args";
  if (!(c.K % 256 == 0 && c.ldx % 8 == 0 && c.x % 16 == 0 && c.ldw % 8 == 0 && c.w3 % 16 == 0 && c.ldw >= c.K))
    return "lora_rows: K % 256, 16-B aligned rows of x and of the pieces";
  if (!(c.ldx * 2 * (c.M - 1) + 2 * c.K < ((int64_t)1 << 32) &&
        c.ldw * 2 * 3 * (c.r > 32 ? c.r : 32) < ((int64_t)1 << 32)))
    return "lora_rows: 32-bit DMA offsets";
  if (c.split && !(c.K2 >= 3 * c.r && c.K2 % 64 == 0 && c.ld_split >= c.K2)) return "lora_rows: split needs K2 >= 3r, %64";
  if (!lora_rank_ok(c.r)) return "lora_rows: rank must be " LTX_LORA_RANK_TEXT;
  return nullptr;
}
// the dY-family routes of ltx_lora_rows apply to a call that passed lora_rows_check: token-sized M in
// whole row groups, K in whole 512-column blocks, 16-B rows of out, 8-B rows of the split
inline bool rows_token_route(const RowsCall& c, const LoraSwitches& sw) {
  if (!sw.rows_dy || c.M < LORA_TOKEN_ROWS || c.M % 32 != 0 || c.K % DY_COLS != 0) return false;
  if (c.ldo % 4 != 0 || c.out % 16 != 0) return false;
  return !c.split || (c.ld_split % 4 == 0 && c.sp % 8 == 0 && (c.K2 - 3 * c.r) % 4 == 0);
}
// ... and among them the whole-contraction route (K = 512 / 1024 / 2048: no partials, no finish).
// ltx_lora_rows_grouped is one launch exactly where this holds for every group's operands.
inline bool rows_full_route(const RowsCall& c, const LoraSwitches& sw) {
  return rows_token_route(c, sw) && sw.rows_full && (c.K == 512 || c.K == 1024 || c.K == 2048);
}
// ltx_lora_rows, first match: whole contraction per block > column-split lora_dy_kernel<R, 1> +
// finish (partials in the stream's workspace) > lora_rows_kernel (4 waves x K/4 per 32-row block,
// 4-slot ring: 16.3 us at M = 14336, K = 2048, r = 16 against 19.9 us for lora_down_kernel; 8 waves
// x K/8 with a 3-slot ring: 17.8 us).
// groups >= 1 (ltx_lora_rows_grouped; c = group 0, group g writes out + g go and split + g gs): where
// the whole-contraction route holds for every group's operands, its grouped kernel with (group,
// rank slice) in grid y; everywhere else the one-adapter plan once per group (pl.times).
inline LoraPlan plan_lora_rows(const RowsCall& c, const LoraSite& e, int64_t groups = 0, int64_t go = 0,
                               int64_t gs = 0) {
  LoraPlan pl;
  bool full = rows_full_route(c, e.sw);
  for (int64_t g = 1; g < groups && full; ++g) {
    RowsCall cg = c;
    cg.out += (uintptr_t)(g * go * 4);
    cg.sp += (uintptr_t)(g * gs * 2);
    full = rows_full_route(cg, e.sw);
  }
  if (full) {
    const int64_t nsl = c.r > 16 ? c.r / 16 : 1;  // y: 16-wide rank slices
    pl.add(groups ? LK_ROWS_FULL_GROUPED : LK_ROWS_FULL, RF_RG, (int)(c.K / 512), LTX_RF_NR, 512,
           (c.M + RF_RG * 32 - 1) / (RF_RG * 32), nsl * (groups ? groups : 1));
    return pl;
  }
  pl.times = groups ? (int)groups : 1;
  pl.dy = dy_layout(c.M, c.K, 0, c.r, 1, 1);
  if (rows_token_route(c, e.sw) && e.fits(pl.dy.total)) {
    pl.ws = e.ws;
    pl.add(LK_DY, 1, 0, 0, 512, pl.dy.CS * pl.dy.NSL, pl.dy.RS);
    pl.add(LK_DY_FINISH, 0, 0, 0, 256, pl.dy.finish_grid());
    return pl;
  }
  pl.add(LK_ROWS, 4, 4, 0, 256, (c.M + 31) / 32, c.r > 32 ? c.r / 32 : 1);  // y: 32-wide rank slices
  return pl;
}

// ltx_lora_wgrad, first match: one adapter at token-sized M through the dB product of
// lora_dy_kernel<R, 2> + finish (lora_wgrad_kernel spends ~9 us of f32 MFMA issue on the same product
// at M = 14336, N = 2048, r = 16) > lora_wgrad_kernel over row splits + lora_wgrad_finish_kernel
// (partials in the stream's workspace) > lora_wgrad_kernel with one split (each block owns its outputs).
struct WgradCall {  // y has passed the entry's checks: 16-B aligned rows
  int64_t M, N, r, ldy, ldu, groups, gd;
  uintptr_t dw;
};
inline LoraPlan plan_lora_wgrad(const WgradCall& c, const LoraSite& e) {
  LoraPlan pl;
  pl.dy = dy_layout(c.M, c.N, 0, c.r, 1, 2);
  if (c.groups == 1 && e.sw.wgrad_rows && c.M >= LORA_TOKEN_ROWS && c.M % 32 == 0 && c.N % DY_COLS == 0 &&
      c.ldy * 2 * 32 < ((int64_t)1 << 32) && c.ldu >= c.r && e.fits(pl.dy.total)) {
    pl.ws = e.ws;
    pl.add(LK_DY, 2, 0, 0, 512, pl.dy.CS * pl.dy.NSL, pl.dy.RS);
    pl.add(LK_DY_FINISH, 0, 0, 0, 256, pl.dy.finish_grid());
    return pl;
  }
  // ~512 blocks of 128 columns x >= 512 rows (8 waves x 4-quad steps): enough waves to stream y.
  // ~512 blocks (two per CU): 17.9 us vs 20.0 us with 256 at M = 14336, N = 2048, r = 16. Splits
  // of >= 256 rows in multiples of 32 (a wave's row quads stay aligned; the last 128-row step of a
  // split may be partial): M = 14336 -> 32 splits of 448 rows = exactly 512 blocks
  const int nb = (int)((c.N + 127) / 128);
  const int target = 512;
  int splits = (int)((target + nb * c.groups - 1) / (nb * c.groups));
  const int max_splits = (int)((c.M + 255) / 256);
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  int rps = (int)((c.M + splits - 1) / splits);
  rps = (rps + 31) / 32 * 32;
  splits = (int)((c.M + rps - 1) / rps);
  // S > 1: per-split partials in the stream's workspace (caller-owned, stream-ordered), summed in
  // order by the finish kernel; with no room for them, one split
  const bool aligned = c.dw % 16 == 0 && (c.N * c.r) % 4 == 0 && (c.groups == 1 || c.gd % 4 == 0);
  const bool parts = splits > 1 && aligned && e.fits(c.groups * splits * c.N * c.r);
  if (splits > 1 && !parts) {
    splits = 1;
    rps = (int)c.M;
  }
  pl.splits = splits;
  pl.rps = rps;
  // ranks above 32: r / 32 rank slices per 128 columns (consecutive blockIdx.x)
  pl.add(LK_WGRAD, 0, 0, 0, 512, nb * (c.r > 32 ? c.r / 32 : 1), splits, c.groups);
  if (parts) pl.ws = e.ws;
  if (parts) pl.add(LK_WGRAD_FINISH, 0, 0, 0, 256, (c.N * c.r / 4 + 255) / 256, c.groups);
  return pl;
}

// what the checker and the planner read of an ltx_lora_dy / ltx_lora_dy_dA / ltx_lora_dy_dA_grouped
// call: K = 0 without the dA product; groups = 0 for the one-adapter entries (gw = r, gs = K2)
struct DyCall {
  int64_t M, N, K, r, groups;
  int64_t ldy, ldu, ldw3, ldx, ldw_out, gw, ld_split, K2, gs, on, oj, ona, oja;
  uintptr_t y, w3, x, w, split;
};
// the argument checks the three entries share: null, or the text of the first one that fails (the
// entry puts its own name in front)
inline const char* lora_dy_check(const DyCall& c) {
  const int64_t G = c.groups ? c.groups : 1;
  if (!(c.M >= 32 && c.M % 32 == 0 && c.N % DY_COLS == 0 && c.K % DY_COLS == 0 && lora_rank_ok(c.r)))
    return "M % 32 == 0, N % 512 == 0, K % 512 == 0, rank " LTX_LORA_RANK_TEXT;
  if (c.groups && c.N > DY_MAXCS * DY_COLS) return "N <= 2048 per group";
  if (!(c.ldy % 8 == 0 && c.y % 16 == 0 && (!c.groups || c.ldy >= G * c.N) && c.ldw3 % 8 == 0 && c.w3 % 16 == 0 &&
        c.ldw3 >= c.N))
    return "16-B aligned rows of dY (every group's columns) and of the pieces";
  if (c.K && !(c.ldx % 8 == 0 && c.x % 16 == 0 && c.ldx >= c.K)) return "16-B aligned rows of x";
  if (!(c.ldy * 2 * 32 < ((int64_t)1 << 32) && c.ldx * 2 * 32 < ((int64_t)1 << 32))) return "32-bit DMA offsets";
  if (!(c.gw >= c.r && c.gs >= c.K2 && c.ldw_out >= (G - 1) * c.gw + c.r && c.ldu >= c.r && c.K2 >= 3 * c.r &&
        c.K2 % 64 == 0 && c.ld_split >= (G - 1) * c.gs + c.K2))
    return "output strides: every group's w / split columns inside the row, disjoint";
  if (!(c.ldw_out % 4 == 0 && c.gw % 4 == 0 && c.w % 16 == 0 && c.ld_split % 4 == 0 && c.gs % 4 == 0 && c.split % 8 == 0))
    return "16-B aligned w rows, 8-B aligned split rows";
  if (!((c.on == c.r && c.oj == 1) || (c.on == 1 && c.oj == c.N))) return "dB must be a dense [N,r] or [r,N]";
  if (c.K && !((c.ona == c.r && c.oja == 1) || (c.ona == 1 && c.oja == c.K))) return "dA must be a dense [K,r] or [r,K]";
  return nullptr;
}
// The dY pass (w and dB partials), with K the x pass reading w from those partials (up to N = 2048
// MODE 6, every partial in flight; beyond it MODE 14, a loop), and one finish. Grouped: the groups in
// grid z of the dY pass, (group, rank slice) pairs per x tile in grid x of the x pass, grid y of the finish.
inline LoraPlan plan_lora_dy(int64_t M, int64_t N, int64_t K, int64_t r, int64_t groups) {
  LoraPlan pl;
  const int64_t G = groups ? groups : 1;
  const DyLayout& d = pl.dy = dy_layout(M, N, K, r, G);
  pl.add(groups ? LK_DY_GROUPED : LK_DY, 3, 0, 0, 512, d.CS * d.NSL, d.RS, G);
  if (K) pl.add(groups ? LK_DY_GROUPED : LK_DY, d.CS <= DY_MAXCS ? 6 : 14, 0, 0, 512, d.CSx * d.NSL * G, d.RS);
  pl.add(groups ? LK_DY_FINISH_GROUPED : LK_DY_FINISH, 0, 0, 0, 256, d.finish_grid(), G);
  return pl;
}

// rocprof's names of the plan's kernels, without argument lists, joined by " + " in launch order
inline void describe_lora_plan(const LoraPlan& pl, int64_t r, char* buf, size_t len) {
  size_t at = 0;
  buf[0] = '\0';
  for (int t = 0; t < pl.times; ++t)
    for (int i = 0; i < pl.n; ++i) {
      const LoraLaunch& l = pl.l[i];
      const LoraKernelDef& k = LORA_KERNELS[l.k];
      char targs[48] = "";
      int m = k.nargs < 0 ? 0 : snprintf(targs, sizeof targs, "<%d", (int)r);
      for (int j = 0; j < k.nargs; ++j) m += snprintf(targs + m, sizeof targs - m, ", %d", l.a[j]);
      if (k.nargs >= 0) snprintf(targs + m, sizeof targs - m, ">");
      m = snprintf(buf + at, len - at, "%sltx::%s%s", at ? " + " : "", k.name, targs);
      if (m > 0) at = at + (size_t)m < len - 1 ? at + (size_t)m : len - 1;
    }
}

}  // namespace ltx
