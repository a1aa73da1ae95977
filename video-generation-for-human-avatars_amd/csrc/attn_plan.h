// The attention dispatch, host only: the LTX_ATTN_* switch table, the kernel table and the two
// planners that ltx_attn_fwd / ltx_attn_bwd_ex launch from and ltx_attn_describe names (DESIGN
// "Attention dispatch plan"). Nothing here reads the environment or touches a device: a plan is a
// function of the call, the switch values, the CU count, the stream's workspace and the build.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace ltx {

// key ranges of at most this many run the one-pass kernels (one 8-wave workgroup holds them all)
constexpr int BWD1_KEYS = 256;
constexpr int BWD1_THREADS = 512;
constexpr int W1_KEYS = 256;   // keys per workgroup of the one-wave-per-SIMD dK/dV kernels
constexpr int W1P_MAXIT = 63;  // items per workgroup of the persistent kernels (table rows, + the null row)

#ifndef LTX_ATTN_W8_DEFAULT
#define LTX_ATTN_W8_DEFAULT 1
#endif

// The switch values, read once (first launch) and again by ltx_attn_reload_switches(). The member
// initialisers are the shipping configuration; ATTN_SWITCHES below says how each is parsed.
struct AttnSwitches {
  int xcd = 1, bwd1 = 1, w8 = LTX_ATTN_W8_DEFAULT, skip = 1, fwd1 = 1, fwd1_rows = 1, bwd1_qs = 0, bwd1_few = 1,
      qsplit = 1, dkdv_w1 = 2, dq_w1 = 2, dq_pipe = 1, dq_nbuf = 4, fwd_w1 = 0, fwd_pipe = 1, fwd_f32sum = 1,
      dkdv_pipe = 1, dkdv_nbuf = 4;
};

enum AttnSwitchRule {
  SW_OFF0,      // "0..." switches a default-on path off
  SW_ON1,       // "1..." switches a default-off path on
  SW_NUM,       // atoi of a non-empty value
  SW_NUM_OFF0,  // atoi unless empty or "0..."
  SW_NBUF,      // "3..." selects three LDS buffers, anything else four
};
struct AttnSwitchDef {
  const char* env;
  int AttnSwitches::*field;
  AttnSwitchRule rule;
};
constexpr AttnSwitchDef ATTN_SWITCHES[] = {
    {"LTX_ATTN_XCD", &AttnSwitches::xcd, SW_OFF0},              // 0: hardware block order
    {"LTX_ATTN_BWD1", &AttnSwitches::bwd1, SW_OFF0},            // 0: split dQ + dK/dV kernels for every key range
    {"LTX_ATTN_W8", &AttnSwitches::w8, SW_NUM},                 // bit 0 8-wave tiled forward, bit 1 8-wave dK/dV
    {"LTX_ATTN_SKIP", &AttnSwitches::skip, SW_OFF0},            // 0: one-pass kernels keep all-padding key blocks
    {"LTX_ATTN_FWD1", &AttnSwitches::fwd1, SW_OFF0},            // 0: tiled forward for every key range
    {"LTX_ATTN_FWD1_ROWS", &AttnSwitches::fwd1_rows, SW_OFF0},  // 0: the one-pass forward stores O in 32-B pieces
    {"LTX_ATTN_BWD1_QS", &AttnSwitches::bwd1_qs, SW_ON1},       // 1: query-split one-pass backward, biased ranges
    {"LTX_ATTN_BWD1_FEW", &AttnSwitches::bwd1_few, SW_OFF0},    // 0: the 8 x 32-key schedule for few unmasked keys
    {"LTX_ATTN_QSPLIT", &AttnSwitches::qsplit, SW_OFF0},        // 0: one workgroup per (batch, head) at any H * B
    {"LTX_ATTN_DKDV_W1", &AttnSwitches::dkdv_w1, SW_NUM},       // 2 persistent, 1 per block, 0 pipe, 12..16 / 22 diag
    {"LTX_ATTN_DQ_W1", &AttnSwitches::dq_w1, SW_NUM},           // likewise for dQ (diag: 12 / 13 / 22)
    {"LTX_ATTN_DQ_PIPE", &AttnSwitches::dq_pipe, SW_NUM},       // 0: the plain dQ kernel
    {"LTX_ATTN_DQ_NBUF", &AttnSwitches::dq_nbuf, SW_NBUF},
    {"LTX_ATTN_FWD_W1", &AttnSwitches::fwd_w1, SW_NUM_OFF0},    // one-wave forward (`make fwdw1` builds), 12 stamped
    {"LTX_ATTN_FWD_PIPE", &AttnSwitches::fwd_pipe, SW_NUM},     // 0: attn_q_kernel<64, 0, false, 8>
    {"LTX_ATTN_FWD_F32SUM", &AttnSwitches::fwd_f32sum, SW_OFF0},  // 0: row sums by v_dot2c over the bf16 weights
    {"LTX_ATTN_DKDV_PIPE", &AttnSwitches::dkdv_pipe, SW_NUM},   // 0: the plain dK/dV kernel
    {"LTX_ATTN_DKDV_NBUF", &AttnSwitches::dkdv_nbuf, SW_NBUF},
};
constexpr int ATTN_NSWITCH = (int)(sizeof(ATTN_SWITCHES) / sizeof(ATTN_SWITCHES[0]));

// value of one switch from its environment string (null: unset)
inline int parse_attn_switch(AttnSwitchRule rule, const char* e, int dflt) {
  const char c = e ? e[0] : '\0';
  switch (rule) {
    case SW_OFF0: return c == '0' ? 0 : 1;
    case SW_ON1: return c == '1' ? 1 : 0;
    case SW_NUM: return c ? std::atoi(e) : dflt;
    case SW_NUM_OFF0: return (c && c != '0') ? std::atoi(e) : 0;
    case SW_NBUF: return c == '3' ? 3 : 4;
  }
  return dflt;
}

// Every kernel instantiation the attention entry points launch: X(id, threads per workgroup, kernel).
// The kernel text, written the way rocprof prints it (every template argument, ", " between them),
// is both what the launch switch instantiates and the name ltx_attn_describe reports. The planners
// index the rows after a base id, so the order inside a group is part of the table.
#define LTX_ATTN_KERNELS_MAIN(X)                                                        \
  X(AK_FWD1, 512, attn_fwd1_kernel<64, false, false>) /* + 2 * bias + rows */            \
  X(AK_FWD1_FT, 512, attn_fwd1_kernel<64, false, true>)                                 \
  X(AK_FWD1_TF, 512, attn_fwd1_kernel<64, true, false>)                                 \
  X(AK_FWD1_TT, 512, attn_fwd1_kernel<64, true, true>)                                  \
  X(AK_Q32, 256, attn_q_kernel<32, 0, false, 4>) /* + 2 * (dQ: mode 1) + bias */        \
  X(AK_Q32_0T, 256, attn_q_kernel<32, 0, true, 4>)                                      \
  X(AK_Q32_1F, 256, attn_q_kernel<32, 1, false, 4>)                                     \
  X(AK_Q32_1T, 256, attn_q_kernel<32, 1, true, 4>)                                      \
  X(AK_Q64, 256, attn_q_kernel<64, 0, false, 4>)                                        \
  X(AK_Q64_0T, 256, attn_q_kernel<64, 0, true, 4>)                                      \
  X(AK_Q64_1F, 256, attn_q_kernel<64, 1, false, 4>)                                     \
  X(AK_Q64_1T, 256, attn_q_kernel<64, 1, true, 4>)                                      \
  X(AK_Q64_W8, 512, attn_q_kernel<64, 0, false, 8>) /* + bias */                        \
  X(AK_Q64_W8_T, 512, attn_q_kernel<64, 0, true, 8>)                                    \
  X(AK_DKDV32, 256, attn_dkdv_kernel<32, false, 4>) /* + bias */                        \
  X(AK_DKDV32_T, 256, attn_dkdv_kernel<32, true, 4>)                                    \
  X(AK_DKDV64, 256, attn_dkdv_kernel<64, false, 4>)                                     \
  X(AK_DKDV64_T, 256, attn_dkdv_kernel<64, true, 4>)                                    \
  X(AK_DKDV64_W8, 512, attn_dkdv_kernel<64, false, 8>)                                  \
  X(AK_DKDV64_W8_T, 512, attn_dkdv_kernel<64, true, 8>)                                 \
  X(AK_BWD1, 512, attn_bwd1_kernel<64, false, false>) /* + biased (+ 1: its QS form) */ \
  X(AK_BWD1_TF, 512, attn_bwd1_kernel<64, true, false>)                                 \
  X(AK_BWD1_TT, 512, attn_bwd1_kernel<64, true, true>)                                  \
  X(AK_BWD1_FINISH, 256, attn_bwd1_finish_kernel<64>)
#define LTX_ATTN_KERNELS_PIPE(X)                                                   \
  X(AK_FWD_PIPE, 512, attn_fwd_pipe_kernel<false>) /* + f32sum */                  \
  X(AK_FWD_PIPE_T, 512, attn_fwd_pipe_kernel<true>)                                \
  X(AK_DKDV_PIPE, 256, attn_dkdv_pipe_kernel<false, 3>) /* + 2 * bias + (NB 4) */  \
  X(AK_DKDV_PIPE_F4, 256, attn_dkdv_pipe_kernel<false, 4>)                         \
  X(AK_DKDV_PIPE_T3, 256, attn_dkdv_pipe_kernel<true, 3>)                          \
  X(AK_DKDV_PIPE_T4, 256, attn_dkdv_pipe_kernel<true, 4>)                          \
  X(AK_DQ_PIPE, 256, attn_dq_pipe_kernel<3>) /* + (NB 4) */                        \
  X(AK_DQ_PIPE_4, 256, attn_dq_pipe_kernel<4>)                                     \
  X(AK_DKDV_W1, 256, attn_dkdv_w1_kernel<0>)                                       \
  X(AK_DKDV_W1P, 256, attn_dkdv_w1p_kernel<0>)                                     \
  X(AK_DQ_W1, 256, attn_dq_w1_kernel<0>)                                           \
  X(AK_DQ_W1P, 256, attn_dq_w1p_kernel<0>)
// only in `make fwdw1` builds (AttnSite::fwd_w1)
#define LTX_ATTN_KERNELS_FWD_W1(X) X(AK_FWD_W1, 256, attn_fwd_w1_kernel)
// only in `make diag` builds (AttnSite::diag): the stamped timing variants, + (mode - 12)
#define LTX_ATTN_KERNELS_DIAG(X)                      \
  X(AK_DKDV_W1_V, 256, attn_dkdv_w1_kernel<1>)        \
  X(AK_DKDV_W1_V2, 256, attn_dkdv_w1_kernel<2>)       \
  X(AK_DKDV_W1_V3, 256, attn_dkdv_w1_kernel<3>)       \
  X(AK_DKDV_W1_V4, 256, attn_dkdv_w1_kernel<4>)       \
  X(AK_DKDV_W1_V5, 256, attn_dkdv_w1_kernel<5>)       \
  X(AK_DKDV_W1P_V, 256, attn_dkdv_w1p_kernel<1>)      \
  X(AK_DQ_W1_V, 256, attn_dq_w1_kernel<1>)            \
  X(AK_DQ_W1_V2, 256, attn_dq_w1_kernel<2>)           \
  X(AK_DQ_W1P_V, 256, attn_dq_w1p_kernel<1>)
#define LTX_ATTN_KERNELS(X) \
  LTX_ATTN_KERNELS_MAIN(X) LTX_ATTN_KERNELS_PIPE(X) LTX_ATTN_KERNELS_FWD_W1(X) LTX_ATTN_KERNELS_DIAG(X)

enum AttnKernelId {
#define LTX_X(id, threads, ...) id,
  LTX_ATTN_KERNELS(LTX_X)
#undef LTX_X
  AK_COUNT
};
inline const char* attn_kernel_name(AttnKernelId k) {
  static const char* const names[] = {
#define LTX_X(id, threads, ...) "ltx::" #__VA_ARGS__,
      LTX_ATTN_KERNELS(LTX_X)
#undef LTX_X
  };
  return names[k];
}
inline AttnKernelId ak(AttnKernelId base, int i) { return (AttnKernelId)(base + i); }

// what the planners read of a call
struct AttnCall {
  int HD, B, H, Nq, Nk;
  bool key_bias, dq_f32, delta_ready;
  int64_t ldq, ldk, ldv, lddo;  // row strides the persistent kernels' buffer descriptors span
};
// ... and of where it runs
struct AttnSite {
  AttnSwitches sw;
  int cus;
  float* ws;        // the stream's workspace (never dereferenced here)
  size_t ws_bytes;
  bool fwd_w1, diag;  // the build carries attn_fwd_w1_kernel / the stamped variants
};

struct AttnLaunch {
  AttnKernelId k;
  unsigned gx, gy, gz;
  float* part;  // AttnParams::part for this launch: query-split partials or diagnostic stamps
};
struct AttnPlan {
  AttnLaunch l[2];  // in launch order
  int n = 0;
  bool delta = false;      // attn_delta_kernel<HD> runs first
  bool split_bwd = false;  // l = {dQ, dK/dV}: two kernels, named dK/dV first
  int xcd_order = 0, skip_masked = 0, few_keys = 0, qsplit = 1;
  const char* err = nullptr;  // a diagnostic variant whose stamps do not fit the workspace
  int HD = 64;

  AttnLaunch& add(AttnKernelId k, int64_t gx, int64_t gy = 1, int64_t gz = 1) {
    l[n] = AttnLaunch{k, (unsigned)gx, (unsigned)gy, (unsigned)gz, nullptr};
    return l[n++];
  }
  // a stamped variant: `per` bytes per workgroup in the stream's workspace
  void stamps(AttnLaunch& a, const AttnSite& e, size_t per) {
    a.part = e.ws;
    if (e.ws == nullptr || e.ws_bytes < (size_t)a.gx * a.gy * a.gz * per) err = "stamps: workspace";
  }
};

inline bool attn_needs_bias(const AttnCall& c) { return c.key_bias || (c.Nk % 64) != 0; }

// Forward, first match: one-pass (Nk <= 256) > pipelined (no bias; the one-wave kernel where the
// build has it and LTX_ATTN_FWD_W1 asks) > 8-wave tiled > 4-wave tiled. Head dim 32 is 4-wave tiled.
inline AttnPlan plan_attn_fwd(const AttnCall& c, const AttnSite& e) {
  const AttnSwitches& w = e.sw;
  AttnPlan pl;
  pl.HD = c.HD;
  pl.xcd_order = w.xcd;
  pl.skip_masked = w.skip;
  const int bias = attn_needs_bias(c);
  if (c.HD == 64 && c.Nk <= BWD1_KEYS && w.fwd1) {  // every key staged once per (batch, head)
    // two workgroups per (batch, head) when that still leaves >= 8 slices each: 2 per CU
    // (more when H * B leaves the chip short of 256 workgroups: inference, config X at B = 1)
    const int nsl = (c.Nq + 31) / 32, hb = c.H * c.B;
    int z = nsl >= 16 ? 2 : 1;
    if (z == 2 && hb < 128) z = std::max(2, std::min(nsl / 8, (256 + hb - 1) / hb));
    pl.add(ak(AK_FWD1, 2 * bias + (w.fwd1_rows != 0)), c.H, c.B, z);
  } else if (c.HD == 64 && !bias && w.fwd_pipe != 0) {
    if (e.fwd_w1 && w.fwd_w1 != 0 && c.Nk % 64 == 0 && c.Nk >= 256) {
      AttnLaunch& a = pl.add(AK_FWD_W1, (c.Nq + 255) / 256, c.H, c.B);
      if (w.fwd_w1 == 12) pl.stamps(a, e, 4 * 8 * 8);
    } else {
      pl.add(ak(AK_FWD_PIPE, w.fwd_f32sum != 0), (c.Nq + 255) / 256, c.H, c.B);
    }
  } else if (c.HD == 64 && (w.w8 & 1)) {
    pl.add(ak(AK_Q64_W8, bias), (c.Nq + 255) / 256, c.H, c.B);
  } else {
    pl.add(ak(c.HD == 64 ? AK_Q64 : AK_Q32, bias), (c.Nq + 127) / 128, c.H, c.B);
  }
  return pl;
}

// the persistent kernels apply when every workgroup's items fit its table and the operands they
// read through buffer descriptors span less than 4 GiB; dQ only in bf16
inline bool attn_w1p_fits(int64_t items, int64_t rows, int64_t ld, int cus) {
  return items <= (int64_t)W1P_MAXIT * cus && (uint64_t)rows * (uint64_t)ld * 2 < 0xffffffffull;
}

// Backward, first match: one-pass (head dim 64, Nk <= 256; split over the queries under 128 (batch,
// head) pairs when the partials fit the workspace) > pipelined pair (head dim 64, no 8-wave dK/dV:
// per side persistent > one wave per SIMD > pipe, biased ranges on attn_q_kernel + the biased pipe)
// > plain pair.
inline AttnPlan plan_attn_bwd(const AttnCall& c, const AttnSite& e) {
  const AttnSwitches& w = e.sw;
  AttnPlan pl;
  pl.HD = c.HD;
  pl.delta = !c.delta_ready;
  pl.xcd_order = w.xcd;
  pl.skip_masked = w.skip;
  pl.few_keys = w.skip && w.bwd1_few;
  const int bias = attn_needs_bias(c);
  if (c.HD == 64 && c.Nk <= BWD1_KEYS && w.bwd1) {  // every key in one workgroup
    const int biased = c.key_bias || c.Nk != BWD1_KEYS;
    const int ntot = (c.Nq + 63) / 64, hb = c.H * c.B;
    if (hb < 128 && ntot >= 4 && w.qsplit) {
      // S depends on the shape alone, so the dK / dV summation order does too; when its f32 partials
      // [2][S][B][Nk][H * 64] do not fit the stream's workspace the unsplit kernel runs instead
      // (never a smaller S)
      const int S = std::min(ntot / 2, (256 + hb - 1) / hb);
      if (S > 1 && e.ws != nullptr && (size_t)2 * S * c.B * c.Nk * c.H * 64 * sizeof(float) <= e.ws_bytes) {
        pl.qsplit = S;
        pl.add(ak(AK_BWD1, biased), c.H, c.B, S).part = e.ws;
        pl.add(AK_BWD1_FINISH, ((int64_t)c.B * c.Nk * c.H * 64 / 8 + 255) / 256).part = e.ws;
        return pl;
      }
    }
    pl.add(ak(AK_BWD1, biased ? 1 + w.bwd1_qs : 0), c.H, c.B);
    return pl;
  }
  pl.split_bwd = true;
  const bool k8 = c.HD == 64 && ((w.w8 >> 1) & 1);
  const int64_t gq = (c.Nq + 127) / 128;
  if (c.HD == 64 && !k8 && w.dkdv_pipe != 0) {
    const int64_t qb = (c.Nq + 255) / 256, kb = (c.Nk + W1_KEYS - 1) / W1_KEYS;
    const int mq = w.dq_w1, mk = w.dkdv_w1;
    if (bias) {
      pl.add(AK_Q64_1T, gq, c.H, c.B);
    } else if ((mq == 2 || mq == 22) && !c.dq_f32 &&
               attn_w1p_fits(qb * c.H * c.B, c.Nk, std::max(c.ldk, c.ldv), e.cus)) {
      AttnLaunch& a = pl.add(e.diag && mq == 22 ? AK_DQ_W1P_V : AK_DQ_W1P, std::min<int64_t>(qb * c.H * c.B, e.cus));
      if (a.k == AK_DQ_W1P_V) pl.stamps(a, e, 4 * 12 * 8);
    } else if (mq != 0) {
      const bool v = e.diag && (mq == 12 || mq == 13);
      AttnLaunch& a = pl.add(v ? ak(AK_DQ_W1_V, mq - 12) : AK_DQ_W1, qb, c.H, c.B);
      if (v) pl.stamps(a, e, 4 * 12 * 8);
    } else if (w.dq_pipe != 0) {
      pl.add(ak(AK_DQ_PIPE, w.dq_nbuf == 4), gq, c.H, c.B);
    } else {
      pl.add(AK_Q64_1F, gq, c.H, c.B);
    }
    if (!bias && (mk == 2 || mk == 22) && attn_w1p_fits(kb * c.H * c.B, c.Nq, std::max(c.ldq, c.lddo), e.cus)) {
      AttnLaunch& a = pl.add(e.diag && mk == 22 ? AK_DKDV_W1P_V : AK_DKDV_W1P, std::min<int64_t>(kb * c.H * c.B, e.cus));
      if (a.k == AK_DKDV_W1P_V) pl.stamps(a, e, 4 * 12 * 8);
    } else if (!bias && mk != 0) {
      const bool v = e.diag && mk >= 12 && mk <= 16;
      AttnLaunch& a = pl.add(v ? ak(AK_DKDV_W1_V, mk - 12) : AK_DKDV_W1, kb, c.H, c.B);
      if (v) pl.stamps(a, e, 4 * 12 * 8);
    } else {
      pl.add(ak(AK_DKDV_PIPE, 2 * bias + (w.dkdv_nbuf == 4)), (c.Nk + 127) / 128, c.H, c.B);
    }
    return pl;
  }
  pl.add(ak(c.HD == 64 ? AK_Q64 : AK_Q32, 2 + bias), gq, c.H, c.B);
  if (k8) pl.add(ak(AK_DKDV64_W8, bias), (c.Nk + 255) / 256, c.H, c.B);
  else pl.add(ak(c.HD == 64 ? AK_DKDV64 : AK_DKDV32, bias), (c.Nk + 127) / 128, c.H, c.B);
  return pl;
}

// rocprof's names of the plan's kernels joined by " + ": the delta kernel first, then dK/dV before
// dQ, the query-split finish kernel last
inline void describe_attn_plan(const AttnPlan& pl, char* buf, size_t len) {
  size_t at = 0;
  auto put = [&](const char* name) {
    const int m = snprintf(buf + at, len - at, "%s%s", at ? " + " : "", name);
    if (m > 0) at = std::min(len - 1, at + (size_t)m);
  };
  buf[0] = '\0';
  if (pl.delta) put(pl.HD == 64 ? "ltx::attn_delta_kernel<64>" : "ltx::attn_delta_kernel<32>");
  for (int i = 0; i < pl.n; ++i) put(attn_kernel_name(pl.l[pl.split_bwd ? pl.n - 1 - i : i].k));
}

}  // namespace ltx
