// The block programs of lora_dy.hip's kernels, included into each kernel's braces: once with the
// block indices DY_BX / DY_BY = blockIdx.x / blockIdx.y (the one-adapter kernels: the same token
// stream as before the grouped launches existed, so the same code), once with the indices and
// operands of one group of a grouped launch. LTX_DY_BODY selects the program:
//   1  lora_dy_kernel          (template <int R, int MODE>; y, ldy, u, ldu, w3, ldw, part_w, part_b,
//                               M, N, part_u, CSu, alpha_u)
//   2  lora_dy_finish_kernel   (template <int R>; its argument list)
//   3  lora_rows_full_kernel   (template <int R, int RG, int CH, int NR>; DY_BX = row tile,
//                               DY_BY = 16-wide rank slice)
// No include guard: every inclusion is one kernel body.
#if LTX_DY_BODY == 1
  constexpr int RP = R >= 16 ? R : 16;    // padded rank: the stride of the pieces and of the partials
  constexpr int SW = dy_sw(R);             // this block's rank slice j0 .. j0 + SW
  constexpr int NSL = dy_nsl(R);
  constexpr int DY_G = dy_g(R);
  constexpr int DY_UPAD = DY_G * 32 + 4;   // u^T row length in LDS (floats; +4 spreads the banks)
  constexpr int JT = SW / 16;
  constexpr int NF = 3 * JT;
  constexpr int RING = 8 * DY_NR * 4096;
  constexpr int UT = SW * DY_UPAD * 4;
  static_assert(lora_rank_ok(R), "rank 8, 16, 32, 64 or 128");
  // ONE shared array (the DMA target): the ring, then u^T of the block's rows
  __shared__ __attribute__((aligned(16))) char smem[RING + UT];
  float* ut = (float*)(smem + RING);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cs = DY_BX / NSL, rs = DY_BY;
  const int j0 = (DY_BX % NSL) * SW;
  const int c0 = cs * DY_COLS + wave * 64;
  const int mb = rs * DY_G * 32;

  // DMA: piece i of a slot = rows 8i .. 8i+7; lane -> row 8i + (lane >> 3), physical chunk lane & 7
  uint32_t yo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 8 * i + (lane >> 3);
    yo[i] = (uint32_t)(row * ldy + (((lane & 7) ^ swz<64>(row)) * 8)) * 2;
  }
  const uint32_t lring = lds_u32(smem + wave * (DY_NR * 4096));
  auto dma = [&](int g) {
    const char* sb = (const char*)(y + (int64_t)(mb + 32 * g) * ldy + c0);  // M % 32 == 0
    const uint32_t l = lring + (g % DY_NR) * 4096;
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %5\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %5\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(yo[0]), "v"(yo[1]), "v"(yo[2]), "v"(yo[3]), "s"(sb), "s"(l)
        : "memory", "scc");
  };
  const int ng = min(DY_G, (M - mb + 31) / 32);  // row groups of this block
  // B^T pieces of this wave's 64 columns: [k half][piece x JT] (ltx_lora_rows' fragment layout).
  // Loaded first and retired, then handed to hipcc as asm outputs: its own waits for these loads
  // are counted without the asm DMA, and inside the slot loop they drained the prefetched slots
  // (vmcnt(5) .. vmcnt(0) before every slot's MFMAs)
  s16x8 bp[2][NF];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int t = 0; t < JT && (MODE & 1); ++t) {
      const bf16_t* src = w3 + (int64_t)(p * RP + j0 + t * 16 + (lane & 15)) * ldw + c0 + (lane >> 4) * 8;
      bp[0][p * JT + t] = *(const s16x8*)src;
      bp[1][p * JT + t] = *(const s16x8*)(src + 32);
    }
  if constexpr ((MODE & 1) != 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int f = 0; f < NF; ++f) asm volatile("" : "+v"(bp[h][f]));
  }
  // the first slots' DMA goes out ahead of the u^T staging loads, so their latencies overlap
  for (int g = 0; g < DY_NR - 1; ++g)
    if (g < ng) dma(g);

  // u^T of rows mb .. mb + 32G (zero past M): all loads in flight before the first LDS write (a
  // rolled loop waited out one load round trip per element, ~2 us per block)
  constexpr int UPT = (DY_G * 32 * SW + 511) / 512;
  float uv[UPT];
  if constexpr ((MODE & 8) != 0) {
    // u from more than DY_MAXCS w partials (the dY pass ran on N > 2048 columns, e.g. the feed-forward's
    // 8192): DY_MAXCS partials per element in flight at a time, added in c order from 0 into one running
    // sum -- the order of lora_dy_finish_kernel, so u is bitwise the w that kernel writes. A separate
    // branch: the MODE-6 instantiations (CSu <= DY_MAXCS) keep their code
    float accu[UPT];
#pragma unroll
    for (int i = 0; i < UPT; ++i) accu[i] = 0.f;
    for (int cb = 0; cb < CSu; cb += DY_MAXCS) {
      float pv[UPT][DY_MAXCS];
#pragma unroll
      for (int i = 0; i < UPT; ++i) {
        const int e = tid + 512 * i, j = j0 + e / (DY_G * 32), rr = e % (DY_G * 32), m = mb + rr;
        const bool ok = e < DY_G * 32 * SW && m < M && j < R;
#pragma unroll
        for (int c = 0; c < DY_MAXCS; ++c)
          pv[i][c] = part_u[((int64_t)(cb + c < CSu ? cb + c : 0) * RP + (ok ? j : 0)) * M + (ok ? m : 0)];
      }
#pragma unroll
      for (int i = 0; i < UPT; ++i)
#pragma unroll
        for (int c = 0; c < DY_MAXCS; ++c)
          if (cb + c < CSu) accu[i] += pv[i][c];
    }
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int e = tid + 512 * i, j = j0 + e / (DY_G * 32), rr = e % (DY_G * 32), m = mb + rr;
      uv[i] = (e < DY_G * 32 * SW && m < M && j < R) ? accu[i] * alpha_u : 0.f;
    }
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int e = tid + 512 * i;
      if (e < DY_G * 32 * SW) ut[(e / (DY_G * 32)) * DY_UPAD + e % (DY_G * 32)] = uv[i];
    }
  } else if constexpr ((MODE & 4) != 0) {  // u from the w partials: e -> (j, row), rows fastest (coalesced)
    // every partial load in flight before the first add (CSu <= DY_MAXCS; loads past CSu or past the
    // block's rows read partial 0 / row 0 and are not added); then the sum in c order from 0
    float pv[UPT][DY_MAXCS];
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int e = tid + 512 * i, j = j0 + e / (DY_G * 32), rr = e % (DY_G * 32), m = mb + rr;
      const bool ok = e < DY_G * 32 * SW && m < M && j < R;
#pragma unroll
      for (int c = 0; c < DY_MAXCS; ++c)
        pv[i][c] = part_u[((int64_t)(c < CSu ? c : 0) * RP + (ok ? j : 0)) * M + (ok ? m : 0)];
    }
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int e = tid + 512 * i, j = j0 + e / (DY_G * 32), rr = e % (DY_G * 32), m = mb + rr;
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < DY_MAXCS; ++c)
        if (c < CSu) acc += pv[i][c];
      uv[i] = (e < DY_G * 32 * SW && m < M && j < R) ? acc * alpha_u : 0.f;
    }
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int e = tid + 512 * i;
      if (e < DY_G * 32 * SW) ut[(e / (DY_G * 32)) * DY_UPAD + e % (DY_G * 32)] = uv[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int e = tid + 512 * i, rr = e / SW, j = j0 + e % SW, m = mb + rr;
      uv[i] = ((MODE & 2) && e < DY_G * 32 * SW && m < M && j < R) ? u[(int64_t)m * ldu + j] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int e = tid + 512 * i;
      if ((MODE & 2) && e < DY_G * 32 * SW) ut[(e % SW) * DY_UPAD + e / SW] = uv[i];
    }
  }
  __syncthreads();  // u^T staged; every ordinary load retired before the counted waits below

  // row reads (w product): rows 16q + (lane & 15), logical chunk 4h + (lane >> 4)
  int roff[2][2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = 16 * q + (lane & 15);
      roff[q][h] = row * 128 + (((4 * h + (lane >> 4)) ^ swz<64>(row)) * 16);
    }
  // transposed reads (dB product): k-slot 8g + jj = row 4g + jj (jj < 4) / 16 + 4g + jj - 4
  const int g4 = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  int toffs[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) toffs[nb] = toff<64>(4 * g4 + qq, 2 * nb + (pp >> 1)) + 8 * (pp & 1);
  auto tr4 = [](const char* a) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a);
  };

  f32x4 wacc[DY_G][2][JT];
  f32x4 bacc[JT][4];
#pragma unroll
  for (int t = 0; t < JT; ++t)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) bacc[t][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int g = 0; g < DY_G; ++g) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int t = 0; t < JT; ++t) wacc[g][q][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (g >= ng) continue;
    // slot g landed: only the slots issued after it (at most DY_NR - 2) stay in flight
    const int younger = min(DY_NR - 2, ng - 1 - g);
    if (younger >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const char* sl = smem + wave * (DY_NR * 4096) + (g % DY_NR) * 4096;
    s16x8 xf[2][2];
#pragma unroll
    for (int q = 0; q < 2 && (MODE & 1); ++q)
#pragma unroll
      for (int h = 0; h < 2; ++h) xf[q][h] = *(const s16x8*)(sl + roff[q][h]);
    s16x8 yb[4];
#pragma unroll
    for (int nb = 0; nb < 4 && (MODE & 2); ++nb) {
      const s16x4 b0 = tr4(sl + toffs[nb]), b1 = tr4(sl + toffs[nb] + 16 * 128);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        yb[nb][j] = b0[j];
        yb[nb][4 + j] = b1[j];
      }
    }
    // u pieces of this group's rows in the k-slot order: [piece][t]
    s16x8 up[3][JT];
#pragma unroll
    for (int t = 0; t < JT && (MODE & 2); ++t) {
      const float* ur = ut + (16 * t + (lane & 15)) * DY_UPAD + 32 * g + 4 * g4;
      const f32x4 lo4 = *(const f32x4*)ur, hi4 = *(const f32x4*)(ur + 16);
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const float v = jj < 4 ? lo4[jj] : hi4[jj - 4];
        const bf16_t a = f2bf(v);
        const float r1 = v - bf2f(a);
        const bf16_t b = f2bf(r1);
        const bf16_t c = f2bf(r1 - bf2f(b));
        up[0][t][jj] = (short)a;
        up[1][t][jj] = (short)b;
        up[2][t][jj] = (short)c;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot g read: its ring slot may be refilled
    if (g + DY_NR - 1 < ng) dma(g + DY_NR - 1);
#pragma unroll
    for (int h = 0; h < 2 && (MODE & 1); ++h)
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int t = 0; t < JT; ++t)
#pragma unroll
          for (int q = 0; q < 2; ++q)
            wacc[g][q][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[q][h], bp[h][p * JT + t], wacc[g][q][t], 0, 0, 0);
#pragma unroll
    for (int p = 0; p < 3 && (MODE & 2); ++p)
#pragma unroll
      for (int t = 0; t < JT; ++t)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          bacc[t][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(up[p][t], yb[nb], bacc[t][nb], 0, 0, 0);
  }
  // dB partial: C[j][n] -> part_b[rs][n][j], lane: n = c0 + 16 nb + (lane & 15), j = 16t + 4 g4 + 0..3
#pragma unroll
  for (int t = 0; t < JT && (MODE & 2); ++t)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const int n = c0 + 16 * nb + (lane & 15);
      *(f32x4*)(part_b + ((int64_t)rs * N + n) * RP + j0 + 16 * t + 4 * g4) = bacc[t][nb];
    }
  if constexpr (!(MODE & 1)) return;
  // w partial: the 8 waves' [j][32G rows] sums through LDS (the ring is free once all waves are
  // past their last slot; a C fragment's 4 values are 4 consecutive rows of one j: one 16-B write),
  // then one column-split partial part_w[cs][j][m] per row quad (16-B reads and stores). The
  // partials overlay the ring and, for 32-wide slices, the head of u^T (read for the last time
  // before the barrier)
  __syncthreads();
  constexpr int WROW = DY_G * 32 + 4;  // floats per (wave, j) row; +4 spreads the banks
  float* part = (float*)smem;
  static_assert(8 * SW * WROW * 4 <= RING + UT, "w partials fit the ring and the u^T area");
#pragma unroll
  for (int g = 0; g < DY_G; ++g)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int t = 0; t < JT; ++t)
        *(f32x4*)(part + (wave * SW + 16 * t + (lane & 15)) * WROW + 32 * g + 16 * q + 4 * g4) = wacc[g][q][t];
  __syncthreads();
  for (int e = tid; e < SW * DY_G * 8; e += 512) {  // (j, row quad)
    const int j = e / (DY_G * 8), r4 = 4 * (e % (DY_G * 8));
    if (mb + r4 >= M) continue;  // M % 32 == 0: a quad is all in or all out
    f32x4 sum = *(const f32x4*)(part + j * WROW + r4);
#pragma unroll
    for (int w = 1; w < 8; ++w) {
      const f32x4 v = *(const f32x4*)(part + (w * SW + j) * WROW + r4);
      sum[0] += v[0]; sum[1] += v[1]; sum[2] += v[2]; sum[3] += v[3];
    }
    *(f32x4*)(part_w + ((int64_t)cs * RP + j0 + j) * M + mb + r4) = sum;
  }
#elif LTX_DY_BODY == 2
  constexpr int RP = R >= 16 ? R : 16;
  if ((int)DY_BX < nwb) {
    // thread (j quad q, row m), m fastest (the partial reads coalesce): w[m][4q..4q+3],
    // split[m][4q..] = split[m][R + 4q..] = hi, split[m][2R + 4q..] = lo, and the zero padding
    // columns 3R + 4q + kR < K2 (the R / 4 quads of a row cover 3R .. K2 between them)
    constexpr int NQ = R / 4;
    const int64_t e = (int64_t)DY_BX * 256 + threadIdx.x;
    if (e >= (int64_t)M * NQ) return;
    const int q = (int)(e / M), m = (int)(e % M);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int c = 0;
    for (; c + 4 <= CS; c += 4) {  // 16 loads in flight, summed in split order
      float t[4][4];
#pragma unroll
      for (int cc = 0; cc < 4; ++cc)
#pragma unroll
        for (int k = 0; k < 4; ++k) t[cc][k] = part_w[((int64_t)(c + cc) * RP + 4 * q + k) * M + m];
#pragma unroll
      for (int cc = 0; cc < 4; ++cc)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += t[cc][k];
    }
    for (; c < CS; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += part_w[((int64_t)c * RP + 4 * q + k) * M + m];
    f32x4 wv;
    uint32_t hi[2], lo[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) wv[k] = v[k] * alpha;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const bf16_t h0 = f2bf(wv[2 * k]), h1 = f2bf(wv[2 * k + 1]);
      hi[k] = (uint32_t)h0 | ((uint32_t)h1 << 16);
      lo[k] = (uint32_t)f2bf(wv[2 * k] - bf2f(h0)) | ((uint32_t)f2bf(wv[2 * k + 1] - bf2f(h1)) << 16);
    }
    *(f32x4*)(w + (int64_t)m * ldw_out + 4 * q) = wv;
    if (split == nullptr) return;
    bf16_t* sr = split + (int64_t)m * lds;
    *(u32x2*)(sr + 4 * q) = (u32x2){hi[0], hi[1]};
    *(u32x2*)(sr + R + 4 * q) = (u32x2){hi[0], hi[1]};
    *(u32x2*)(sr + 2 * R + 4 * q) = (u32x2){lo[0], lo[1]};
    for (int c = 3 * R + 4 * q; c < K2; c += R) *(u32x2*)(sr + c) = (u32x2){0u, 0u};
    return;
  }
  __shared__ float red[4][64];
  const int blk = (int)DY_BX - nwb;
  if (blk < nbb) finish_rows<R>(part_b, RS, N, alpha, dw, on, oj, accumulate, blk, red);
  else finish_rows<R>(part_a, RS, Na, alpha_a, dwa, ona, oja, acc_a, blk - nbb, red);
#elif LTX_DY_BODY == 3
  constexpr int RP = R >= 16 ? R : 16;
  // ranks above 16: 16-wide rank slices, one per DY_BY of the same launch (a wave keeps the
  // pieces of its slice for all CH chunks in registers: 24 CH VGPRs per 16 columns); j0 = slice origin
  constexpr int SW = 16;
  constexpr int RW = R < SW ? R : SW;
  constexpr int JT = SW / 16;
  constexpr int NF = 3 * JT;
  constexpr int NS = RG * CH;  // slots per wave
  constexpr int RING = 8 * NR * 4096;
  constexpr int PROW = RG * 32 + 4;  // floats per (wave, j) partial row; +4 spreads the banks
  static_assert(lora_rank_ok(R), "rank 8, 16, 32, 64 or 128");
  static_assert(8 * SW * PROW * 4 <= RING, "wave partials fit the ring");
  const int j0 = DY_BY * SW;
  __shared__ __attribute__((aligned(16))) char smem[RING];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = wave * 64 * CH;
  const int mb = DY_BX * RG * 32;
  const int ng = min(RG, (M - mb) / 32);  // M % 32 == 0
  const int ns = ng * CH;

  uint32_t yo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 8 * i + (lane >> 3);
    yo[i] = (uint32_t)(row * ldx + (((lane & 7) ^ swz<64>(row)) * 8)) * 2;
  }
  const uint32_t lring = lds_u32(smem + wave * (NR * 4096));
  auto dma = [&](int s) {  // slot s = (group s / CH, chunk s % CH)
    const char* sb = (const char*)(x + (int64_t)(mb + 32 * (s / CH)) * ldx + c0 + 64 * (s % CH));
    const uint32_t l = lring + (s % NR) * 4096;
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %5\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %5\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(yo[0]), "v"(yo[1]), "v"(yo[2]), "v"(yo[3]), "s"(sb), "s"(l)
        : "memory", "scc");
  };
  // the ring's first slots go out first; the pieces' loads overlap them, then everything retires
  // (hipcc's own waits for the pieces are counted without the asm DMA)
  for (int s = 0; s < NR - 1; ++s)
    if (s < ns) dma(s);
  s16x8 bp[CH][2][NF];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int t = 0; t < JT; ++t) {
        const bf16_t* src = w3 + (int64_t)(p * RP + j0 + t * 16 + (lane & 15)) * ldw + c0 + 64 * c + (lane >> 4) * 8;
        bp[c][0][p * JT + t] = *(const s16x8*)src;
        bp[c][1][p * JT + t] = *(const s16x8*)(src + 32);
      }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int f = 0; f < NF; ++f) asm volatile("" : "+v"(bp[c][h][f]));

  int roff[2][2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = 16 * q + (lane & 15);
      roff[q][h] = row * 128 + (((4 * h + (lane >> 4)) ^ swz<64>(row)) * 16);
    }
  f32x4 acc[RG][2][JT];
#pragma unroll
  for (int g = 0; g < RG; ++g)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int t = 0; t < JT; ++t) acc[g][q][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s >= ns) break;
    const int g = s / CH, c = s % CH;
    const int younger = min(NR - 2, ns - 1 - s);  // slots issued after s
    if (younger >= 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (younger == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const char* sl = smem + wave * (NR * 4096) + (s % NR) * 4096;
    s16x8 xf[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int h = 0; h < 2; ++h) xf[q][h] = *(const s16x8*)(sl + roff[q][h]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot s read: its ring slot may be refilled
    if (s + NR - 1 < ns) dma(s + NR - 1);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int t = 0; t < JT; ++t)
#pragma unroll
          for (int q = 0; q < 2; ++q)
            acc[g][q][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[q][h], bp[c][h][p * JT + t], acc[g][q][t], 0, 0, 0);
  }
  // the 8 wave partials [j][rows] through LDS (the ring is free once every wave is past its last
  // slot), then thread (row m, j quad q) sums them in wave order and writes u[m][4q..] and the
  // [hi | hi | lo | 0..] split row (as lora_dy_finish_kernel)
  __syncthreads();
  float* part = (float*)smem;
#pragma unroll
  for (int g = 0; g < RG; ++g)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int t = 0; t < JT; ++t)
        *(f32x4*)(part + (wave * SW + 16 * t + (lane & 15)) * PROW + 32 * g + 16 * q + 4 * (lane >> 4)) = acc[g][q][t];
  __syncthreads();
  constexpr int NQ = RW / 4;
  for (int e = tid; e < RG * 32 * NQ; e += 512) {
    const int q = e / (RG * 32), rr = e % (RG * 32), m = mb + rr;
    if (m >= M) continue;
    f32x4 wv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v = part[(4 * q + k) * PROW + rr];
#pragma unroll
      for (int w = 1; w < 8; ++w) v += part[(w * SW + 4 * q + k) * PROW + rr];
      wv[k] = v * alpha;
    }
    const int jq = j0 + 4 * q;  // the quad's first column in the whole rank
    *(f32x4*)(out + (int64_t)m * ldo + jq) = wv;
    if (split == nullptr) continue;
    uint32_t hi[2], lo[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const bf16_t h0 = f2bf(wv[2 * k]), h1 = f2bf(wv[2 * k + 1]);
      hi[k] = (uint32_t)h0 | ((uint32_t)h1 << 16);
      lo[k] = (uint32_t)f2bf(wv[2 * k] - bf2f(h0)) | ((uint32_t)f2bf(wv[2 * k + 1] - bf2f(h1)) << 16);
    }
    bf16_t* sr = split + (int64_t)m * lds;
    *(u32x2*)(sr + jq) = (u32x2){hi[0], hi[1]};
    *(u32x2*)(sr + R + jq) = (u32x2){hi[0], hi[1]};
    *(u32x2*)(sr + 2 * R + jq) = (u32x2){lo[0], lo[1]};
    for (int cc = 3 * R + jq; cc < K2; cc += R) *(u32x2*)(sr + cc) = (u32x2){0u, 0u};
  }
#else
#error "LTX_DY_BODY must be 1, 2 or 3"
#endif
