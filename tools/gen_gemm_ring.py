"""Generates video-generation-for-human-avatars_amd/csrc/gemm_ring_body.h: the hand-scheduled K loop of
gemm_ring_kernel (gemm_ring.h) as inline-asm strings, one per m-fragment count MF (7: 224-row
tiles, 8: 256-row tiles). The emitted loop is body3() (+ ext_body2() for the K extension); body()
below (a 4-slot ring of 32-deep half-tiles, 64-B LDS rows) and body2() (2 x 64-deep stages, one
mid-tile barrier) are the variants measured before it and kept for reference: the docstrings of
body2() / body3() describe the adopted layout and schedule, this one the first variant.

Geometry (per workgroup): a BMT x 256 output tile (BMT = 16 * MF * 2), 4 waves at one wave per SIMD,
wave w owns rows (w >> 1) * 16 * MF .. and columns (w & 1) * 128 .. as MF x 8 fragments of
v_mfma_f32_16x16x32_bf16 (accumulators in AGPRs). K is walked in 32-deep half-steps j = 0 .. H - 1.
LDS is a ring of S = 4 slots, one half-step each: [X: BMT rows x 64 B][W: 256 rows x 64 B], 16-B
chunk c of row r stored at c ^ g((r >> 2) & 3), g = {0, 2, 3, 1} (conflict-free fragment reads; the
LDS-DMA writes lane-linear, so the same XOR is applied to the per-lane SOURCE chunk).

Phase P(j) (56 or 64 MFMAs on the fragments F(j) in registers):
  s_waitcnt vmcnt(16) lgkmcnt(0); s_barrier     -- every wave's DMA of half-step j + 1 has landed
                                                   and every wave has finished reading slot j % S
  MFMAs on F(j); between them: ds_read F(j + 1) from slot (j + 1) % S (first MF + 8 gaps),
  LDS-DMA of half-step j + S into slot j % S (8 pieces of 1 KiB per wave, one every 5 MFMAs, M0
  written one MFMA ahead of its piece: the M0 -> LDS-DMA wait state).
The DMA of half-step j + S therefore has two whole phases (~1800 cycles) to land before the wait at
the start of P(j + S - 1). F(j) / F(j + 1) alternate between two register sets; the loop body is
the 4 phases of one ring turn (2 K-tiles), and a last turn without DMA drains the ring with
vmcnt(16) / (8) / (0). Requires H % 4 == 0 (K % 128 == 0) and H >= 4.

Operands (see gemm_ring.hip): %0 .. : accumulators acc[i * MF + jm] ("+a", i = n-fragment 0..7,
jm = m-fragment), then the fragment registers ("=&v", set 0 W[0..7] X[0..MF-1], set 1 likewise),
then named operands.
"""
import os
import sys

S = 4
G = [0, 2, 3, 1]


def body(MF):
    NA = 8 * MF                  # accumulator tuples
    NFR = 8 + MF                 # fragment registers per set
    SLOT = MF * 32 * 64 + 256 * 64
    XREG = 0                     # X region offset inside a slot
    WREG = MF * 32 * 64
    fr = lambda st, k: "%" + str(NA + st * NFR + k)   # k < 8: W frag k; k >= 8: X frag k - 8
    acc = lambda i, jm: "%" + str(i * MF + jm)
    L = []
    a = L.append

    def reads(st, slot):
        # 8 W fragments then MF X fragments of the half-step in `slot` into register set st
        out = []
        wb = "%[wr0]" if slot < 2 else "%[wr2]"
        xb = "%[xr0]" if slot < 2 else "%[xr2]"
        so = (slot % 2) * SLOT
        for i in range(8):
            out.append(f"ds_read_b128 {fr(st, i)}, {wb} offset:{so + WREG + i * 1024}")
        for jm in range(MF):
            out.append(f"ds_read_b128 {fr(st, 8 + jm)}, {xb} offset:{so + XREG + jm * 1024}")
        return out

    def dmas(slot):
        # 8 pieces of this wave into `slot`: X piece p (p even: X, p odd: W), M0 then the load
        out = []
        for p in range(8):
            srd = "%[xsrd]" if p % 2 == 0 else "%[wsrd]"
            m0 = f"s_add_u32 m0, %[d{p}], {slot * SLOT}"
            ld = f"buffer_load_dwordx4 %[o{p}], {srd}, %[koff] offen lds"
            out.append((m0, ld))
        return out

    def advance():
        return ["s_add_u32 %[koff], %[koff], 64"]

    def phase(p, vm, with_dma, last):
        # ring position p (0..3): computes set p % 2, reads slot (p + 1) % S into the other set
        st = p % 2
        a(f"s_waitcnt vmcnt({vm}) lgkmcnt(0)")
        a("s_barrier")
        rd = [] if last else reads(1 - st, (p + 1) % S)
        dm = dmas(p) if with_dma else []
        mf = [(i, jm) for i in range(8) for jm in range(MF)]
        nm = len(mf)
        # slot plan after MFMA q: the fragment reads in every second gap from the start, the DMA
        # pieces spread evenly over the phase (odd gaps), M0 one gap ahead of its piece
        after = {q: [] for q in range(nm)}
        for k, r in enumerate(rd):
            after[2 * k].append(r)
        if dm:
            step = (nm - 6) // 8
            for k, (m0, ld) in enumerate(dm):
                q = 3 + k * step
                after[q - 1].append(m0)
                after[q].append(ld)
            after[3 + 7 * step + 1].extend(advance())
        for q, (i, jm) in enumerate(mf):
            a(f"v_mfma_f32_16x16x32_bf16 {acc(i, jm)}, {fr(st, i)}, {fr(st, 8 + jm)}, {acc(i, jm)}")
            L.extend(after[q])

    a("s_nop 4")  # SGPR operands fresh from v_readfirstlane -> buffer descriptor / soffset reads
    a("s_mov_b32 %[keep], m0")
    # prologue: half-steps 0..3 into slots 0..3, then F(0)
    for slot in range(S):
        for m0, ld in dmas(slot):
            a(m0)
            a("s_nop 0")
            a(ld)
        L.extend(advance())
    a("s_waitcnt vmcnt(24)")
    a("s_barrier")
    L.extend(reads(0, 0))
    a("s_cmp_eq_u32 %[iters], 0")
    a("s_cbranch_scc1 L_tail_%=")
    a("L_loop_%=:")
    for p in range(S):
        phase(p, 16, True, False)
    a("s_sub_u32 %[iters], %[iters], 1")
    a("s_cmp_eq_u32 %[iters], 0")
    a("s_cbranch_scc0 L_loop_%=")
    a("L_tail_%=:")
    for p, vm in enumerate([16, 8, 0, 0]):
        phase(p, vm, False, p == S - 1)
    a("s_mov_b32 m0, %[keep]")
    a("s_nop 15")
    a("s_nop 15")
    return L


def ext_body(MF, H2):
    """The K extension (the fused LoRA tiles, K2 = 32 * H2 <= 128) after the main loop: its H2
    half-steps go into ring slots 0 .. H2 - 1 in one burst (the main loop's last barrier already
    retired every read of the ring), then fragments + MFMAs per half-step in order -- the same
    accumulation order as gemm_nt_kernel_t, whose extension tiles also come last."""
    NA = 8 * MF
    NFR = 8 + MF
    SLOT = MF * 32 * 64 + 256 * 64
    WREG = MF * 32 * 64
    fr = lambda st, k: "%" + str(NA + st * NFR + k)
    acc = lambda i, jm: "%" + str(i * MF + jm)
    L = []
    a = L.append

    def reads(st, slot):
        out = []
        so = slot * SLOT if slot < 2 else (slot - 2) * SLOT
        wb = "%[wr0]" if slot < 2 else "%[wr2]"
        xb = "%[xr0]" if slot < 2 else "%[xr2]"
        for i in range(8):
            out.append(f"ds_read_b128 {fr(st, i)}, {wb} offset:{so + WREG + i * 1024}")
        for jm in range(MF):
            out.append(f"ds_read_b128 {fr(st, 8 + jm)}, {xb} offset:{so + jm * 1024}")
        return out

    a("s_nop 4")
    a("s_mov_b32 %[keep], m0")
    for h in range(H2):
        for p in range(8):
            srd = "%[xsrd]" if p % 2 == 0 else "%[wsrd]"
            a(f"s_add_u32 m0, %[d{p}], {h * SLOT}")
            a("s_nop 0")
            a(f"buffer_load_dwordx4 %[o{p}], {srd}, %[koff] offen lds")
        a("s_add_u32 %[koff], %[koff], 64")
    a("s_waitcnt vmcnt(0)")
    a("s_barrier")
    L.extend(reads(0, 0))
    for h in range(H2):
        st = h % 2
        a("s_waitcnt lgkmcnt(0)")
        rd = reads(1 - st, h + 1) if h + 1 < H2 else []
        mf = [(i, jm) for i in range(8) for jm in range(MF)]
        for q, (i, jm) in enumerate(mf):
            a(f"v_mfma_f32_16x16x32_bf16 {acc(i, jm)}, {fr(st, i)}, {fr(st, 8 + jm)}, {acc(i, jm)}")
            if q % 2 == 0 and q // 2 < len(rd):
                a(rd[q // 2])
    a("s_mov_b32 m0, %[keep]")
    a("s_nop 15")
    a("s_nop 15")
    return L


def body2(MF):
    """Variant 2 of the K loop (gemm_ring2_kernel): LDS stages of whole 64-deep K-tiles in 128-B
    rows (2 stages, 120 / 128 KiB), so every LDS-DMA instruction moves 8 full 128-B lines (the ring's
    32-deep slots split every line over two instructions). K-tile t (stage t % 2) is two phases:
      P0(t): MFMAs on F0 = (t, k-half 0); ds_read (t, k-half 1) -> F1;
      s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier   -- tile t+1 landed (its DMA ran during P1(t-1)),
                                                    every wave done reading stage t % 2
      P1(t): MFMAs on F1; ds_read (t+1, k-half 0) -> F0; LDS-DMA of tile t+2 into stage t % 2,
             one piece per ~3.6 MFMAs.
    One barrier per K-tile; the DMA of tile t+2 has P0(t+1) (~900 cycles) behind its last piece.
    Chunk c of row r at c ^ (r & 7) (gemm_nt_kernel_t's swizzle, conflict-free fragment reads)."""
    NA = 8 * MF
    NFR = 8 + MF
    XT = MF * 32 * 128            # X region of a stage
    ST = XT + 256 * 128           # stage bytes
    NP = MF + 8                   # DMA pieces per wave per K-tile (X: MF, W: 8)
    fr = lambda st, k: "%" + str(NA + st * NFR + k)
    acc = lambda i, jm: "%" + str(i * MF + jm)
    L = []
    a = L.append

    def reads(st, stage, kh):
        out = []
        for i in range(8):
            out.append(f"ds_read_b128 {fr(st, i)}, %[wr{stage}{kh}] offset:{i * 2048}")
        for jm in range(MF):
            out.append(f"ds_read_b128 {fr(st, 8 + jm)}, %[xr{stage}{kh}] offset:{jm * 2048}")
        return out

    def dmas(stage):
        out = []
        for i in range(MF):  # X piece i of this wave: rows (w + 4i) * 8 ..
            out.append((f"s_add_u32 m0, %[mx], {stage * ST + i * 4096}",
                        f"buffer_load_dwordx4 %[ox{i}], %[xsrd], %[koff] offen lds"))
        for i in range(8):
            out.append((f"s_add_u32 m0, %[mw], {stage * ST + i * 4096}",
                        f"buffer_load_dwordx4 %[ow{i}], %[wsrd], %[koff] offen lds"))
        # interleave X / W pieces
        xs, ws = out[:MF], out[MF:]
        mixed = []
        for k in range(max(len(xs), len(ws))):
            if k < len(ws):
                mixed.append(ws[k])
            if k < len(xs):
                mixed.append(xs[k])
        return mixed

    mf = [(i, jm) for i in range(8) for jm in range(MF)]
    nm = len(mf)

    def phase(st, rd, dm):
        after = {q: [] for q in range(nm)}
        for k, r in enumerate(rd):
            after[2 * k].append(r)
        if dm:
            qs = [1 + (k * (nm - 3)) // len(dm) for k in range(len(dm))]
            for (m0, ld), q in zip(dm, qs):
                after[q - 1].append(m0)
                after[q].append(ld)
            after[min(qs[-1] + 1, nm - 1)].append("s_add_u32 %[koff], %[koff], 128")
        for q, (i, jm) in enumerate(mf):
            a(f"v_mfma_f32_16x16x32_bf16 {acc(i, jm)}, {fr(st, i)}, {fr(st, 8 + jm)}, {acc(i, jm)}")
            L.extend(after[q])

    def tile(stage, with_dma, last):
        a("s_waitcnt lgkmcnt(0)")
        phase(0, reads(1, stage, 1), [])
        a("s_waitcnt vmcnt(0) lgkmcnt(0)")
        a("s_barrier")
        phase(1, [] if last else reads(0, 1 - stage, 0), dmas(stage) if with_dma else [])

    a("s_nop 4")
    a("s_mov_b32 %[keep], m0")
    for stage in range(2):  # tiles 0 and 1
        for m0, ld in dmas(stage):
            a(m0)
            a("s_nop 0")
            a(ld)
        a("s_add_u32 %[koff], %[koff], 128")
    a(f"s_waitcnt vmcnt({NP})")
    a("s_barrier")
    L.extend(reads(0, 0, 0))
    a("s_cmp_eq_u32 %[iters], 0")
    a("s_cbranch_scc1 L_tail_%=")
    a("L_loop_%=:")
    tile(0, True, False)
    tile(1, True, False)
    a("s_sub_u32 %[iters], %[iters], 1")
    a("s_cmp_eq_u32 %[iters], 0")
    a("s_cbranch_scc0 L_loop_%=")
    a("L_tail_%=:")
    tile(0, False, False)
    tile(1, False, True)
    a("s_mov_b32 m0, %[keep]")
    a("s_nop 15")
    a("s_nop 15")
    return L


def body3(MF, marked=False):
    """marked: the same stream cut into the pieces main() emits as macros ("#NAME" lines ahead of each:
    HEAD, the two loop tiles LT0 / LT1, LOOPEND, the two tail tiles TAIL0 / TAIL1, END), the loop
    tiles' DMA operands as tokens (@W@ / @X@ offsets, @WS@ / @XS@ buffers) that main() turns into
    macro parameters, so that the long K extensions reuse the loop tiles on their own operands.

    Variant 3 (gemm_ring2_kernel's LDS layout and operands, LTX_GEMM_RING=3): the DMA of the
    tile after next gets ~1.5x the latency slack. Each K-tile t (stage s = t % 2) is three segments:
      S1 (k-half 0, all MFMAs): ds_read (t, k-half 1) -> F1;
         s_waitcnt lgkmcnt(0); s_barrier     -- M1: every wave done reading stage s
      S2 (first half of k-half 1): the W pieces of tile t+2 into stage s (weights: L2 / HBM, first);
         s_waitcnt vmcnt(8); s_barrier       -- M2: tile t+1 landed (only the 8 W pieces just
                                                issued may be in flight)
      S3 (second half of k-half 1): ds_read (t+1, k-half 0) -> F0 beside the X pieces of tile t+2.
    A piece issued in S2(t) / S3(t) is waited for at M2(t+1): >= S1 + S2 of the next tile
    (~84 MFMAs, ~1350 cycles) behind it, against ~56 MFMAs in variant 2."""
    NA = 8 * MF
    NFR = 8 + MF
    XT = MF * 32 * 128
    ST = XT + 256 * 128
    NP = MF + 8
    fr = lambda st, k: "%" + str(NA + st * NFR + k)
    acc = lambda i, jm: "%" + str(i * MF + jm)
    L = []
    a = L.append

    def reads(st, stage, kh):
        out = []
        for i in range(8):
            out.append(f"ds_read_b128 {fr(st, i)}, %[wr{stage}{kh}] offset:{i * 2048}")
        for jm in range(MF):
            out.append(f"ds_read_b128 {fr(st, 8 + jm)}, %[xr{stage}{kh}] offset:{jm * 2048}")
        return out

    def wdma(stage, tok=False):
        o, srd = ("@W@", "@WS@") if tok else ("ow", "wsrd")
        return [(f"s_add_u32 m0, %[mw], {stage * ST + i * 4096}",
                 f"buffer_load_dwordx4 %[{o}{i}], %[{srd}], %[koff] offen lds") for i in range(8)]

    def xdma(stage, tok=False):
        o, srd = ("@X@", "@XS@") if tok else ("ox", "xsrd")
        return [(f"s_add_u32 m0, %[mx], {stage * ST + i * 4096}",
                 f"buffer_load_dwordx4 %[{o}{i}], %[{srd}], %[koff] offen lds") for i in range(MF)]

    mf = [(i, jm) for i in range(8) for jm in range(MF)]
    nm = len(mf)
    half = nm // 2

    def run(st, qs, rd, dm, koff_after=False):
        """MFMAs qs (indices into mf) on set st; reads rd in even gaps from the first, DMA pieces dm
        in the odd gaps spread over the segment (M0 one gap ahead)"""
        n = len(qs)
        after = {q: [] for q in range(n)}
        for k, r in enumerate(rd):
            g = 2 * k if 2 * k < n else n - 1 - (2 * k - n)
            after[g].append(r)
        if dm:
            step = max(2, (n - 2) // len(dm))
            for k, (m0, ld) in enumerate(dm):
                q = min(1 + k * step, n - 1)
                after[q - 1].append(m0)
                after[q].append(ld)
        if koff_after:
            after[n - 1].append("s_add_u32 %[koff], %[koff], 128")
        for g, q in enumerate(qs):
            i, jm = mf[q]
            a(f"v_mfma_f32_16x16x32_bf16 {acc(i, jm)}, {fr(st, i)}, {fr(st, 8 + jm)}, {acc(i, jm)}")
            L.extend(after[g])

    def tile(stage, with_dma, last):
        a("s_waitcnt lgkmcnt(0)")
        run(0, range(nm), reads(1, stage, 1), [])
        a("s_waitcnt lgkmcnt(0)")
        a("s_barrier")
        run(1, range(half), [], wdma(stage, marked) if with_dma else [])
        a("s_waitcnt vmcnt(8)" if with_dma else "s_waitcnt vmcnt(0)")
        a("s_barrier")
        run(1, range(half, nm), [] if last else reads(0, 1 - stage, 0), xdma(stage, marked) if with_dma else [],
            koff_after=with_dma)

    def mark(name):
        if marked:
            a("#" + name)

    mark("HEAD")
    a("s_nop 4")
    a("s_mov_b32 %[keep], m0")
    for stage in range(2):  # tiles 0 and 1
        for m0, ld in wdma(stage) + xdma(stage):
            a(m0)
            a("s_nop 0")
            a(ld)
        a("s_add_u32 %[koff], %[koff], 128")
    a(f"s_waitcnt vmcnt({NP})")
    a("s_barrier")
    L.extend(reads(0, 0, 0))
    a("s_cmp_eq_u32 %[iters], 0")
    a("s_cbranch_scc1 L_tail_%=")
    a("L_loop_%=:")
    mark("LT0")
    tile(0, True, False)
    mark("LT1")
    tile(1, True, False)
    mark("LOOPEND")
    a("s_sub_u32 %[iters], %[iters], 1")
    a("s_cmp_eq_u32 %[iters], 0")
    a("s_cbranch_scc0 L_loop_%=")
    a("L_tail_%=:")
    mark("TAIL0")
    tile(0, False, False)
    mark("TAIL1")
    tile(1, False, True)
    mark("END")
    a("s_mov_b32 m0, %[keep]")
    a("s_nop 15")
    a("s_nop 15")
    return L


# The long K extensions of LoRA ranks 64 / 128 (K2 = 192 / 384: 3 / 6 tiles) continue the main loop's
# pipeline instead of following it in bursts (ext_body2: each burst exposes a DMA latency, measured
# slower than gemm_nt_kernel_t at these lengths): after the loop, %[koff]
# restarts at 0 and loop-tile pairs on the extension's operands (XD) run in place of the tail -- the
# main K's last two tiles issue the DMA of extension tiles 0 and 1, extension tile e that of tile
# e + 2 -- then the ordinary tail tiles finish. No new instruction text: the pieces of body3(marked).
#   K2 = 384: XD XD XD TAIL0 TAIL1 (tiles T-2, T-1, e0 .. e3 with DMA; e4, e5 without)
#   K2 = 192: XD XD TAIL0          (e1's DMA asks for a tile past K2: the buffer bounds make it zeros
#             or the next row's bytes, into a stage nobody computes on again; e2 = TAIL0 prefetches
#             that stage's first fragments into dead registers, retired by the added lgkmcnt(0))
# Same tiles, same k-half order as gemm_nt_kernel_t: bitwise its sums. The closing barrier keeps the
# epilogue's C image off a slower wave's last reads (ext_body2()).
MAIN_OPS = '("ow", "ox", "wsrd", "xsrd")'
EXT_OPS = '("ew", "ex", "w2srd", "x2srd")'
LONG_EXT = {3: ["XD", "XD", "TAIL0", '"s_waitcnt lgkmcnt(0)\\n\\t"'], 6: ["XD", "XD", "XD", "TAIL0", "TAIL1"]}


def emit_pieces(txt, define, MF):
    """body3(MF, marked) as the macros LTX_RING_<PIECE>_MF<MF> (LT0 / LT1 take the DMA operand names),
    LTX_RING_BODY_MF<MF> composed of them (the same string as before) and the long extensions."""
    pieces, name = {}, None
    for l in body3(MF, marked=True):
        if l.startswith("#"):
            name = l[1:]
            pieces[name] = []
        else:
            pieces[name].append(l)
    flat = [l for n in pieces for l in pieces[n]]
    plain = lambda l: l.replace("@W@", "ow").replace("@X@", "ox").replace("@WS@", "wsrd").replace("@XS@", "xsrd")
    assert [plain(l) for l in flat] == body3(MF)
    m = lambda n: f"LTX_RING_{n}_MF{MF}"
    for n, lines in pieces.items():
        define(txt, m(n) + ("(W, X, WS, XS)" if n in ("LT0", "LT1") else ""), lines)
    loop = f"{m('HEAD')} {m('LT0')}{MAIN_OPS} {m('LT1')}{MAIN_OPS} {m('LOOPEND')}"
    txt.append(f"#define LTX_RING_BODY_MF{MF} {loop} {m('TAIL0')} {m('TAIL1')} {m('END')}\n")
    txt.append(f"#define {m('XD')} {m('LT0')}{EXT_OPS} {m('LT1')}{EXT_OPS}\n")
    for T2, seq in LONG_EXT.items():
        body = " ".join(s if s.startswith('"') else m(s) for s in seq)
        txt.append(f'#define LTX_RING_BODY_EXT{T2}_MF{MF} {loop} "s_mov_b32 %[koff], 0\\n\\t" {body} '
                   f'"s_barrier\\n\\t" {m("END")}\n')


def ext_body2(MF, T2):
    """The K extension (LoRA tiles, K2 = 64 * T2, T2 <= 2) for gemm_ring_kernel's layout, appended
    to body3() in the SAME asm statement (one asm statement per kernel: a second one with the same
    accumulator operands made hipcc copy and spill the 224 / 256 AGPRs around it). Every read of both
    stages retired at the main loop's last barrier, so the T2 extension tiles go into stages
    0 .. T2 - 1 in one burst (operands ex*/ew*/x2srd/w2srd: the extension's own offsets and
    buffers), then k-half by k-half as the main loop (the accumulation order of gemm_nt_kernel_t,
    whose extension tiles also come last). A closing barrier keeps the epilogue's C image (which
    overlays stage 0) from landing while a slower wave still reads the last k-half."""
    NA = 8 * MF
    NFR = 8 + MF
    XT = MF * 32 * 128
    ST = XT + 256 * 128
    fr = lambda st, k: "%" + str(NA + st * NFR + k)
    acc = lambda i, jm: "%" + str(i * MF + jm)
    L = []
    a = L.append

    def reads(st, stage, kh):
        out = []
        for i in range(8):
            out.append(f"ds_read_b128 {fr(st, i)}, %[wr{stage}{kh}] offset:{i * 2048}")
        for jm in range(MF):
            out.append(f"ds_read_b128 {fr(st, 8 + jm)}, %[xr{stage}{kh}] offset:{jm * 2048}")
        return out

    a("s_mov_b32 %[koff], 0")
    for stage in range(T2):
        for i in range(8):
            a(f"s_add_u32 m0, %[mw], {stage * ST + i * 4096}")
            a("s_nop 0")
            a(f"buffer_load_dwordx4 %[ew{i}], %[w2srd], %[koff] offen lds")
        for i in range(MF):
            a(f"s_add_u32 m0, %[mx], {stage * ST + i * 4096}")
            a("s_nop 0")
            a(f"buffer_load_dwordx4 %[ex{i}], %[x2srd], %[koff] offen lds")
        a("s_add_u32 %[koff], %[koff], 128")
    a("s_waitcnt vmcnt(0)")
    a("s_barrier")
    L.extend(reads(0, 0, 0))
    halves = [(stage, kh) for stage in range(T2) for kh in range(2)]
    mf = [(i, jm) for i in range(8) for jm in range(MF)]
    for h, (stage, kh) in enumerate(halves):
        st = h % 2
        a("s_waitcnt lgkmcnt(0)")
        rd = reads(1 - st, *halves[h + 1]) if h + 1 < len(halves) else []
        for q, (i, jm) in enumerate(mf):
            a(f"v_mfma_f32_16x16x32_bf16 {acc(i, jm)}, {fr(st, i)}, {fr(st, 8 + jm)}, {acc(i, jm)}")
            if q % 2 == 0 and q // 2 < len(rd):
                a(rd[q // 2])
    a("s_barrier")
    a("s_mov_b32 m0, %[keep]")
    a("s_nop 15")
    a("s_nop 15")
    return L


def body4(MF):
    """The K loop with THREE X stages and two W stages (gemm_ring_kernel, round 4): the X pieces of
    tile t+3 (not t+2) go out in S3(t) into tile t's X stage, so an X piece has ~2 K-tiles to land
    instead of ~1; W keeps two stages (W pieces of t+2 in S2(t)). LDS: X stages 3 x 32 MF x 128 B,
    then W stages 2 x 256 x 128 B (MF = 8: exactly 160 KiB). Segments and reads as body3(); X
    stage t % 3, W stage t % 2, so the loop body is 6 K-tiles (period lcm(2, 3)); the last
    R = T - 6 G tiles (R in 2, 4, 6, 8 for even T; G = floor((T - 3) / 6) loop passes, %[iters])
    are one of four tails, chosen at run time, whose DMA and waits stop at tile T - 1.
    %[koff] = byte offset of tile t+2 during tile t (W(t+2)), %[koffx] = koff + 128 (X(t+3)): two
    SGPRs, since an LDS-DMA instruction's immediate offset moves its LDS destination too.
    Every accumulator takes its K in the same 32-deep steps in the same order as body3()."""
    NA = 8 * MF
    NFR = 8 + MF
    XT = MF * 32 * 128
    WT = 256 * 128
    NP = MF + 8
    fr = lambda st, k: "%" + str(NA + st * NFR + k)
    acc = lambda i, jm: "%" + str(i * MF + jm)
    L = []
    a = L.append

    def reads(st, xs, ws, kh):
        out = []
        for i in range(8):
            out.append(f"ds_read_b128 {fr(st, i)}, %[wr{ws}{kh}] offset:{i * 2048}")
        for jm in range(MF):
            out.append(f"ds_read_b128 {fr(st, 8 + jm)}, %[xr{xs}{kh}] offset:{jm * 2048}")
        return out

    def wdma(ws, ko="koff"):
        return [(f"s_add_u32 m0, %[mw], {ws * WT + i * 4096}",
                 f"buffer_load_dwordx4 %[ow{i}], %[wsrd], %[{ko}] offen lds") for i in range(8)]

    def xdma(xs, ko="koffx"):
        return [(f"s_add_u32 m0, %[mx], {xs * XT + i * 4096}",
                 f"buffer_load_dwordx4 %[ox{i}], %[xsrd], %[{ko}] offen lds") for i in range(MF)]

    mf = [(i, jm) for i in range(8) for jm in range(MF)]
    nm = len(mf)
    half = nm // 2

    def run(st, qs, rd, dm, koff_after=False):
        n = len(qs)
        after = {q: [] for q in range(n)}
        for k, r in enumerate(rd):
            g = 2 * k if 2 * k < n else n - 1 - (2 * k - n)
            after[g].append(r)
        if dm:
            step = max(2, (n - 2) // len(dm))
            for k, (m0, ld) in enumerate(dm):
                q = min(1 + k * step, n - 1)
                after[q - 1].append(m0)
                after[q].append(ld)
        if koff_after:
            after[n - 1].append("s_add_u32 %[koff], %[koff], 128")
            after[n - 1].append("s_add_u32 %[koffx], %[koffx], 128")
        for g, q in enumerate(qs):
            i, jm = mf[q]
            a(f"v_mfma_f32_16x16x32_bf16 {acc(i, jm)}, {fr(st, i)}, {fr(st, 8 + jm)}, {acc(i, jm)}")
            L.extend(after[g])

    def tile(t, T):
        """K-tile with global index t of T (t, T may be symbolic-relative: only t % 6 and the
        distances to T matter); DMA W(t+2) if t+2 < T, X(t+3) if t+3 < T"""
        xs, ws = t % 3, t % 2
        w_ok, x_ok, nxt = t + 2 < T, t + 3 < T, t + 1 < T
        a("s_waitcnt lgkmcnt(0)")
        run(0, range(nm), reads(1, xs, ws, 1), [])
        a("s_waitcnt lgkmcnt(0)")
        a("s_barrier")
        run(1, range(half), [], wdma(ws) if w_ok else [])
        # M2: tile t+1 landed; issued after its W pieces: X(t+2) (S3 of t-1) and W(t+2) (S2 of t)
        newer = (MF + 8) if w_ok else 0
        a(f"s_waitcnt vmcnt({newer})")
        a("s_barrier")
        run(1, range(half, nm), reads(0, (t + 1) % 3, (t + 1) % 2, 0) if nxt else [],
            xdma(xs) if x_ok else [], koff_after=True)

    a("s_nop 4")
    a("s_mov_b32 %[keep], m0")
    # prologue: X0 W0 X1 W1 X2 (koff stepping from 0); then koff = tile 2's offset
    for t in range(2):
        for m0, ld in xdma(t % 3, "koff") + wdma(t % 2):
            a(m0)
            a("s_nop 0")
            a(ld)
        a("s_add_u32 %[koff], %[koff], 128")
    a("s_add_u32 %[koffx], %[koff], 128")
    a("s_cmp_eq_u32 %[tail], 2")  # T == 2: no X2
    a("s_cbranch_scc1 L_p2_%=")
    for m0, ld in xdma(2, "koff"):
        a(m0)
        a("s_nop 0")
        a(ld)
    a(f"s_waitcnt vmcnt({NP + MF})")  # tile 0 landed (X1 W1 X2 may be in flight)
    a("s_branch L_p3_%=")
    a("L_p2_%=:")
    a(f"s_waitcnt vmcnt({NP})")
    a("L_p3_%=:")
    a("s_barrier")
    L.extend(reads(0, 0, 0, 0))
    BIG = 1 << 20  # loop tiles: every DMA condition holds
    a("s_cmp_eq_u32 %[iters], 0")
    a("s_cbranch_scc1 L_tails_%=")
    a("L_loop_%=:")
    for t in range(6):
        tile(t, BIG)
    a("s_sub_u32 %[iters], %[iters], 1")
    a("s_cmp_eq_u32 %[iters], 0")
    a("s_cbranch_scc0 L_loop_%=")
    a("L_tails_%=:")
    # tails: R remaining tiles, starting at a multiple of 6 (stages 0 / 0)
    a("s_cmp_eq_u32 %[tail], 2")
    a("s_cbranch_scc1 L_t2_%=")
    a("s_cmp_eq_u32 %[tail], 4")
    a("s_cbranch_scc1 L_t4_%=")
    a("s_cmp_eq_u32 %[tail], 6")
    a("s_cbranch_scc1 L_t6_%=")
    for R in (8, 6, 4, 2):
        if R != 8:
            a(f"L_t{R}_%=:")
        for t in range(R):
            tile(t, R)
        if R != 2:
            a("s_branch L_end_%=")
    a("L_end_%=:")
    a("s_mov_b32 m0, %[keep]")
    a("s_nop 15")
    a("s_nop 15")
    return L


def ext_body4(MF, T2):
    """The K extension (K2 = 64 T2) for body4()'s LDS layout: ext tile i into X stage i and W
    stage i (all reads of the main loop retired at its last barrier), then k-half by k-half; the
    closing barrier keeps the epilogue's C image off a slower wave's last reads (ext_body2())."""
    NA = 8 * MF
    NFR = 8 + MF
    XT = MF * 32 * 128
    WT = 256 * 128
    fr = lambda st, k: "%" + str(NA + st * NFR + k)
    acc = lambda i, jm: "%" + str(i * MF + jm)
    L = []
    a = L.append

    def reads(st, stage, kh):
        out = []
        for i in range(8):
            out.append(f"ds_read_b128 {fr(st, i)}, %[wr{stage}{kh}] offset:{i * 2048}")
        for jm in range(MF):
            out.append(f"ds_read_b128 {fr(st, 8 + jm)}, %[xr{stage}{kh}] offset:{jm * 2048}")
        return out

    a("s_mov_b32 %[koff], 0")
    for stage in range(T2):
        for i in range(8):
            a(f"s_add_u32 m0, %[mw], {stage * WT + i * 4096}")
            a("s_nop 0")
            a(f"buffer_load_dwordx4 %[ew{i}], %[w2srd], %[koff] offen lds")
        for i in range(MF):
            a(f"s_add_u32 m0, %[mx], {stage * XT + i * 4096}")
            a("s_nop 0")
            a(f"buffer_load_dwordx4 %[ex{i}], %[x2srd], %[koff] offen lds")
        a("s_add_u32 %[koff], %[koff], 128")
    a("s_waitcnt vmcnt(0)")
    a("s_barrier")
    L.extend(reads(0, 0, 0))
    halves = [(stage, kh) for stage in range(T2) for kh in range(2)]
    mf = [(i, jm) for i in range(8) for jm in range(MF)]
    for h, (stage, kh) in enumerate(halves):
        st = h % 2
        a("s_waitcnt lgkmcnt(0)")
        rd = reads(1 - st, *halves[h + 1]) if h + 1 < len(halves) else []
        for q, (i, jm) in enumerate(mf):
            a(f"v_mfma_f32_16x16x32_bf16 {acc(i, jm)}, {fr(st, i)}, {fr(st, 8 + jm)}, {acc(i, jm)}")
            if q % 2 == 0 and q // 2 < len(rd):
                a(rd[q // 2])
    a("s_barrier")
    a("s_mov_b32 m0, %[keep]")
    a("s_nop 15")
    a("s_nop 15")
    return L


def main():
    """Writes the default header (body3 / ext_body2: what every build compiles) and, with
    --x3 PATH, the measured-and-not-adopted three-X-stage bodies (body4 / ext_body4) into their own
    header for the `make x3` A/B build only (gemm_ring.h includes it under LTX_RING_X3)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = sys.argv[1:]
    x3 = None
    if "--x3" in args:
        i = args.index("--x3")
        x3 = args[i + 1] if i + 1 < len(args) else os.path.join(root, "tools", "experiments",
                                                                 "gemm_ring_body_x3.h")
        del args[i:i + 2]
    out = args[0] if args else os.path.join(root, "video-generation-for-human-avatars_amd", "csrc",
                                            "gemm_ring_body.h")

    def header(what):
        return ["// GENERATED by tools/gen_gemm_ring.py -- do not edit by hand.", what, "#pragma once", ""]

    def define(txt, name, lines):
        tok = lambda l: l.replace("@WS@", '" WS "').replace("@XS@", '" XS "').replace("@W@", '" W "').replace("@X@", '" X "')
        txt.append(f"#define {name} \\\n" + " \\\n".join(f'  "{tok(l)}\\n\\t"' for l in lines) + "\n")
    txt = header("// The hand-scheduled K loop of gemm_ring_kernel (gemm_ring.h): body3() and ext_body2() of the\n"
                 "// generator (body() / body2() / body4() are measured-and-not-adopted variants, DESIGN.md §7).")
    for MF in (7, 8):
        main = body3(MF)
        emit_pieces(txt, define, MF)
        assert main[-3:] == ["s_mov_b32 m0, %[keep]", "s_nop 15", "s_nop 15"]
        for T2 in (1, 2):
            define(txt, f"LTX_RING_BODY_EXT{T2}_MF{MF}", main[:-3] + ext_body2(MF, T2))
    open(out, "w").write("\n".join(txt))
    print(out)
    if x3:
        txt = header("// The three-X-stage K loop (body4 / ext_body4): `make x3` only (gemm_ring.h LTX_RING_X3).")
        for MF in (7, 8):
            main4 = body4(MF)
            assert main4[-3:] == ["s_mov_b32 m0, %[keep]", "s_nop 15", "s_nop 15"]
            define(txt, f"LTX_RING4_BODY_MF{MF}", main4)
            for T2 in (1, 2):
                define(txt, f"LTX_RING4_BODY_EXT{T2}_MF{MF}", main4[:-3] + ext_body4(MF, T2))
        open(x3, "w").write("\n".join(txt))
        print(x3)


if __name__ == "__main__":
    main()
