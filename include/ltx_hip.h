/* ltx_hip.h -- C ABI of libltxhip.so, the MI355X (gfx950) kernels behind the LTX-Video 2B
 * LoRA training step of lusinlu/Video-Generation-for-Human-Avatars.
 *
 * The reference has no native layer: every entry point below replaces a torch / diffusers /
 * peft eager op sequence on the path ltx_video/training.py:94-166 drives. Each declaration
 * cites the reference call site it stands in for. The Python host mirror
 * (video-generation-for-human-avatars_amd/ltx_amd) binds these with ctypes; INTEGRATION.md shows
 * the binding a maintainer of the reference would add.
 *
 * Conventions
 *  - Plain pointers to DEVICE memory, int64 sizes / leading dims in ELEMENTS, row-major.
 *  - "bf16" buffers hold raw bfloat16 bits; "f32" buffers IEEE float.
 *  - Caller owns every buffer (inputs, outputs, saved-for-backward, workspaces); nothing is
 *    retained or freed across calls.
 *  - `stream` is a hipStream_t; every call is asynchronous and stream-ordered, no host sync.
 *  - Return 0 (LTX_OK) or an error code (a hipError_t value, or LTX_ERR_*); shape / alignment
 *    checks run on the host before any launch. ltx_last_error() gives a thread-local message.
 */
#ifndef LTX_HIP_H_
#define LTX_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  LTX_OK = 0,
  LTX_ERR_BAD_ARG = 1000,
  LTX_ERR_UNSUPPORTED = 1001,
};

/* GEMM epilogues (ltx_gemm_bf16_nt `epilogue`). y = bf16(acc + bias) first, then: */
enum {
  LTX_EPI_STORE = 0,            /* C = y                                        nn.Linear */
  LTX_EPI_GELU = 1,             /* aux0 <- int16 rint(32767 gelu_tanh'(y) / 2) (optional, the backward's factor);
                                   C = bf16(gelu_tanh(y)), y = bf16(acc + bias)
                                   attention.py:1237-1238 (diffusers GELU tanh), PixArt proj */
  LTX_EPI_GATED_RESIDUAL = 2,   /* C = bf16(R + bf16(gate[b] * y)); R = aux0, gate = aux1 row b =
                                   m / rows_per_batch (row stride ld1); aux2 <- y (optional, ld2:
                                   the gate's gradient, train_mode='full') attention.py:265-268,305-308 */
  LTX_EPI_LORA = 3,             /* C = bf16(y + alpha * U[m,:].Lb[n,:]); U = aux1 f32 [M,rank],
                                   Lb = aux2 f32 [N,rank]      peft lora.Linear, training.py:50-68 */
  LTX_EPI_LORA_RESIDUAL = 4,    /* C = bf16(R + bf16(LORA)); R = aux0        attention.py:285 */
  LTX_EPI_GELU_BWD = 5,         /* C = bf16(bf16(acc) * q * 2 / 32767); q = aux0 (int16, as LTX_EPI_GELU stores it) */
  LTX_EPI_ACCUM = 6,            /* C = bf16(R + bf16(acc)); R = aux0 (may alias C); with aux1 (gate
                                   rows, one per batch) also aux2 = bf16(C * gate[m / rows_per_batch])
                                   (the backward's gate multiply, bitwise ltx_gate_mul_bf16) */
  LTX_EPI_LORA_DGRAD_ACCUM = 7, /* C = [R +] bf16(bf16(acc) + bf16(alpha * Wd[m,:].A[:,n]));
                                   Wd = aux1 f32 [M,rank], A = aux2 f32 [rank,N], R = aux0 opt. */
  LTX_EPI_STORE_ROWDOT = 8,     /* C = y, and the attention backward's delta of the rows:
                                   aux1 f32 [B, N/hd, rows_per_batch] gets, per hd-column head h
                                   (hd = rank: 32 or 64), sum_c bf16(y)[m, hd*h+c] * O[m, hd*h+c]
                                   (O = aux0, ld0): C is dO,
                                   O the attention output (rowsum(dO*O) of ltx_attn_bwd) */
};

int ltx_abi_version(void);
const char* ltx_last_error(void);
/* Device properties the host mirror checks before running (gfx arch number, CU count). */
int ltx_device_info(int* gfx_arch, int* num_cus);

/* ---- K1: SymmetricPatchifier (symmetric_patchifier.py:33-84), bit exact ---------------------- */
/* latents [B,C,F,H,W] bf16 -> tokens [B,F*H*W,C] bf16                    (patchify :55-65) */
int ltx_patchify_bf16(const void* latents, void* tokens, int64_t B, int64_t C, int64_t F,
                      int64_t H, int64_t W, void* stream);
/* tokens [B,F*H*W,C] -> latents [B,C,F,H,W]                              (unpatchify :67-84) */
int ltx_unpatchify_bf16(const void* tokens, void* latents, int64_t B, int64_t C, int64_t F,
                        int64_t H, int64_t W, void* stream);
/* coords [B,3,F*H*W] int64 (t,h,w), w fastest                   (get_latent_coords :33-51) */
int ltx_latent_coords(int64_t* coords, int64_t B, int64_t F, int64_t H, int64_t W, void* stream);

/* ---- K4: rectified flow (rf.py:376-426, training.py:138-146) ----------------------------------- */
/* x_t = bf16((1-t)x0 + t*eps), v = bf16(eps - x0) in f32; x0/eps [B,N,C] bf16, t [B] f32 */
int ltx_rf_noise_velocity(const void* tokens, const void* noise, const float* t, void* x_t,
                          void* v_target, int64_t B, int64_t NC, void* stream);
/* The same arithmetic with f32 results, as the reference's RectifiedFlowScheduler.add_noise /
 * build_velocity_target return them (rf.py:376-386, 400-426: f32 [B] timesteps promote the
 * result); tokens / noise bf16 or f32 (the *_f32 flags). x_t or v_target may be null. */
int ltx_rf_noise_velocity_f32(const void* tokens, int tokens_f32, const void* noise, int noise_f32,
                              const float* t, float* x_t, float* v_target, int64_t B, int64_t NC,
                              void* stream);
/* ---- K2: conditioning lerp of Transformer3DModel.forward (transformer3d.py:447-466) ----------- */
/* tokens [B,F*H*W,C] -> out tokens: frame 0 = lerp(x, ref, 0.85), frames >=1 lerp(x, pose, 0.5),
 * torch.lerp float formula, bf16 result. ref [B,C,1,H,W], pose [B,C,F,H,W]. out may alias tokens. */
int ltx_condition_lerp(const void* tokens, const void* ref, const void* pose, void* out,
                       int64_t B, int64_t C, int64_t F, int64_t H, int64_t W, void* stream);
/* Fused K1+K4+K2 for one train step: latents/pose [B,C,F,H,W], ref [B,C,1,H,W], noise [B,N,C]
 * (all bf16), t [B] f32 -> x_t (pre-lerp, optional), model_in (post-lerp) and v_target, [B,N,C]. */
int ltx_rf_prepare_tokens(const void* latents, const void* ref, const void* pose,
                          const void* noise, const float* t, void* x_t, void* model_in,
                          void* v_target, int64_t B, int64_t C, int64_t F, int64_t H, int64_t W,
                          void* stream);

/* ---- K8: RMSNorm (no affine) + AdaLN modulate (attention.py:223-239, 288-290) --------------- */
/* y = bf16(bf16(bf16(x*rstd) * onep[b]) + shift[b]); rstd = rsqrt(mean(x^2)+eps) (f32, saved).
 * x [M,D] bf16; shift/onep rows of D bf16 with row stride ld_mod per batch b = m / rows_per_batch. */
int ltx_rmsnorm_modulate_fwd(const void* x, const void* shift, const void* onep, int64_t ld_mod,
                             void* y, float* rstd, int64_t M, int64_t D, int64_t rows_per_batch,
                             float eps, void* stream);
/* dx = [dres +] d/dx of the above given dy (mirrors eager autograd roundings). dx may alias dres. */
int ltx_rmsnorm_modulate_bwd(const void* dy, const void* x, const float* rstd, const void* onep,
                             int64_t ld_mod, const void* dres, void* dx, int64_t M, int64_t D,
                             int64_t rows_per_batch, void* stream);
/* ltx_rmsnorm_modulate_bwd that also writes gout = bf16(bf16(dx) * gate[b]) (gate rows of D bf16,
 * row stride ld_gate per batch b = m / rows_per_batch): the previous block's FF-output gradient
 * (ltx_gate_mul_bf16 of this dx, bitwise) from the same pass. gout = null: plain backward. */
int ltx_rmsnorm_modulate_bwd_gated(const void* dy, const void* x, const float* rstd, const void* onep,
                                   int64_t ld_mod, const void* dres, void* dx, int64_t M, int64_t D,
                                   int64_t rows_per_batch, const void* gate, int64_t ld_gate,
                                   void* gout, void* stream);
/* modulation rows: out[b,j,:] = bf16(sst[j,:] + tmod[b*ld_tmod + j*ld_j + :]) and, for the
 * rows flagged in scale_mask (bit j), onep = bf16(1 + that) (attention.py:229-239 with ld_j = D;
 * transformer3d.py:554-560 with ld_j = 0, the embedded timestep broadcast). out/onep [B,P,D]. */
int ltx_ada_modulation(const void* sst, const void* tmod, int64_t ld_tmod, int64_t ld_j,
                       void* out, void* onep_out, int64_t B, int64_t P, int64_t D,
                       int64_t scale_mask, void* stream);
/* out = bf16(x + y) row-wise (bf16 `.grad += new_grad`, torch's AccumulateGrad for a bf16 leaf):
 * 16-B aligned rows, N % 8 == 0; out may alias x. */
int ltx_add_bf16(const void* x, int64_t ldx, const void* y, int64_t ldy, void* out, int64_t ldo, int64_t M,
                 int64_t N, void* stream);
/* out = bf16(R + bf16(gate[m / rows_per_batch] * y)) (the LTX_EPI_GATED_RESIDUAL epilogue as its
 * own pass, attention.py:305-308): the FF-down product runs as a plain library GEMM (y = bf16(x.W^T
 * + b)) and this applies the gate and residual. 16-B aligned rows, N % 8 == 0; out may alias R. */
int ltx_gated_residual_bf16(const void* r, int64_t ldr, const void* gate, int64_t ld_gate, const void* y,
                            int64_t ldy, void* out, int64_t ldo, int64_t M, int64_t N, int64_t rows_per_batch,
                            void* stream);
/* out = bf16(dy * gate[b]) per row, b = m / rows_per_batch (grad of `gate * y`,
 * attention.py:265-266, 305-306). dy/out [M,D] dense, gate rows of ld_gate. */
int ltx_gate_mul_bf16(const void* dy, const void* gate, int64_t ld_gate, void* out, int64_t M,
                      int64_t D, int64_t rows_per_batch, void* stream);

/* ---- K17: output LayerNorm (no affine) + modulate (transformer3d.py:554-561) ---------------- */
int ltx_layernorm_modulate_fwd(const void* x, const void* shift, const void* onep, int64_t ld_mod,
                               void* y, float* mean, float* rstd, int64_t M, int64_t D,
                               int64_t rows_per_batch, float eps, void* stream);
int ltx_layernorm_modulate_bwd(const void* dy, const void* x, const float* mean,
                               const float* rstd, const void* onep, int64_t ld_mod, void* dx,
                               int64_t M, int64_t D, int64_t rows_per_batch, void* stream);

/* ---- K9 tail: q/k RMSNorm (affine, eps 1e-5, across all heads) + 3-D RoPE ------------------- */
/* RoPE cos/sin table (precompute_freqs_cis, transformer3d.py:209-277): omega [D/6] f32 is the
 * reference's `theta ** linspace(0,1,D//6) * pi/2` (computed once on the host),
 * phi = omega[j] * (grid[b,a,n]/max_pos[a]*2 - 1), D%6 leading pad dims (cos 1, sin 0), both
 * rounded to bf16 as the reference's tables are; grid is [B,3,N] int64 (grid_is_float == 0) or
 * f32. Output cs [B*N, D/2] u32 = bf16 cos | bf16 sin << 16 per element pair (16-B aligned).
 * Pass B = 1 when all batches share their coordinates (then cs_batch_rows = 0 below). */
/* Packs the reference's own RoPE pair (cos, sin) of precompute_freqs_cis (transformer3d.py:270-277:
 * bf16 [rows, D] with row stride ld, every value repeated for the element pair 2i, 2i+1) into the
 * table layout of ltx_rope_table: cs[r, i] = cos[r, 2i] | sin[r, 2i] << 16 (the operator-level
 * Attention.set_processor plug-in, attention.py:532-552, receives freqs_cis as that pair). */
int ltx_rope_pack_bf16(const void* cos, const void* sin, int64_t ld, int64_t rows, int64_t D, uint32_t* cs,
                       void* stream);
int ltx_rope_table(const void* indices_grid, int grid_is_float, int64_t B, int64_t N, int64_t D,
                   const float* omega, float max_pos_t, float max_pos_h, float max_pos_w, uint32_t* cs,
                   void* stream);
/* q_out = rope(bf16(bf16(q_in * rstd) * q_weight)) (attention.py:996-1012, RoPE :917-932), same
 * for k; token m = b*N + n reads table row b*cs_batch_rows + n (cs_batch_rows = N, or 0 for a
 * batch-shared table). rope == 0 skips the rotation (cross-attention; rope_cs may be null).
 * k_in / k_out may be null (q only). Saves f32 rstd_q / rstd_k [M] (M = B*N rows). */
int ltx_qk_norm_rope_fwd(const void* q_in, int64_t ldq_in, const void* k_in, int64_t ldk_in,
                         void* q_out, int64_t ldq_out, void* k_out, int64_t ldk_out,
                         const void* q_weight, const void* k_weight, float* rstd_q,
                         float* rstd_k, const uint32_t* rope_cs, int64_t cs_batch_rows, int64_t B,
                         int64_t N, int64_t D, int rope, float eps, void* stream);
/* Backward: incoming dq (f32 when dq_is_f32, else bf16; it is rounded to bf16 first, as SDPA's
 * backward returns bf16) -> dq_raw bf16, the gradient w.r.t. q_in; same for k. */
int ltx_qk_norm_rope_bwd(const void* dq_in, int64_t ldq_in, int dq_is_f32, const void* dk_in,
                         int64_t ldk_in, int dk_is_f32, const void* q_raw, int64_t ldq_raw,
                         const void* k_raw, int64_t ldk_raw, const void* q_weight,
                         const void* k_weight, const float* rstd_q, const float* rstd_k,
                         void* dq_out, int64_t ldq_out, void* dk_out, int64_t ldk_out,
                         const uint32_t* rope_cs, int64_t cs_batch_rows, int64_t B, int64_t N,
                         int64_t D, int rope, void* stream);
/* ltx_qk_norm_rope_fwd / _bwd without RoPE, q only, for `groups` independent row blocks in one
 * launch: the attn2 k_norm (attention.py:434-436, RMSNorm eps 1e-5 with its own weight per block)
 * of the text keys of every transformer block. Group g: rows x + g*x_gs + m*ldx (m < rows), weight
 * + g*w_gs, rstd + g*r_gs; outputs likewise. Bitwise the per-group ungrouped calls. */
int ltx_qk_norm_fwd_grouped(const void* x, int64_t ldx, int64_t x_gs, void* y, int64_t ldy, int64_t y_gs,
                            const void* weight, int64_t w_gs, float* rstd, int64_t r_gs, int64_t rows,
                            int64_t groups, int64_t D, float eps, void* stream);
int ltx_qk_norm_bwd_grouped(const void* dy, int64_t lddy, int64_t dy_gs, const void* x, int64_t ldx, int64_t x_gs,
                            const void* weight, int64_t w_gs, const float* rstd, int64_t r_gs, void* dx,
                            int64_t lddx, int64_t dx_gs, int64_t rows, int64_t groups, int64_t D, void* stream);

/* ---- K10/K14: flash attention (F.scaled_dot_product_attention, attention.py:1057-1064) ------- */
/* Q [B,Nq,H,d] (row stride ldq per token, head h at column h*d), K/V [B,Nk,H,d], O likewise;
 * lse [B,H,Nq] f32 in log2 units (saved for the backward); key_bias [B,Nk] f32 added to the scaled scores
 * (encoder mask bias, transformer3d.py:441-445) or null. d in {32, 64}. kv_batch_rows = Nk, or 0
 * when every batch attends to the same K/V/key_bias rows (the training step's one prompt
 * expanded over the batch, training.py:415): then K/V/key_bias hold one batch. dK/dV (backward)
 * stay per batch [B*Nk rows]; their batch sum is the gradient of the shared rows. */
int ltx_attn_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                 int64_t ldv, void* o, int64_t ldo, float* lse, const float* key_bias, int64_t B,
                 int64_t H, int64_t Nq, int64_t Nk, int64_t kv_batch_rows, int64_t d, float scale,
                 void* stream);
/* The attention path's LTX_ATTN_* A/B switches are read from the environment once, at the first
 * attention launch. A caller of this C API that changes an LTX_ATTN_* variable afterwards MUST call
 * ltx_attn_reload_switches() for the change to take effect: it re-reads every switch and publishes
 * the new table under a lock (a launch on another host thread sees the old table or the new one,
 * never a mixture). ltx_attn_switch_name(i) is the environment name of switch i, NULL past the
 * last one. */
int ltx_attn_reload_switches(void);
const char* ltx_attn_switch_name(int i);
/* The demangled names (as rocprofv3 prints them, without the argument list) of the kernels
 * ltx_attn_fwd (backward = 0) or ltx_attn_bwd_ex (backward = 1) would launch for this call on
 * `stream`, joined by " + ": attn_delta_kernel first when it runs (delta_ready = 0), then the dK/dV
 * kernel, then the dQ kernel; the finish kernel of the query-split one-pass backward last. Host
 * only, nothing is launched: the same plan the entry points launch from, so it depends on the
 * switches last read, the CU count (256 without a device) and the workspace of `stream`. The
 * strides are those of the entry points (only the persistent backward kernels' limits read them);
 * the forward ignores dq_is_f32, delta_ready and lddo. Writes a NUL-terminated string of at most
 * len bytes. */
int ltx_attn_describe(int backward, int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t d,
                      int has_key_bias, int dq_is_f32, int delta_ready, int64_t ldq, int64_t ldk,
                      int64_t ldv, int64_t lddo, void* stream, char* buf, int64_t len);
/* Backward (deterministic, no atomics): delta[b,h,i] = sum_d dO*O (f32, caller workspace
 * [B,H,Nq]); dQ [B,Nq,H,d] (f32 if dq_is_f32 else bf16, row stride lddq), dK/dV bf16. lse as
 * written by ltx_attn_fwd (log2 units). */
int ltx_attn_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                 int64_t ldv, const void* o, int64_t ldo, const void* dout, int64_t lddo,
                 const float* lse, const float* key_bias, float* delta_ws, void* dq,
                 int64_t lddq, int dq_is_f32, void* dk, int64_t lddk, void* dv, int64_t lddv,
                 int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t kv_batch_rows, int64_t d,
                 float scale, void* stream);

/* ---- bf16 MFMA GEMM: C[M,N] = epilogue(A[M,K] . W[N,K]^T) ------------------------------------ */
/* nn.Linear forward (W as stored) and dgrad (W^T packed once: frozen weights). K % 64 == 0,
 * N % 8 == 0, leading dims % 8 == 0, 16-B aligned operands. rank in {8,16,32} for the LORA
 * epilogues (the in-epilogue f32 adapter product the model no longer uses: its adapters ride the
 * K extension A2 / W2, any K2 % 64 == 0, which carries ranks up to 128). */
int ltx_gemm_bf16_nt(const void* A, int64_t lda, const void* W, int64_t ldw, void* C,
                     int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue,
                     const void* bias, const void* aux0, int64_t ld0, const void* aux1,
                     int64_t ld1, const void* aux2, int64_t ld2, float alpha, int64_t rank,
                     int64_t rows_per_batch, void* stream);

/* Same GEMM with a K extension: C = epilogue(A[M,K].W[N,K]^T + A2[M,K2].W2[N,K2]^T), K2 % 64 == 0
 * (0 = none). Used to fuse the peft LoRA branch into the K loop with ltx_lora_split_bf16 operands:
 * y = x.W^T + b + s*(x.A^T).B^T (training.py:50-68) in one f32 accumulation. */
int ltx_gemm_bf16_nt_ext(const void* A, int64_t lda, const void* W, int64_t ldw, const void* A2,
                         int64_t lda2, const void* W2, int64_t ldw2, int64_t K2, void* C,
                         int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue,
                         const void* bias, const void* aux0, int64_t ld0, const void* aux1,
                         int64_t ld1, const void* aux2, int64_t ld2, float alpha, int64_t rank,
                         int64_t rows_per_batch, void* stream);

/* ltx_gemm_bf16_nt_ext with a GROUPED K extension: output columns [g*G, (g+1)*G) (G =
 * ext_group_cols, a multiple of 256 dividing N) read their A2 rows at column offset
 * g*ext_group_stride. One launch then computes several projections of one shared input that
 * each carry their own fused LoRA operand: the attn2 text K/V of all 28 blocks
 * (attention.py:1004-1014 per block, with the peft adapters of training.py:50-68).
 * ext_group_cols = 0 is ltx_gemm_bf16_nt_ext. */
int ltx_gemm_bf16_nt_gext(const void* A, int64_t lda, const void* W, int64_t ldw, const void* A2,
                          int64_t lda2, const void* W2, int64_t ldw2, int64_t K2,
                          int64_t ext_group_cols, int64_t ext_group_stride, void* C, int64_t ldc,
                          int64_t M, int64_t N, int64_t K, int epilogue, const void* bias,
                          const void* aux0, int64_t ld0, const void* aux1, int64_t ld1,
                          const void* aux2, int64_t ld2, float alpha, int64_t rank,
                          int64_t rows_per_batch, void* stream);

/* Tuning knob for A/B measurements (process-global): 0 = the dispatcher's own choice (the ring
 * kernel where it applies), 15 = gemm_nt_kernel_t at the dispatcher's tile height, 13 / 14 =
 * gemm_nt_kernel_t forced to 256 / 224-row tiles, 20 = the ring kernel (bitwise equal to 15).
 * Any other value is LTX_ERR_BAD_ARG. */
int ltx_gemm_set_variant(int variant);
/* The demangled name (as rocprofv3 prints it) of the main kernel ltx_gemm_bf16_nt_ext would launch
 * for this call on `stream` (the dispatcher's tile / split-K choice); bench.py groups its
 * per-launch HIP-event timings by it. Writes a NUL-terminated string of at most len bytes. */
int ltx_gemm_describe(int64_t M, int64_t N, int64_t K, int64_t K2, int epilogue, int64_t rank,
                      void* stream, char* buf, int64_t len);
/* Caller-owned f32 workspace for split-K on small grids (e.g. the M = 256 text-side GEMMs): the
 * library keeps the pointer until the next call (stream-ordered reuse by consecutive GEMMs on
 * one stream); bytes = 0 disables split-K. */
int ltx_gemm_set_workspace(void* ptr, int64_t bytes);
/* Split-K workspace for GEMMs launched on `stream` (overrides the default one for that stream):
 * GEMMs on concurrent streams each need their own partials buffer. */
int ltx_gemm_set_stream_workspace(void* stream, void* ptr, int64_t bytes);

/* ltx_attn_bwd with delta_ws already holding delta[b,h,q] = sum_d dO*O (f32 [B,H,Nq]), e.g.
 * written by the dO-producing GEMM's LTX_EPI_STORE_ROWDOT epilogue: the delta pass is skipped.
 * delta_ready = 0 is ltx_attn_bwd. */
int ltx_attn_bwd_ex(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                    int64_t ldv, const void* o, int64_t ldo, const void* dout, int64_t lddo,
                    const float* lse, const float* key_bias, float* delta_ws, int delta_ready,
                    void* dq, int64_t lddq, int dq_is_f32, void* dk, int64_t lddk, void* dv,
                    int64_t lddv, int64_t B, int64_t H, int64_t Nq, int64_t Nk,
                    int64_t kv_batch_rows, int64_t d, float scale, void* stream);

/* ---- LoRA skinny contractions in f32 (peft lora_A / lora_B, training.py:50-68) --------------- */
/* out[m,j] = alpha * sum_k x[m,k] * Wr[j,k], Wr element (j,k) at Wr[j*wj + k*wk]; x bf16 [M,K]
 * (ldx), out f32 [M,r] (ldo). lora_A forward (u = x.A^T: wj = K, wk = 1) and the lora_B dgrad
 * (w = s*dY.B with B f32 [N,r]: wj = 1, wk = r). r in {8, 16, 32, 64, 128}: that set holds for
 * every ltx_lora_* entry point (ranks above 32 run as 32-wide rank slices of one launch, 16-wide
 * in ltx_lora_rows' whole-K kernel). When split != null the rows
 * are also written as the activation K-extension operand (bf16 [M, K2], ld_split: role 0 of
 * ltx_lora_split_bf16 with scale 1), saving that launch. */
int ltx_lora_down(const void* x, int64_t ldx, const float* Wr, int64_t wj, int64_t wk,
                  float* out, int64_t ldo, int64_t M, int64_t K, int64_t r, float alpha,
                  void* split, int64_t ld_split, int64_t K2, void* stream);
/* ltx_lora_down over `groups` adapters in one launch: group g reads x + g*gx, Wr + g*gw and
 * writes out + g*go, split + g*gs (element offsets; 0 = shared operand). The text-side lora_A of
 * all blocks' attn2 to_k / to_v (one shared input, 56 adapters) and their lora_B dgrads. */
int ltx_lora_down_grouped(const void* x, int64_t ldx, const float* Wr, int64_t wj, int64_t wk,
                          float* out, int64_t ldo, int64_t M, int64_t K, int64_t r, float alpha,
                          void* split, int64_t ld_split, int64_t K2, int64_t groups, int64_t gx,
                          int64_t gw, int64_t go, int64_t gs, void* stream);
/* 3-term bf16 split of an f32 [R, r] matrix (element (i,j) at src[i*rs + j*cs], times scale) into
 * a K-extension operand out [R, K2] (K2 = round_up(3r, 64)): role 0 (activation) rows
 * [hi|hi|lo|0], role 1 (weight) rows [hi|lo|hi|0]; their dot product reproduces the f32 product
 * to ~2^-16 relative. */
int ltx_lora_split_bf16(const float* src, int64_t rs, int64_t cs, float scale, int64_t R,
                        int64_t r, int role, void* out, int64_t ldo, int64_t K2, void* stream);
/* Three bf16 pieces (hi, mid, lo: 24 significant bits) of an f32 [r, K] operand, element (j,k)
 * at src[j*rs + k*cs]: out bf16 [3*RP, K] (ldo), row p*RP + j = piece p of row j, RP = max(r, 16)
 * with zero rows past r. The operand of ltx_lora_rows. */
int ltx_lora_pieces(const float* src, int64_t rs, int64_t cs, int64_t r, int64_t K, void* out,
                    int64_t ldo, void* stream);
/* ltx_lora_down for token-sized M on the bf16 matrix core: out[m,j] = alpha * sum_k x[m,k] *
 * (w3[j] + w3[RP+j] + w3[2RP+j])[k] with w3 the ltx_lora_pieces of the f32 weight (exact bf16
 * products, f32 sums: peft's f32 contraction to summation order). K % 512 == 0. split as in
 * ltx_lora_down. */
int ltx_lora_rows(const void* x, int64_t ldx, const void* w3, int64_t ldw, float* out, int64_t ldo,
                  int64_t M, int64_t K, int64_t r, float alpha, void* split, int64_t ld_split,
                  int64_t K2, void* stream);
/* dW(n,j) (+)= alpha * sum_m Y[m,n] * U[m,j] at dw[n*on + j*oj] (f32; overwritten, or added to
 * when accumulate != 0, e.g. straight into a .grad buffer across micro-steps):
 * lora_B grad (Y = dY, U = u: on = r, oj = 1) and lora_A grad (Y = x, U = w: on = 1, oj = K).
 * Y bf16 [M,N] (ldy), U f32 [M,r] (ldu). Deterministic: split-M partial sums go to the stream's
 * GEMM workspace (ltx_gemm_set_stream_workspace / ltx_gemm_set_workspace) and are added in split
 * order by a second kernel; without room there one workgroup per output column block covers all M. */
int ltx_lora_wgrad(const void* y, int64_t ldy, const float* u, int64_t ldu, float* dw,
                   int64_t on, int64_t oj, int64_t M, int64_t N, int64_t r, float alpha,
                   int accumulate, void* stream);
/* ltx_lora_wgrad over `groups` adapters in one launch: group g reads y + g*gy, u + g*gu and
 * writes dw + g*gd (element offsets; 0 = shared y or u; the outputs must not overlap). */
int ltx_lora_wgrad_grouped(const void* y, int64_t ldy, const float* u, int64_t ldu, float* dw,
                           int64_t on, int64_t oj, int64_t M, int64_t N, int64_t r, float alpha,
                           int accumulate, int64_t groups, int64_t gy, int64_t gu, int64_t gd,
                           void* stream);

/* One pass over dY for a token-sized adapter's backward (replaces the ltx_lora_rows call on dY
 * plus the ltx_lora_wgrad call for lora_B, transformer3d backward): w[m,j] = alpha * sum_n Y[m,n] *
 * (w3[j] + w3[RP+j] + w3[2RP+j])[n] (f32, ldw_out) with its K-extension split row [hi|hi|lo|0..]
 * (bf16 [M, K2], ld_split) and dw[n*on + j*oj] (+)= alpha * sum_m Y[m,n] * U[m,j] (accumulate != 0
 * adds into the buffer). Y bf16 [M,N] (ldy), U f32 [M,r] (ldu), w3 = ltx_lora_pieces of B^T.
 * M % 32 == 0, N % 512 == 0, rank 8, 16, 32, 64 or 128: up to rank 32 one stream of dY from HBM
 * feeds both products; ranks 64 / 128 run 2 / 4 rank slices of 32 in the same launch, each
 * streaming its dY tile again. workspace: ltx_lora_dy_workspace floats (f32). */
int ltx_lora_dy(const void* y, int64_t ldy, const float* u, int64_t ldu, const void* w3, int64_t ldw3,
                int64_t M, int64_t N, int64_t r, float alpha, float* w, int64_t ldw_out, void* split,
                int64_t ld_split, int64_t K2, float* dw, int64_t on, int64_t oj, int accumulate,
                float* workspace, void* stream);
/* f32 workspace size (in floats) of ltx_lora_dy for an [M, N] dY at rank r */
int ltx_lora_dy_workspace(int64_t M, int64_t N, int64_t r, int64_t* floats);
/* ltx_lora_dy plus the same adapter's lora_A gradient (the rest of peft lora.Linear's backward,
 * training.py:50-68: dA = alpha_a * x^T . w with w the f32 term above, as ltx_lora_wgrad(x, w,
 * alpha_a) computes it): dwa[k*ona + j*oja] (+)= alpha_a * sum_m X[m,k] * w[m,j] (acc_a != 0 adds),
 * X bf16 [M,K] (ldx), K % 512 == 0, any N % 512 == 0 (the feed-forward's 8192 included: the dA
 * pass sums w from the N / 512 column partials of the dY pass in the finish kernel's order, four
 * loads in flight at a time beyond N = 2048; calls with N <= 2048 run the code they always ran).
 * Three launches instead of ltx_lora_dy's two plus
 * ltx_lora_wgrad's two; every output bitwise those calls' (dA where ltx_lora_wgrad takes its
 * token-sized path, M >= 2048; below, the same products in another f32 order). The grouped form
 * below keeps N <= 2048 per group.
 * workspace: ltx_lora_dy_dA_workspace. */
int ltx_lora_dy_dA(const void* y, int64_t ldy, const float* u, int64_t ldu, const void* w3, int64_t ldw3,
                   const void* x, int64_t ldx, int64_t M, int64_t N, int64_t K, int64_t r, float alpha,
                   float* w, int64_t ldw_out, void* split, int64_t ld_split, int64_t K2, float* dw,
                   int64_t on, int64_t oj, int accumulate, float alpha_a, float* dwa, int64_t ona,
                   int64_t oja, int acc_a, float* workspace, void* stream);
int ltx_lora_dy_dA_workspace(int64_t M, int64_t N, int64_t K, int64_t r, int64_t* floats);
/* ltx_lora_rows for `groups` (<= 4) adapters of one rank that share x (the q / k / v adapters of a
 * LoRA-wrapped self-attention: one modulated norm output, three lora_A): w3[g] = group g's
 * ltx_lora_pieces (host array of device pointers), group g writes out + g*go and split + g*gs
 * (element offsets: column blocks of shared [M, .] buffers). One launch with (group, rank slice)
 * as a grid dimension wherever ltx_lora_rows runs its whole-contraction kernel (M >= 2048,
 * M % 32 == 0, K = 512 / 1024 / 2048), so each row tile of x leaves HBM once; elsewhere the
 * one-adapter calls. Every output is bitwise ltx_lora_rows' on the same operands. */
int ltx_lora_rows_grouped(const void* x, int64_t ldx, const void* const* w3, int64_t ldw, float* out,
                          int64_t ldo, int64_t go, int64_t M, int64_t K, int64_t r, float alpha,
                          void* split, int64_t ld_split, int64_t K2, int64_t gs, int64_t groups,
                          void* stream);
/* ltx_lora_dy_dA for `groups` (<= 4) adapters of one rank on the column blocks of a packed dY
 * [M, groups*N] (ldy; group g = columns g*N ..) that share X (the fused dQKV and the self-attention's
 * input): u[g], w3[g] (pieces of B_g^T), dw[g], dwa[g] are host arrays of device pointers; group g's
 * w goes to w + g*gw, its split row to split + g*gs (column blocks of shared [M, .] buffers). Three
 * launches (the dY pass with the groups as a grid dimension, one pass over X serving all groups * r
 * columns of w, one finish) instead of three per adapter; X leaves HBM once. Deterministic (no
 * atomics); every output bitwise ltx_lora_dy_dA's on the column slice.
 * workspace: ltx_lora_dy_dA_grouped_workspace floats. */
int ltx_lora_dy_dA_grouped(const void* y, int64_t ldy, const float* const* u, int64_t ldu,
                           const void* const* w3, int64_t ldw3, const void* x, int64_t ldx, int64_t M,
                           int64_t N, int64_t K, int64_t r, int64_t groups, float alpha, float* w,
                           int64_t ldw_out, int64_t gw, void* split, int64_t ld_split, int64_t K2,
                           int64_t gs, float* const* dw, int64_t on, int64_t oj, int accumulate,
                           float alpha_a, float* const* dwa, int64_t ona, int64_t oja, int acc_a,
                           float* workspace, void* stream);
int ltx_lora_dy_dA_grouped_workspace(int64_t M, int64_t N, int64_t K, int64_t r, int64_t groups,
                                     int64_t* floats);
/* The demangled names (as rocprofv3 prints them, without the argument list) of the kernels an
 * adapter entry would launch for this call on `stream`, joined by " + " in launch order, e.g.
 * "ltx::lora_dy_kernel<16, 3> + ltx::lora_dy_kernel<16, 6> + ltx::lora_dy_finish_kernel<16>". Host
 * only, nothing is launched: the same plan the entries launch from (csrc/lora_plan.h), so it depends on
 * the LTX_LORA_WGRAD_ROWS / LTX_LORA_ROWS_DY / LTX_LORA_ROWS_FULL values the library read and on the
 * workspace of `stream`. Every pointer is taken as 16-B aligned.
 *   op DOWN:  ltx_lora_down(_grouped) on x [M, K]
 *   op ROWS:  ltx_lora_rows on x [M, K] (ld_in), pieces (ld_w), out (ld_out)
 *   op WGRAD: ltx_lora_wgrad(_grouped) on y [M, N] (ld_in), u [M, r] (ld_w)
 *   op DY:    ltx_lora_dy on dY [M, N] (ld_in), pieces (ld_w), w (ld_out)
 *   op DY_DA: ltx_lora_dy_dA, also x [M, K]
 * A leading dimension of 0 stands for the dense one. groups = 0: the one-adapter entry; groups >= 1:
 * the _grouped entry (ROWS, DY_DA: up to 4) with out / split columns of group g at g * r / g * K2.
 * split: the call also writes the K-extension operand (DOWN, ROWS). An argument the entry would
 * reject, a rank outside 8 / 16 / 32 / 64 / 128 among them, is LTX_ERR_BAD_ARG here too. Writes a
 * NUL-terminated string of at most len bytes. */
enum { LTX_LORA_OP_DOWN = 0, LTX_LORA_OP_ROWS = 1, LTX_LORA_OP_WGRAD = 2, LTX_LORA_OP_DY = 3, LTX_LORA_OP_DY_DA = 4 };
int ltx_lora_describe(int op, int64_t M, int64_t N, int64_t K, int64_t ld_in, int64_t ld_w, int64_t ld_out,
                      int64_t r, int64_t groups, int split, void* stream, char* buf, int64_t len);

/* ---- LoRA dropout (peft lora_dropout; DESIGN.md "LoRA dropout") -------------------------------
 * The mask is a pure function of (key, sid, row m, column k): Philox4x32-10 with counter
 * (m, k / 8, sid, 0) and key (key & 0xffffffff, key >> 32) gives four words o[0..3]; element k uses
 * the 16-bit lane j = k % 8 (low half of o[j / 2] for even j, high half for odd j) and is KEPT iff
 * lane >= T (T = round(p * 65536) clamped to [1, 65535]). One Philox call serves 8 columns. */
/* xd[m,k] = keep(m,k) ? x[m,k] : 0 (bf16 [M,K], row strides ldx / ldo in elements, K % 8 == 0,
 * 16-B aligned rows; exact: the 1 / (1 - T / 65536) scale is the consumer's alpha). */
int ltx_lora_dropout_apply(const void* x, int64_t ldx, void* out, int64_t ldo, int64_t M, int64_t K,
                           uint64_t key, int64_t sid, int64_t T, void* stream);
/* The masked input-gradient term of `groups` (1..3) dropped-out adapters that share an output:
 * dx[m,k] = bf16(f32(dx[m,k]) + t), t = c * sum_g keep_g(m,k) * sum_j w[m, g*r + j] * A_g[j*lda + k]
 * (f32: the j sum an fma chain in j order on the exact-f32 matrix core, the g sum in g order, then
 * the multiply by c); with gq != null (int16 [M,K], ldg: the GELU epilogue's derivative store)
 * t = (t * gq[m,k]) * (2 / 32767). dx bf16 [M,K] (lddx) in place, w f32 [M, groups*r] (ldw), A = host
 * array of `groups` device pointers to f32 [r, K] (row stride lda), sids = host array of the groups'
 * mask streams. K % 8 == 0, rank 8, 16, 32, 64 or 128. Deterministic, no atomics. */
int ltx_lora_up_masked_add(void* dx, int64_t lddx, const float* w, int64_t ldw, const float* const* A,
                           int64_t lda, const int64_t* sids, int64_t groups, int64_t M, int64_t K,
                           int64_t r, uint64_t key, int64_t T, float c, const void* gq, int64_t ldg,
                           void* stream);

/* ---- DoRA (peft use_dora; DESIGN.md "DoRA (use_dora)"; csrc/dora.hip) --------------------------
 * y = c (.) (x W^T + s (x A^T) B^T) + b with c_j = m_j / ||W[j,:] + s (B A)[j,:]||_2 (the norm takes
 * no gradient). The column scale is folded into the operands of the unchanged GEMMs. */
/* Per output row j of W bf16 [N,K] (ldw), A f32 [r,K] (lda, unit column stride), B f32 [N,r] (element
 * (j,i) at B[j*brs + i*bcs]) and m f32 [N]: norm[j] = ||V[j,:]||_2 of V = f32(W) + (s B) A (f32, the
 * rank sum an fma chain in rank order; V is not stored), c[j] = m[j] / norm[j] (0 where norm[j] == 0),
 * w_eff[j,:] = bf16(c[j] * f32(W[j,:])) (bf16 [N,K], ldo; one rounding) and sb_eff[j,:] = c[j] * (s *
 * B[j,:]) (dense f32 [N,r]: the src of ltx_lora_split_bf16 / ltx_lora_pieces with scale 1). K % 8 == 0,
 * any N, r in {8, 16, 32, 64, 128}. Deterministic, no atomics. */
int ltx_dora_fold(const void* W, int64_t ldw, const float* A, int64_t lda, const float* B, int64_t brs,
                  int64_t bcs, const float* m, float s, int64_t N, int64_t K, int64_t r, float* norm,
                  float* c, void* w_eff, int64_t ldo, float* sb_eff, void* stream);
/* The magnitude gradient: out[n] (+)= m[n] != 0 ? (1 / m[n]) * sum_rows f32(dY[row,n]) * (f32(Y[row,n])
 * - f32(bias[n])) : 0. dY, Y bf16 [M,N] with their own leading dimensions (column blocks of packed
 * buffers), bias bf16 [N] or null, m and out f32 [N]. Any M, N % 8 == 0. Products and sums in f32, in
 * two fixed-order levels: row-split partials in the caller's workspace (ltx_dora_mag_grad_workspace
 * floats), then the splits in order. One pass over dY and Y (4 M N bytes). */
int ltx_dora_mag_grad(const void* dY, int64_t lddy, const void* Y, int64_t ldy, const void* bias,
                      const float* m, int64_t M, int64_t N, float* out, int accumulate,
                      float* workspace, void* stream);
int ltx_dora_mag_grad_workspace(int64_t M, int64_t N, int64_t* splits, int64_t* floats);
/* out[j*on + i*oj] += (alpha * c[j]) * src[j*r + i] for src dense f32 [N,r]: the c_j row scale of a
 * lora_B gradient that the plain dB kernels wrote (unscaled, accumulate = 0) into a scratch. */
int ltx_dora_rowscale_add(const float* src, const float* c, float alpha, int64_t N, int64_t r,
                          float* out, int64_t on, int64_t oj, void* stream);

/* ---- small ops -------------------------------------------------------------------------------- */
/* AdaLayerNormSingle sinusoid: out[b,:] = bf16([cos(s*t*f), sin(s*t*f)]) (256 ch), s = scale */
int ltx_timestep_embedding(const float* t, float scale, void* out, int64_t B, int64_t dim,
                           void* stream);
int ltx_silu_bf16(const void* x, void* y, int64_t n, void* stream);
/* bf16 [R,C] (ld_in) -> [C,R] (ld_out) */
int ltx_transpose_bf16(const void* in, int64_t ld_in, void* out, int64_t ld_out, int64_t R,
                       int64_t C, void* stream);
/* column sums of bf16 [M,N] -> bf16 [N] (bias grads; f32 accumulation) */
int ltx_colsum_bf16(const void* x, int64_t ldx, void* out, int64_t M, int64_t N, void* stream);
/* out[r,:] = bf16(sum_b x[b*rows + r, :]) (f32 accumulation): gradient of rows shared by all
 * batches (the expanded prompt, training.py:415 -- autograd's sum over the expanded dim). */
int ltx_batch_sum_bf16(const void* x, int64_t ldx, int64_t B, int64_t rows, int64_t cols,
                       void* out, int64_t ldo, void* stream);
/* F.mse_loss(out, v) (mean) + its backward seed and std(v) (training.py:159-166):
 * stats[0] = sum (o-v)^2 in f32 over bf16-rounded squares, stats[1] = sum v, stats[2] = sum v^2,
 * stats[3] = 0; stats is f32[4 + 768]: the tail holds 256 per-block partials of each sum, added
 * in a fixed order (deterministic). out / v / dout 16-B aligned.
 * dout = bf16(bf16(bf16(o-v) * 2/n) * gscale). */
int ltx_mse_fwd_bwd(const void* out, const void* v, void* dout, float* stats, int64_t n,
                    float grad_scale, void* stream);

/* ---- weighted velocity loss (csrc/loss.hip; DESIGN.md "Loss weights") ---------------------------
 * Per-token loss weights of a [B, F, H, W] latent grid, token n = (f*H + h)*W + w, all f32:
 *   box  = bbox[b] = (x_min, y_min, x_max, y_max) in [0,1], padded by face_pad times its width and
 *          height on each side, then clipped to [0,1]; a NaN coordinate or a box that is empty after
 *          the clip gives cov = 0 for the whole sample, and so does bbox == null;
 *   ox   = min(1, max(0, min(x1, (w+1)/W) - max(x0, w/W)) * W), oy likewise with h and H;
 *   cov  = ox * oy, the share of the token's cell that the box covers;
 *   raw[b,n]   = frame_w[f] * (1 + (face_weight - 1) * cov) * user_w[b,n];
 *   raw_sum[b] = sum_n raw[b,n]; wt[b,n] = raw[b,n] * (sample_w[b] * N / raw_sum[b]), 0 where
 *                raw_sum[b] == 0 -- each sample's weights average to sample_w[b].
 * A null frame_w / sample_w / user_w is all ones. face_weight > 0, face_pad >= 0. One workgroup per
 * sample; the sum is taken in a fixed order (strided per-thread sums, the wave shuffle tree, four waves
 * in order) without atomics, bitwise run to run. Any B, F, H, W >= 1. */
int ltx_loss_token_weights(const float* bbox,      /* [B,4] x_min,y_min,x_max,y_max in [0,1], or null */
                           const float* frame_w,   /* [F] >= 0, or null (= 1)                          */
                           const float* sample_w,  /* [B], or null (= 1): the timestep factor          */
                           const float* user_w,    /* [B,N] >= 0, or null (= 1)                        */
                           float face_weight, float face_pad,
                           float* wt,              /* [B,N] out, N = F*H*W, token n = (f*H + h)*W + w  */
                           float* raw_sum,         /* [B] out                                          */
                           int64_t B, int64_t F, int64_t H, int64_t W, void* stream);
/* ltx_mse_fwd_bwd with a weight per token: out / v / dout bf16 [rows, C] dense (16-B aligned), element
 * i of the n = rows * C belongs to token i / C. Per element d = bf16(o - v), q = bf16(d * d) and
 * dout = bf16(f32(bf16(bf16(d * 2/n) * grad_scale)) * wt[token]), round to nearest even: ltx_mse_fwd_bwd's
 * seed, then one multiply and one rounding. stats[0] = sum wt * q, stats[1] = sum v, stats[2] = sum v^2,
 * stats[3] = sum q (the unweighted sum); stats is f32[4 + 4*256]: the tail holds 256 per-block partials
 * of each sum, added in ltx_mse_fwd_bwd's fixed order. The traversal is ltx_mse_fwd_bwd's (16-B vectors
 * over n / 8, then the scalar tail), so for every C: with wt == 1 stats[0..2], stats[3] and dout are
 * bitwise ltx_mse_fwd_bwd's stats[0..2], stats[0] and dout, and for any wt stats[1..3] are bitwise its
 * stats[1], stats[2], stats[0]. C % 8 == 0 loads one weight per vector. dout may be null. */
int ltx_wmse_fwd_bwd(const void* out, const void* v, const float* wt /* [rows] */,
                     void* dout /* nullable */, float* stats /* f32[4 + 4*256] */,
                     int64_t rows, int64_t C, float grad_scale, void* stream);
/* The robust (pseudo-Huber) velocity loss (DESIGN.md "Robust loss"): out / v / dout bf16
 * [B, rows_per_sample, C] dense (16-B aligned), n = B * rows_per_sample * C elements; element i belongs to
 * token i / C and to sample i / (rows_per_sample * C). Per element, in f32 from the bf16 values:
 *   e = o - v, r = sqrt(e*e + c*c), l = k * (e*e) / (r + c) (== k * (r - c)), g = dl/do = k * e / r,
 *   c = c[sample] > 0, k = 2*c (LTX_ROBUST_HUBER: e^2 as c grows, 2*c*|e| for |e| >> c) or
 *   2 (LTX_ROBUST_SMOOTH_L1: 2*|e| as c shrinks);
 *   dout = bf16(wt[token] * g * grad_scale / n), computed in f32 and rounded once, to nearest even.
 * The square root and the two divisions are the hardware's 1-ulp v_sqrt_f32 / v_rcp_f32.
 * e == 0 gives l == 0 and dout == 0 exactly; non-finite inputs give non-finite sums and seeds.
 * stats[0] = sum wt * l, stats[4] = sum l, and stats[1] = sum v, stats[2] = sum v^2,
 * stats[3] = sum bf16(d*d) with d = bf16(o - v), the last three bitwise ltx_mse_fwd_bwd's stats[1],
 * stats[2], stats[0] for every shape and any wt: the traversal is ltx_mse_fwd_bwd's (16-B vectors over
 * n / 8, then the scalar tail, on its fixed grid) and the 256 per-block partials of each sum, kept in the
 * tail of stats (f32[8 + 5*256]), are added in its fixed order: no atomics, bitwise run to run.
 * C % 8 == 0 loads one weight and one threshold per vector; otherwise a vector may straddle tokens and
 * samples, and both are indexed per element. wt == null: every weight 1 (stats[0] == stats[4], bitwise
 * what a wt of ones gives). dout may be null (forward only). Refused before any launch: a null out, v, c
 * or stats, a kind other than the two below, a non-positive B, rows_per_sample or C. */
enum { LTX_ROBUST_HUBER = 1, LTX_ROBUST_SMOOTH_L1 = 2 };
int ltx_robust_loss_fwd_bwd(const void* out, const void* v, const float* wt /* [B*rows_per_sample] or null */,
                            const float* c /* [B] */, int kind, void* dout /* nullable */,
                            float* stats /* f32[8 + 5*256] */, int64_t B, int64_t rows_per_sample, int64_t C,
                            float grad_scale, void* stream);
/* torch.optim.AdamW single-tensor step (training.py:270-271): f32 or bf16 param/state.
 * is_bf16 selects the dtype of param/grad/exp_avg/exp_avg_sq (all the same). */
int ltx_adamw_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n,
                   int is_bf16, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int64_t step, void* stream);
/* ltx_adamw_step for many tensors of one dtype in one launch (the LoRA / caption-projection
 * optimizer step, training.py:270-271): table = device int64 [nchunks][6] of (param, grad,
 * exp_avg, exp_avg_sq, first element, count <= 2048); all tensors at the same step. */
int ltx_adamw_multi(const int64_t* table, int64_t nchunks, int is_bf16, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int64_t step, void* stream);

/* ---- global gradient-norm clip over the ltx_adamw_multi chunk table (csrc/optim.hip) ------------ */
/* part[b] (device f64, b < nchunks) = sum of squares of row b's gradient elements, each converted to
 * f64 and squared exactly; fixed order (strided per-thread sums, the wave shuffle tree, four wave sums
 * in order), no atomics. is_bf16 is the dtype of the table's tensors. A second dtype's launch is given
 * part + the first's nchunks. */
int ltx_grad_sumsq_multi(const int64_t* table, int64_t nchunks, int is_bf16, double* part, void* stream);
/* One block adds part[0 .. nparts) in a fixed order (strided sums, then a fixed-shape tree) and writes
 * the 16-byte device record at out (8-byte aligned): { f64 sumsq; f32 norm = (float)sqrt(sumsq);
 * f32 coef = min(1, max_norm / (norm + 1e-6f)) in f32 (max_norm <= 0: coef = 1, the norm is still
 * written) }. torch.nn.utils.clip_grad_norm_'s coefficient with error_if_nonfinite=False, on an f64
 * norm. */
int ltx_grad_clip_coef(const double* part, int64_t nparts, float max_norm, void* out, void* stream);
/* ltx_adamw_multi on g' = R(g * *coef) in place of g (R: round to bf16 for bf16 tensors, identity for
 * f32 -- what grad.mul_(coef) would leave); coef is read from device memory (the record's third
 * field), the gradients themselves are not written. */
int ltx_adamw_multi_clip(const int64_t* table, int64_t nchunks, int is_bf16, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int64_t step, const float* coef, void* stream);

/* ---- EMA of the trainable weights, fused into the multi-tensor AdamW step (csrc/optim.hip) ------- */
/* The EMA table: device int64 [nchunks][8] of (param, grad, exp_avg, exp_avg_sq, first element,
 * count <= 2048, shadow, stash). shadow is the tensor's f32 moving average (f32 for bf16 parameters too),
 * stash a buffer of the parameter's dtype and size; both are indexed like the parameter. A field an
 * entry point does not read may be 0: stash for ltx_adamw_multi_ema; grad, exp_avg and exp_avg_sq for
 * the two swap entries. One block per row, 256 threads.
 *
 * ltx_adamw_multi_ema: ltx_adamw_multi (coef_or_null == null) or ltx_adamw_multi_clip (coef_or_null: the
 * device coefficient) -- param, exp_avg and exp_avg_sq bitwise theirs -- and, for each element, with p'
 * the parameter value the step stores (for bf16 the value just rounded to bf16),
 *   shadow <- shadow - one_minus_decay * (shadow - float(p'))
 * as three separately rounded f32 operations (subtract, multiply, subtract; never an FMA): diffusers'
 * EMAModel.step s_param.sub_(one_minus_decay * (s_param - param)) on an f32 shadow. one_minus_decay is
 * (float)(1.0 - decay), computed by the caller in double; it must lie in [0, 1]. */
int ltx_adamw_multi_ema(const int64_t* table, int64_t nchunks, int is_bf16, float lr, float beta1, float beta2,
                        float eps, float weight_decay, int64_t step, const float* coef_or_null,
                        float one_minus_decay, void* stream);
/* stash[i] = param[i]; param[i] = R(shadow[i]) over the EMA table's rows (R: round to nearest even to
 * bf16 for bf16 parameters, identity for f32). One launch per dtype. */
int ltx_ema_load_multi(const int64_t* table, int64_t nchunks, int is_bf16, void* stream);
/* param[i] = stash[i] over the EMA table's rows: undoes ltx_ema_load_multi. */
int ltx_ema_restore_multi(const int64_t* table, int64_t nchunks, int is_bf16, void* stream);

/* ---- stochastically rounded bf16 parameters with f32 moments (csrc/optim.hip, csrc/philox.h) ------ */
/* The mixed step of a bf16 parameter with a bf16 gradient: P = float(p), G = float(g) (with a coefficient
 * G = float(bf16(G * *coef))), (P', M', V') exactly ltx_adamw_multi's f32 arithmetic on (P, G, M, V) with
 * f32 exp_avg / exp_avg_sq, and p' = SR(P', r): for a finite P' the bf16 bits are (bits(P') + r) >> 16,
 * NaN and +-inf take round-to-nearest. The 16-bit r of element i is lane i & 7 (low half of word
 * (i & 7) / 2 for an even lane, high half for an odd one) of Philox4x32-10 on the counter
 * (lo32(i >> 3), hi32(i >> 3), ordinal, step mod 2^32) under the key (seed lo, seed hi); it does not
 * depend on the chunking or the access width.
 *
 * The table: device int64 [nchunks][8] of (param bf16, grad bf16, exp_avg f32, exp_avg_sq f32, first
 * element, count <= 2048, shadow f32 or 0, ordinal in [0, 2^32)); first element is a multiple of 8. With
 * ema != 0 the shadow follows the value stored, shadow <- shadow - one_minus_decay * (shadow - float(p')),
 * as in ltx_adamw_multi_ema. Rows whose tensors are all 16-byte aligned move 16 bytes per lane per access
 * and make one generator call per 8 elements. */
int ltx_adamw_multi_sr(const int64_t* table, int64_t nchunks, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int64_t step, const float* coef_or_null, int ema, float one_minus_decay,
                       uint64_t seed, void* stream);

/* ---- Prodigy, the learning-rate-free optimizer, over the chunk table (csrc/prodigy.hip) ---------- */
/* The Prodigy table: device int64 [nchunks][10] of (param, grad, exp_avg, exp_avg_sq, first element,
 * count <= 2048, s, p0, shadow, stash). exp_avg, exp_avg_sq, s and p0 have the parameter's dtype; shadow
 * (the f32 EMA of the parameter) and stash are 0 without the EMA, and the Prodigy entry points never read
 * stash. One block per row, 256 threads; rows whose tensors are all 16-byte aligned move 16 bytes per
 * lane per access, the others one element.
 *
 * is_bf16 = 2 in ltx_prodigy_moments_multi, and ltx_prodigy_apply_multi_sr, are the mixed step of a bf16
 * parameter (see ltx_adamw_multi_sr): param, grad and p0 bf16, exp_avg, exp_avg_sq and s f32, the f32
 * instantiation's arithmetic on float(p), float(g) (with a coefficient, float(bf16(g * *coef))) and
 * float(p0), and the table's last field the parameter's ordinal in place of the stash.
 *
 * The record: 8 device f64 { d, d_max, d_numerator, d_denom, d_hat, dlr, k, applied }, 8-byte aligned;
 * the caller initialises it to { d0, d0, 0, 0, 0, 0, 0, 0 }. Hyper-parameters arrive as doubles; every
 * scalar derived from d is formed in f64 on the device and cast to f32 where torch would cast a Python
 * float alpha / value. R rounds to the tensor's dtype (identity for f32).
 *
 * ltx_prodigy_moments_multi (pass 1), per element, with d and k read from the record and
 * dlr = d lr bc, bc = use_bias_correction ? sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) : 1:
 *   g    = grad;  g = R(g * *coef_or_null) when given (grad itself is not written);
 *   g    = R(fma(coupled_weight_decay, p, g)) when coupled_weight_decay != 0;
 *   exp_avg    = R(fma(f32(d (1 - beta1)), g, R(exp_avg * beta1)))
 *   exp_avg_sq = R(fma(f32(d d (1 - beta2)), g * g, R(exp_avg_sq * beta2)))
 *   s          = R(fma(f32((d / d0) (safeguard_warmup ? d : dlr)), g, R(s * beta3)))
 * (torch's add_(alpha) / addcmul_ are one fused multiply-add on the device), and
 *   part[2 b] = sum over row b of R(p0 - p) * g (an f32 product, added in f64),
 *   part[2 b + 1] = sum over row b of the stored |s|,
 * overwritten, in a fixed order: each lane its elements in order, the wave butterfly, four waves in
 * order. A second dtype's launch is given part + 2 * the first's nchunks. */
int ltx_prodigy_moments_multi(const int64_t* table, int64_t nchunks, int is_bf16, const double* record, double lr,
                              double beta1, double beta2, double beta3, double d0, double coupled_weight_decay,
                              int use_bias_correction, int safeguard_warmup, const float* coef_or_null, double* part,
                              void* stream);
/* One block adds the nrows (num, den) pairs of part in a fixed order (strided sums, a fixed-shape tree)
 * and updates the record in f64:
 *   dlr = d lr bc;  d_denom = SUM den;  if d_denom == 0: applied = 0, nothing else changes; otherwise
 *   d_numerator = beta3 d_numerator + (d / d0) dlr SUM num;  d_hat = d_coef d_numerator / d_denom;
 *   if d == d0: d = max(d, d_hat);  d_max = max(d_max, d_hat);  d = min(d_max, d growth_rate);
 *   k = k + 1;  applied = 1. */
int ltx_prodigy_d_update(const double* part, int64_t nrows, double* record, double lr, double beta1, double beta2,
                         double beta3, double d0, double d_coef, double growth_rate, int use_bias_correction,
                         void* stream);
/* Pass 2, a no-op when the record's applied is 0; per element, with the record's new d and the dlr the
 * step started from:
 *   den = R(R(sqrt(exp_avg_sq)) + f32(d eps));
 *   p = R(fma(f32(-decoupled_weight_decay dlr), p, p)) when decoupled_weight_decay != 0;
 *   p = R(fma(f32(-dlr), exp_avg / den, p))     (torch's addcdiv_ on the device);
 * and with ema != 0, shadow <- shadow - one_minus_decay * (shadow - float(p)) as in ltx_adamw_multi_ema. */
int ltx_prodigy_apply_multi(const int64_t* table, int64_t nchunks, int is_bf16, const double* record, double eps,
                            double decoupled_weight_decay, int ema, float one_minus_decay, void* stream);
/* Pass 2 of the mixed step: ltx_prodigy_apply_multi's f32 arithmetic on float(p) and the f32 moments, the
 * result stored as SR(p', r) with r from (seed, the row's ordinal, step, element) as in ltx_adamw_multi_sr;
 * the shadow follows the value stored. `step` is the parameters' step count after its increment. */
int ltx_prodigy_apply_multi_sr(const int64_t* table, int64_t nchunks, const double* record, double eps,
                               double decoupled_weight_decay, int ema, float one_minus_decay, uint64_t seed,
                               int64_t step, void* stream);

/* ---- the non-finite guard of the optimizer step (csrc/optim.hip, csrc/prodigy.hip, csrc/chunk_io.h) -- */
/* A step whose gradients are not all finite is skipped on the device: it writes the guard record and
 * nothing else. The record: 32 device bytes, 8-byte aligned, { f64 sumsq; f32 norm; f32 coef; i32 applied;
 * i32 0; i64 skipped } -- ltx_grad_clip_coef's record in its first 16 bytes.
 *
 * ltx_grad_guard_record takes ltx_grad_clip_coef's place behind ltx_grad_sumsq_multi: the same fixed-order
 * sum of part[0 .. nparts) and the same { sumsq, norm, coef } (max_norm <= 0: coef = 1), then
 * applied = 1 when sumsq is finite, else 0 (a NaN element makes the sum NaN, an infinite one +inf or NaN,
 * and finite f32 / bf16 elements cannot overflow f64: the test is exact), and
 * skipped = (prev_or_null ? its skipped : 0) + (1 - applied). prev_or_null, the previous step's record, is
 * read before out is written and may be out itself. */
int ltx_grad_guard_record(const double* part, int64_t nparts, float max_norm, const void* prev_or_null, void* out,
                          void* stream);
/* ltx_adamw_multi (coef_or_null == null, ema == 0), ltx_adamw_multi_clip (coef_or_null) or
 * ltx_adamw_multi_ema (ema != 0, on the 8-field table) behind the guard: every workgroup reads
 * guard->applied once and returns before its first store when it is 0; when it is 1 the step is bitwise
 * the unguarded entry point's (the same row function). coef_or_null is usually &guard->coef. */
int ltx_adamw_multi_guard(const int64_t* table, int64_t nchunks, int is_bf16, float lr, float beta1, float beta2,
                          float eps, float weight_decay, int64_t step, const float* coef_or_null, int ema,
                          float one_minus_decay, const void* guard, void* stream);
/* ltx_adamw_multi_sr behind the guard, in the same way. */
int ltx_adamw_multi_sr_guard(const int64_t* table, int64_t nchunks, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int64_t step, const float* coef_or_null, int ema,
                             float one_minus_decay, uint64_t seed, const void* guard, void* stream);
/* ltx_prodigy_moments_multi behind the guard: a skipped step's pass 1 writes neither exp_avg, exp_avg_sq
 * and s nor its row partials. */
int ltx_prodigy_moments_multi_guard(const int64_t* table, int64_t nchunks, int is_bf16, const double* record,
                                    double lr, double beta1, double beta2, double beta3, double d0,
                                    double coupled_weight_decay, int use_bias_correction, int safeguard_warmup,
                                    const float* coef_or_null, double* part, const void* guard, void* stream);
/* ltx_prodigy_d_update behind the guard: a skipped step does not read part, sets the record's applied to 0
 * and leaves d, d_max, d_numerator, d_denom, d_hat, dlr and k. ltx_prodigy_apply_multi and
 * ltx_prodigy_apply_multi_sr are gated on that field already (a no-op when applied is 0), so pass 2 has no
 * guarded entry point of its own. */
int ltx_prodigy_d_update_guard(const double* part, int64_t nrows, double* record, double lr, double beta1,
                               double beta2, double beta3, double d0, double d_coef, double growth_rate,
                               int use_bias_correction, const void* guard, void* stream);

/* ---- max-norm regularisation of the LoRA adapters (DESIGN.md "Max-norm (scale_weight_norms)";
 * csrc/max_norm.hip) ------------------------------------------------------------------------------ */
/* After the optimizer's update, every adapter pair (A f32 [r, K], B f32 [N, r], s) with
 * norm = |s| ||B A||_F above the cap has A and B multiplied by f = f32(sqrt(cap / norm)). No entry point
 * reads anything back, none uses atomics, every sum has a fixed order.
 *
 * The pair table: 12 int64 per pair { A, B, N, K, r, the bits of the f64 s, the first f64 of the pair's A
 * partials in ws, of its B partials, the pair's first workgroup, slab, slabs of K, slabs of N }; r one of
 * 8, 16, 32, 64, 128, A and B dense. ltx_max_norm_plan (host only) gives for one pair out[0 .. 6) = { slab,
 * slabs of K, slabs of N, workgroups, f64 of the A partials, f64 of the B partials }. */
int ltx_max_norm_plan(int64_t N, int64_t K, int64_t r, int64_t* out);
/* sumsq[p] = ||B A||_F^2 = sum_ij (B^T B)_ij (A A^T)_ij of every pair, in f64 and without forming B A: one
 * launch of nwg workgroups (the sum of the plans') writes the Gram tiles' per-slab partials to ws, a second
 * of one workgroup per pair adds the slabs in order and contracts the two matrices. */
int ltx_max_norm_sumsq(const int64_t* table, int64_t npairs, int64_t nwg, double* ws, double* sumsq, void* stream);
/* Per pair, in f64: norm = |s| sqrt(sumsq), ratio = norm <= cap ? 1 : cap / norm, factor[p] = f32(sqrt(ratio)),
 * scaled = norm ratio; record (16 bytes) = { i32 pairs with ratio != 1; f32 mean of scaled; f32 max of scaled;
 * i32 0 }. With a guard record whose applied is 0 every ratio is 1. */
int ltx_max_norm_finish(const int64_t* table, const double* sumsq, int64_t npairs, double cap,
                        const void* guard_or_null, float* factor, void* record, void* stream);
/* The chunk table of the paired tensors, 5 int64 per row { param f32, its f32 EMA shadow or 0, first element,
 * count <= 2048, pair }, one workgroup per row: a row whose factor[pair] is 1 stores nothing; otherwise
 * p <- fl32(p f) and, with a shadow, shadow <- fl32(shadow - fl32(one_minus_decay fl32(p_before - p_after))).
 * With a guard record whose applied is 0 it returns before the first store. */
int ltx_max_norm_scale_multi(const int64_t* rows, int64_t nrows, const float* factor, float one_minus_decay,
                             const void* guard_or_null, void* stream);

/* ---- train_mode='full' parameter gradients (csrc/paramgrad.hip) --------- */
/* Weight gradient of the q/k RMSNorm weights: partials[(which * splits + s) * D + d] (f32) =
 * sum over row split s of bf16(dn * bf16(x_raw * rstd)), dn = RoPE^T of the incoming gradient (the
 * roundings of ltx_qk_norm_rope_bwd); which = 0 (q) / 1 (k, when dk_in != null). Reduce with
 * ltx_colsum_finish (G = 1 or 2 per call site, S = splits). */
int ltx_qk_norm_wgrad(const void* dq_in, int64_t ldq_in, int dq_is_f32, const void* dk_in,
                      int64_t ldk_in, int dk_is_f32, const void* q_raw, int64_t ldq_raw,
                      const void* k_raw, int64_t ldk_raw, const float* rstd_q, const float* rstd_k,
                      const uint32_t* rope_cs, int64_t cs_batch_rows, int64_t B, int64_t N, int64_t D,
                      int rope, int64_t splits, float* partials, void* stream);
/* Column sums over row groups (M = G * rows_per_group), f32 partials [G, splits, D]:
 * mode 0: a; 1: bf16(a*b); 2: bf16(a * bf16(b * r[m])) (RMSNorm scale grad);
 * 3: bf16(a * bf16((b - mean[m]) * r[m])) (LayerNorm scale grad). */
int ltx_group_colsum(const void* a, int64_t lda, const void* b, int64_t ldb, const float* r,
                     const float* mean, int mode, int64_t M, int64_t D, int64_t rows_per_group,
                     int64_t splits, float* partials, void* stream);
/* bf16 result of the partials: per group out[g*ldo + d] = bf16(sum_s), or with sum_groups
 * out[d] = bf16(sum_g bf16(sum_s)); accumulate adds into out (bf16 .grad accumulation). */
int ltx_colsum_finish(const float* partials, int64_t G, int64_t S, int64_t D, int sum_groups,
                      int accumulate, void* out, int64_t ldo, void* stream);
/* torch silu_backward in bf16: dx = bf16(dy * s * (1 + x * (1 - s))), s = sigmoid(x); with dres
 * (nullable) dx = bf16(dres + that) */
int ltx_silu_bwd_bf16(const void* x, const void* dy, const void* dres, void* dx, int64_t n,
                      void* stream);

/* ---- ZeRO-2 optimizer buffers (BASELINE config Z; csrc/zero.hip) ------------------------------ */
int ltx_cast_bf16_f32(const void* src, float* dst, int64_t n, void* stream);
int ltx_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
/* out (one f64 on the device) [+]= sum x^2; deterministic when the stream has a GEMM workspace
 * (per-block f64 partials there, added in block order), else one f64 atomic per block */
int ltx_sumsq_f32(const float* x, int64_t n, double* out, int accumulate, void* stream);
/* coef = inv_world * min(1, max_norm / (sqrt(sumsq) * inv_world + 1e-6)) (max_norm <= 0: 1),
 * written to *coef; x *= coef (the averaged, global-norm-clipped gradient shard; DeepSpeed
 * gradient_clipping) -- read from device memory, no host sync. */
int ltx_clip_scale_f32(float* x, int64_t n, const double* sumsq, float max_norm, float inv_world,
                       float* coef, void* stream);

/* ---- inference denoising step (csrc/denoise.hip) ------------------------------ */
/* RoPE indices_grid of an inference call: latent coords * (sf_t, sf_h, sf_w) with the causal
 * first-frame fix (vae_encode.py:215-226), as float32 with the time axis / frame_rate
 * (pipeline_ltx_video.py:1121-1122). out [B,3,F*H*W] f32; pixel_out [B,3,N] int64 or null. */
int ltx_pixel_coords_f32(float* out, int64_t* pixel_out, int64_t B, int64_t F, int64_t H,
                         int64_t W, int64_t sf_t, int64_t sf_h, int64_t sf_w, int causal_fix,
                         float frame_rate, void* stream);
/* Skip-layer (STG) blend, eager bf16: out = bf16(bf16(a*m) + bf16(c*bf16(1-m))), m =
 * mask[row / rows_per_batch] (bf16 [B]): AttentionSkip / AttentionValues before to_out
 * (attention.py:1071-1085), TransformerBlock on the block output (attention.py:312-319). */
int ltx_skip_blend_bf16(const void* a, int64_t lda, const void* c, int64_t ldc, const void* mask,
                        void* out, int64_t ldo, int64_t M, int64_t D, int64_t rows_per_batch,
                        void* stream);
/* RectifiedFlowScheduler.step, deterministic (rf.py:305-374) + denoising_step's keep
 * (pipeline_ltx_video.py:1346-1379): dt = t - max{sched[k] < t - 1e-6} (0 if none),
 * out = sample - dt * v over [BN, C]; timestep f32 [1] (global) or [BN] (per_token);
 * round_v = eager semantics of a 0-dim dt times a bf16 prediction (dt and the product rounded
 * to bf16); cond_mask f32 [BN] or null: out = sample where !(t_cond - 1e-6 < 1 - cond_mask).
 * sample / v / out each f32 or bf16 (flags). */
int ltx_rf_euler_step(const void* sample, int sample_f32, const void* v, int v_f32,
                      const float* timestep, int per_token, const float* sched, int64_t nsched,
                      const float* cond_mask, float t_cond, int round_v, void* out, int out_f32,
                      int64_t BN, int64_t C, void* stream);
/* CFG / CFG* / STG / STG rescaling of the batched prediction pred [nc*B, L] bf16 (chunks
 * uncond | text | perturbed, only the active ones) -> out [B, L] bf16, per-op bf16 rounding as
 * pipeline_ltx_video.py:1229-1268 evaluates it eagerly. workspace >= B * 258 floats. */
int ltx_guidance_bf16(const void* pred, int64_t B, int64_t L, int do_cfg, int do_stg,
                      float guidance_scale, float stg_scale, float rescaling_scale, int cfg_star,
                      float* workspace, int64_t ws_floats, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LTX_HIP_H_ */
