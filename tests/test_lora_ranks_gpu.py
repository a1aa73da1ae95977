"""LoRA ranks 32, 64 and 128 through the fused adapter path on the MI355X: the adapter kernels
(ltx_lora_down / rows / wgrad / pieces / split), the one-pass backward (ltx_lora_dy, ltx_lora_dy_dA),
the GEMM K extension at K2 = 192 / 384 and one LTX-2B-width block against the oracle.

Tolerances are those of tests/test_kernels_gpu.py (test_lora_kernels, test_lora_dy_one_pass,
test_lora_rows_token_sized: f32 adapters as exact three-piece bf16 products summed in f32, so
rel-Frobenius < 1e-5 against fp32 torch and < 1e-6 between two summation orders of the same
products) and of tests/model_utils.py (noise_crit / loss_crit at their defaults)."""
import pytest
import torch

import ltx_oracle as O
from model_utils import (build_model, build_step, grads_by_canonical, is_lora_trainable, loss_crit, noise_crit,
                         oracle_step, rel, synth_inputs)

pytestmark = pytest.mark.gpu

DEV = "cuda"
RANKS = [32, 64, 128]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from ltx_amd import _lib as L
    L.ensure_device()
    return L


def g(*shape, dtype=torch.bfloat16, scale=1.0, seed=0):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale).to(dtype).to(DEV)


# M: one row group / ragged, below every token-sized gate / the lora_dy_dA and wgrad-rows gate /
# the lora_down -> lora_rows gate
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M", [32, 517, 2048, 8192])
def test_lora_kernels_ranks(M, r):
    from ltx_amd import ops
    K, N = 2048, 2048
    x = g(M, K, seed=1)
    A = torch.randn(r, K, device=DEV) / K ** 0.5
    Bm = torch.randn(N, r, device=DEV) * 0.05
    u, su = ops.lora_down(x, A, split=True)
    assert rel(u, x.float() @ A.t()) < 1e-5
    assert su.shape == (M, ops.lora_k2(r))
    assert torch.equal(su, ops.lora_split(u, "act"))  # fused split == standalone split
    dy = g(M, N, seed=2)
    w = ops.lora_down(dy, Bm, alpha=0.5, transposed=True)
    assert rel(w, 0.5 * dy.float() @ Bm) < 1e-5
    dB = ops.lora_wgrad(dy, u, alpha=0.5)
    assert rel(dB, 0.5 * dy.float().t() @ u) < 1e-5
    dA = ops.lora_wgrad(x, w, transpose_out=True)
    assert rel(dA, w.t() @ x.float()) < 1e-5
    # accumulate into an existing buffer (the .grad path): buf + product
    buf = torch.randn(N, r, device=DEV)
    ref = buf + 0.5 * dy.float().t() @ u
    ops.lora_wgrad(dy, u, alpha=0.5, out=buf, accumulate=True)
    assert rel(buf, ref) < 1e-5
    # the model's forward call: with the cached pieces, M >= 8192 routes to ltx_lora_rows
    u2, su2 = ops.lora_down(x, A, split=True, pieces=lambda: ops.lora_pieces(A))
    assert rel(u2, x.float() @ A.t()) < 1e-5
    assert torch.equal(su2, ops.lora_split(u2, "act"))
    # the weight-side operand [hi | lo | hi | 0..] in lora_k2(r) columns
    K2 = ops.lora_k2(r)
    sw = ops.lora_split(Bm, "weight", 0.5)
    hi = (Bm * 0.5).bfloat16()
    lo = (Bm * 0.5 - hi.float()).bfloat16()
    assert sw.shape == (N, K2)
    assert torch.equal(sw[:, :r], hi) and torch.equal(sw[:, r:2 * r], lo) and torch.equal(sw[:, 2 * r:3 * r], hi)
    assert K2 == 3 * r or float(sw[:, 3 * r:].abs().max()) == 0


# (32, 512): the smallest N and a single group; (1760, 1024): ragged row split (55 groups of 32 do
# not divide into blocks of 4 or 7 groups); (2048, 2048): the dA merge's bitwise range
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M,N", [(32, 512), (1760, 1024), (2048, 2048)])
def test_lora_dy_one_pass_ranks(M, N, r):
    from ltx_amd import ops
    dy = g(M, N, seed=3)
    u = torch.randn(M, r, device=DEV)
    Bm = torch.randn(N, r, device=DEV) * 0.05
    pieces = ops.lora_pieces(Bm, transposed=True)
    assert ops.lora_dy_fits(dy, r)
    buf0 = torch.randn(N, r, device=DEV)
    buf = buf0.clone()
    ref_dB = buf + 0.5 * dy.float().t() @ u
    w, sp = ops.lora_dy(dy, u, pieces, r, 0.5, buf)
    assert rel(w, 0.5 * dy.float() @ Bm) < 1e-5
    assert torch.equal(sp, ops.lora_split(w, "act"))
    assert rel(buf, ref_dB) < 1e-5
    # deterministic: the same call again, bitwise
    bufb = buf0.clone()
    wb, spb = ops.lora_dy(dy, u, pieces, r, 0.5, bufb)
    assert torch.equal(w, wb) and torch.equal(sp, spb) and torch.equal(buf, bufb)
    # against the two-kernel path it replaces
    w2, sp2 = ops.lora_rows(dy, pieces, r, alpha=0.5, split=True)
    assert rel(w, w2) < 1e-6
    buf2 = torch.zeros(N, r, device=DEV)
    ops.lora_dy(dy, u, pieces, r, 0.5, buf2, accumulate=False)
    assert rel(buf2, ops.lora_wgrad(dy, u, alpha=0.5)) < 1e-6
    # with the adapter's dA = x^T . w in the same call: w, split and dB bitwise the call above; dA
    # bitwise ltx_lora_wgrad(x, w) where that takes its token-sized path (M >= 2048), else to f32 order
    K = 1024 if N != 1024 else 512
    x = g(M, K, seed=9)
    assert ops.lora_dy_da_fits(dy, x, r) == (M >= 2048)
    bB1, bA1 = torch.randn(N, r, device=DEV), torch.randn(r, K, device=DEV)
    bB2, bA2 = bB1.clone(), bA1.clone()
    bB3, bA3 = bB1.clone(), bA1.clone()
    w1, sp1 = ops.lora_dy(dy, u, pieces, r, 0.5, bB1)
    ops.lora_wgrad(x, w1, transpose_out=True, out=bA1, accumulate=True)
    w2, sp2 = ops.lora_dy(dy, u, pieces, r, 0.5, bB2, x=x, dA_out=bA2)
    assert torch.equal(w1, w2) and torch.equal(sp1, sp2) and torch.equal(bB1, bB2)
    if M >= 2048:
        assert torch.equal(bA1, bA2)
    else:
        assert rel(bA2, bA1) < 1e-6
    w3, sp3 = ops.lora_dy(dy, u, pieces, r, 0.5, bB3, x=x, dA_out=bA3)
    assert torch.equal(w2, w3) and torch.equal(sp2, sp3) and torch.equal(bB2, bB3) and torch.equal(bA2, bA3)
    bA4 = torch.zeros(r, K, device=DEV)
    ops.lora_dy(dy, u, pieces, r, 0.5, torch.zeros(N, r, device=DEV), x=x, dA_out=bA4, dA_accumulate=False)
    assert rel(bA4, w1.t() @ x.float()) < 1e-5


# K = 512: the smallest whole-contraction (lora_rows_full) K; K = 2048: the model's
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("K", [512, 2048])
def test_lora_rows_token_sized_ranks(K, r):
    from ltx_amd import ops
    M = 2048
    x = g(M, K, seed=7)
    A = torch.randn(r, K, device=DEV) / K ** 0.5
    pieces = ops.lora_pieces(A)
    u, su = ops.lora_rows(x, pieces, r, alpha=0.5, split=True)
    assert rel(u, 0.5 * x.float() @ A.t()) < 1e-5
    assert torch.equal(su, ops.lora_split(u, "act"))
    K2 = ops.lora_k2(r)
    big = torch.full((M, 2 * K2), 7.0, dtype=torch.bfloat16, device=DEV)
    outb = torch.full((M, 2 * r), 3.0, device=DEV)
    u2, _ = ops.lora_rows(x, pieces, r, alpha=0.5, out=outb[:, r:], split=True, split_out=big[:, K2:])
    assert torch.equal(u2, u) and torch.equal(big[:, K2:], su)
    assert float((big[:, :K2] - 7.0).abs().max()) == 0 and float((outb[:, :r] - 3.0).abs().max()) == 0


def _variant(v):
    from ltx_amd import _lib, ops
    _lib.load().ltx_gemm_set_variant(v)
    ops._GEMM_NAMES.clear()  # the name cache does not key on the variant


# (7000, 2056, 384): the smallest shape tests/test_gemm_ring_gpu.py sends to the ring kernel, ragged
# in M and N; (14336, 2048, 128): its shortest K (one pass of the main loop before the extension);
# (5000, 2048, 2048): ragged M (neither 224- nor 256-row tiles divide it) at the model's width
@pytest.mark.parametrize("K2", [192, 384])
@pytest.mark.parametrize("M,N,K", [(7000, 2056, 384), (14336, 2048, 128), (5000, 2048, 2048)])
def test_gemm_k_extension_192_384(M, N, K, K2):
    from ltx_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(K2 + M)
    a = torch.randn(M, K, device="cuda", generator=gen).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5).bfloat16()
    a2 = torch.randn(M, K2 + 8, device="cuda", generator=gen).bfloat16()[:, :K2]  # strided view
    w2 = (torch.randn(N, K2, device="cuda", generator=gen) / K2 ** 0.5).bfloat16()
    b = torch.randn(N, device="cuda", generator=gen).bfloat16()
    R = torch.randn(M, N, device="cuda", generator=gen).bfloat16()
    try:
        # the ring kernel with 3 / 6 extension tiles is what the default dispatch launches, for the
        # plain store and for the accumulate epilogue (<6>)
        for epi, tag in (("store", "<0, 0, "), ("accum", "<6, 0, ")):
            name = ops.gemm_kernel_name(M, N, K, K2, epi)
            assert "gemm_ring_kernel" + tag in name and name.endswith(f", {K2 // 64}>(ltx::GemmParams)"), name
        _variant(15)
        r0 = ops.gemm(a, w, bias=b, ext=(a2, w2))
        c0 = R.clone()
        ops.gemm(a, w, epilogue="accum", aux0=c0, out=c0, ext=(a2, w2))
        _variant(0)
        r1 = ops.gemm(a, w, bias=b, ext=(a2, w2))
        c1 = R.clone()
        ops.gemm(a, w, epilogue="accum", aux0=c1, out=c1, ext=(a2, w2))
    finally:
        _variant(0)
    torch.cuda.synchronize()
    assert torch.equal(r0, r1) and torch.equal(c0, c1)
    ref = a.float() @ w.float().t() + b.float() + a2.float() @ w2.float().t()
    assert rel(r1, ref) < 1e-2


@pytest.mark.parametrize("K2", [192, 384])
@pytest.mark.parametrize("L", [256, 2048])
def test_gemm_grouped_text_kv_extension_192_384(L, K2):
    """The batched text K/V form (ltx_gemm_bf16_nt_gext): column group g of the output takes its own
    K2 columns of the activation operand; 2 blocks x (k, v) = 4 groups of D columns. 256 text rows
    (the model's prompt length: the 128-row kernel) and 2048 (a full round of large tiles: the ring)."""
    from ltx_amd import ops
    D, G = 2048, 4
    gen = torch.Generator(device="cuda").manual_seed(K2)
    a = torch.randn(L, D, device="cuda", generator=gen).bfloat16()
    w = (torch.randn(G * D, D, device="cuda", generator=gen) / D ** 0.5).bfloat16()
    a2 = torch.randn(L, G * K2, device="cuda", generator=gen).bfloat16()
    w2 = (torch.randn(G * D, K2, device="cuda", generator=gen) / K2 ** 0.5).bfloat16()
    b = torch.randn(G * D, device="cuda", generator=gen).bfloat16()
    try:
        if L == 2048:
            name = ops.gemm_kernel_name(L, G * D, D, K2, "store")
            assert "gemm_ring_kernel<0, 0, " in name and name.endswith(f", {K2 // 64}>(ltx::GemmParams)"), name
        _variant(15)
        r0 = ops.gemm(a, w, bias=b, ext=(a2, w2), ext_group=(D, K2))
        _variant(0)
        r1 = ops.gemm(a, w, bias=b, ext=(a2, w2), ext_group=(D, K2))
    finally:
        _variant(0)
    torch.cuda.synchronize()
    assert torch.equal(r0, r1)
    for gi in range(G):
        ref = (a.float() @ w[gi * D:(gi + 1) * D].float().t() + b[gi * D:(gi + 1) * D].float()
               + a2[:, gi * K2:(gi + 1) * K2].float() @ w2[gi * D:(gi + 1) * D].float().t())
        assert rel(r1[:, gi * D:(gi + 1) * D], ref) < 1e-2, gi


_ORACLE = {}


def _block_case(r):
    """One LTX-2B-width block, B = 8 samples of 2x16x16 (N = 512, M = 4096: past the token-sized
    gates), one shared prompt of 256 tokens (16 valid); the oracle's fp32 and bf16 steps, computed
    once per rank and left unchanged."""
    if r not in _ORACLE:
        from ltx_amd.transformer3d import OURS_TRANSFORMER_CONFIG
        cfg = dict(OURS_TRANSFORMER_CONFIG, num_layers=1)
        params = O.make_params(cfg, 100 + r, lora_rank=r, requires_grad=False)
        d = synth_inputs(8, 2, 16, 16, 256, 16, seed=7 + r, device=DEV)
        refs = {dt: oracle_step(params, cfg, d, dt, is_lora_trainable, device=DEV)
                for dt in (torch.float32, torch.bfloat16)}
        _ORACLE[r] = (cfg, params, d, refs)
    return _ORACLE[r]


def _sample(model, d):
    B = d["in.latents"].shape[0]
    tok, coords = O.patchify(d["in.latents"].bfloat16())
    x = O.add_noise(tok, d["out.noise"], d["out.t"]).bfloat16()
    with torch.no_grad():
        return model(hidden_states=x, indices_grid=coords.to(DEV),
                     ref_image_hidden_states=d["in.ref_image_latents"].bfloat16(),
                     pose_hidden_states=d["in.pose_latents"].bfloat16(),
                     encoder_hidden_states=d["in.prompt_embeds"].bfloat16().expand(B, -1, -1),
                     timestep=d["out.t"], encoder_attention_mask=d["in.prompt_attention_mask"].expand(B, -1)).sample


@pytest.mark.parametrize("r", RANKS)
def test_block_2b_width_against_oracle(r):
    cfg, params, d, refs = _block_case(r)
    lora_b = [k for k in params if "lora_B" in k]
    assert len(lora_b) == 4
    for k in lora_b:  # with a zero B every dA is identically zero and the case proves nothing
        assert float(params[k].float().abs().max()) > 0, k
    model = build_model(cfg, params, r, device=DEV)
    out = _sample(model, d)
    lb = build_step(model, d)
    grads = {k: v.clone() for k, v in grads_by_canonical(model).items()}
    (s32, g32, l32), (s16, g16, l16) = refs[torch.float32], refs[torch.bfloat16]
    noise_crit(f"r={r} sample", out, s16, s32)
    loss_crit(f"r={r}", lb, l16, l32)
    names = [k for k in g32 if "lora_" in k]
    assert len(names) == 8 and any("caption_projection" in k for k in g32)
    for k in g32:
        assert grads[k] is not None and float(grads[k].abs().max()) > 0, k
        noise_crit(f"r={r} {k}", grads[k], g16[k], g32[k])
    # a second identical step: bitwise the same gradients (fixed-order partial sums, no atomics)
    for p in model.parameters():
        p.grad = None
    lb2 = build_step(model, d)
    again = grads_by_canonical(model)
    assert lb2 == lb
    for k in grads:
        assert torch.equal(again[k], grads[k]), k


def test_unsupported_rank_raises_at_adapter_creation():
    from ltx_amd.transformer3d import OURS_TRANSFORMER_CONFIG
    cfg = dict(OURS_TRANSFORMER_CONFIG, num_layers=1)
    with pytest.raises(ValueError, match=r"8, 16, 32, 64, 128"):
        build_model(cfg, {}, 24, device=DEV)
