"""LoRA adapters on the self-attention projections through the fused block on the MI355X: the
grouped adapter kernels (ltx_lora_rows_grouped, ltx_lora_dy_dA_grouped), the packed QKV GEMM with the
grouped K extension, and the model with lora_targets 'attn1' / 'attn1+attn2' against the oracle.

Tolerances are those of tests/test_kernels_gpu.py and tests/test_lora_ranks_gpu.py (f32 adapters as
exact three-piece bf16 products summed in f32: rel-Frobenius < 1e-5 against fp32 torch; bf16 GEMMs
< 1e-2 against fp32) and of tests/model_utils.py (noise_crit / loss_crit at their defaults). The
grouped kernels run the one-adapter block program on each group's operands, so every output keeps
the one-adapter kernel's summation order: the comparisons with the separate calls are BITWISE."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

import ltx_oracle as O
from lora_attn1_utils import attn1_params, build_targets_model
from model_utils import (build_model, build_step, grads_by_canonical, is_lora_trainable, loss_crit, noise_crit,
                         oracle_step, rel, synth_inputs)

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G3 = 3


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from ltx_amd import _lib as L
    L.ensure_device()
    return L


def g(*shape, dtype=torch.bfloat16, scale=1.0, seed=0):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale).to(dtype).to(DEV)


# ---------------------------------------------------------------------------------------------
# kernel (a): the grouped token-sized down-projection
# ---------------------------------------------------------------------------------------------
# (2048, 512): the smallest whole-contraction K at the token-sized gate; (8192, 2048): past the
# model's gate (lora_down -> lora_rows at M >= 8192) at the model's width
@pytest.mark.parametrize("r", [8, 16, 32, 128])
@pytest.mark.parametrize("M,K", [(2048, 512), (8192, 2048)])
def test_lora_rows_grouped(M, K, r):
    from ltx_amd import ops
    x = g(M, K, seed=11)
    As = [torch.randn(r, K, device=DEV) / K ** 0.5 for _ in range(G3)]
    pieces = [ops.lora_pieces(A) for A in As]
    K2 = ops.lora_k2(r)
    # the groups' columns sit in wider pre-filled buffers, a gap of one block between them
    outb = torch.full((M, 7 * r), 3.0, device=DEV)
    big = torch.full((M, 7 * K2), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.lora_rows_grouped(x, pieces, r, alpha=0.5, out=outb[:, r:2 * r], split=True, split_out=big[:, K2:2 * K2],
                          group_strides=(2 * r, 2 * K2))
    for gi in range(G3):
        u, su = ops.lora_rows(x, pieces[gi], r, alpha=0.5, split=True)
        c, c2 = (2 * gi + 1) * r, (2 * gi + 1) * K2
        assert torch.equal(outb[:, c:c + r], u), gi  # bitwise the one-adapter call
        assert torch.equal(big[:, c2:c2 + K2], su), gi
        assert rel(outb[:, c:c + r], 0.5 * x.float() @ As[gi].t()) < 1e-5
        assert torch.equal(su, ops.lora_split(u, "act"))
    for gi in range(4):  # the columns between and around the groups come back untouched
        assert float((outb[:, 2 * gi * r:(2 * gi + 1) * r] - 3.0).abs().max()) == 0
        assert float((big[:, 2 * gi * K2:(2 * gi + 1) * K2] - 7.0).abs().max()) == 0
    # the default layout: new side-by-side buffers; without the split
    u3, s3 = ops.lora_rows_grouped(x, pieces, r, alpha=0.5, split=True)
    assert u3.shape == (M, G3 * r) and s3.shape == (M, G3 * K2)
    assert torch.equal(u3, torch.cat([outb[:, (2 * gi + 1) * r:(2 * gi + 2) * r] for gi in range(G3)], 1))
    assert torch.equal(s3, torch.cat([big[:, (2 * gi + 1) * K2:(2 * gi + 2) * K2] for gi in range(G3)], 1))
    assert torch.equal(ops.lora_rows_grouped(x, pieces, r, alpha=0.5), u3)


def test_lora_rows_grouped_below_the_one_launch_gate():
    """M = 512 (below the token-sized gate) and K = 768 (no whole-contraction kernel): the entry
    issues the one-adapter calls, bitwise."""
    from ltx_amd import ops
    r = 16
    for M, K in ((512, 2048), (2048, 768)):
        x = g(M, K, seed=12)
        As = [torch.randn(r, K, device=DEV) / K ** 0.5 for _ in range(G3)]
        pieces = [ops.lora_pieces(A) for A in As]
        u3, s3 = ops.lora_rows_grouped(x, pieces, r, split=True)
        for gi in range(G3):
            u, su = ops.lora_rows(x, pieces[gi], r, split=True)
            assert torch.equal(u3[:, gi * r:(gi + 1) * r], u) and torch.equal(s3[:, gi * 64:(gi + 1) * 64], su)


# ---------------------------------------------------------------------------------------------
# kernel (b): the packed one-pass backward
# ---------------------------------------------------------------------------------------------
# (32, 512, 512): one row group at the smallest widths; (1760, 1024, 512): the ragged row split of
# the existing dy test; (2048, 2048, 2048): the bitwise range of the dA merge
@pytest.mark.parametrize("r", [8, 32, 64])
@pytest.mark.parametrize("M,N,K", [(32, 512, 512), (1760, 1024, 512), (2048, 2048, 2048)])
def test_lora_dy_grouped(M, N, K, r):
    from ltx_amd import ops
    dy = g(M, G3 * N, seed=21)
    x = g(M, K, seed=22)
    us = [torch.randn(M, r, device=DEV) for _ in range(G3)]
    Bs = [torch.randn(N, r, device=DEV) * 0.05 for _ in range(G3)]
    pieces = [ops.lora_pieces(Bm, transposed=True) for Bm in Bs]
    K2 = ops.lora_k2(r)
    dB0 = [torch.randn(N, r, device=DEV) for _ in range(G3)]
    dA0 = [torch.randn(r, K, device=DEV) for _ in range(G3)]
    dB, dA = [t.clone() for t in dB0], [t.clone() for t in dA0]
    w, sp = ops.lora_dy_grouped(dy, us, pieces, r, 0.5, dB, x, dA)
    assert w.shape == (M, G3 * r) and sp.shape == (M, G3 * K2)
    for gi in range(G3):
        bB, bA = dB0[gi].clone(), dA0[gi].clone()
        ys = dy[:, gi * N:(gi + 1) * N]
        w1, sp1 = ops.lora_dy(ys, us[gi], pieces[gi], r, 0.5, bB, x=x, dA_out=bA)
        # bitwise the one-adapter call on the column slice
        assert torch.equal(w[:, gi * r:(gi + 1) * r], w1), gi
        assert torch.equal(sp[:, gi * K2:(gi + 1) * K2], sp1), gi
        assert torch.equal(dB[gi], bB) and torch.equal(dA[gi], bA), gi
        # and fp32 torch
        assert rel(w1, 0.5 * ys.float() @ Bs[gi]) < 1e-5
        assert rel(dB[gi], dB0[gi] + 0.5 * ys.float().t() @ us[gi]) < 1e-5
        assert rel(dA[gi], dA0[gi] + w1.t() @ x.float()) < 1e-5
    # deterministic: the same call again, bitwise
    dB2, dA2 = [t.clone() for t in dB0], [t.clone() for t in dA0]
    w2, sp2 = ops.lora_dy_grouped(dy, us, pieces, r, 0.5, dB2, x, dA2)
    assert torch.equal(w, w2) and torch.equal(sp, sp2)
    assert all(torch.equal(a, b) for a, b in zip(dB + dA, dB2 + dA2))
    # overwrite instead of accumulate
    dB3, dA3 = [torch.full_like(t, 5.0) for t in dB0], [torch.full_like(t, 5.0) for t in dA0]
    ops.lora_dy_grouped(dy, us, pieces, r, 0.5, dB3, x, dA3, accumulate=False, dA_accumulate=False)
    for gi in range(G3):
        assert rel(dB3[gi], 0.5 * dy[:, gi * N:(gi + 1) * N].float().t() @ us[gi]) < 1e-5
        assert rel(dA3[gi], w[:, gi * r:(gi + 1) * r].t() @ x.float()) < 1e-5


# ---------------------------------------------------------------------------------------------
# the packed QKV GEMM with the grouped K extension
# ---------------------------------------------------------------------------------------------
def _variant(v):
    from ltx_amd import _lib, ops
    _lib.load().ltx_gemm_set_variant(v)
    ops._GEMM_NAMES.clear()  # the name cache does not key on the variant


@pytest.mark.parametrize("K2", [64, 192])
def test_gemm_qkv_grouped_extension(K2):
    """x1 . Wqkv^T with q / k / v each reading its own K2 columns of the [M, 3 K2] adapter operand
    (ltx_gemm_bf16_nt_gext, ext_group = (D, K2)), as tests/test_lora_ranks_gpu.py checks the text K/V
    form: the two kernels agree bitwise, and rel < 1e-2 against fp32."""
    from ltx_amd import ops
    D, M = 2048, 2048
    gen = torch.Generator(device="cuda").manual_seed(K2)
    a = torch.randn(M, D, device="cuda", generator=gen).bfloat16()
    w = (torch.randn(G3 * D, D, device="cuda", generator=gen) / D ** 0.5).bfloat16()
    a2 = torch.randn(M, G3 * K2, device="cuda", generator=gen).bfloat16()
    w2 = (torch.randn(G3 * D, K2, device="cuda", generator=gen) / K2 ** 0.5).bfloat16()
    b = torch.randn(G3 * D, device="cuda", generator=gen).bfloat16()
    try:
        _variant(15)
        r0 = ops.gemm(a, w, bias=b, ext=(a2, w2), ext_group=(D, K2))
        _variant(0)
        r1 = ops.gemm(a, w, bias=b, ext=(a2, w2), ext_group=(D, K2))
    finally:
        _variant(0)
    torch.cuda.synchronize()
    assert torch.equal(r0, r1)
    for gi in range(G3):
        ref = (a.float() @ w[gi * D:(gi + 1) * D].float().t() + b[gi * D:(gi + 1) * D].float()
               + a2[:, gi * K2:(gi + 1) * K2].float() @ w2[gi * D:(gi + 1) * D].float().t())
        assert rel(r1[:, gi * D:(gi + 1) * D], ref) < 1e-2, gi


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
_TINY = {}
R_TINY = 8


def _tiny_case(targets):
    """Config T (two layers) with the inputs of the attn1 golden, r = 8; the oracle's fp32 and bf16
    steps, computed once per target set and left unchanged."""
    if targets not in _TINY:
        with open(os.path.join(GOLD, "tiny_lora_attn1_step.json")) as f:
            meta = json.load(f)
        raw = load_file(os.path.join(GOLD, "tiny_lora_attn1_step.safetensors"))
        d = {k: v.to(DEV) for k, v in raw.items() if k.startswith("in.") or k in ("out.t", "out.noise")}
        d["out.noise"] = d["out.noise"].bfloat16()
        cfg = meta["config"]
        params = attn1_params(cfg, meta["param_seed"], R_TINY, targets=tuple(targets.split("+")))
        refs = {dt: oracle_step(params, cfg, d, dt, is_lora_trainable, device=DEV)
                for dt in (torch.float32, torch.bfloat16)}
        _TINY[targets] = (cfg, params, d, refs)
    return _TINY[targets]


def _sample(model, d, grad=False):
    B = d["in.latents"].shape[0]
    tok, coords = O.patchify(d["in.latents"].bfloat16())
    x = O.add_noise(tok, d["out.noise"], d["out.t"]).bfloat16()
    with torch.enable_grad() if grad else torch.no_grad():
        return model(hidden_states=x, indices_grid=coords.to(DEV),
                     ref_image_hidden_states=d["in.ref_image_latents"].bfloat16(),
                     pose_hidden_states=d["in.pose_latents"].bfloat16(),
                     encoder_hidden_states=d["in.prompt_embeds"].bfloat16().expand(B, -1, -1),
                     timestep=d["out.t"], encoder_attention_mask=d["in.prompt_attention_mask"].expand(B, -1)).sample


def _against_oracle(tag, model, d, refs, n_attn1):
    out = _sample(model, d)
    lb = build_step(model, d)
    grads = {k: v.clone() if v is not None else None for k, v in grads_by_canonical(model).items()}
    (s32, g32, l32), (s16, g16, l16) = refs[torch.float32], refs[torch.bfloat16]
    noise_crit(f"{tag} sample", out, s16, s32)
    loss_crit(tag, lb, l16, l32)
    assert sorted(grads) == sorted(g32) and any("caption_projection" in k for k in g32)
    attn1 = [k for k in g32 if ".attn1." in k and "lora_" in k]
    assert len(attn1) == n_attn1
    for k in g32:
        # (on the parent commit the attn1 adapters never enter the forward: these grads stay None)
        assert grads[k] is not None and float(grads[k].abs().max()) > 0, k
        noise_crit(f"{tag} {k}", grads[k], g16[k], g32[k])
    return lb, grads


@pytest.mark.parametrize("targets", ["attn1", "attn1+attn2"])
def test_tiny_model_against_oracle(targets):
    cfg, params, d, refs = _tiny_case(targets)
    for k in params:
        if "lora_B" in k:  # with a zero B every dA is identically zero and the case proves nothing
            assert float(params[k].float().abs().max()) > 0, k
    model = build_targets_model(cfg, params, R_TINY, targets)
    _against_oracle(f"tiny {targets}", model, d, refs, n_attn1=2 * 4 * 2)


@pytest.mark.parametrize("targets", ["attn1", "attn1+attn2"])
def test_gradient_checkpointing_is_bitwise(targets):
    cfg, params, d, _ = _tiny_case(targets)
    res = []
    for ckpt in (False, True):
        m = build_targets_model(cfg, params, R_TINY, targets)
        m.train()
        m.gradient_checkpointing = ckpt
        res.append((build_step(m, d), grads_by_canonical(m)))
    (l1, g1), (l2, g2) = res
    assert l1 == l2
    for k in g1:
        assert g2[k] is not None and torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("targets", ["attn1", "attn1+attn2"])
def test_forward_only_equals_training_forward(targets):
    """_forward_tokens without grad (nothing kept, text K/V on the side stream) gives bitwise the
    sample of the training forward (activations kept; with attn2 adapters, the text stack)."""
    cfg, params, d, _ = _tiny_case(targets)
    model = build_targets_model(cfg, params, R_TINY, targets)
    a = _sample(model, d, grad=False)
    b = _sample(model, d, grad=True)
    assert b.requires_grad and torch.equal(a, b.detach())


def test_default_targets_are_bitwise_todays_model():
    """No lora_targets: outputs and gradients of one step are bitwise those of a model built by the
    unchanged tests/model_utils.build_model."""
    cfg, _, d, _ = _tiny_case("attn1+attn2")
    params = attn1_params(cfg, 31, R_TINY, targets=("attn2",))
    a = build_model(cfg, params, R_TINY, device=DEV)
    b = build_targets_model(cfg, params, R_TINY, None)
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    assert torch.equal(_sample(a, d), _sample(b, d))
    la, lb = build_step(a, d), build_step(b, d)
    ga, gb = grads_by_canonical(a), grads_by_canonical(b)
    assert la == lb
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_full_mode_with_attn1_adapters_raises():
    """train_mode='full' on a model that carries adapters keeps raising, for attn1 as for attn2."""
    from ltx_amd.lora import inject_lora, lora_target_modules
    from model_utils import build_full_model
    cfg, _, d, _ = _tiny_case("attn1")
    model = build_full_model(cfg, O.make_params(cfg, 77, lora_rank=0, requires_grad=False), device=DEV)
    inject_lora(model, lora_target_modules(len(model.transformer_blocks), "attn1"), R_TINY, R_TINY)
    with pytest.raises(NotImplementedError, match="without LoRA"):
        build_step(model, d)


def test_unload_repacks_the_fused_qkv_weight():
    from ltx_amd.lora import unload_lora
    cfg, params, d, _ = _tiny_case("attn1")
    model = build_targets_model(cfg, params, R_TINY, "attn1")
    _sample(model, d)  # packs the base weights
    blk = model.transformer_blocks[0]
    before = blk.packed()["qkv_w"].clone()
    a1 = blk.attn1
    merged = torch.cat([m.merged_weight() for m in (a1.to_q, a1.to_k, a1.to_v)], 0)
    unload_lora(model)
    want = torch.cat([a1.to_q.weight, a1.to_k.weight, a1.to_v.weight], 0)  # the merged base weights
    assert torch.equal(blk.packed()["qkv_w"], want) and not torch.equal(want, before)
    # both are W + s B A rounded to bf16 (the in-place merge and merged_weight round one f32 sum each)
    assert rel(want, merged) < 2.0 ** -8 and rel(before, merged) > 10 * rel(want, merged)


_BLOCK = {}


def _block_case(r):
    """One LTX-2B-width block, B = 8 samples of 4x16x16 (N = 1024, M = 8192: past the token-sized
    gates), one shared prompt of 256 tokens (16 valid); the oracle's fp32 and bf16 steps, computed
    once per rank and left unchanged."""
    if r not in _BLOCK:
        from ltx_amd.transformer3d import OURS_TRANSFORMER_CONFIG
        cfg = dict(OURS_TRANSFORMER_CONFIG, num_layers=1)
        params = attn1_params(cfg, 300 + r, r)
        d = synth_inputs(8, 4, 16, 16, 256, 16, seed=17 + r, device=DEV)
        refs = {dt: oracle_step(params, cfg, d, dt, is_lora_trainable, device=DEV)
                for dt in (torch.float32, torch.bfloat16)}
        _BLOCK[r] = (cfg, params, d, refs)
    return _BLOCK[r]


@pytest.mark.parametrize("r", [16, 64])
def test_block_2b_width_against_oracle(r):
    cfg, params, d, refs = _block_case(r)
    model = build_targets_model(cfg, params, r, "attn1+attn2")
    lb, grads = _against_oracle(f"2b r={r}", model, d, refs, n_attn1=8)
    # a second identical step: bitwise the same gradients (fixed-order partial sums, no atomics)
    for p in model.parameters():
        p.grad = None
    lb2 = build_step(model, d)
    again = grads_by_canonical(model)
    assert lb2 == lb
    for k in grads:
        assert torch.equal(again[k], grads[k]), k


def test_block_2b_width_grouped_equals_separate(monkeypatch):
    """LTX_LORA_QKV_GROUPED selects the grouped or the one-adapter kernels for the q / k / v adapters:
    the same gradients bitwise, either way."""
    cfg, params, d, _ = _block_case(16)
    res = []
    for flag in ("1", "0"):
        monkeypatch.setenv("LTX_LORA_QKV_GROUPED", flag)
        model = build_targets_model(cfg, params, 16, "attn1+attn2")
        res.append((build_step(model, d), grads_by_canonical(model)))
    assert res[0][0] == res[1][0]
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_processor_matches_fused_block_attn1():
    """HipAttnProcessor on the LoRA-wrapped attn1 (the unfused operator path, one projection at a
    time) against the fused block's attn1 contribution. With attn2.to_out.0 and ff.net.2 zeroed the
    block returns h1 = bf16(h + g_msa * attn1(x1)), so its contribution is h1 - h.
    Tolerance, from the formats: both paths round the attention output and the projection to bf16
    (2 x 2^-8 relative to the contribution), and the block rounds h1 itself to bf16 (2^-9 |h1|)."""
    from ltx_amd import ops, transformer3d as T3
    cfg, params, d, _ = _tiny_case("attn1")
    cfg1 = dict(cfg, num_layers=1)
    params = {k: v.clone() for k, v in params.items() if "transformer_blocks.1." not in k}
    for k in ("attn2.to_out.0.weight", "attn2.to_out.0.bias", "ff.net.2.weight", "ff.net.2.bias"):
        params["transformer_blocks.0." + k].zero_()
    model = build_targets_model(cfg1, params, R_TINY, "attn1")
    seen = {}
    orig = T3._BlockFn.apply

    def recording(blk, sh, keep, skip, h, enc2, mods, onep, *ab):
        out = orig(blk, sh, keep, skip, h, enc2, mods, onep, *ab)
        seen.update(blk=blk, sh=sh, h=h, mods=mods, onep=onep, out=out)
        return out
    T3._BlockFn.apply = recording
    try:
        _sample(model, d)
    finally:
        del T3._BlockFn.apply  # back to torch.autograd.Function's own
    blk, sh, h, mods, onep, h1 = (seen[k] for k in ("blk", "sh", "h", "mods", "onep", "out"))
    B, N, D = sh.B, sh.N, sh.D
    with torch.no_grad():
        x1, _ = ops.rmsnorm_modulate_fwd(h, mods[:, 0], onep[:, 1], mods.stride(0), sh.rpm, blk.norm_eps)
        y = blk.attn1(x1.view(B, N, D), freqs_cis=sh.rope)
    c_proc = mods[:, 2].float()[:, None, :] * y.float().view(B, N, D)
    c_block = h1.float().view(B, N, D) - h.float().view(B, N, D)
    bound = 2 * 2.0 ** -8 + 2.0 ** -9 * float(h1.float().norm() / c_proc.norm())
    assert float(c_proc.norm()) > 0 and rel(c_block, c_proc) < bound, (rel(c_block, c_proc), bound)
