"""LoRA adapters on the feed-forward linears through the fused block on the MI355X: the one-pass
adapter backward at the feed-forward's widths (ltx_lora_dy_dA past N = 2048), the K = 8192
down-projection, the ring GEMM's GELU / GELU-backward / store / gated-residual epilogues with the K
extension, and the model with config.lora_ff against the reference's own step
(tests/golden/tiny_lora_ff_step) and against the chain-rule reference on the oracle
(tests/lora_ff_utils.py, validated in tests/test_lora_ff_cpu.py).

Tolerances are those of tests/test_kernels_gpu.py and tests/test_lora_ranks_gpu.py (f32 adapters as
exact three-piece bf16 products summed in f32: rel-Frobenius < 1e-5 against fp32 torch; bf16 GEMMs
< 1e-2 against fp32; the GELU derivative image within one code of ops.gelu_grad_q and 2^-14 of ATen)
and of tests/model_utils.py (noise_crit / loss_crit at their defaults)."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

import ltx_oracle as O
from lora_ff_utils import build_ff_model, chain_oracle_step, ff_params
from model_utils import build_model, build_step, grads_by_canonical, loss_crit, noise_crit, rel, synth_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from ltx_amd import _lib as L
    L.ensure_device()
    return L


def g(*shape, dtype=torch.bfloat16, scale=1.0, seed=0):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale).to(dtype).to(DEV)


# ---------------------------------------------------------------------------------------------
# kernels: the one-pass backward past N = 2048, and with the wide tensor as x
# ---------------------------------------------------------------------------------------------
def _dy_da_case(M, N, K, r):
    from ltx_amd import ops
    dy, x = g(M, N, seed=31), g(M, K, seed=32)
    u = torch.randn(M, r, device=DEV)
    Bm = torch.randn(N, r, device=DEV) * 0.05
    pieces = ops.lora_pieces(Bm, transposed=True)
    assert ops.lora_dy_fits(dy, r) and ops.lora_dy_da_fits(dy, x, r)
    dB0, dA0 = torch.randn(N, r, device=DEV), torch.randn(r, K, device=DEV)
    dB, dA = dB0.clone(), dA0.clone()
    w, sp = ops.lora_dy(dy, u, pieces, r, 0.5, dB, x=x, dA_out=dA)
    # bitwise the call without x, and lora_wgrad on that w
    dBs, dAs = dB0.clone(), dA0.clone()
    w1, sp1 = ops.lora_dy(dy, u, pieces, r, 0.5, dBs)
    ops.lora_wgrad(x, w1, transpose_out=True, out=dAs, accumulate=True)
    assert torch.equal(w, w1) and torch.equal(sp, sp1) and torch.equal(dB, dBs)
    assert torch.equal(dA, dAs)
    # a repeat call, bitwise
    dB2, dA2 = dB0.clone(), dA0.clone()
    w2, sp2 = ops.lora_dy(dy, u, pieces, r, 0.5, dB2, x=x, dA_out=dA2)
    assert torch.equal(w, w2) and torch.equal(sp, sp2) and torch.equal(dB, dB2) and torch.equal(dA, dA2)
    # fp32 torch
    assert rel(w, 0.5 * dy.float() @ Bm) < 1e-5
    assert rel(dB, dB0 + 0.5 * dy.float().t() @ u) < 1e-5
    assert rel(dA, dA0 + w.t() @ x.float()) < 1e-5


# N = 2560: five column partials, the smallest count past the old limit of four and no multiple of it;
# M = 2080 = 65 row groups: ragged for both row-group sizes (7 and 4 groups per block); ranks 8 / 32 /
# 64: both slice widths and a two-slice launch
@pytest.mark.parametrize("r", [8, 32, 64])
@pytest.mark.parametrize("M,N,K", [(2048, 2560, 512), (2080, 8192, 512), (2048, 8192, 2048)])
def test_lora_dy_da_wide(M, N, K, r):
    """Fails on the parent commit: lora_dy_da_fits is false past N = 2048 and ltx_lora_dy_dA returns a
    bad-argument error."""
    _dy_da_case(M, N, K, r)


@pytest.mark.parametrize("r", [8, 32, 64])
@pytest.mark.parametrize("M", [2048, 2080])
def test_lora_dy_da_wide_x(M, r):
    """The other orientation (ff.net.2's adapter): dY [M, 2048], x = the GELU output [M, 8192]."""
    _dy_da_case(M, 2048, 8192, r)


@pytest.mark.parametrize("r", [8, 32, 128])
@pytest.mark.parametrize("M", [2048, 2080])
def test_lora_rows_k8192(M, r):
    """u2 = act . A2^T: the token-sized down-projection at the feed-forward's inner width."""
    from ltx_amd import ops
    K = 8192
    x = g(M, K, seed=41)
    A = torch.randn(r, K, device=DEV) / K ** 0.5
    pieces = ops.lora_pieces(A)
    u, su = ops.lora_rows(x, pieces, r, alpha=0.5, split=True)
    assert rel(u, 0.5 * x.float() @ A.t()) < 1e-5
    assert torch.equal(su, ops.lora_split(u, "act"))
    u2, su2 = ops.lora_rows(x, pieces, r, alpha=0.5, split=True)
    assert torch.equal(u, u2) and torch.equal(su, su2)


# ---------------------------------------------------------------------------------------------
# the feed-forward GEMMs' epilogues with the K extension
# ---------------------------------------------------------------------------------------------
def _variant(v):
    from ltx_amd import _lib, ops
    _lib.load().ltx_gemm_set_variant(v)
    ops._GEMM_NAMES.clear()  # the name cache does not key on the variant


@pytest.mark.parametrize("K2", [64, 192])
@pytest.mark.parametrize("epi,M,N,K", [("gelu", 2048, 8192, 2048), ("gelu_bwd", 2048, 8192, 2048),
                                       ("store", 8192, 2048, 8192), ("gated_residual", 8192, 2048, 8192)])
def test_gemm_ff_epilogues_with_extension(epi, M, N, K, K2):
    """The four GEMMs of an adapted feed-forward (FF1 forward, the GELU backward, dx2 at the transposed
    shape, FF2 forward): the ring kernel against gemm_nt_kernel_t (variant 15) bitwise, and fp32."""
    import torch.nn.functional as F
    from ltx_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(K2 + len(epi))
    a = torch.randn(M, K, device="cuda", generator=gen).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5).bfloat16()
    a2 = torch.randn(M, K2, device="cuda", generator=gen).bfloat16()
    w2 = (torch.randn(N, K2, device="cuda", generator=gen) / K2 ** 0.5).bfloat16()
    b = torch.randn(N, device="cuda", generator=gen).bfloat16()
    nb = 4
    kw = {}
    if epi == "gelu_bwd":
        fq = ops.gelu_grad_q(torch.randn(M, N, device="cuda", generator=gen).bfloat16())
        kw = dict(aux0=fq)
        b = None
    elif epi == "gated_residual":
        res = torch.randn(M, N, device="cuda", generator=gen).bfloat16()
        gate = torch.randn(nb, N, device="cuda", generator=gen).bfloat16()
        kw = dict(aux0=res, aux1=gate, rows_per_batch=M // nb)
    outs, pres = [], []
    try:
        for v in (15, 0):
            _variant(v)
            if epi == "gelu":
                pres.append(torch.empty(M, N, dtype=torch.int16, device=DEV))
                kw = dict(aux0=pres[-1])
            outs.append(ops.gemm(a, w, bias=b, epilogue=epi, ext=(a2, w2), **kw))
        yb = ops.gemm(a, w, bias=b, ext=(a2, w2)) if epi == "gelu" else None
    finally:
        _variant(0)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    acc = a.float() @ w.float().t() + a2.float() @ w2.float().t() + (b.float() if b is not None else 0.0)
    if epi == "gelu":
        assert torch.equal(pres[0], pres[1])
        assert rel(outs[1], F.gelu(acc, approximate="tanh")) < 1e-2
        # the derivative image, as tests/test_kernels_gpu.py holds it: against the build's own bf16
        # pre-activation (the plain store with the same extension)
        dq = ops.gelu_grad_q(yb)
        assert int((pres[1].int() - dq.int()).abs().max()) <= 1
        assert float((pres[1].float() / ops.GELU_Q - torch.ops.aten.gelu_backward(
            torch.ones_like(yb, dtype=torch.float32), yb.float(), approximate="tanh")).abs().max()) < 2 ** -14
    elif epi == "gelu_bwd":
        assert rel(outs[1], acc * fq.float() * (2.0 / 32767.0)) < 1e-2
    elif epi == "store":
        assert rel(outs[1], acc) < 1e-2
    else:
        assert rel(outs[1], res.float() + gate.float().repeat_interleave(M // nb, 0) * acc) < 1e-2


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
R_TINY = 8
_TINY = {}


def _golden():
    if "gold" not in _TINY:
        with open(os.path.join(GOLD, "tiny_lora_ff_step.json")) as f:
            meta = json.load(f)
        raw = load_file(os.path.join(GOLD, "tiny_lora_ff_step.safetensors"))
        _TINY["gold"] = (meta, {k: v.to(DEV) for k, v in raw.items()})
    return _TINY["gold"]


def _tiny_inputs():
    _, raw = _golden()
    d = {k: v for k, v in raw.items() if k.startswith("in.") or k in ("out.t", "out.noise")}
    d["out.noise"] = d["out.noise"].bfloat16()
    return d


def _tiny_case(targets):
    """Config T (two layers), the inputs of the golden, r = 8. targets "attn2": the references are the
    golden's two runs of the reference itself. Other target sets (a tuple; () = feed-forward adapters
    only): the chain-rule reference on the oracle, fp32 and bf16, computed once and left unchanged.
    Returns (cfg, params, inputs, {dtype: (sample, grads, loss)})."""
    if targets not in _TINY:
        meta, raw = _golden()
        cfg, d = meta["config"], _tiny_inputs()
        if targets == "attn2":
            params = ff_params(cfg, meta["param_seed"], R_TINY)
            l16 = float(((raw["out.sample"].float() - raw["out.v_target"].float()) ** 2).mean())
            refs = {torch.bfloat16: (raw["out.sample"], {k[5:]: v for k, v in raw.items() if k.startswith("grad.")}, l16),
                    torch.float32: (raw["out32.sample"], {k[7:]: v for k, v in raw.items() if k.startswith("grad32.")},
                                    float(raw["out32.loss"]))}
        else:
            params = ff_params(cfg, meta["param_seed"], R_TINY, targets=targets)
            refs = {dt: chain_oracle_step(params, cfg, d, dt, device=DEV) for dt in (torch.float32, torch.bfloat16)}
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


def _against_refs(tag, model, d, refs, n_ff):
    out = _sample(model, d)
    lb = build_step(model, d)
    grads = {k: v.clone() if v is not None else None for k, v in grads_by_canonical(model).items()}
    (s32, g32, l32), (s16, g16, l16) = refs[torch.float32], refs[torch.bfloat16]
    e = noise_crit(f"{tag} sample", out, s16, s32)
    print(f"{tag}: sample {e[0]:.3e} (ref bf16 {e[1]:.3e}) loss {lb:.6f} / {l16:.6f} / {l32:.6f}")
    loss_crit(tag, lb, l16, l32)
    assert sorted(grads) == sorted(g32) == sorted(g16) and any("caption_projection" in k for k in g32)
    ff = [k for k in g32 if ".ff." in k and "lora_" in k]
    assert len(ff) == n_ff
    for k in g32:
        # (on the parent commit the feed-forward adapters cannot be placed at all)
        assert grads[k] is not None and float(grads[k].abs().max()) > 0, k
        e = noise_crit(f"{tag} {k}", grads[k], g16[k], g32[k])
        if ".ff." in k:
            print(f"{tag}: {k} {e[0]:.3e} (ref bf16 {e[1]:.3e})")
    return lb, grads


def test_tiny_model_against_the_reference_step():
    """attn2 + ff against the reference's own bf16 and fp32 steps (the golden's two runs)."""
    cfg, params, d, refs = _tiny_case("attn2")
    for k in params:
        if "lora_B" in k:  # with a zero B every dA is identically zero and the case proves nothing
            assert float(params[k].float().abs().max()) > 0, k
    model = build_ff_model(cfg, params, R_TINY, "attn2")
    _against_refs("tiny attn2+ff", model, d, refs, n_ff=8)


@pytest.mark.parametrize("targets", [("attn1", "attn2"), ()])
def test_tiny_model_against_the_chain_rule_reference(targets):
    """attn1 + attn2 + ff, and feed-forward adapters alone (inject_lora(..., feed_forward=True), no
    attention adapter): the oracle with merged feed-forward weights and the chain rule."""
    cfg, params, d, refs = _tiny_case(targets)
    model = build_ff_model(cfg, params, R_TINY, targets if targets == () else "+".join(targets))
    _against_refs(f"tiny {targets}+ff", model, d, refs, n_ff=8)


def test_gradient_checkpointing_is_bitwise():
    cfg, params, d, _ = _tiny_case("attn2")
    res = []
    for ckpt in (False, True):
        m = build_ff_model(cfg, params, R_TINY, "attn2")
        m.train()
        m.gradient_checkpointing = ckpt
        res.append((build_step(m, d), grads_by_canonical(m)))
    (l1, g1), (l2, g2) = res
    assert l1 == l2
    for k in g1:
        assert g2[k] is not None and torch.equal(g1[k], g2[k]), k


def test_forward_only_equals_training_forward():
    cfg, params, d, _ = _tiny_case("attn2")
    model = build_ff_model(cfg, params, R_TINY, "attn2")
    a = _sample(model, d, grad=False)
    b = _sample(model, d, grad=True)
    assert b.requires_grad and torch.equal(a, b.detach())


@pytest.mark.parametrize("ff", [None, False])
def test_without_lora_ff_the_step_is_bitwise_todays(ff):
    """No lora_ff (or False): outputs and gradients of one step are bitwise those of a model built by
    the unchanged tests/model_utils.build_model."""
    cfg, params, d, _ = _tiny_case("attn2")
    a = build_model(cfg, params, R_TINY, device=DEV)
    b = build_ff_model(cfg, params, R_TINY, None, ff=ff)
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    assert torch.equal(_sample(a, d), _sample(b, d))
    la, lb = build_step(a, d), build_step(b, d)
    ga, gb = grads_by_canonical(a), grads_by_canonical(b)
    assert la == lb
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_full_mode_with_ff_adapters_raises():
    """train_mode='full' on a model that carries feed-forward adapters raises before the first launch."""
    from ltx_amd.lora import inject_lora, lora_ff_target_modules
    from model_utils import build_full_model
    cfg, _, d, _ = _tiny_case("attn2")
    model = build_full_model(cfg, O.make_params(cfg, 77, lora_rank=0, requires_grad=False), device=DEV)
    inject_lora(model, lora_ff_target_modules(len(model.transformer_blocks)), R_TINY, R_TINY, feed_forward=True)
    with pytest.raises(NotImplementedError, match="without LoRA"):
        build_step(model, d)


def test_unload_repacks_the_ff_weights():
    """After unload_lora the forward is bitwise that of a plain model loaded from merged_state_dict
    (a stale ff1_wT / ff2_wT or forward weight would show)."""
    from ltx_amd.lora import merged_state_dict, unload_lora
    from ltx_amd.patchifier import SymmetricPatchifier
    from ltx_amd.transformer3d import Transformer3DModel
    cfg, params, d, _ = _tiny_case("attn2")
    model = build_ff_model(cfg, params, R_TINY, "attn2")
    adapted = _sample(model, d)
    build_step(model, d)  # the backward packs ff1_wT / ff2_wT
    blk = model.transformer_blocks[0]
    before = blk.packed()["ff2_wT"].clone()
    sd = {k: v.clone() for k, v in merged_state_dict(model).items()}
    unload_lora(model)
    assert not torch.equal(blk.packed()["ff2_wT"], before)
    assert torch.equal(blk.packed()["ff2_wT"], blk.ff.net[2].weight.t())
    with torch.device("meta"):
        plain = Transformer3DModel.from_config(cfg)
    plain.load_state_dict(sd, assign=True, strict=True)
    plain.patchifier = SymmetricPatchifier(1)
    a, b = _sample(model, d), _sample(plain, d)
    assert torch.equal(a, b)
    # the merged model computes the adapted one's function up to the bf16 rounding of W + s B A
    assert rel(a, adapted) < 2e-2 and not torch.equal(a, adapted)


_BLOCK = {}


def _block_case(r):
    """One LTX-2B-width block, B = 8 samples of 2x16x16 (N = 512, M = 4096: past the token-sized gates),
    one shared prompt of 256 tokens (16 valid), adapters on attn2 + ff; the chain-rule references,
    computed once per rank and left unchanged."""
    if r not in _BLOCK:
        from ltx_amd.transformer3d import OURS_TRANSFORMER_CONFIG
        cfg = dict(OURS_TRANSFORMER_CONFIG, num_layers=1)
        params = ff_params(cfg, 400 + r, r)
        d = synth_inputs(8, 2, 16, 16, 256, 16, seed=23 + r, device=DEV)
        refs = {dt: chain_oracle_step(params, cfg, d, dt, device=DEV) for dt in (torch.float32, torch.bfloat16)}
        _BLOCK[r] = (cfg, params, d, refs)
    return _BLOCK[r]


@pytest.mark.parametrize("r", [16, 64])
def test_block_2b_width_against_the_chain_rule_reference(r):
    """The fp32 reference is the oracle with merged feed-forward weights plus the chain rule, which is
    exact. The bf16 yardstick is the same construction on the oracle's bf16 run, whose merged weight
    W + s B A is rounded to bf16 where the reference keeps B and A in fp32 beside a bf16 W: a PROXY for
    the reference's bf16 noise, not the reference. tests/golden/tiny_lora_ff_step is the check against
    the real bf16 reference (test_tiny_model_against_the_reference_step)."""
    cfg, params, d, refs = _block_case(r)
    model = build_ff_model(cfg, params, r, "attn2")
    lb, grads = _against_refs(f"2b r={r}", model, d, refs, n_ff=4)
    # a second identical step: bitwise the same gradients (fixed-order partial sums, no atomics)
    for p in model.parameters():
        p.grad = None
    lb2 = build_step(model, d)
    again = grads_by_canonical(model)
    assert lb2 == lb
    for k in grads:
        assert torch.equal(again[k], grads[k]), k


def test_block_2b_width_merged_wide_backward_equals_separate(monkeypatch):
    """LTX_LORA_FF_DY_DA=1 runs the feed-forward adapters' backward through the merged ltx_lora_dy_dA
    (for dY = d_f [M, 8192] the wide dA pass) where the default keeps dA a separate ltx_lora_wgrad
    call, and LTX_LORA_DY_DA=0 keeps every adapter's dA separate: the same dB, dA and, through w, the
    same upstream gradients, bitwise; so are the kept and the recomputed x2."""
    cfg, params, d, _ = _block_case(16)
    res = []
    for env in ({"LTX_LORA_FF_DY_DA": "1"}, {}, {"LTX_LORA_FF_DY_DA": "1", "LTX_LORA_DY_DA": "0"},
                {"LTX_LORA_FF_DY_DA": "1", "LTX_LORA_FF_KEEP_X2": "0"}):
        for var in ("LTX_LORA_FF_DY_DA", "LTX_LORA_DY_DA", "LTX_LORA_FF_KEEP_X2"):
            monkeypatch.delenv(var, raising=False)
        for var, flag in env.items():
            monkeypatch.setenv(var, flag)
        model = build_ff_model(cfg, params, 16, "attn2")
        res.append((build_step(model, d), grads_by_canonical(model)))
    for other in res[1:]:
        assert res[0][0] == other[0]
        for k in res[0][1]:
            assert torch.equal(res[0][1][k], other[1][k]), k
