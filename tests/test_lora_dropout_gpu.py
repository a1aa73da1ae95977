"""LoRA dropout (peft lora_dropout) on the MI355X: the two kernels against the numpy statement of the
mask (ltx_lora_dropout_apply bitwise; ltx_lora_up_masked_add bitwise on exact inputs and within one
bf16 step of f64 on random ones) and the model under dropout against the reference's own step with
the same masks (tests/golden/tiny_lora_dropout_step, tools/gen_golden_lora_dropout.py), to the noise
criterion of tests/test_lora_ff_gpu.py (tests/model_utils.py noise_crit / loss_crit at their defaults)."""
import json
import os

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

import ltx_oracle as O
from lora_ff_utils import ff_params, train_config
from model_utils import build_step, grads_by_canonical, loss_crit, noise_crit
from params import canonical_name

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from ltx_amd import _lib as L
    L.ensure_device()
    return L


def _mask(key, sid, M, K, p):
    from ltx_amd.lora import lora_dropout_mask_reference
    return torch.from_numpy(lora_dropout_mask_reference(key, sid, M, K, p)).to(DEV)


def _bits(t):
    return t.view(torch.int16)


# ---------------------------------------------------------------------------------------------
# ltx_lora_dropout_apply
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", [0, 57])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("M,K", [(40, 128), (40, 8192), (4128, 128)])
def test_dropout_apply_is_bitwise_x_times_mask(M, K, p, sid):
    from ltx_amd import ops
    key = 0xA5A5F00D12345678
    T, _ = ops.lora_dropout_threshold(p)
    gen = torch.Generator(device="cpu").manual_seed(M + K)
    x = torch.randn(M, K, generator=gen).bfloat16().to(DEV)
    keep = _mask(key, sid, M, K, p)
    want = torch.where(keep, x, torch.zeros_like(x))
    got = ops.lora_dropout_apply(x, key, sid, T)
    assert torch.equal(_bits(got), _bits(want))
    assert 0 < int((~keep).sum()) < M * K
    # a row stride larger than K, in and out: the same rows, and nothing written beside them
    wide = torch.full((M, K + 64), 7.0, dtype=torch.bfloat16, device=DEV)
    wide[:, 8:8 + K] = x
    out = torch.full((M, K + 32), -3.0, dtype=torch.bfloat16, device=DEV)
    ops.lora_dropout_apply(wide[:, 8:8 + K], key, sid, T, out=out[:, 16:16 + K])
    assert torch.equal(_bits(out[:, 16:16 + K]), _bits(want))
    assert bool((out[:, :16] == -3.0).all()) and bool((out[:, 16 + K:] == -3.0).all())


# ---------------------------------------------------------------------------------------------
# ltx_lora_up_masked_add
# ---------------------------------------------------------------------------------------------
def _bf16_round(a64):
    """f64 numpy -> the nearest bf16 (as f64), through torch's round-to-nearest-even (f64 -> f32 is
    exact for the values used here or an extra rounding far below a bf16 step)."""
    return torch.from_numpy(a64).to(torch.float32).bfloat16().double().numpy()


def _exact_case(M, K, r, G, with_g, seed):
    """w in {-2..2}, A in {-1, 0, 1} / 8, dx multiples of 1/4 in [-4, 4], p = 0.5 (c = 2): every sum is
    exact in f32 and the result a bf16 value, so the kernel must give the numpy evaluation bitwise. The
    g case takes q in {0, 32767} (g = 0 or 2 * 32767 / 32767): t * q is still exact, the factor 2 / 32767
    is not, so the numpy evaluation follows the kernel's f32 operation order (t = c * sum;
    t = (t * q) * (2 / 32767 in f32); f32 add; one bf16 rounding), every step correctly rounded."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-2, 3, size=(M, G * r)).astype(np.float32)
    As = [rng.integers(-1, 2, size=(r, K)).astype(np.float32) / 8.0 for _ in range(G)]
    dx = rng.integers(-16, 17, size=(M, K)).astype(np.float32) / 4.0
    q = rng.choice(np.array([0, 32767], dtype=np.int16), size=(M, K)) if with_g else None
    return w, As, dx, q


def _masked_add_numpy_f32(w, As, dx, q, keeps, c):
    """the kernel's statement in f32 numpy (exact inputs: any summation order gives these values)"""
    r = As[0].shape[0]
    tot = np.zeros_like(dx, dtype=np.float32)
    for g, (A, keep) in enumerate(zip(As, keeps)):
        tot = tot + np.where(keep, w[:, g * r:(g + 1) * r] @ A, np.float32(0)).astype(np.float32)
    t = (tot * np.float32(c)).astype(np.float32)
    if q is not None:
        t = ((t * q.astype(np.float32)).astype(np.float32) * (np.float32(2.0) / np.float32(32767.0))).astype(np.float32)
    return (dx + t).astype(np.float32)


@pytest.mark.parametrize("M,K,r,G,with_g", [(64, 256, 8, 1, False), (64, 256, 16, 1, False), (64, 256, 32, 1, False),
                                            (64, 256, 64, 1, False), (64, 256, 128, 1, False),
                                            (64, 256, 16, 3, False), (64, 512, 16, 1, True)])
def test_masked_add_exact_inputs_bitwise(M, K, r, G, with_g):
    from ltx_amd import ops
    key, p = 0x0BADC0FFEE123457, 0.5
    T, c = ops.lora_dropout_threshold(p)
    assert T == 32768 and c == 2.0
    w, As, dx, q = _exact_case(M, K, r, G, with_g, seed=r + G + K)
    sids = [3 + 16 * g for g in range(G)]
    from ltx_amd.lora import lora_dropout_mask_reference
    keeps = [lora_dropout_mask_reference(key, s, M, K, p) for s in sids]
    want32 = _masked_add_numpy_f32(w, As, dx, q, keeps, c)
    want = torch.from_numpy(want32).bfloat16()
    if not with_g:  # exact all the way: the f32 value is itself a bf16 value
        assert torch.equal(want.float(), torch.from_numpy(want32))
    d = torch.from_numpy(dx).bfloat16().to(DEV)
    assert torch.equal(d.float().cpu(), torch.from_numpy(dx))
    got = ops.lora_up_masked_add(d, torch.from_numpy(w).to(DEV), [torch.from_numpy(a).to(DEV) for a in As], sids,
                                 key, T, c, g=None if q is None else torch.from_numpy(q).to(DEV))
    assert got is d
    assert torch.equal(_bits(d.cpu()), _bits(want))
    assert not torch.equal(d.float().cpu(), torch.from_numpy(dx))  # something was added


@pytest.mark.parametrize("M,K,r,G,with_g", [(200, 136, 16, 3, False), (130, 264, 64, 1, True), (72, 128, 8, 2, False)])
def test_masked_add_random_inputs(M, K, r, G, with_g):
    """p = 0.1, random operands, ragged M (no multiple of the 64-row block or the 16-row tile) and K (no
    multiple of the 128-column block), a strided dx: every element within one bf16 step of the f64
    evaluation rounded to bf16, none left out, nothing written outside, two runs bitwise equal."""
    from ltx_amd import ops
    from ltx_amd.lora import lora_dropout_mask_reference
    key, p = 0x1234567800000001, 0.1
    T, c = ops.lora_dropout_threshold(p)
    rng = np.random.default_rng(M + K + r)
    w = rng.standard_normal((M, G * r)).astype(np.float32)
    As = [(rng.standard_normal((r, K)) / np.sqrt(r)).astype(np.float32) for _ in range(G)]
    dx0 = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).bfloat16()
    q = (rng.integers(-5000, 32768, size=(M, K)).astype(np.int16)) if with_g else None
    sids = [9 + 16 * g for g in range(G)]
    keeps = [lora_dropout_mask_reference(key, s, M, K, p) for s in sids]
    tot = np.zeros((M, K))
    for g in range(G):
        tot += np.where(keeps[g], w[:, g * r:(g + 1) * r].astype(np.float64) @ As[g].astype(np.float64), 0.0)
    t = tot * float(c)
    if q is not None:
        t = t * q.astype(np.float64) * (2.0 / 32767.0)
    exact = dx0.double().numpy() + t
    want = _bf16_round(exact)
    outs = []
    for _ in range(2):
        buf = torch.full((M, K + 24), 5.0, dtype=torch.bfloat16, device=DEV)
        buf[:, 8:8 + K] = dx0.to(DEV)
        ops.lora_up_masked_add(buf[:, 8:8 + K], torch.from_numpy(w).to(DEV), [torch.from_numpy(a).to(DEV) for a in As],
                               sids, key, T, c, g=None if q is None else torch.from_numpy(q).to(DEV))
        assert bool((buf[:, :8] == 5.0).all()) and bool((buf[:, 8 + K:] == 5.0).all())
        outs.append(buf[:, 8:8 + K].cpu())
    assert torch.equal(_bits(outs[0].contiguous()), _bits(outs[1].contiguous()))
    got = outs[0].double().numpy()
    # one bf16 step (8 significant bits: 2^(e - 7) in the binade 2^e) of the rounded f64 value. The f32
    # sums carry up to ~2^-21 of the operands' magnitude (|dx| + |t| < 2^4: ~2^-17), which is a whole
    # bf16 step only for results below 2^-10 (dx and t cancelling): there the step of 2^-10 stands in
    mag = np.maximum(np.abs(want), 2.0 ** -10)
    step = 2.0 ** (np.floor(np.log2(mag)) - 7)
    worst = float(np.max(np.abs(got - want) / step))
    print(f"masked add M={M} K={K} r={r} G={G}: worst |got - bf16(f64)| = {worst:.3f} bf16 steps")
    assert worst <= 1.0
    # no element left out: wherever the masked term is not negligible the output moved off dx
    moved = np.abs(t) > np.abs(dx0.double().numpy()) * 2.0 ** -6 + 1e-3
    assert moved.any() and bool((got[moved] != dx0.double().numpy()[moved]).all())


# ---------------------------------------------------------------------------------------------
# the model (config T) against the reference's step under the same masks
# ---------------------------------------------------------------------------------------------
R_TINY = 8
_TINY = {}


def _golden():
    if "gold" not in _TINY:
        with open(os.path.join(GOLD, "tiny_lora_dropout_step.json")) as f:
            meta = json.load(f)
        raw = load_file(os.path.join(GOLD, "tiny_lora_dropout_step.safetensors"))
        shared = load_file(os.path.join(GOLD, meta["inputs_from"] + ".safetensors"))
        d = {k: v.to(DEV) for k, v in shared.items() if k.startswith("in.") or k in ("out.t", "out.noise")}
        d["out.noise"] = d["out.noise"].bfloat16()
        raw = {k: v.to(DEV) for k, v in raw.items()}
        cfg = meta["config"]
        params = ff_params(cfg, meta["param_seed"], R_TINY, targets=("attn1", "attn2"))
        l16 = float(((raw["out.sample"].float() - raw["out.v_target"].float()) ** 2).mean())
        refs = {torch.bfloat16: (raw["out.sample"], {k[5:]: v for k, v in raw.items() if k.startswith("grad.")}, l16),
                torch.float32: (raw["out32.sample"], {k[7:]: v for k, v in raw.items() if k.startswith("grad32.")},
                                float(raw["out32.loss"]))}
        _TINY["gold"] = (meta, cfg, params, d, refs)
    return _TINY["gold"]


def _build(cfg, params, p, key=None, set_attr=True):
    """The model with adapters on attn1 + attn2 + ff at config.lora_dropout = p (set_attr=False: the
    attribute left absent), in training mode."""
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.patchifier import SymmetricPatchifier
    from ltx_amd.transformer3d import Transformer3DModel
    tc = train_config(R_TINY, "attn1+attn2", True)
    if set_attr:
        setattr(tc, "lora_dropout", p)
    with torch.device("meta"):
        m = Transformer3DModel.from_config(cfg)
        apply_training_strategy(m, tc, "lora_audio")
    sd = {name: params[canonical_name(name)].detach().to(DEV).clone() for name, _ in m.named_parameters()}
    m.load_state_dict(sd, assign=True, strict=True)
    for n, q in m.named_parameters():
        q.requires_grad_(("lora_" in n) or ("caption_projection" in n))
    m.patchifier = SymmetricPatchifier(1)
    m.lora_dropout_key = key
    m.train()
    return m


def _sample(model, d, grad=False, expand=True):
    B = d["in.latents"].shape[0]
    tok, coords = O.patchify(d["in.latents"].bfloat16())
    x = O.add_noise(tok, d["out.noise"], d["out.t"]).bfloat16()
    enc, msk = d["in.prompt_embeds"].bfloat16(), d["in.prompt_attention_mask"]
    enc, msk = (enc.expand(B, -1, -1), msk.expand(B, -1)) if expand else (enc.repeat(B, 1, 1), msk.repeat(B, 1))
    with torch.enable_grad() if grad else torch.no_grad():
        return model(hidden_states=x, indices_grid=coords.to(DEV),
                     ref_image_hidden_states=d["in.ref_image_latents"].bfloat16(),
                     pose_hidden_states=d["in.pose_latents"].bfloat16(), encoder_hidden_states=enc,
                     timestep=d["out.t"], encoder_attention_mask=msk).sample


def _step(model, d):
    for q in model.parameters():
        q.grad = None
    lb = build_step(model, d)
    return lb, {k: v.clone() for k, v in grads_by_canonical(model).items()}


def _dropout_run():
    """one step of the dropout model under the golden's key, computed once and left unchanged"""
    if "run" not in _TINY:
        meta, cfg, params, d, _ = _golden()
        model = _build(cfg, params, meta["lora_dropout"], key=meta["lora_dropout_key"])
        _TINY["run"] = (model, *_step(model, d))
    return _TINY["run"]


def test_tiny_model_against_the_reference_step_under_dropout():
    """attn1 + attn2 + ff at p = 0.25 against the reference's own bf16 and fp32 steps with the same
    masks. Fails on the parent commit (config.lora_dropout is ignored there: no mask at all)."""
    meta, cfg, params, d, refs = _golden()
    model, lb, grads = _dropout_run()
    assert model.last_lora_dropout_key == meta["lora_dropout_key"]
    # the training-mode forward with grad enabled (train_step passes the shared-stride prompt)
    out = _sample(model, d, grad=True).detach()
    (s32, g32, l32), (s16, g16, l16) = refs[torch.float32], refs[torch.bfloat16]
    e = noise_crit("dropout sample", out, s16, s32)
    print(f"dropout: sample {e[0]:.3e} (ref bf16 {e[1]:.3e}) loss {lb:.6f} / {l16:.6f} / {l32:.6f}")
    loss_crit("dropout", lb, l16, l32)
    assert sorted(grads) == sorted(g32) == sorted(g16) and any("caption_projection" in k for k in g32)
    assert len([k for k in g32 if "lora_" in k]) == 2 * 10 * 2
    for k in g32:
        assert grads[k] is not None and float(grads[k].abs().max()) > 0, k
        e = noise_crit(f"dropout {k}", grads[k], g16[k], g32[k])
        print(f"dropout: {k} {e[0]:.3e} (ref bf16 {e[1]:.3e})")


def test_same_key_is_bitwise_and_another_key_differs():
    meta, cfg, params, d, _ = _golden()
    model, lb, grads = _dropout_run()
    lb2, again = _step(model, d)
    assert lb2 == lb
    for k in grads:
        assert torch.equal(again[k], grads[k]), k
    model.lora_dropout_key = meta["lora_dropout_key"] + 1
    try:
        _, other = _step(model, d)
        assert model.last_lora_dropout_key == meta["lora_dropout_key"] + 1
    finally:
        model.lora_dropout_key = meta["lora_dropout_key"]
    for k in grads:
        if "lora_A" in k:
            assert not torch.equal(other[k], grads[k]), k
    # no fixed key: one is drawn per forward from torch's default CPU generator
    model.lora_dropout_key = None
    try:
        torch.manual_seed(5)
        _sample(model, d, grad=True)
        k1 = model.last_lora_dropout_key
        _sample(model, d, grad=True)
        k2 = model.last_lora_dropout_key
        torch.manual_seed(5)
        _sample(model, d, grad=True)
        assert k1 != k2 and model.last_lora_dropout_key == k1 and 0 <= k1 < 2 ** 64
    finally:
        model.lora_dropout_key = meta["lora_dropout_key"]


def test_gradient_checkpointing_is_bitwise_under_dropout():
    meta, cfg, params, d, _ = _golden()
    model, lb, grads = _dropout_run()
    model.gradient_checkpointing = True
    try:
        lb2, ck = _step(model, d)
    finally:
        model.gradient_checkpointing = False
    assert lb2 == lb
    for k in grads:
        assert torch.equal(ck[k], grads[k]), k


def test_eval_and_no_grad_are_the_p0_model():
    meta, cfg, params, d, _ = _golden()
    model, _, _ = _dropout_run()
    plain = _build(cfg, params, 0.0)
    want = _sample(plain, d)
    dropped = _sample(model, d, grad=True).detach()
    assert not torch.equal(dropped, want)  # the training forward does drop
    assert torch.equal(_sample(model, d, grad=False), want)  # no_grad in training mode
    model.eval()
    try:
        assert torch.equal(_sample(model, d, grad=False), want)
        assert torch.equal(_sample(model, d, grad=True).detach(), want)  # eval() with grad enabled
    finally:
        model.train()


def test_shared_stride_prompt_takes_the_per_sample_text_path():
    """B = 2 with the prompt as a stride-0 expansion (the shared-prompt shortcut's trigger) gives bitwise
    the result of the same prompt materialised per sample, and the golden's per-sample masks show in the
    to_k / to_v adapters (test_tiny_model_against_the_reference_step_under_dropout runs on the expanded
    prompt): the shortcut is bypassed."""
    meta, cfg, params, d, _ = _golden()
    model, _, _ = _dropout_run()
    a = _sample(model, d, grad=True, expand=True).detach()
    b = _sample(model, d, grad=True, expand=False).detach()
    assert d["in.latents"].shape[0] == 2 and torch.equal(a, b)


def test_p0_launches_exactly_the_kernels_of_no_attribute():
    """config.lora_dropout = 0.0 and the attribute left absent: the same LaunchTimer kernel names, in
    order, for a training step, and bitwise the same gradients; with p > 0 the two new kernels appear."""
    from ltx_amd import ops
    meta, cfg, params, d, _ = _golden()
    names, res = [], []
    for set_attr in (True, False):
        m = _build(cfg, params, 0.0, set_attr=set_attr)
        timer = ops.LaunchTimer()
        ops.set_launch_timer(timer)
        try:
            res.append(_step(m, d))
        finally:
            ops.set_launch_timer(None)
        names.append([rec[0] for rec in timer.records])
        assert m.last_lora_dropout_key is None  # nothing was drawn
    assert names[0] == names[1] and len(names[0]) > 0
    assert not any("dropout" in n or "masked_add" in n for n in names[0])
    assert res[0][0] == res[1][0]
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    model, _, _ = _dropout_run()
    timer = ops.LaunchTimer()
    ops.set_launch_timer(timer)
    try:
        _step(model, d)
    finally:
        ops.set_launch_timer(None)
    got = [rec[0] for rec in timer.records]
    # per block: ten masked inputs each way, and seven masked adds in the backward (q / k / v share one,
    # to_k / to_v share one); the first block's input takes no gradient, so its dx1 add is not run
    assert sum(n == "ltx::lora_dropout_apply_kernel" for n in got) == 2 * 2 * 10
    assert sum(n.startswith("ltx::lora_up_masked_add_kernel") for n in got) == 2 * 7 - 1
