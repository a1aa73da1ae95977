"""DoRA (peft use_dora) on the MI355X: the kernels of csrc/dora.hip (ltx_dora_fold bitwise on exactly
representable inputs and against float64 on random ones, ltx_dora_mag_grad likewise, the dB row scale)
and the model: a fresh DoRA adapter (c = 1) is bitwise plain LoRA, the tiny model against the
reference's own DoRA step (tests/golden/tiny_lora_dora_step, tools/gen_golden_lora_dora.py) to the
noise criterion of tests/test_lora_ff_gpu.py (tests/model_utils.py noise_crit / loss_crit at their
defaults), determinism, the cache refresh after an optimizer step, export, and the off switch.
Every test here fails on the parent commit (no ltx_dora_* entry points, no use_dora)."""
import os

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

import ltx_oracle as O
from lora_attn1_utils import attn1_params
from lora_dora_utils import GOLD, MAG, NAME, build_dora_model, dora_names, golden_meta, golden_params
from model_utils import build_model, build_step, grads_by_canonical, loss_crit, noise_crit, synth_inputs
from params import canonical_name

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS32 = 2.0 ** -23


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from ltx_amd import _lib as L
    L.ensure_device()
    return L


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------
# ltx_dora_fold
# ---------------------------------------------------------------------------------------------
def _exact_fold_case(N, K, r, seed):
    """s = 1/2, B in {-2, 0, 2} (s B in {-1, 0, 1}), A in {-1, 0, 1}, V = W + s B A with 4^e entries of
    +-1 per row and zeros elsewhere, so ||V_j|| = 2^e exactly; W = V - s B A are integers of magnitude
    <= r + 1 <= 129 (bf16 values). m_j = +-2^q ||V_j||: c_j = +-2^q, and c W, c s B are exact. Row 1 has
    m = 0, row 2 has V = 0 (norm 0: c = 0 by the kernel's rule), row 3 a negative m."""
    rng = np.random.default_rng(seed)
    s = 0.5
    A = rng.integers(-1, 2, size=(r, K)).astype(np.float64)
    B = 2.0 * rng.integers(-1, 2, size=(N, r)).astype(np.float64)
    V = np.zeros((N, K))
    emax = 3 if K == 128 else 5
    for j in range(N):
        e = int(rng.integers(0, emax + 1))
        idx = rng.choice(K, size=4 ** e, replace=False)
        V[j, idx] = rng.choice([-1.0, 1.0], size=4 ** e)
    V[2] = 0.0
    W = V - s * (B @ A)
    assert np.abs(W).max() <= 129
    norm = np.sqrt((V * V).sum(1))
    q = rng.integers(-2, 3, size=N).astype(np.float64)
    m = norm * 2.0 ** q
    m[1] = 0.0
    m[2] = 3.0
    m[3] = -m[3]
    c = np.where(norm != 0, m / np.where(norm != 0, norm, 1.0), 0.0)
    return s, W, A, B, m, norm, c


@pytest.mark.parametrize("r", [8, 32, 128])
@pytest.mark.parametrize("K", [128, 2048])
@pytest.mark.parametrize("N", [16, 40])
def test_dora_fold_exact_inputs_bitwise(N, K, r):
    from ltx_amd import ops
    s, W, A, B, m, norm, c = _exact_fold_case(N, K, r, seed=N + K + r)
    f32 = lambda a: torch.from_numpy(a).to(torch.float32)
    Wb = f32(W).bfloat16()
    assert torch.equal(Wb.double(), torch.from_numpy(W))  # the inputs are bf16 values
    want_w = (f32(c)[:, None] * Wb.float()).bfloat16()
    assert torch.equal(want_w.double(), torch.from_numpy(c[:, None] * W))  # and so are the outputs
    want_sb = f32(c[:, None] * (s * B))
    for strided in (False, True):
        if strided:  # W a column block of a wider buffer (ldw > K), B a column block too
            wide = torch.full((N, K + 72), 7.0, dtype=torch.bfloat16, device=DEV)
            wide[:, 8:8 + K] = Wb.to(DEV)
            Wd = wide[:, 8:8 + K]
            bw = torch.full((N, r + 3), 5.0, dtype=torch.float32, device=DEV)
            bw[:, 1:1 + r] = f32(B).to(DEV)
            Bd = bw[:, 1:1 + r]
        else:
            Wd, Bd = Wb.to(DEV), f32(B).to(DEV)
        gn, gc, gw, gwT, gsb = ops.dora_fold(Wd, f32(A).to(DEV), Bd, f32(m).to(DEV), s)
        assert torch.equal(gn.cpu(), f32(norm)) and torch.equal(gc.cpu(), f32(c))
        assert float(gc[1]) == 0.0 and float(gn[2]) == 0.0 and float(gc[2]) == 0.0 and float(gc[3]) < 0
        assert torch.equal(_bits(gw.cpu()), _bits(want_w))
        assert tuple(gwT.shape) == (K, N) and torch.equal(_bits(gwT.cpu()), _bits(want_w.t()))
        assert torch.equal(gsb.cpu(), want_sb)
        assert float(gw[1].float().abs().max()) == 0.0 and float(gw[0].float().abs().max()) > 0.0
        # the existing split / pieces kernels consume c (.) s B unchanged
        assert torch.equal(_bits(ops.lora_split(gsb, "weight", 1.0)),
                           _bits(ops.lora_split(want_sb.to(DEV), "weight", 1.0)))


@pytest.mark.parametrize("r", [16, 128])
def test_dora_fold_random_inputs(r):
    """N = 200 (and 203, no multiple of the 8 rows a workgroup owns), K = 2048, m = norm |1 + 0.2 randn|:
    norm and c against the float64 statement, at most twice the error of torch's own f32
    statement linalg.norm(W.float() + s B @ A, dim=1) on the same inputs plus 2^-23 (relative, maximum
    over the rows); W_eff against bf16(c64 W): every element within one bf16 step, at most 1 % of them
    different at all (a c off by 1e-6 relative moves about 5e-4 of the products across a rounding
    boundary; the f32 torch statement is held to the same cap first, on the CPU)."""
    from ltx_amd import ops
    for N in (200, 203):
        K, s = 2048, 0.75
        g = torch.Generator().manual_seed(1000 + r + N)
        W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
        A = torch.randn(r, K, generator=g) / K ** 0.5
        B = 0.05 * torch.randn(N, r, generator=g)
        n64 = torch.linalg.norm(W.double() + s * (B.double() @ A.double()), dim=1)
        m = (n64 * (1 + 0.2 * torch.randn(N, generator=g, dtype=torch.float64)).abs()).float()
        c64 = m.double() / n64
        n32 = torch.linalg.norm(W.float() + s * (B @ A), dim=1)  # torch's f32 statement, on the CPU
        c32 = m / n32
        gn, gc, gw, gwT, gsb = ops.dora_fold(W.to(DEV), A.to(DEV), B.to(DEV), m.to(DEV), s)
        relmax = lambda a, ref: float(((a.double() - ref).abs() / ref.abs()).max())
        en_t, en_k = relmax(n32, n64), relmax(gn.cpu(), n64)
        ec_t, ec_k = relmax(c32, c64), relmax(gc.cpu(), c64)
        print(f"fold N={N} r={r}: norm rel err kernel {en_k:.3e} torch f32 {en_t:.3e}; c kernel {ec_k:.3e} torch {ec_t:.3e}")
        assert en_k <= 2 * en_t + EPS32 and ec_k <= 2 * ec_t + EPS32
        want = (c64[:, None] * W.double()).float().bfloat16()
        stmt = (c32[:, None] * W.float()).bfloat16()
        frac_t = float((_bits(stmt) != _bits(want)).float().mean())
        frac_k = float((_bits(gw.cpu()) != _bits(want)).float().mean())
        print(f"fold N={N} r={r}: W_eff elements off bf16(c64 W): kernel {frac_k:.2e}, torch f32 statement {frac_t:.2e}")
        assert frac_t < 0.01  # the cap is usable on this seed
        assert frac_k <= 0.01
        # within one bf16 step: adjacent bf16 bit patterns (no sign change at these magnitudes)
        d = (_bits(gw.cpu()).int() - _bits(want).int()).abs()
        assert int(d.max()) <= 1
        assert torch.equal(_bits(gwT.cpu()), _bits(gw.cpu().t()))
        e_sb = relmax(gsb.cpu(), c64[:, None] * (s * B.double()) + 1e-300)
        assert e_sb <= 2 * ec_t + 3 * EPS32, e_sb  # c (.) s B: two more f32 roundings (s B, then c x)


# ---------------------------------------------------------------------------------------------
# ltx_dora_mag_grad and the dB row scale
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [128, 2048])
@pytest.mark.parametrize("M", [32, 200, 4096])
def test_dora_mag_grad_exact_inputs_bitwise(M, N):
    """dY in {-2..2}, Y in {-4..4}, b in {-1, 0, 1}, m = +-2^q (one column 0): every product and sum is
    exact in f32, so the kernel gives the numpy evaluation bitwise. dY and Y are column blocks of wider
    buffers (ld > N); bias present and null; accumulate on and off."""
    from ltx_amd import ops
    rng = np.random.default_rng(M + N)
    dY = rng.integers(-2, 3, size=(M, N)).astype(np.float32)
    Y = rng.integers(-4, 5, size=(M, N)).astype(np.float32)
    b = rng.integers(-1, 2, size=N).astype(np.float32)
    m = (2.0 ** rng.integers(-1, 3, size=N) * rng.choice([-1.0, 1.0], size=N)).astype(np.float32)
    m[7] = 0.0
    out0 = (rng.integers(-16, 17, size=N) / 4.0).astype(np.float32)
    wide_dy = torch.full((M, N + 24), 9.0, dtype=torch.bfloat16, device=DEV)
    wide_y = torch.full((M, 2 * N + 8), -9.0, dtype=torch.bfloat16, device=DEV)
    wide_dy[:, 16:16 + N] = torch.from_numpy(dY).to(DEV)
    wide_y[:, N:2 * N] = torch.from_numpy(Y).to(DEV)
    dy_v, y_v = wide_dy[:, 16:16 + N], wide_y[:, N:2 * N]
    for bias in (b, None):
        tot = (dY.astype(np.float64) * (Y - (0 if bias is None else bias)).astype(np.float64)).sum(0)
        assert np.abs(tot).max() < 2 ** 24
        safe = np.where(m != 0, m, np.float32(1))
        val = np.where(m != 0, (np.float32(1) / safe) * tot.astype(np.float32), np.float32(0)).astype(np.float32)
        bt = None if bias is None else torch.from_numpy(bias).bfloat16().to(DEV)
        for acc in (False, True):
            out = torch.from_numpy(out0).to(DEV)
            got = ops.dora_mag_grad(dy_v, y_v, bt, torch.from_numpy(m).to(DEV), out, accumulate=acc)
            assert got is out
            want = (out0 + val).astype(np.float32) if acc else val
            assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), (bias is None, acc)
            assert float(out[7]) == (float(out0[7]) if acc else 0.0)
    assert float(np.abs(val).max()) > 0


def test_dora_mag_grad_random_inputs():
    """Ragged M, ld > N: against float64, at most twice the error of torch's own f32 statement
    (dY.float() * (Y.float() - b.float())).sum(0) / m on the same inputs plus 2^-23 (maximum over the
    columns, relative to the largest |dm|); two calls bitwise equal."""
    from ltx_amd import ops
    M, N = 1003, 264
    g = torch.Generator().manual_seed(77)
    dY = torch.randn(M, N, generator=g).bfloat16()
    Y = torch.randn(M, N, generator=g).bfloat16()
    b = (0.1 * torch.randn(N, generator=g)).bfloat16()
    m = (1 + 0.2 * torch.randn(N, generator=g)).abs().float() + 0.1
    ref = (dY.double() * (Y.double() - b.double())).sum(0) / m.double()
    stmt = (dY.float() * (Y.float() - b.float())).sum(0) / m
    wide = torch.zeros(M, 2 * N + 16, dtype=torch.bfloat16, device=DEV)
    wide[:, 8:8 + N], wide[:, 16 + N:16 + 2 * N] = dY.to(DEV), Y.to(DEV)
    outs = []
    for _ in range(2):
        out = torch.empty(N, dtype=torch.float32, device=DEV)
        ops.dora_mag_grad(wide[:, 8:8 + N], wide[:, 16 + N:16 + 2 * N], b.to(DEV), m.to(DEV), out, accumulate=False)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    scale = float(ref.abs().max())
    e_k = float((outs[0].double() - ref).abs().max()) / scale
    e_t = float((stmt.double() - ref).abs().max()) / scale
    print(f"mag_grad M={M} N={N}: max err / max|dm| kernel {e_k:.3e}, torch f32 statement {e_t:.3e}")
    assert e_k <= 2 * e_t + EPS32


def test_dora_rowscale_add_exact():
    from ltx_amd import ops
    rng = np.random.default_rng(5)
    N, r = 40, 16
    src = rng.integers(-8, 9, size=(N, r)).astype(np.float32)
    c = (2.0 ** rng.integers(-2, 3, size=N)).astype(np.float32)
    g0 = rng.integers(-4, 5, size=(N, r)).astype(np.float32)
    want = g0 + (0.5 * c)[:, None] * src
    out = torch.from_numpy(g0).to(DEV)
    ops.dora_rowscale_add(out, torch.from_numpy(src).to(DEV), torch.from_numpy(c).to(DEV), 0.5)
    assert np.array_equal(out.cpu().numpy(), want)
    outT = torch.from_numpy(np.ascontiguousarray(g0.T)).to(DEV)
    ops.dora_rowscale_add(outT, torch.from_numpy(src).to(DEV), torch.from_numpy(c).to(DEV), 0.5, transpose_out=True)
    assert np.array_equal(outT.cpu().numpy(), want.T)


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
R_TINY = 8
_TINY = {}


def _golden():
    if "gold" not in _TINY:
        meta = golden_meta()
        raw = load_file(os.path.join(GOLD, NAME + ".safetensors"))
        shared = load_file(os.path.join(GOLD, meta["inputs_from"] + ".safetensors"))
        d = {k: v.to(DEV) for k, v in shared.items() if k.startswith("in.") or k in ("out.t", "out.noise")}
        d["out.noise"] = d["out.noise"].bfloat16()
        params = golden_params(meta, raw)
        raw = {k: v.to(DEV) for k, v in raw.items()}
        l16 = float(((raw["out.sample"].float() - raw["out.v_target"].float()) ** 2).mean())
        refs = {torch.bfloat16: (raw["out.sample"], {k[5:]: v for k, v in raw.items() if k.startswith("grad.")}, l16),
                torch.float32: (raw["out32.sample"], {k[7:]: v for k, v in raw.items() if k.startswith("grad32.")},
                                float(raw["out32.loss"]))}
        _TINY["gold"] = (meta, meta["config"], params, d, refs)
    return _TINY["gold"]


def _per_sample(d):
    """the same batch with the prompt materialised per sample (no stride-0 expansion: the per-sample
    text path, K / V of B L text rows)"""
    B = d["in.latents"].shape[0]
    e = dict(d)
    e["in.prompt_embeds"] = d["in.prompt_embeds"].repeat(B, 1, 1)
    e["in.prompt_attention_mask"] = d["in.prompt_attention_mask"].repeat(B, 1)
    return e


def _sample(model, d, grad=False):
    B = d["in.latents"].shape[0]
    tok, coords = O.patchify(d["in.latents"].bfloat16())
    x = O.add_noise(tok, d["out.noise"], d["out.t"]).bfloat16()
    enc, msk = d["in.prompt_embeds"].bfloat16(), d["in.prompt_attention_mask"]
    if enc.shape[0] != B:
        enc, msk = enc.expand(B, -1, -1), msk.expand(B, -1)
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


def _dora_run():
    """one step of the golden DoRA model with the shared prompt, computed once and left unchanged"""
    if "run" not in _TINY:
        meta, cfg, params, d, _ = _golden()
        model = build_dora_model(cfg, params, R_TINY)
        model.train()
        _TINY["run"] = (model, *_step(model, d))
    return _TINY["run"]


@pytest.mark.parametrize("prompt", ["shared", "per_sample"])
def test_tiny_model_against_the_golden_dora_step(prompt):
    """The reference's own bf16 and fp32 DoRA steps (m = norm (1 + 0.2 randn), B non-zero): noise_crit at
    its defaults on the sample and on every trainable gradient, the eight magnitude vectors included,
    loss_crit on the loss; with the shared prompt (batch-summed dK / dV as the magnitudes' dY) and with
    per-sample prompts."""
    meta, cfg, params, d, refs = _golden()
    if prompt == "shared":
        model, lb, grads = _dora_run()
        dd = d
    else:
        dd = _per_sample(d)
        model = build_dora_model(cfg, params, R_TINY)
        model.train()
        lb, grads = _step(model, dd)
    out = _sample(model, dd)
    (s32, g32, l32), (s16, g16, l16) = refs[torch.float32], refs[torch.bfloat16]
    e = noise_crit(f"dora {prompt} sample", out, s16, s32)
    print(f"dora {prompt}: sample {e[0]:.3e} (ref bf16 {e[1]:.3e}) loss {lb:.6f} / {l16:.6f} / {l32:.6f}")
    loss_crit(f"dora {prompt}", lb, l16, l32)
    assert sorted(grads) == sorted(g32) == sorted(g16) and any("caption_projection" in k for k in g32)
    assert len([k for k in g32 if k.endswith(MAG)]) == 8 and len([k for k in g32 if "lora_" in k]) == 24
    for k in g32:
        assert grads[k] is not None and float(grads[k].abs().max()) > 0, k
        e = noise_crit(f"dora {prompt} {k}", grads[k], g16[k], g32[k])
        if "lora_" in k:
            print(f"dora {prompt}: {k} {e[0]:.3e} (ref bf16 {e[1]:.3e})")


def test_two_steps_and_gradient_checkpointing_are_bitwise():
    meta, cfg, params, d, _ = _golden()
    model, lb, grads = _dora_run()
    lb2, again = _step(model, d)
    assert lb2 == lb
    for k in grads:
        assert torch.equal(again[k], grads[k]), k
    model.gradient_checkpointing = True
    try:
        lb3, ck = _step(model, d)
    finally:
        model.gradient_checkpointing = False
    assert lb3 == lb
    for k in grads:
        assert torch.equal(ck[k], grads[k]), k
    # forward only (no_grad) is the training forward
    assert torch.equal(_sample(model, d), _sample(model, d, grad=True).detach())


def _set_fresh_magnitudes(model):
    """m <- the fold kernel's own norm, so c = m / norm = 1 exactly (what a freshly wrapped adapter has)"""
    from ltx_amd.transformer3d import LoraLinear
    n = 0
    for lin in model.modules():
        if isinstance(lin, LoraLinear):
            norm = lin.dora_operands()["norm"].clone()
            with torch.no_grad():
                lin.lora_magnitude_vector["default"].weight.copy_(norm)
            op = lin.dora_operands()
            assert bool((op["c"] == 1.0).all()) and torch.equal(_bits(op["w"]), _bits(lin.base_layer.weight))
            n += 1
    return n


def _fresh_is_plain(cfg, params, d, r, monkeypatch):
    """A DoRA model with c = 1 against a plain-LoRA model holding the same A and B (B non-zero). The DoRA
    model takes the per-block text path (it has no text stack); the plain model is put on the same path
    with the existing LTX_TEXT_BATCH switch: the environment variable is read once at import into
    transformer3d._TEXT_BATCH, which is set to False here for both models."""
    import ltx_amd.transformer3d as T
    monkeypatch.setattr(T, "_TEXT_BATCH", False)
    for k in params:
        if "lora_B" in k:
            assert float(params[k].float().abs().max()) > 0, k
    plain = build_model(cfg, params, r, device=DEV)
    dora = build_dora_model(cfg, params, r)
    assert plain._text_structure() is None and dora._text_structure() is None
    assert _set_fresh_magnitudes(dora) == 4 * cfg["num_layers"]
    plain.train(), dora.train()
    assert torch.equal(_bits(_sample(plain, d)), _bits(_sample(dora, d)))
    (lp, gp), (ld, gd) = _step(plain, d), _step(dora, d)
    assert lp == ld
    assert sorted(gp) == sorted(k for k in gd if not k.endswith(MAG)) and len(gd) == len(gp) + 4 * cfg["num_layers"]
    for k in gp:
        assert torch.equal(gp[k], gd[k]), k
    return gd


def test_fresh_dora_is_plain_lora_bitwise_tiny(monkeypatch):
    meta, cfg, params, d, _ = _golden()
    gd = _fresh_is_plain(cfg, {k: v for k, v in params.items() if not k.endswith(MAG)}, d, R_TINY, monkeypatch)
    assert all(float(gd[k].abs().max()) > 0 for k in gd if k.endswith(MAG))


def test_fresh_dora_is_plain_lora_bitwise_block_2b(monkeypatch):
    """One block at LTX-2B widths (D = 2048) with B = 4 samples of 2 x 16 x 16 (2048 token rows: the ring
    GEMM classes, ltx_lora_dy_dA and the 256-column grouped K-extension forms on the effective operands);
    the magnitude gradients are finite and non-zero."""
    from ltx_amd.transformer3d import OURS_TRANSFORMER_CONFIG
    r = 16
    cfg = dict(OURS_TRANSFORMER_CONFIG, num_layers=1)
    params = attn1_params(cfg, 500 + r, r, targets=("attn2",))
    d = synth_inputs(4, 2, 16, 16, 256, 16, seed=41, device=DEV)
    gd = _fresh_is_plain(cfg, params, d, r, monkeypatch)
    mags = [k for k in gd if k.endswith(MAG)]
    assert len(mags) == 4
    for k in mags:
        assert bool(torch.isfinite(gd[k]).all()) and float(gd[k].abs().max()) > 0, k


def test_forward_after_an_optimizer_step_uses_the_stepped_weights():
    """One FusedAdamW step (in-place kernel updates, no torch version bump), then the forward equals,
    bitwise, that of a fresh model loaded from the stepped state dict: a stale W_eff, W_eff^T or
    c (.) s B would show."""
    from ltx_amd.training import FusedAdamW
    meta, cfg, params, d, _ = _golden()
    model = build_dora_model(cfg, params, R_TINY)
    model.train()
    before = _sample(model, d)
    _step(model, d)
    FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-2).step()
    after = _sample(model, d)
    assert not torch.equal(before, after)
    stepped = {canonical_name(n): p.detach().clone() for n, p in model.named_parameters()}
    for n in dora_names(cfg["num_layers"]):
        assert not torch.equal(stepped[n + MAG].cpu(), params[n + MAG])
    fresh = build_dora_model(cfg, stepped, R_TINY)
    fresh.train()
    assert torch.equal(_bits(after), _bits(_sample(fresh, d)))
    # ... and the backward's operands too
    (l1, g1), (l2, g2) = _step(model, d), _step(fresh, d)
    assert l1 == l2
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_unload_equals_a_model_loaded_from_the_merged_dict():
    from ltx_amd.lora import merged_state_dict, unload_lora
    from ltx_amd.patchifier import SymmetricPatchifier
    from ltx_amd.transformer3d import Transformer3DModel
    from model_utils import rel
    meta, cfg, params, d, _ = _golden()
    model = build_dora_model(cfg, params, R_TINY)
    adapted = _sample(model, d)
    sd = {k: v.clone() for k, v in merged_state_dict(model).items()}
    assert not any("lora_" in k for k in sd)
    unload_lora(model)
    with torch.device("meta"):
        plain = Transformer3DModel.from_config(cfg)
    plain.load_state_dict(sd, assign=True, strict=True)
    plain.patchifier = SymmetricPatchifier(1)
    a, b = _sample(model, d), _sample(plain, d)
    assert torch.equal(a, b)
    # the merged model computes the adapted one's function up to the bf16 rounding of c (W + s B A)
    assert rel(a, adapted) < 2e-2 and not torch.equal(a, adapted)


def test_use_dora_false_launches_exactly_the_kernels_of_plain_lora():
    """config.use_dora = False and the attribute left absent: the LaunchTimer kernel names of a training
    step, in order, are those of a model built by the unchanged tests/model_utils.build_model, with
    bitwise the same gradients and no DoRA kernel; with use_dora the three new kernels appear."""
    from ltx_amd import ops
    meta, cfg, params, d, _ = _golden()
    plain_params = {k: v for k, v in params.items() if not k.endswith(MAG)}
    names, res = [], []
    for how in ("build_model", False, None):
        m = (build_model(cfg, plain_params, R_TINY, device=DEV) if how == "build_model"
             else build_dora_model(cfg, plain_params, R_TINY, dora=how))
        m.train()
        timer = ops.LaunchTimer()
        ops.set_launch_timer(timer)
        try:
            res.append(_step(m, d))
        finally:
            ops.set_launch_timer(None)
        names.append([rec[0] for rec in timer.records])
    assert names[0] == names[1] == names[2] and len(names[0]) > 0
    assert not any("dora" in n for n in names[0])
    for other in res[1:]:
        assert res[0][0] == other[0]
        for k in res[0][1]:
            assert torch.equal(res[0][1][k], other[1][k]), k
    model = build_dora_model(cfg, params, R_TINY)
    model.train()
    timer = ops.LaunchTimer()
    ops.set_launch_timer(timer)
    try:
        _step(model, d)
    finally:
        ops.set_launch_timer(None)
    got = [rec[0] for rec in timer.records]
    # per block: four folds (once per weight version), four magnitude reductions, four dB row scales
    assert sum(n.startswith("ltx::dora_fold_kernel") for n in got) == 2 * 4
    assert sum(n == "ltx::dora_mag_grad_kernel" for n in got) == 2 * 4
    assert sum(n == "ltx::dora_rowscale_add_kernel" for n in got) == 2 * 4
