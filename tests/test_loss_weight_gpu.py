"""The loss weights on the MI355X: ltx_loss_token_weights against its float64 statement,
ltx_wmse_fwd_bwd against the shipped ltx_mse_fwd_bwd (bitwise where the arithmetic is the same) and
against float64, and the weighted train step of one LTX-2B-width block against the pinned oracle run
live with the same weighted loss.

Tolerances. Token weights, relative 1e-5 per element: about 10 f32 roundings per element plus a
summation chain of at most ceil(N / 256) + 16 additions, each 2^-24, is under 3e-6 for N <= 7488.
stats[0], relative 1e-5: the same chain over per-thread sums of at most ceil(n / 65536) products.
dout against float64, relative 1e-2 per element, the bound the feature request set from four bf16
roundings at 2^-9 each, (1 + 2^-9)^4 - 1 = 7.84e-3, plus f32 slop. 2^-9 is a rounding's error at the top
of a binade; at the bottom it is 2^-8, and of the four roundings the multiply by grad_scale = 1/16 is
exact, so the worst case of the other three is (1 + 2^-8)^3 - 1 = 1.18e-2. Measured on these seeded
inputs: 7.40e-3 at (2, 64, 128) and 9.66e-3 at (3, 1001, 7), inside the bound as set. The step:
model_utils.noise_crit / loss_crit at their defaults, relative to the oracle's own bf16 noise on the same
weighted loss."""
import pytest
import torch

import ltx_oracle as O
from loss_weight_utils import (STEP_KEYS, StepCapture, closed_form_factor, config, oracle_weighted_step, step_boxes,
                               weight_inputs, within_relative)
from model_utils import build_model, is_lora_trainable, loss_crit, noise_crit, synth_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEW_KERNELS = ("ltx::loss_token_weights_kernel", "ltx::wmse_kernel<true>")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from ltx_amd import _lib as L
    L.ensure_device()
    return L


def g(*shape, dtype=torch.bfloat16, scale=1.0, seed=0):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale).to(dtype).to(DEV)


# ---------------------------------------------------------------------------------------------
# ltx_loss_token_weights
# ---------------------------------------------------------------------------------------------
# (2,3,4,5): odd sizes, N = 60 below one pass of the 256 threads; (1,1,1,1): a single token;
# (3,2,16,16): N = 512, two strided passes, a NaN box and an empty one; (2,7,16,16): the flagship's token
# grid per frame with an odd frame count, N = 1792
WEIGHT_SHAPES = [(2, 3, 4, 5), (1, 1, 1, 1), (3, 2, 16, 16), (2, 7, 16, 16)]
NULLABLE = ("bbox", "frame_w", "sample_w", "user_w")


@pytest.mark.parametrize("shape", WEIGHT_SHAPES)
def test_token_weights_against_the_f64_statement(shape):
    """Every subset of the four nullable inputs: wt and raw_sum within relative 1e-5 of the float64
    statement on the same f32 inputs, exact zeros where it has them, and a second call bitwise the same."""
    from ltx_amd import ops
    from ltx_amd.training import token_loss_weights_ref
    B, F, H, W = shape
    inp = weight_inputs(B, F, H, W, seed=sum(shape), device=DEV)
    for mask in range(1 << len(NULLABLE)):
        kw = {k: (inp[k] if (mask >> i) & 1 else None) for i, k in enumerate(NULLABLE)}
        wt, raw_sum = ops.loss_token_weights(B, F, H, W, DEV, face_weight=4.0, face_pad=0.1, **kw)
        ref_wt, ref_sum = token_loss_weights_ref(B, F, H, W, face_weight=4.0, face_pad=0.1, **kw)
        assert wt.shape == (B, F * H * W) and wt.dtype == torch.float32 and raw_sum.shape == (B,)
        ok_w, worst_w = within_relative(wt, ref_wt, 1e-5)
        ok_s, worst_s = within_relative(raw_sum, ref_sum, 1e-5)
        given = [k for k in NULLABLE if kw[k] is not None]
        print(f"{shape} {given}: worst relative error wt {worst_w:.3e}, raw_sum {worst_s:.3e}")
        assert ok_w and ok_s, (shape, given, worst_w, worst_s)
        again, sum_again = ops.loss_token_weights(B, F, H, W, DEV, face_weight=4.0, face_pad=0.1, **kw)
        assert torch.equal(wt, again) and torch.equal(raw_sum, sum_again), (shape, given)
        # each sample's weights average to its factor
        want_mean = inp["sample_w"].double() if kw["sample_w"] is not None else torch.ones(B, dtype=torch.float64,
                                                                                            device=DEV)
        assert torch.allclose(wt.double().mean(dim=1), want_mean, rtol=1e-5, atol=0), (shape, given)


@pytest.mark.parametrize("shape", WEIGHT_SHAPES)
def test_token_weights_of_ones_are_exactly_one(shape):
    from ltx_amd import ops
    B, F, H, W = shape
    N = F * H * W
    wt, raw_sum = ops.loss_token_weights(B, F, H, W, DEV)
    assert bool((wt == 1.0).all()) and bool((raw_sum == float(N)).all())
    # the same with every input given and equal to one: a real box under face_weight 1 changes nothing
    inp = weight_inputs(B, F, H, W, seed=1, device=DEV)
    ones = dict(frame_w=torch.ones(F, device=DEV), sample_w=torch.ones(B, device=DEV),
                user_w=torch.ones(B, N, device=DEV))
    wt, raw_sum = ops.loss_token_weights(B, F, H, W, DEV, bbox=inp["bbox"], face_weight=1.0, face_pad=0.1, **ones)
    assert bool((wt == 1.0).all()) and bool((raw_sum == float(N)).all())


def test_token_weights_refuse_bad_arguments():
    from ltx_amd import _lib, ops
    with pytest.raises(_lib.LtxHipError):
        ops.loss_token_weights(2, 1, 4, 4, DEV, face_weight=0.0)
    with pytest.raises(_lib.LtxHipError):
        ops.loss_token_weights(2, 1, 4, 4, DEV, face_pad=-0.5)
    with pytest.raises(ValueError):
        ops.loss_token_weights(2, 1, 4, 4, DEV, bbox=torch.zeros(2, 3, device=DEV))
    with pytest.raises(_lib.LtxHipError):
        ops.loss_token_weights(2, 1, 4, 4, DEV, frame_w=torch.ones(1))  # a CPU tensor


# ---------------------------------------------------------------------------------------------
# ltx_wmse_fwd_bwd
# ---------------------------------------------------------------------------------------------
# the shapes of test_kernels_gpu.test_mse_and_adamw: (2, 64, 128) takes the one-weight-per-vector path
# (C % 8 == 0), (3, 1001, 7) the per-element one, with vectors that straddle tokens and a scalar tail
WMSE_SHAPES = [(2, 64, 128), (3, 1001, 7)]
GS = 1 / 16


def _operands(shape):
    return g(*shape, seed=1), g(*shape, seed=2)


@pytest.mark.parametrize("shape", WMSE_SHAPES)
def test_wmse_with_ones_is_the_shipped_loss(shape):
    from ltx_amd import ops
    o, v = _operands(shape)
    rows = o.numel() // shape[-1]
    s0, d0 = ops.mse_fwd_bwd(o, v, grad_scale=GS)
    s1, d1 = ops.wmse_fwd_bwd(o, v, torch.ones(rows, device=DEV), GS, True)
    assert torch.equal(s1[:3], s0[:3]) and torch.equal(s1[3], s0[0])
    assert torch.equal(d1, d0)
    # the weights may come shaped like the tokens
    s2, d2 = ops.wmse_fwd_bwd(o, v, torch.ones(shape[:-1], device=DEV), GS, True)
    assert torch.equal(s2, s1) and torch.equal(d2, d1)


@pytest.mark.parametrize("shape", WMSE_SHAPES)
def test_wmse_with_arbitrary_weights(shape):
    from ltx_amd import ops
    o, v = _operands(shape)
    C = shape[-1]
    n = o.numel()
    rows = n // C
    gen = torch.Generator(device="cpu").manual_seed(3)
    wt = torch.rand(rows, generator=gen) * 2.0 + 0.01
    wt[torch.rand(rows, generator=gen) < 0.2] = 0.0
    wt = wt.to(DEV)
    assert 0 < int((wt == 0).sum()) < rows
    s0, d0 = ops.mse_fwd_bwd(o, v, grad_scale=GS)
    s1, d1 = ops.wmse_fwd_bwd(o, v, wt, GS, True)
    # the unweighted sums are the shipped kernel's, bit for bit
    assert torch.equal(s1[3], s0[0]) and torch.equal(s1[1], s0[1]) and torch.equal(s1[2], s0[2])
    # the seed is the shipped seed times the weight, one multiply and one rounding, done here in torch
    want = (d0.float().reshape(rows, C) * wt[:, None]).bfloat16().reshape(d0.shape)
    assert torch.equal(d1, want)
    # the weighted sum against float64 over the bf16-rounded squares
    diff = o - v
    q = diff * diff
    assert q.dtype == torch.bfloat16
    ref0 = float((wt.double()[:, None] * q.double().reshape(rows, C)).sum())
    err0 = abs(float(s1[0]) - ref0) / ref0
    print(f"{shape}: stats[0] relative error {err0:.3e}")
    assert err0 <= 1e-5
    # every element of the seed against float64
    ref_d = 2.0 * wt.double()[:, None] * (o.double() - v.double()).reshape(rows, C) * GS / n
    ok, worst = within_relative(d1.reshape(rows, C), ref_d, 1e-2)
    print(f"{shape}: dout worst relative error {worst:.3e}")
    assert ok, worst
    # deterministic, and forward-only gives the same sums and no seed
    s2, d2 = ops.wmse_fwd_bwd(o, v, wt, GS, True)
    assert torch.equal(s2, s1) and torch.equal(d2, d1)
    s3, d3 = ops.wmse_fwd_bwd(o, v, wt, GS, False)
    assert d3 is None and torch.equal(s3, s1)


def test_wmse_refuses_mismatched_weights():
    from ltx_amd import _lib, ops
    o, v = _operands((2, 64, 128))
    with pytest.raises(ValueError):
        ops.wmse_fwd_bwd(o, v, torch.ones(127, device=DEV), 1.0, True)
    with pytest.raises(_lib.LtxHipError):
        ops.wmse_fwd_bwd(o, v, torch.ones(128), 1.0, True)  # a CPU tensor


# ---------------------------------------------------------------------------------------------
# the step: one LTX-2B-width block, B = 8 samples of 2 x 16 x 16 tokens (tests/test_lora_ranks_gpu.py's)
# ---------------------------------------------------------------------------------------------
RANK = 32
SHAPE = (8, 2, 16, 16)
_CASE = {}


def _case():
    """The model, its inputs and the unconfigured step, built once and left unchanged."""
    if not _CASE:
        from ltx_amd.transformer3d import OURS_TRANSFORMER_CONFIG
        cfg = dict(OURS_TRANSFORMER_CONFIG, num_layers=1)
        params = O.make_params(cfg, 100 + RANK, lora_rank=RANK, requires_grad=False)
        B, F, H, W = SHAPE
        d = synth_inputs(B, F, H, W, 256, 16, seed=7 + RANK, device=DEV)
        model = build_model(cfg, params, RANK, device=DEV)
        _CASE.update(cfg=cfg, params=params, d=d, model=model, boxes=step_boxes(B, DEV),
                     plain=StepCapture(model, d, config()))
    return _CASE


def _same_step(got, plain):
    assert torch.equal(got.loss, plain.loss) and torch.equal(got.rel_mse, plain.rel_mse)
    assert torch.equal(got.nrmse, plain.nrmse)
    assert torch.equal(got.sample, plain.sample)
    assert set(got.grads) == set(plain.grads) and len(got.grads) > 0
    for k, v in plain.grads.items():
        assert v is not None and float(v.abs().max()) > 0, k
        assert torch.equal(got.grads[k], v), k


def test_weighted_step_matches_the_oracle_with_the_weighted_loss():
    from ltx_amd.training import token_loss_weights_ref
    c = _case()
    B, F, H, W = SHAPE
    d, model, plain = c["d"], c["model"], c["plain"]
    # the oracle's weights: the float64 statement, the timestep factor from its closed form
    frame_w = torch.tensor([STEP_KEYS["loss_frame0_weight"]] + [1.0] * (F - 1), device=DEV)
    wt_ref, _ = token_loss_weights_ref(B, F, H, W, bbox=c["boxes"], frame_w=frame_w,
                                       sample_w=closed_form_factor(d["out.t"], STEP_KEYS["loss_timestep_weighting"]),
                                       face_weight=STEP_KEYS["loss_face_weight"])
    assert float(wt_ref.max() / wt_ref[wt_ref > 0].min()) > 8  # the weighting is not a formality
    refs = {dt: oracle_weighted_step(c["params"], c["cfg"], d, dt, is_lora_trainable, wt_ref, device=DEV)
            for dt in (torch.float32, torch.bfloat16)}
    got = StepCapture(model, d, config(**STEP_KEYS), {"face_bbox": c["boxes"]})
    (s32, g32, l32), (s16, g16, l16) = refs[torch.float32], refs[torch.bfloat16]
    e_b, e_r = loss_crit("weighted loss", got.ld["_wmse_f32"], l16, l32)
    print(f"_wmse_f32 {float(got.ld['_wmse_f32']):.6f} vs fp32 oracle {l32:.6f} (bf16 oracle {l16:.6f}): "
          f"{e_b:.3e} vs {e_r:.3e}")
    assert len(g32) > 0 and set(g32) == set(got.grads)
    for k in g32:
        assert got.grads[k] is not None and float(got.grads[k].abs().max()) > 0, k
        e_b, e_r = noise_crit(k, got.grads[k], g16[k], g32[k])
        print(f"{k}: build {e_b:.3e} vs reference bf16 noise {e_r:.3e}")
    # the weighting changes the backward seed and nothing in front of it
    assert torch.equal(got.sample, plain.sample)
    assert set(got.ld) == {"transformer_mse", "_mse_f32", "transformer_wmse", "_wmse_f32"}
    assert torch.equal(got.ld["_mse_f32"], plain.ld["_mse_f32"])
    assert torch.equal(got.ld["transformer_mse"], plain.ld["transformer_mse"])
    assert torch.equal(got.ld["transformer_wmse"], got.ld["_wmse_f32"].bfloat16())
    assert torch.equal(got.loss, 1.0 * got.ld["transformer_wmse"])
    assert not torch.equal(got.ld["_wmse_f32"], got.ld["_mse_f32"])
    assert any(not torch.equal(got.grads[k], plain.grads[k]) for k in g32)
    # two launches more than the unconfigured step, the rest the same kernels in the same order
    assert [n for n in got.launches if n not in NEW_KERNELS] == plain.launches
    assert [got.launches.count(n) for n in NEW_KERNELS] == [1, 1]


def test_keys_at_their_defaults_are_the_unconfigured_step():
    c = _case()
    plain = c["plain"]
    tc = config(loss_face_weight=1.0, loss_face_pad=0.0, loss_frame0_weight=1.0, loss_timestep_weighting="none")
    got = StepCapture(c["model"], c["d"], tc, {"face_bbox": c["boxes"]})
    assert got.launches == plain.launches and len(plain.launches) > 0
    assert not any(n in NEW_KERNELS or "wmse" in n or "loss_token" in n for n in got.launches)
    assert set(got.ld) == set(plain.ld) == {"transformer_mse", "_mse_f32"}
    assert torch.equal(got.ld["_mse_f32"], plain.ld["_mse_f32"])
    _same_step(got, plain)


def test_weights_of_one_through_the_weighted_path():
    c = _case()
    plain = c["plain"]
    B, F, H, W = SHAPE
    got = StepCapture(c["model"], c["d"], config(), {"loss_weights": torch.ones(B, F, H, W, device=DEV)})
    assert [got.launches.count(n) for n in NEW_KERNELS] == [1, 1]  # the weighted path did run
    _same_step(got, plain)
    assert torch.equal(got.ld["_wmse_f32"], plain.ld["_mse_f32"])
    assert torch.equal(got.ld["_mse_f32"], plain.ld["_mse_f32"])
    # [B, N] weights, forward only: the same loss and no gradient
    fwd = StepCapture(c["model"], c["d"], config(), {"loss_weights": torch.ones(B, F * H * W, device=DEV)},
                      backward=False)
    assert torch.equal(fwd.loss, plain.loss) and all(v is None for v in fwd.grads.values())


def test_validate_epoch_keeps_its_value_under_a_weighted_config():
    from ltx_amd.scheduler import RectifiedFlowScheduler
    from ltx_amd.validation import validate_epoch
    c = _case()
    d, model = c["d"], c["model"]
    batch = {"latents": d["in.latents"], "ref_image_latents": d["in.ref_image_latents"],
             "pose_latents": d["in.pose_latents"], "face_bbox": c["boxes"]}
    vals = []
    try:
        for tc in (config(), config(loss_face_pad=0.1, **STEP_KEYS)):
            torch.manual_seed(11)
            vals.append(validate_epoch(model, [batch, batch], RectifiedFlowScheduler(), model.patchifier, tc,
                                       d["in.prompt_embeds"], d["in.prompt_attention_mask"], DEV))
    finally:
        model.train()
    assert isinstance(vals[0], float) and vals[0] > 0 and vals[0] == vals[1]
