"""Shared by tests/test_loss_weight_cpu.py and tests/test_loss_weight_gpu.py: hand-computable weight
cases, seeded kernel inputs, and the weighted train step of the build and of the pinned oracle."""
import math
import types

import torch

# settings of the step-level parity test: a face weight, a first-frame weight and a timestep weighting
# at once, with boxes that cut token cells (16 x 16 cells: no coordinate below is a multiple of 1/16)
STEP_KEYS = dict(loss_face_weight=4.0, loss_frame0_weight=0.25, loss_timestep_weighting="cosmap")


def config(**extra):
    """A TrainConfig with the optional keys set the way the YAML loader sets them (setattr)."""
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="-")
    for k, v in extra.items():
        setattr(tc, k, v)
    return tc


def step_boxes(B, device="cpu"):
    """[B, 4] f32 face boxes that cut cells of a 16 x 16 grid, one per sample, all different."""
    i = torch.arange(B, dtype=torch.float32)
    x0, y0 = 0.21 + 0.03 * i, 0.13 + 0.02 * i
    return torch.stack([x0, y0, x0 + 0.37, y0 + 0.45], dim=1).to(device)


def closed_form_factor(t, scheme):
    """The timestep factor in float64, written out independently of training.timestep_loss_weight."""
    t = t.detach().double()
    if scheme == "sigma_sqrt":
        return t ** -2
    assert scheme == "cosmap"
    return 2.0 / (math.pi * (1.0 - 2.0 * t + 2.0 * t ** 2))


def weight_inputs(B, F, H, W, seed, device):
    """Seeded inputs of ltx_loss_token_weights: boxes that cut cells (with B > 2 one box with a NaN and one
    that is empty, x_max < x_min), frame weights with a small first frame, positive sample factors, caller
    weights with exact zeros."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    lo = torch.rand(B, 2, generator=g) * 0.5
    size = 0.15 + torch.rand(B, 2, generator=g) * 0.4
    bbox = torch.cat([lo, lo + size], dim=1)
    if B > 2:
        bbox[1, 2] = float("nan")
        bbox[2] = torch.tensor([0.6, 0.2, 0.4, 0.5])
    frame_w = 0.5 + torch.rand(F, generator=g)
    frame_w[0] = 0.25
    sample_w = 0.3 + 2.0 * torch.rand(B, generator=g)
    user_w = torch.rand(B, F * H * W, generator=g) * 2.0
    user_w[torch.rand(B, F * H * W, generator=g) < 0.2] = 0.0
    if F * H * W == 1:
        user_w[:] = 0.75  # a single token with weight 0 would make the whole sample 0
    return {k: v.float().contiguous().to(device) for k, v in
            dict(bbox=bbox, frame_w=frame_w, sample_w=sample_w, user_w=user_w).items()}


def within_relative(got, ref, tol):
    """max over elements of |got - ref| / |ref| (0 / 0 counts as 0, x / 0 as inf) <= tol, with the figure."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs()
    relerr = torch.where(ref != 0, err / ref.abs().clamp(min=1e-300), torch.where(err == 0, err, err / 0.0))
    worst = float(relerr.max()) if relerr.numel() else 0.0
    return worst <= tol, worst


class StepCapture:
    """One train_step of the build on the inputs of model_utils.synth_inputs, with what the tests compare:
    the returned scalars, the loss dict, the model's output (caught on its way out of _forward_tokens),
    every trainable gradient by canonical name, and the LaunchTimer kernel names in launch order."""

    def __init__(self, model, d, tc, batch_extra=None, backward=True):
        from ltx_amd import ops
        from ltx_amd.scheduler import RectifiedFlowScheduler
        from ltx_amd.training import train_step
        from model_utils import grads_by_canonical
        for p in model.parameters():
            p.grad = None
        batch = {"latents": d["in.latents"], "ref_image_latents": d["in.ref_image_latents"],
                 "pose_latents": d["in.pose_latents"]}
        batch.update(batch_extra or {})
        caught = {}
        inner = model._forward_tokens

        def forward_tokens(*a, **k):
            caught["sample"] = inner(*a, **k)
            return caught["sample"]
        timer = ops.LaunchTimer()
        model._forward_tokens = forward_tokens
        ops.set_launch_timer(timer)
        try:
            self.loss, self.rel_mse, self.nrmse, self.ld = train_step(
                model, batch, RectifiedFlowScheduler(), model.patchifier, tc, d["in.prompt_embeds"],
                d["in.prompt_attention_mask"], t=d["out.t"], noise=d["out.noise"], backward=backward)
        finally:
            ops.set_launch_timer(None)
            del model._forward_tokens  # the instance attribute: the class's method is back
        self.sample = caught["sample"].detach()
        self.launches = [rec[0] for rec in timer.records]
        self.grads = {k: (None if v is None else v.clone()) for k, v in grads_by_canonical(model).items()}


def oracle_weighted_step(params, cfg, d, dtype, trainable, wt, device="cuda"):
    """model_utils.oracle_step with the loss replaced by the weighted one: the pinned oracle's train step on
    the device in `dtype` (adapters f32), its loss (wt[..., None] * (sample - v_target)^2).mean() in f32:
    (sample, {name: grad}, that loss as a float)."""
    import ltx_oracle as O
    q = {k: v.detach().to(device).to(torch.float32 if ("lora_" in k or dtype == torch.float32) else dtype)
         .requires_grad_(trainable(k)) for k, v in params.items()}
    r = O.train_step(q, cfg, d["in.latents"], d["in.ref_image_latents"], d["in.pose_latents"],
                     d["in.prompt_embeds"], d["in.prompt_attention_mask"], t=d["out.t"],
                     noise=d["out.noise"].to(dtype))
    loss = (wt.to(device).float()[..., None] * (r["sample"].float() - r["v_target"].float()) ** 2).mean()
    loss.backward()
    return r["sample"].detach(), {k: v.grad for k, v in q.items() if v.requires_grad}, float(loss)


def namespace(**kw):
    return types.SimpleNamespace(**kw)
