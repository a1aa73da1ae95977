"""Shared by tests/test_robust_loss_cpu.py and tests/test_robust_loss_gpu.py: the threshold schedules'
closed forms written out independently of training.huber_threshold, seeded kernel inputs with residuals on
both sides of the threshold, and the pinned oracle's train step with its loss replaced by the robust one."""
import torch

KINDS = {"huber": 1, "smooth_l1": 2}


def closed_form_threshold(t, schedule, huber_c):
    """The threshold per sample in float64, in the forms of kohya's schedules at timestep / T = t and the
    rectified flow's sigma = t / (1 - t)."""
    t = t.detach().double()
    if schedule == "constant":
        return torch.full_like(t, huber_c)
    if schedule == "exponential":
        alpha = -torch.log(torch.tensor(huber_c, dtype=torch.float64))  # exp(-alpha * timestep / T)
        return torch.exp(-alpha * t)
    assert schedule == "snr"
    # (1 - c) / (1 + sigma)^2 + c with 1 / (1 + sigma) = 1 - t, which also holds at t = 1 (sigma = inf)
    return (1.0 - huber_c) * (1.0 - t) ** 2 + huber_c


def robust_inputs(shape, seed, weights, device="cpu"):
    """Seeded operands of ltx_robust_loss_fwd_bwd at (B, rows, C): bf16 out and v whose residuals are
    ~N(0, 1) (bf16-rounded), about 1 % of the positions with out == v, thresholds drawn per sample from
    {0.05, 0.3, 1.0} (with three samples or more each value occurs), and with `weights` positive f32 token
    weights with exact zeros -- all of the last sample's when there is more than one sample."""
    B, rows, C = shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    v = torch.randn(B, rows, C, generator=g).bfloat16()
    out = (v.float() + torch.randn(B, rows, C, generator=g)).bfloat16()
    same = torch.rand(B, rows, C, generator=g) < 0.01
    if out.numel() >= 100:
        same.view(-1)[7] = True
    out = torch.where(same, v, out)
    levels = torch.tensor([0.05, 0.3, 1.0])
    c = levels[(torch.arange(B) + int(torch.randint(0, 3, (1,), generator=g))) % 3].float().contiguous()
    wt = None
    if weights:
        wt = torch.rand(B, rows, generator=g) * 2.0 + 0.01
        wt[torch.rand(B, rows, generator=g) < 0.2] = 0.0
        if B > 1:
            wt[-1] = 0.0
        if B * rows == 1:
            wt[:] = 0.75  # a single token with weight 0 would check nothing
        wt = wt.float().contiguous().to(device)
    return out.to(device), v.to(device), c.to(device), wt


def oracle_robust_step(params, cfg, d, dtype, trainable, c, kind, wt=None, device="cuda"):
    """model_utils.oracle_step with the loss replaced by the robust one: the pinned oracle's train step on
    the device in `dtype` (adapters f32), then on its own sample and v_target, in torch f32,
      e = sample - v_target, r = sqrt(e^2 + c_b^2), l = k_b e^2 / (r + c_b), k_b = 2 c_b (kind 1) | 2 (kind 2),
      loss = (wt[..., None] * l).mean() (wt None: ones), c [B], wt [B, N].
    Returns (sample, {name: grad}, that loss as a float)."""
    import ltx_oracle as O
    q = {k: v.detach().to(device).to(torch.float32 if ("lora_" in k or dtype == torch.float32) else dtype)
         .requires_grad_(trainable(k)) for k, v in params.items()}
    r = O.train_step(q, cfg, d["in.latents"], d["in.ref_image_latents"], d["in.pose_latents"],
                     d["in.prompt_embeds"], d["in.prompt_attention_mask"], t=d["out.t"],
                     noise=d["out.noise"].to(dtype))
    cb = c.to(device).float().reshape(-1, 1, 1)
    e = r["sample"].float() - r["v_target"].float()
    k = 2.0 * cb if kind == 1 else torch.full_like(cb, 2.0)
    l = k * (e * e) / (torch.sqrt(e * e + cb * cb) + cb)
    if wt is not None:
        l = wt.to(device).float()[..., None] * l
    loss = l.mean()
    loss.backward()
    return r["sample"].detach(), {k: v.grad for k, v in q.items() if v.requires_grad}, float(loss.detach())
