"""Training step, fused AdamW and data-parallel gradient averaging.

train_step keeps the reference signature and semantics (ltx_video/training.py:94-166):
LogNormal(mu, sigma) timesteps -> r/(1+r) -> batch-quantile clamp, optional resolution shift,
noise ~ randn_like(tokens), x_t = (1-t)x0 + t*eps, v = eps - x0, model forward, MSE loss.
Differences that are deliberate and documented:
  * the train-step prologue (patchify + add_noise + velocity + conditioning lerp) is one kernel;
  * the backward is seeded directly with d(loss)/d(out) from the fused MSE kernel
    (grad scale = transformer_loss_weight / gradient_accumulation_steps, the reference's
    `loss / accum` then `.backward()`), so no host sync happens inside the step;
  * t is sampled on `device` exactly as the reference (training.py:124-132: LogNormal on the
    device RNG, then randn_like for the noise, so a seeded run draws the same t and noise); the
    quantile clamp takes the bounds as 0-dim device tensors instead of `float(t_low)`, which gives
    the same f32 result without the device->host round trip in every micro-step.
"""
import collections
import contextlib
import ctypes
import functools
import math

import torch
import torch.distributed as dist

from . import ops
from .patchifier import SymmetricPatchifier


_LOGN_PARAMS = {}  # (mu, sigma, device) -> the LogNormal's 0-dim device loc / scale
_QUANTILES = {}  # (q_min, q_max, device, dtype) -> the two quantile levels as one device tensor


def sample_timesteps(batch, config, device):
    """training.py:124-132: LogNormal(mu, sigma).sample((B,)) -> r/(1+r) -> batch-quantile clamp.

    The draw is the distribution's own arithmetic written out, without its three host syncs per
    micro-step (each drains the device queue, so the step prologue then ran host-bound with the
    GPU idle): torch.tensor(x, device=cuda) is a blocking H2D copy, the distribution validates
    its arguments by reading a device bool back, and torch.normal(mean, std) checks
    std.min() >= 0 with .item(). torch.normal(mean, std) is normal_(0, 1) on its output, then
    output.mul_(std).add_(mean) (ATen normal_out_impl), and LogNormal.sample exponentiates it:
    the same generator draw and the same f32 roundings here."""
    mu = config.rf_log_normal_mu if config.rf_log_normal_mu is not None else 0.0
    sigma = config.rf_log_normal_sigma if config.rf_log_normal_sigma is not None else 1.0
    key = (float(mu), float(sigma), str(torch.device(device)))
    params = _LOGN_PARAMS.get(key)
    if params is None:
        params = (torch.tensor(mu, device=device), torch.tensor(sigma, device=device))
        _LOGN_PARAMS[key] = params
    loc, scale = params
    z = torch.empty(batch, dtype=loc.dtype, device=device).normal_(0.0, 1.0)
    raw = z.mul_(scale).add_(loc).exp_()
    t_raw = raw / (1 + raw)
    # both bounds from one sort: quantile with a q tensor runs the scalar form's arithmetic per q
    # (q as an f32 tensor, rank q (n - 1), the same lerp), so the values are those of two calls
    qkey = (float(config.rf_quantile_min), float(config.rf_quantile_max), str(torch.device(device)), t_raw.dtype)
    qs = _QUANTILES.get(qkey)
    if qs is None:
        qs = torch.tensor([qkey[0], qkey[1]], dtype=t_raw.dtype, device=device)
        _QUANTILES[qkey] = qs
    t_low, t_high = torch.quantile(t_raw, qs).unbind(0)
    # clamp against the 0-dim f32 bounds: the reference's float(t_low) is the same f32 value
    # (exact in double, cast back to f32 by clamp), so only the host sync differs
    return t_raw.clamp(min=t_low, max=t_high)


def train_step(model, batch, scheduler, patchifier, config, prompt_embeds, prompt_attention_mask,
               device=None, t=None, noise=None, backward=True):
    """Returns (loss, rel_mse, nrmse, loss_dict) like the reference; runs the backward too when
    `backward` (the reference calls loss.backward() in train_one_epoch, training.py:203).

    With a loss key of loss_weights_from_config off its default, or batch["loss_weights"] (f32 [B, N] or
    [B, F, H, W], >= 0), the loss is the weighted mean(wt (out - v)^2): the token weights come from
    ltx_loss_token_weights (batch["face_bbox"], f32 [B, 4], when it is there) and ltx_wmse_fwd_bwd takes
    ltx_mse_fwd_bwd's place. loss, rel_mse and nrmse are then the weighted loss's, loss_dict gains
    "transformer_wmse" / "_wmse_f32", and "transformer_mse" / "_mse_f32" stay the unweighted mean.

    With `loss_type` huber or smooth_l1 (robust_loss_from_config) ltx_robust_loss_fwd_bwd takes the place of
    either: the loss is mean(wt l), l the pseudo-Huber term against the sample's threshold
    (huber_threshold on the step's shifted t; wt as above, or ones). loss, rel_mse and nrmse are that
    loss's, loss_dict gains "transformer_robust" / "_robust_f32" (and no "transformer_wmse": the weighted
    squared error would be a sum the kernel does not otherwise need), and "transformer_mse" / "_mse_f32"
    stay the unweighted squared error, bitwise the plain step's."""
    dt = torch.bfloat16
    device = device or model.device
    latents = batch["latents"].to(device=device, dtype=dt)
    ref = batch["ref_image_latents"].to(device=device, dtype=dt)
    pose = batch["pose_latents"].to(device=device, dtype=dt)
    B, C, F, H, W = latents.shape
    N = F * H * W
    # the loss weights (loss_weights_from_config; None and no batch["loss_weights"]: the reference's plain
    # mse, today's launches). The refusals come before anything is launched.
    lw = loss_weights_from_config(config)
    robust = robust_loss_from_config(config)
    user_w = batch.get("loss_weights")
    weighted = lw is not None or user_w is not None
    if weighted:
        lw = lw or LossWeights()
        if lw.frame0_weight == 0.0 and F == 1:
            raise ValueError("loss_frame0_weight = 0 with a single latent frame: every token's weight would be 0")
        if user_w is not None:
            if tuple(user_w.shape) not in ((B, N), (B, F, H, W)):
                raise ValueError(f"batch['loss_weights']: expected shape {(B, N)} or {(B, F, H, W)}, got "
                                 f"{tuple(user_w.shape)}")
            user_w = user_w.to(device=device, dtype=torch.float32).reshape(B, N).contiguous()
    # convert first, then expand: the batch stays a stride-0 view, which the model recognises as
    # one prompt shared by the batch (caption projection and text K/V computed once)
    enc = prompt_embeds.to(device=device, dtype=dt).expand(B, -1, -1)
    enc_mask = prompt_attention_mask.to(device).expand(B, -1)
    # one coordinate set broadcast over the batch (identical per sample): one shared RoPE table
    coords = patchifier.get_latent_coords(F, H, W, 1, device).expand(B, -1, -1)
    if t is None:
        t = sample_timesteps(B, config, device)
        t = scheduler.shift_timesteps(torch.Size([B, N, C]), t)
    t = t.to(device=device, dtype=torch.float32)
    if noise is None:
        noise = torch.randn((B, N, C), device=device, dtype=dt)
    _, model_in, v_target = ops.rf_prepare_tokens(latents, ref, pose, noise, t)
    # the conditioning lerp is already applied: hand the model lerp-neutral conditioning views
    out = model._forward_tokens(model_in, coords, enc, t, enc_mask)
    w = float(getattr(config, "transformer_loss_weight", 1.0))
    accum = max(1, int(getattr(config, "gradient_accumulation_steps", 1)))
    n = out.numel()
    wt = None
    if weighted:
        # built on the device and consumed inside the loss kernel: no host read, no torch pass over the
        # tokens
        bbox = batch.get("face_bbox") if lw.face_weight != 1.0 else None  # a missing box: uniform weights
        if bbox is not None:
            bbox = bbox.to(device=device, dtype=torch.float32).reshape(B, 4).contiguous()
        wt, _ = ops.loss_token_weights(B, F, H, W, device, bbox=bbox,
                                       frame_w=_frame_weights(F, lw.frame0_weight, device),
                                       sample_w=timestep_loss_weight(t, lw.timestep_weighting), user_w=user_w,
                                       face_weight=lw.face_weight, face_pad=lw.face_pad)
    if robust is not None:
        # the thresholds from the t the model saw, a few torch ops on [B]; stats[0] is the (weighted) robust
        # sum, stats[1..3] mse_fwd_bwd's sum v, sum v^2 and squared-error sum, bit for bit
        c = huber_threshold(t, robust.schedule, robust.huber_c)
        stats, dout = ops.robust_loss_fwd_bwd(out, v_target, c, ops.ROBUST_KINDS[robust.loss_type], wt=wt,
                                              grad_scale=w / accum, want_grad=backward)
        robust_f32, mse_f32 = stats[0] / n, stats[3] / n
        rob = robust_f32.to(dt)
        loss = w * rob
        loss_dict = {"transformer_mse": mse_f32.to(dt), "_mse_f32": mse_f32, "transformer_robust": rob,
                     "_robust_f32": robust_f32}
    elif weighted:
        # stats[0] is the weighted sum, stats[3] the unweighted one (bitwise mse_fwd_bwd's)
        stats, dout = ops.wmse_fwd_bwd(out, v_target, wt, grad_scale=w / accum, want_grad=backward)
        wmse_f32, mse_f32 = stats[0] / n, stats[3] / n
        wmse, mse = wmse_f32.to(dt), mse_f32.to(dt)
        loss = w * wmse
        loss_dict = {"transformer_mse": mse, "_mse_f32": mse_f32, "transformer_wmse": wmse, "_wmse_f32": wmse_f32}
    else:
        stats, dout = ops.mse_fwd_bwd(out, v_target, grad_scale=w / accum, want_grad=backward)
        mse = (stats[0] / n).to(dt)
        loss = w * mse
        # "_mse_f32": the unrounded f32 mean (parity tests compare losses at 1e-3, below the bf16
        # rounding of the reference's loss scalar); underscore keys are not logged
        loss_dict = {"transformer_mse": mse, "_mse_f32": stats[0] / n}
    std = torch.sqrt(torch.clamp((stats[2] - stats[1] * stats[1] / n) / (n - 1), min=0)).to(dt)
    rel_mse = loss / (std ** 2 + 1e-12)
    nrmse = torch.sqrt(loss) / (std + 1e-12)
    if backward:
        out.backward(dout)
    return loss, rel_mse, nrmse, loss_dict


TIMESTEP_WEIGHTINGS = ("none", "sigma_sqrt", "cosmap")

# What loss_weights_from_config decided; the defaults are the reference's unweighted loss
LossWeights = collections.namedtuple("LossWeights", "face_weight face_pad frame0_weight timestep_weighting",
                                     defaults=(1.0, 0.0, 1.0, "none"))


def loss_weights_from_config(config):
    """LossWeights or None from the optional config keys (setattr, or train.<key> in the YAML; not
    TrainConfig fields). None -- every key absent or at its default -- is the reference's plain
    F.mse_loss, launch for launch:
      `loss_face_weight` (a float > 0, absent = 1): the weight of a token wholly inside the sample's face
          box (batch["face_bbox"]) relative to one outside; a token the box cuts gets the share it covers;
      `loss_face_pad` (a float >= 0, absent = 0): the box grows by this fraction of its width and height
          on each side before it is clipped to the frame -- the allowance for head motion, since the box
          comes from the reference frame and is applied to every latent frame;
      `loss_frame0_weight` (a float >= 0, absent = 1): the weight of the first latent frame's tokens,
          which the model is fed as lerp(x_t, ref, 0.85); train_step refuses 0 when there is one frame;
      `loss_timestep_weighting` ("none", the same as absent, "sigma_sqrt": t^-2, or "cosmap":
          2 / (pi (1 - 2 t + 2 t^2)), SD3's weightings of the rectified-flow loss on the step's shifted t).
    Each sample's token weights are normalised to average to its timestep factor, so the loss scale (and
    with it the learning rate) carries over from unweighted runs. ValueError for anything else: a bool, a
    string where a number belongs, a NaN, a value out of range, an unknown weighting."""
    def number(key, default, ok, what):
        v = getattr(config, key, None)
        if v is None:
            return default
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not ok(float(v)) or math.isinf(float(v)):
            raise ValueError(f"{key} must be {what}, got {v!r}")
        return float(v)
    face = number("loss_face_weight", 1.0, lambda v: v > 0, "a finite float > 0")
    pad = number("loss_face_pad", 0.0, lambda v: v >= 0, "a finite float >= 0")
    frame0 = number("loss_frame0_weight", 1.0, lambda v: v >= 0, "a finite float >= 0")
    scheme = getattr(config, "loss_timestep_weighting", None)
    if scheme is None:
        scheme = "none"
    if not isinstance(scheme, str) or scheme not in TIMESTEP_WEIGHTINGS:
        raise ValueError(f"loss_timestep_weighting {scheme!r} is not one of {', '.join(TIMESTEP_WEIGHTINGS)}")
    lw = LossWeights(face, pad, frame0, scheme)
    return None if lw == LossWeights() else lw


def timestep_loss_weight(t, scheme):
    """The per-sample factor of `loss_timestep_weighting` on the step's (shifted) t, f32 [B], or None for
    "none": torch ops on t's device, nothing is read back. "sigma_sqrt": t^-2; "cosmap":
    2 / (pi (1 - 2 t + 2 t^2))."""
    if scheme == "none":
        return None
    if scheme == "sigma_sqrt":
        return (1.0 / (t * t)).contiguous()
    if scheme == "cosmap":
        return (2.0 / (math.pi * (1.0 - 2.0 * t + 2.0 * (t * t)))).contiguous()
    raise ValueError(f"loss_timestep_weighting {scheme!r} is not one of {', '.join(TIMESTEP_WEIGHTINGS)}")


_FRAME_WEIGHTS = {}  # (F, frame0_weight, device) -> the f32 [F] frame weights on the device


def _frame_weights(F, frame0_weight, device):
    """None for a first-frame weight of 1, else ones with frame0_weight in front (built once per key, with
    device fills: no host-to-device copy in the step)."""
    if frame0_weight == 1.0:
        return None
    key = (int(F), float(frame0_weight), str(torch.device(device)))
    fw = _FRAME_WEIGHTS.get(key)
    if fw is None:
        fw = torch.ones(F, dtype=torch.float32, device=device)
        fw[:1].fill_(frame0_weight)
        _FRAME_WEIGHTS[key] = fw
    return fw


def token_loss_weights_ref(B, F, H, W, bbox=None, frame_w=None, sample_w=None, user_w=None, face_weight=1.0,
                           face_pad=0.0):
    """The statement, in float64 torch ops on the inputs' device, of ltx_loss_token_weights (the kernel
    does the same arithmetic in f32): (wt [B, N], raw_sum [B]), N = F H W, token n = (f H + h) W + w.
      box: bbox[b] = (x_min, y_min, x_max, y_max), padded by face_pad times its width / height on each
           side, clipped to [0, 1]; a NaN coordinate or an empty clipped box: cov = 0 for the sample;
      ox = min(1, max(0, min(x1, (w + 1) / W) - max(x0, w / W)) W), oy likewise with h and H, cov = ox oy;
      raw[b, n] = frame_w[f] (1 + (face_weight - 1) cov) user_w[b, n];
      raw_sum[b] = sum_n raw[b, n]; wt[b, n] = sample_w[b] raw[b, n] N / raw_sum[b], 0 where raw_sum[b] = 0.
    A None input is all ones (bbox None: no box). user_w may be [B, N] or [B, F, H, W]."""
    f64 = torch.float64
    N = F * H * W
    dev = next((x.device for x in (bbox, frame_w, sample_w, user_w) if x is not None), torch.device("cpu"))
    cov = torch.zeros(B, H, W, dtype=f64, device=dev)
    if bbox is not None:
        box = bbox.to(f64).reshape(B, 4)
        valid = ~torch.isnan(box).any(dim=1)
        x0, y0, x1, y1 = box.unbind(1)
        px, py = face_pad * (x1 - x0), face_pad * (y1 - y0)
        x0, x1 = (x0 - px).clamp(0, 1), (x1 + px).clamp(0, 1)
        y0, y1 = (y0 - py).clamp(0, 1), (y1 + py).clamp(0, 1)
        valid = valid & (x1 > x0) & (y1 > y0)
        ws = torch.arange(W, dtype=f64, device=dev)
        hs = torch.arange(H, dtype=f64, device=dev)
        ox = ((torch.minimum(x1[:, None], (ws + 1) / W) - torch.maximum(x0[:, None], ws / W)).clamp(min=0) * W)
        oy = ((torch.minimum(y1[:, None], (hs + 1) / H) - torch.maximum(y0[:, None], hs / H)).clamp(min=0) * H)
        cov = oy.clamp(max=1)[:, :, None] * ox.clamp(max=1)[:, None, :]
        cov = torch.where(valid[:, None, None], cov, torch.zeros_like(cov))
    raw = (1.0 + (float(face_weight) - 1.0) * cov)[:, None].expand(B, F, H, W)
    if frame_w is not None:
        raw = raw * frame_w.to(f64).reshape(1, F, 1, 1)
    raw = raw.reshape(B, N)
    if user_w is not None:
        raw = raw * user_w.to(f64).reshape(B, N)
    raw_sum = raw.sum(dim=1)
    sw = torch.ones(B, dtype=f64, device=dev) if sample_w is None else sample_w.to(f64).reshape(B)
    safe = torch.where(raw_sum != 0, raw_sum, torch.ones_like(raw_sum))
    wt = torch.where((raw_sum != 0)[:, None], sw[:, None] * raw * N / safe[:, None], torch.zeros_like(raw))
    return wt, raw_sum


LOSS_TYPES = ("l2", "huber", "smooth_l1")
HUBER_SCHEDULES = ("constant", "exponential", "snr")

# What robust_loss_from_config decided, when loss_type is off "l2"
RobustLoss = collections.namedtuple("RobustLoss", "loss_type huber_c schedule")


def robust_loss_from_config(config):
    """RobustLoss or None from the optional config keys (setattr, or train.<key> in the YAML; not
    TrainConfig fields). None -- `loss_type` absent or "l2" -- is the reference's squared error, launch for
    launch:
      `loss_type` ("l2", the same as absent, "huber" or "smooth_l1"): the pseudo-Huber forms of the velocity
          loss (ltx_robust_loss_fwd_bwd), quadratic for residuals well below the threshold c and linear well
          above it; "huber" is 2 c (sqrt(e^2 + c^2) - c), which tends to e^2 as c grows; "smooth_l1" is
          2 (sqrt(e^2 + c^2) - c), which tends to 2 |e| as c shrinks;
      `huber_c` (a finite float > 0, absent = 0.1): the threshold at t = 1;
      `huber_schedule` ("constant", "exponential" or "snr", absent = "snr"): how the threshold follows the
          step's shifted t (huber_threshold): loose at low noise, tight at high noise.
    ValueError for an unknown name, a value of the wrong type, huber_c <= 0 or not finite, and for huber_c or
    huber_schedule set without a loss_type that reads them."""
    loss_type = getattr(config, "loss_type", None)
    c = getattr(config, "huber_c", None)
    schedule = getattr(config, "huber_schedule", None)
    if loss_type is None:
        loss_type = "l2"
    if not isinstance(loss_type, str) or loss_type not in LOSS_TYPES:
        raise ValueError(f"loss_type {loss_type!r} is not one of {', '.join(LOSS_TYPES)}")
    if c is not None and (isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c <= 0):
        raise ValueError(f"huber_c must be a finite float > 0, got {c!r}")
    if schedule is not None and (not isinstance(schedule, str) or schedule not in HUBER_SCHEDULES):
        raise ValueError(f"huber_schedule {schedule!r} is not one of {', '.join(HUBER_SCHEDULES)}")
    if loss_type == "l2":
        for key, val in (("huber_c", c), ("huber_schedule", schedule)):
            if val is not None:
                raise ValueError(f"{key} is set but loss_type is 'l2' (or absent): it is read only with "
                                 f"loss_type huber or smooth_l1")
        return None
    return RobustLoss(loss_type, 0.1 if c is None else float(c), "snr" if schedule is None else schedule)


_HUBER_CONSTS = {}  # (schedule, huber_c, B, device) -> the schedule's constant device tensor


def huber_threshold(t, schedule, huber_c):
    """The robust loss's threshold per sample, f32 [B], from the step's (shifted) t in [0, 1]: torch ops on
    t's device, nothing is read back and nothing copied from the host (the constant tensors are filled on
    the device, once per key). "constant": huber_c; "exponential": huber_c ** t; "snr":
    (1 - huber_c) (1 - t)^2 + huber_c, i.e. (1 - c) / (1 + sigma)^2 + c at the rectified flow's
    sigma = t / (1 - t). Both scheduled forms run from 1 at t = 0 to huber_c at t = 1."""
    huber_c = float(huber_c)
    if schedule == "snr":
        u = 1.0 - t
        return ((1.0 - huber_c) * (u * u) + huber_c).contiguous()
    if schedule not in ("constant", "exponential"):
        raise ValueError(f"huber_schedule {schedule!r} is not one of {', '.join(HUBER_SCHEDULES)}")
    B = t.numel() if schedule == "constant" else 0
    key = (schedule, huber_c, B, str(t.device))
    const = _HUBER_CONSTS.get(key)
    if const is None:
        # constant: the [B] thresholds themselves; exponential: the 0-dim base of the power
        const = torch.full((B,) if schedule == "constant" else (), huber_c, dtype=torch.float32, device=t.device)
        _HUBER_CONSTS[key] = const
    if schedule == "constant":
        return const
    return torch.pow(const, t).contiguous()


def robust_loss_ref(out, v, c, kind, wt=None, grad_scale=1.0):
    """The statement, in float64 on the CPU, of ltx_robust_loss_fwd_bwd (the kernel does the loss term in
    f32): out, v [B, ..., C] (their values as given: bf16 tensors are widened exactly), c [B], kind 1
    (huber) or 2 (smooth_l1), wt one weight per row of C, or None for ones. Returns (sums f64 [5], dout f64
    of out's shape, before the kernel's one bf16 rounding):
      e = o - v, r = sqrt(e^2 + c_b^2), l = k_b e^2 / (r + c_b), g = k_b e / r, k_b = 2 c_b | 2;
      sums = (sum wt l, sum v, sum v^2, sum bf16(d d) with d = bf16(o - v), sum l), dout = wt g grad_scale / n."""
    if kind not in (1, 2):
        raise ValueError(f"robust_loss_ref: kind must be 1 (huber) or 2 (smooth_l1), got {kind!r}")
    f64 = torch.float64
    o64, v64 = out.detach().cpu().to(f64), v.detach().cpu().to(f64)
    B, C = out.shape[0], out.shape[-1]
    n = o64.numel()
    tail = (1,) * (out.dim() - 1)
    cb = c.detach().cpu().to(f64).reshape(B, *tail)
    w = torch.ones((), dtype=f64) if wt is None else wt.detach().cpu().to(f64).reshape(*out.shape[:-1], 1)
    k = 2.0 * cb if kind == 1 else torch.full_like(cb, 2.0)
    e = o64 - v64
    r = torch.sqrt(e * e + cb * cb)
    l = k * (e * e) / (r + cb)
    g = k * e / r
    # the shipped loss's squared error: each of the two bf16 ops rounded, as ATen's mse does
    d = (out.detach().cpu() - v.detach().cpu()).bfloat16()
    q = (d * d).bfloat16()
    sums = torch.stack([(w * l).sum(), v64.sum(), (v64 * v64).sum(), q.to(f64).sum(), l.sum()])
    return sums, w * g * (float(grad_scale) / n)


class LRSchedule:
    """Learning rate as a pure function of the optimizer steps already taken: `at(s)` is
    base_lr * factor(s), the factors those of transformers.get_scheduler (so with warm-up the first
    step runs at lr 0, as it does there). With W = warmup_steps and T = total_steps:
      s < W                             s / max(1, W)
      constant, constant_with_warmup    1
      linear                            max(0, (T - s) / max(1, T - W))
      cosine                            max(0, 0.5 (1 + cos(pi (s - W) / max(1, T - W))))
    in Python float arithmetic. Nothing is stored between steps, so a resumed run needs only its
    global_step."""

    NAMES = ("constant", "constant_with_warmup", "linear", "cosine")
    DECAYING = ("linear", "cosine")

    def __init__(self, name, base_lr, warmup_steps=0, total_steps=None):
        if name not in self.NAMES:
            raise ValueError(f"lr_scheduler {name!r} is not one of {', '.join(self.NAMES)}")
        warmup_steps = int(warmup_steps)
        if warmup_steps < 0:
            raise ValueError(f"lr_warmup_steps must be >= 0, got {warmup_steps}")
        if name in self.DECAYING:
            if total_steps is None:
                raise ValueError(f"lr_scheduler {name!r} decays over lr_total_steps, which is not set")
            if int(total_steps) < 0:
                raise ValueError(f"lr_total_steps must be >= 0, got {total_steps}")
        self.name = name
        self.base_lr = float(base_lr)
        self.warmup_steps = warmup_steps
        self.total_steps = None if total_steps is None else int(total_steps)

    def factor(self, s):
        W, T = self.warmup_steps, self.total_steps
        if s < W:
            return float(s) / float(max(1, W))
        if self.name == "linear":
            return max(0.0, float(T - s) / float(max(1, T - W)))
        if self.name == "cosine":
            progress = float(s - W) / float(max(1, T - W))
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))
        return 1.0

    def at(self, s):
        return self.base_lr * self.factor(s)


def schedule_from_config(config, dataloader=None):
    """(max_grad_norm or None, LRSchedule or None) from the optional config keys (setattr, or
    train.<key> in the YAML; not TrainConfig fields): `max_grad_norm` (absent / 0: no clipping),
    `lr_scheduler` (absent = "constant"), `lr_warmup_steps` (absent = 0), `lr_total_steps` (absent =
    num_epochs * (len(dataloader) // gradient_accumulation_steps)). The schedule is None for a
    constant rate without warm-up. ValueError for an unknown scheduler, a negative warm-up or norm,
    and for a decaying schedule with neither lr_total_steps nor a sized loader."""
    max_norm = getattr(config, "max_grad_norm", None)
    if max_norm is not None:
        max_norm = float(max_norm)
        if not max_norm >= 0:
            raise ValueError(f"max_grad_norm must be >= 0, got {max_norm}")
    name = getattr(config, "lr_scheduler", None) or "constant"
    warmup = int(getattr(config, "lr_warmup_steps", 0) or 0)
    total = getattr(config, "lr_total_steps", None)
    if total is None and name in LRSchedule.DECAYING:
        try:
            per_epoch = len(dataloader)
        except TypeError:
            raise ValueError(f"lr_scheduler {name!r} needs lr_total_steps: the dataloader has no "
                             f"length to derive it from") from None
        accum = max(1, int(getattr(config, "gradient_accumulation_steps", 1)))
        total = int(config.num_epochs or 0) * (per_epoch // accum)
    schedule = LRSchedule(name, config.learning_rate or 0.0, warmup, total)
    if name in ("constant", "constant_with_warmup") and warmup == 0:
        schedule = None
    return (max_norm or None), schedule


class EMASchedule:
    """The decay of the exponential moving average of the trained weights as a pure function of n, the
    optimizer steps taken including the current one: `decay_at(n)` is diffusers' EMAModel.get_decay
    (training_utils.py; `--use_ema` in its training scripts) in Python float arithmetic. With
    k = max(0, n - update_after_step - 1):
      k == 0        0.0    (the shadow follows the weights)
      use_warmup    1 - (1 + k / inv_gamma) ** (-power)
      otherwise     (1 + k) / (10 + k)
    then min(., decay), then max(., min_decay). Nothing is stored between steps, so a resumed run needs
    only its step count. diffusers is not a dependency of this project and is not installed where the
    tests run: the formula is pinned to its published behaviour only, by hand-computed values."""

    FIELDS = ("decay", "use_warmup", "inv_gamma", "power", "update_after_step", "min_decay")

    def __init__(self, decay, use_warmup=False, inv_gamma=1.0, power=2 / 3, update_after_step=0, min_decay=0.0):
        decay, inv_gamma, power, min_decay = float(decay), float(inv_gamma), float(power), float(min_decay)
        if not 0.0 < decay <= 1.0:
            raise ValueError(f"ema_decay must be in (0, 1], got {decay}")
        if int(update_after_step) != update_after_step or int(update_after_step) < 0:
            raise ValueError(f"ema_update_after_step must be an integer >= 0, got {update_after_step}")
        if not inv_gamma > 0.0:
            raise ValueError(f"ema_inv_gamma must be > 0, got {inv_gamma}")
        if not 0.0 <= min_decay <= decay:
            raise ValueError(f"ema_min_decay must be in [0, ema_decay = {decay}], got {min_decay}")
        self.decay = decay
        self.use_warmup = bool(use_warmup)
        self.inv_gamma = inv_gamma
        self.power = power
        self.update_after_step = int(update_after_step)
        self.min_decay = min_decay

    def decay_at(self, n):
        k = max(0, int(n) - self.update_after_step - 1)
        if k <= 0:
            return 0.0
        if self.use_warmup:
            cur = 1 - (1 + k / self.inv_gamma) ** -self.power
        else:
            cur = (1 + k) / (10 + k)
        return float(max(min(cur, self.decay), self.min_decay))

    def fields(self):
        """The constructor's arguments as a JSON-able dict (train_state.json's "ema" block)."""
        return {k: getattr(self, k) for k in self.FIELDS}


def ema_from_config(config):
    """EMASchedule or None from the optional config keys (setattr, or train.<key> in the YAML; not
    TrainConfig fields): `ema_decay` (absent or 0: off), `ema_warmup` (a bool), `ema_inv_gamma`,
    `ema_power`, `ema_update_after_step`, `ema_min_decay`; absent ones take EMASchedule's defaults.
    NotImplementedError outside train_mode 'lora_audio' (the full mode's sharded Zero2AdamW is its own
    path), ValueError for what EMASchedule refuses."""
    decay = getattr(config, "ema_decay", None)
    if decay is None or float(decay) == 0.0:
        return None
    train_mode = getattr(config, "train_mode", "full")
    if train_mode != "lora_audio":
        raise NotImplementedError(f"ema_decay with train_mode={train_mode!r}: the EMA of the trained weights "
                                  f"rides FusedAdamW's step, which exists in lora_audio mode only")
    kw = {}
    for key, arg in (("ema_warmup", "use_warmup"), ("ema_inv_gamma", "inv_gamma"), ("ema_power", "power"),
                     ("ema_update_after_step", "update_after_step"), ("ema_min_decay", "min_decay")):
        if getattr(config, key, None) is not None:
            kw[arg] = getattr(config, key)
    return EMASchedule(decay, **kw)


def guard_from_config(config):
    """(skip_nonfinite, max_consecutive_skips or None) from the optional config keys (setattr, or
    train.<key> in the YAML; not TrainConfig fields): `skip_nonfinite` (a bool; absent or false: off, and
    the run is today's) makes FusedAdamW / FusedProdigy skip, on the device, every optimizer step whose
    gradients are not all finite; `max_consecutive_skips` (an int >= 0; absent or 0: no limit) makes
    train_one_epoch raise FloatingPointError once more steps than that were skipped in a row. ValueError for
    a value that is not a bool / not an integer >= 0 and for the limit without the guard;
    NotImplementedError outside train_mode 'lora_audio' or with use_deepspeed (the sharded Zero2AdamW step
    is its own path)."""
    on = getattr(config, "skip_nonfinite", None)
    limit = getattr(config, "max_consecutive_skips", None)
    if on is not None and not isinstance(on, bool):
        raise ValueError(f"skip_nonfinite must be a bool, got {on!r}")
    if limit is not None:
        if isinstance(limit, bool) or not isinstance(limit, int) or limit < 0:
            raise ValueError(f"max_consecutive_skips must be an integer >= 0, got {limit!r}")
        if not on:
            raise ValueError("max_consecutive_skips set without skip_nonfinite: true")
    if not on:
        return False, None
    train_mode = getattr(config, "train_mode", "full")
    if train_mode != "lora_audio" or getattr(config, "use_deepspeed", False):
        raise NotImplementedError(f"skip_nonfinite with train_mode={train_mode!r}, use_deepspeed="
                                  f"{bool(getattr(config, 'use_deepspeed', False))}: the guard rides the step of "
                                  f"FusedAdamW and FusedProdigy, which step the lora_audio trainable set; the "
                                  f"sharded Zero2AdamW path has none")
    return True, (limit or None)


def _check_cap(value, what="scale_weight_norms"):
    """None for None or 0 (off), else the cap as a float; ValueError for a bool, a string or anything else that
    is not a real number, for a negative and for a non-finite value."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"{what} must be a number > 0 (or absent / 0 for off), got {value!r}")
    cap = float(value)
    if not math.isfinite(cap) or cap < 0.0:
        raise ValueError(f"{what} must be a finite number > 0 (or absent / 0 for off), got {value!r}")
    return cap or None


def max_norm_from_config(config):
    """The cap of the max-norm pass, or None, from the optional config key `scale_weight_norms` (setattr, or
    train.scale_weight_norms in the YAML; not a TrainConfig field): kohya's --scale_weight_norms. Absent, None
    or 0: off, and the run is today's. With a cap c > 0 FusedAdamW / FusedProdigy scale, after every optimizer
    step and on the device, the A and B of every adapter whose |s| ||B A||_F exceeds c so that it sits on c
    (DESIGN.md "Max-norm (scale_weight_norms)"). ValueError for a bool, a string, a negative or a non-finite
    value; NotImplementedError outside train_mode 'lora_audio' or with use_deepspeed (the sharded Zero2AdamW
    step is its own path)."""
    cap = _check_cap(getattr(config, "scale_weight_norms", None))
    if cap is None:
        return None
    train_mode = getattr(config, "train_mode", "full")
    if train_mode != "lora_audio" or getattr(config, "use_deepspeed", False):
        raise NotImplementedError(f"scale_weight_norms with train_mode={train_mode!r}, use_deepspeed="
                                  f"{bool(getattr(config, 'use_deepspeed', False))}: the max-norm pass rides the "
                                  f"step of FusedAdamW and FusedProdigy, which step the lora_audio trainable set; "
                                  f"the sharded Zero2AdamW path has none")
    return cap


BF16_UPDATES = ("nearest", "stochastic")


def _check_bf16_update(bf16_update, sr_seed):
    """(mode, seed) validated: ValueError for a mode outside BF16_UPDATES or a seed outside [0, 2^64)."""
    if bf16_update not in BF16_UPDATES:
        raise ValueError(f"bf16_update {bf16_update!r} is not one of {', '.join(BF16_UPDATES)}")
    if isinstance(sr_seed, bool) or not isinstance(sr_seed, int) or not 0 <= sr_seed < 2 ** 64:
        raise ValueError(f"sr_seed must be an integer in [0, 2^64), got {sr_seed!r}")
    return bf16_update, int(sr_seed)


def stochastic_round_bits(seed, ordinal, step, index):
    """The 16-bit random numbers (numpy uint32, the shape of `index`) that round elements `index` of
    parameter `ordinal` at its step `step` under `seed`: Philox4x32-10 (lora.philox4x32_10) on the counter
    (lo32(i >> 3), hi32(i >> 3), ordinal, step mod 2^32) with the key (seed lo, seed hi); element i takes
    the 16-bit lane i & 7 of the four output words, low half of word (i & 7) // 2 for an even lane, high
    half for an odd one (the rule of the LoRA dropout mask). CPU only."""
    import numpy as np

    from .lora import philox4x32_10
    _, seed = _check_bf16_update("stochastic", seed)
    i = np.asarray(index, dtype=np.uint64)
    q = i >> np.uint64(3)
    words = philox4x32_10((q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), int(ordinal) & 0xFFFFFFFF,
                           int(step) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, seed >> 32))
    lane = (i & np.uint64(7)).astype(np.int64)
    word = np.choose(lane >> 1, [np.broadcast_to(w, i.shape) for w in words])
    return (word >> (np.uint32(16) * (lane & 1).astype(np.uint32))) & np.uint32(0xFFFF)


def stochastic_round_bf16(x_f32, seed, ordinal, step, r=None):
    """The statement, on the CPU, of the stochastically rounded bf16 store of
    FusedAdamW / FusedProdigy(bf16_update="stochastic"): `x_f32` (a float32 torch tensor or numpy array,
    the f32 result of parameter `ordinal`'s step number `step`, elements in the tensor's contiguous order)
    rounded to bf16 with the 16-bit random numbers of stochastic_round_bits(seed, ordinal, step, i) -- or
    with `r` (an int or an array of x's shape) in their place. For a finite x the bf16 bits are
    (bits(x) + r) >> 16: the magnitude rounds up with probability (discarded 16 bits) / 2^16, so the
    expected value is x, a representable x stays for every r, and SR(-x) = -SR(x). NaN and +-inf take the
    round-to-nearest conversion. Returns a torch.bfloat16 CPU tensor of x's shape for a tensor, the uint16
    bit patterns for an array."""
    import numpy as np
    is_tensor = torch.is_tensor(x_f32)
    if is_tensor:
        if x_f32.dtype != torch.float32:
            raise TypeError(f"stochastic_round_bf16: expected float32, got {x_f32.dtype}")
        x = x_f32.detach().cpu().contiguous().numpy()
    else:
        x = np.ascontiguousarray(x_f32)
        if x.dtype != np.float32:
            raise TypeError(f"stochastic_round_bf16: expected float32, got {x.dtype}")
    u = x.view(np.uint32).reshape(-1).astype(np.uint64)
    if r is None:
        r = stochastic_round_bits(seed, ordinal, step, np.arange(u.size, dtype=np.uint64))
    r = np.broadcast_to(np.asarray(r, dtype=np.uint64).reshape(-1) & np.uint64(0xFFFF), u.shape)
    bits = ((u + r) >> np.uint64(16)).astype(np.uint16)
    special = (u & np.uint64(0x7F800000)) == np.uint64(0x7F800000)
    if special.any():
        nearest = torch.from_numpy(x.reshape(-1)[special].copy()).to(torch.bfloat16).view(torch.int16).numpy()
        bits[special] = nearest.view(np.uint16)
    bits = bits.reshape(x.shape)
    if is_tensor:
        return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    return bits


# ---- the chunk tables of the optimizer step -----------------------------------------------------
# Every table kernel of FusedAdamW / FusedProdigy walks int64 rows, one block per row of at most CHUNK
# elements of one tensor. The five layouts (`start`, `count`: chunk_rows' two fields; 0: a zero):
LAYOUTS = {
    "adamw": ("param", "grad", "exp_avg", "exp_avg_sq", "start", "count"),  # also what the norm pass reads
    "ema": ("param", "grad", "exp_avg", "exp_avg_sq", "start", "count", "ema", 0),
    "sr": ("param", "grad", "exp_avg", "exp_avg_sq", "start", "count", "ema or 0", "ordinal"),
    "swap": ("param", 0, 0, 0, "start", "count", "ema", "stash"),
    "prodigy": ("param", "grad", "exp_avg", "exp_avg_sq", "start", "count", "s", "p0", "ema or 0", "ordinal or 0"),
}


def chunk_rows(tensors, chunk):
    """The rows of a chunk table: for every (numel, head fields, tail fields) of `tensors`, in order, one
    row head + (start, count) + tail per `chunk` elements, count = min(chunk, numel - start). Pure: needs
    no device."""
    return [tuple(head) + (start, min(chunk, numel - start)) + tuple(tail)
            for numel, head, tail in tensors for start in range(0, numel, chunk)]


def tensor_fields(layout, items, ema=False, ordinals=None):
    """Per tensor of `items` the flat tuple (numel, the four fields in front of start, the fields behind
    count) of LAYOUTS[layout], pointers as integers: what a table is cached on and built from. `items`
    are (parameter, gradient, state) -- for "swap" (parameter, shadow, stash); `ema`: the shadow column
    of "sr" / "prodigy" is in use; `ordinals`: parameter -> ordinal (None: 0)."""
    if layout == "swap":
        return tuple([(p.numel(), p.data_ptr(), 0, 0, 0, s.data_ptr(), t.data_ptr()) for p, s, t in items])
    if layout == "adamw":
        return tuple([(p.numel(), p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())
                      for p, g, st in items])
    if layout == "ema":
        return tuple([(p.numel(), p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                       st["ema"].data_ptr(), 0) for p, g, st in items])
    if layout == "sr":
        return tuple([(p.numel(), p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                       st["ema"].data_ptr() if ema else 0, ordinals[p]) for p, g, st in items])
    assert layout == "prodigy", layout
    return tuple([(p.numel(), p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                   st["s"].data_ptr(), st["p0"].data_ptr(), st["ema"].data_ptr() if ema else 0,
                   0 if ordinals is None else ordinals[p]) for p, g, st in items])


def table_rows(fields, chunk):
    """chunk_rows of tensor_fields' flat tuples"""
    return chunk_rows([(t[0], t[1:5], t[5:]) for t in fields], chunk)


# ---- the two tables of the max-norm pass (csrc/max_norm.hip); not optimizer-step layouts, so not in LAYOUTS
# The pair table, one row per adapter pair: what the Gram, contraction and finish launches read.
MAX_NORM_PAIR = ("A", "B", "N", "K", "r", "scaling (f64 bits)", "A partials", "B partials", "first workgroup",
                 "slab", "slabs of K", "slabs of N")
# The scale table, chunk_rows over the paired tensors: one row per at most CHUNK elements of A or B.
MAX_NORM_ROW = ("param", "shadow or 0", "start", "count", "pair")


def max_norm_pair_rows(pairs):
    """(rows of MAX_NORM_PAIR, workgroups of the Gram launch, f64 of the partials' workspace) for `pairs`, a
    list of (A pointer, B pointer, N, K, r, scaling): every pair's plan from ops.max_norm_plan, its partials
    behind the previous pair's. Pure host code."""
    import struct
    rows, nwg, ws = [], 0, 0
    for a, b, N, K, r, s in pairs:
        slab, sa, sb, wgs, fa, fb = ops.max_norm_plan(N, K, r)
        bits = struct.unpack("<q", struct.pack("<d", float(s)))[0]
        rows.append((a, b, N, K, r, bits, ws, ws + fa, nwg, slab, sa, sb))
        nwg += wgs
        ws += fa + fb
    return rows, nwg, ws


def max_norm_scale_rows(tensors, chunk):
    """Rows of MAX_NORM_ROW for `tensors`, a list of (numel, parameter pointer, shadow pointer or 0, pair)."""
    return chunk_rows([(n, (p, shadow), (pair,)) for n, p, shadow, pair in tensors], chunk)


def _check_norm_pairs(norm_pairs, params):
    """[(name, A, B, scaling)] validated against the optimizer's parameters `params`: ValueError when a pair's
    tensors are not f32 contiguous parameters among them, when the shapes are not A [r, K] / B [N, r] with r one
    of ops.LORA_RANKS, or when a tensor appears in two pairs."""
    known, seen, out = {id(p) for p in params}, set(), []
    for item in norm_pairs:
        if not isinstance(item, (tuple, list)) or len(item) != 4:
            raise ValueError("norm_pairs: (module name, A, B, scaling) tuples expected, as lora.adapter_pairs returns")
        name, A, B, s = item
        for what, t in (("A", A), ("B", B)):
            if not isinstance(t, torch.nn.Parameter) or id(t) not in known:
                raise ValueError(f"norm_pairs: {what} of {name!r} is not a parameter of this optimizer")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"norm_pairs: {what} of {name!r} must be a contiguous f32 tensor, got {t.dtype}, "
                                 f"strides {t.stride()}")
            if id(t) in seen:
                raise ValueError(f"norm_pairs: {what} of {name!r} appears in two pairs")
            seen.add(id(t))
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[1] or A.shape[0] not in ops.LORA_RANKS \
                or A.numel() == 0 or B.numel() == 0:
            raise ValueError(f"norm_pairs: {name!r}: expected A [r, K] and B [N, r] with r one of "
                             f"{', '.join(map(str, ops.LORA_RANKS))}, got {tuple(A.shape)} and {tuple(B.shape)}")
        s = float(s)
        if not math.isfinite(s):
            raise ValueError(f"norm_pairs: {name!r}: the scaling must be finite, got {s}")
        out.append((str(name), A, B, s))
    return out


# One launch of the table step: the bucket's device table and its rows, 0 f32 / 1 bf16 / 2 bf16 with f32
# state and the stochastic store, the param group, the bucket's step count (None where the kernels take
# none) and the 6-field table of the norm pass (None when nothing is clipped)
_Launch = collections.namedtuple("_Launch", "table nrows mode group step norm_table")


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (defaults betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2; the
    reference constructs AdamW(trainable, lr) at training.py:270-271) with one ltx_adamw_step
    kernel per tensor; f32 LoRA adapters and bf16 caption-projection params keep their dtype.

    `max_grad_norm` (None or 0: off, and step() is the unclipped path call for call): the global
    gradient norm over every parameter group's parameters that have a gradient is clipped to it
    (torch.nn.utils.clip_grad_norm_ with an f64 norm), on the device and without a host sync:
    ltx_grad_sumsq_multi per (dtype, step) group over the chunk table, one ltx_grad_clip_coef, then
    ltx_adamw_multi_clip per group, which scales the gradient on the way in -- .grad itself stays
    unscaled. After such a step `grad_norm` (the pre-clip norm) and `clip_coef` are 0-dim f32 device
    tensors; reading them syncs only at float().

    `ema` (an EMASchedule; None: off, and step() is today's, call for call): an exponential moving
    average of every stepped parameter, updated inside the AdamW launch (ltx_adamw_multi_ema per (param
    group, dtype, step) bucket, the clip's norm and coefficient launches in front of them unchanged when
    max_grad_norm is set). state[p]["ema"] is the f32 shadow -- f32 for the bf16 caption projection too:
    at decay 0.9999 the increment is below bf16's resolution and a bf16 shadow would stop moving, which
    is where this departs from diffusers' EMAModel -- created with the moments as p.detach().float(),
    the value before the first step; after a step s = s - omd (s - float(p)) with
    omd = float32(1 - ema.decay_at(ema_steps)), three separately rounded f32 operations. `ema_steps`
    counts the steps taken, `ema_decay` is the last step's decay. A parameter without a gradient at a
    step is not averaged at that step (diffusers averages it anyway; no trainable parameter of this
    model is ever without one). Parameters, moments and steps are bitwise those of ema=None.
    ema_swap_in() / ema_swap_out() / the context manager ema_weights() install the shadows as the
    weights (rounded to the parameter's dtype) for an evaluation or an export and put the live values
    back; step() refuses to run in between.

    `bf16_update` ("nearest": today's step, call for call, bf16 moments and every op rounded to bf16 as
    torch steps a bf16 tensor; "stochastic", with `sr_seed` in [0, 2^64)): a bf16 parameter (its gradient
    must be bf16 too) keeps f32 exp_avg / exp_avg_sq, its step is the f32 arithmetic on float(p), float(g)
    (with the clip, float(bf16(g * coef))), and the result is stored stochastically rounded --
    stochastic_round_bf16, a pure function of (sr_seed, the parameter's index in the concatenation of
    param_groups[*]["params"], its state["step"], the element) -- through ltx_adamw_multi_sr, always the
    table kernels; the bf16 tensor stays the only copy of the weight, and the EMA shadow follows the value
    stored. f32 parameters are stepped bitwise as without the mode. The two values enter param_groups (and
    with them a checkpoint's train_state.json) in stochastic mode only.

    `skip_nonfinite` (False: today's step, call for call): a step whose gradients are not all finite is the
    step that was never called. Every step takes the global f64 sum of squares of the gradients it is about
    to use (the clip's norm pass; without max_grad_norm the guard adds it), which is finite iff every element
    is; ltx_grad_guard_record writes the decision into a 32-byte device record beside the norm and the
    coefficient, and the update launches (ltx_adamw_multi_guard, ltx_adamw_multi_sr_guard) read it and return
    before their first store, so a skipped step writes nothing but that record -- no parameter, moment or
    shadow, no stochastically rounded store -- and nothing syncs. Always the table kernels. The host's counts
    (state["step"], ema_steps, ema_decay) are put back lagged: the step leaves a 16-byte copy of its outcome
    on the way to pinned memory and an event behind it, and the next step() -- or settle(), which state_dict,
    ema_swap_in and io.save_adapter_checkpoint call -- waits for that event and undoes the skipped step's
    increments. After a guarded step `step_applied` is a 0-dim int32 device tensor (1 or 0), `grad_norm` the
    pre-clip norm also without max_grad_norm, `clip_coef` as above when clipping; `skipped_steps` (a Python
    int, settles first) counts the skipped steps and `consecutive_skips` those since the last applied one.
    The value enters param_groups only when on.

    `scale_weight_norms` (None or 0: today's step, call for call; a cap c > 0 with `norm_pairs`, the
    [(module name, A, B, scaling)] of lora.adapter_pairs): kohya's max-norm regularisation. After the update
    launches of every step -- always the table kernels -- every pair whose norm = |s| ||B A||_F exceeds c has
    A and B multiplied by f = float32(sqrt(c / norm)), so the update s B A sits on the cap
    (tests/max_norm_utils.py is the statement). Three entry points over device tables, whatever the number of
    pairs, and nothing syncs: ltx_max_norm_sumsq (the f64 Gram form of ||B A||_F^2, B A never formed),
    ltx_max_norm_finish (norm, ratio, f per pair and the record), ltx_max_norm_scale_multi (the stores; pairs
    at or under the cap store nothing). Moments, Prodigy's s / p0 and DoRA magnitudes are not touched, nor is
    any tensor outside the pairs. With `ema` a scaled element's shadow takes s <- s - omd (p_before - p_after),
    three separately rounded f32 operations, so the shadow stays the average of the weights as stored. Under
    `skip_nonfinite` a skipped step scales nothing. After a step `keys_scaled` (int32: the pairs scaled),
    `avg_key_norm` and `max_key_norm` (f32: mean and maximum of the norms after scaling) are 0-dim device
    tensors, views of a fresh record per step. Every decision is a function of the weights alone, in fixed
    summation orders: data-parallel ranks decide alike without a collective, and nothing enters a checkpoint.
    The value enters param_groups only when on."""

    CHUNK = 2048  # elements per block of the multi-tensor kernel

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 multi_tensor=True, max_grad_norm=None, ema=None, bf16_update="nearest", sr_seed=0,
                 skip_nonfinite=False, scale_weight_norms=None, norm_pairs=None):
        if max_grad_norm is not None and not float(max_grad_norm) >= 0:
            raise ValueError(f"max_grad_norm must be >= 0, got {max_grad_norm}")
        if ema is not None and not isinstance(ema, EMASchedule):
            raise TypeError(f"ema must be an EMASchedule or None, got {type(ema).__name__}")
        self.bf16_update, self.sr_seed = _check_bf16_update(bf16_update, sr_seed)
        cap = _check_cap(scale_weight_norms)
        if cap is not None and not norm_pairs:
            raise ValueError("scale_weight_norms without norm_pairs: pass lora.adapter_pairs(model)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        if self.bf16_update == "stochastic":
            defaults.update(bf16_update=self.bf16_update, sr_seed=self.sr_seed)
        if skip_nonfinite:
            defaults.update(skip_nonfinite=True)
        if cap is not None:
            defaults.update(scale_weight_norms=cap)
        super().__init__(params, defaults)
        # the max-norm pass: the validated pairs, the last step's record (0-dim device views) and the cached
        # device tables with their workspace
        self.norm_pairs = None
        if cap is not None:
            self.norm_pairs = _check_norm_pairs(norm_pairs, [p for g in self.param_groups for p in g["params"]])
        self.keys_scaled = self.avg_key_norm = self.max_key_norm = self.key_factors = None
        self._max_norm_cache = None
        self.multi_tensor = multi_tensor
        self._tables = []  # pinned host tables of the last two builds (alive until their H2D lands)
        self._table_cache = {}  # (layout, slot) -> (tensor_fields, device table, rows, pinned host table)
        self._clip_part = None  # f64 per-row partial sums of the norm pass
        # the last clipped step's device record: f64 sum of squares, f32 pre-clip norm, f32 coefficient
        self.clip_sumsq = self.grad_norm = self.clip_coef = None
        self.ema = ema
        self.ema_steps = 0  # optimizer steps taken with the EMA on
        self.ema_decay = None  # the last step's decay (a Python float)
        self._ema_stash = {}  # parameter -> the buffer its live value waits in while swapped in
        self._ema_swapped = None  # the (device table, rows, is_bf16) launches of the swap-in to undo
        # the non-finite guard: the last guarded step's flag (a 0-dim int32 device tensor), the device record
        # that carries the skipped count, the pinned host slot its outcome is copied to, and what settle()
        # needs to undo the host's counting of a step that turns out skipped
        self.step_applied = None
        self.consecutive_skips = 0  # skipped steps since the last applied one, as far as settled
        self._guard_rec = None  # the last step's 32-byte record (4 f64), or a restored count's
        self._guard_slot = None  # pinned int64[2]: applied (with the zero pad behind it), skipped
        self._guard_pending = None  # (event, states incremented, (ema_steps, ema_decay) before the tick or None)
        self._skipped_steps = 0  # the settled count

    def _skip_nonfinite(self):
        vals = {bool(g.get("skip_nonfinite", False)) for g in self.param_groups}
        if len(vals) > 1:
            raise ValueError("skip_nonfinite differs between parameter groups: the decision is global, over every "
                             "gradient of the step")
        return vals.pop() if vals else False

    def _scale_weight_norms(self):
        """The max-norm cap (0.0: off), one value over the parameter groups: the pairs belong to the optimizer."""
        vals = {float(g.get("scale_weight_norms") or 0.0) for g in self.param_groups}
        if len(vals) > 1:
            raise ValueError(f"scale_weight_norms differs between parameter groups ({sorted(vals)})")
        cap = vals.pop() if vals else 0.0
        if cap > 0 and not self.norm_pairs:
            raise ValueError("scale_weight_norms is set in param_groups, but the optimizer was built without "
                             "norm_pairs")
        return cap

    def settle(self):
        """Wait for the last guarded step's outcome (an event recorded behind a 16-byte copy into pinned host
        memory: the step's own work, not the queue behind it) and, when that step was skipped, put the host's
        counters back where they were before it: every incremented state["step"], ema_steps, ema_decay. step()
        calls this first, so does everything that reads those counters (state_dict, ema_swap_in,
        io.save_adapter_checkpoint). Without a pending outcome it does nothing."""
        pending = self._guard_pending
        if pending is None:
            return
        self._guard_pending = None
        event, touched, ema_before = pending
        event.synchronize()
        applied = int(self._guard_slot[0])
        self._skipped_steps = int(self._guard_slot[1])
        if applied:
            self.consecutive_skips = 0
            return
        self.consecutive_skips += 1
        for st in touched:
            st["step"] -= 1
        if ema_before is not None:
            self.ema_steps, self.ema_decay = ema_before

    @property
    def outcome_pending(self):
        """True while the last guarded step's outcome has not been settled."""
        return self._guard_pending is not None

    @property
    def skipped_steps(self):
        """Steps skipped for non-finite gradients so far (a Python int; settles first)."""
        self.settle()
        return self._skipped_steps

    def _guard_record(self, device):
        """The record the next guarded step reads the skipped count from: the last step's, or a zeroed one."""
        if self._guard_rec is None or self._guard_rec.device != device:
            self._guard_rec = torch.zeros(4, dtype=torch.float64, device=device)
            self._guard_rec[3:].view(torch.int64).fill_(self._skipped_steps)
        return self._guard_rec

    def restore_skipped_steps(self, count, device):
        """A checkpoint's skipped count, on the host and in a fresh device record (io.load_adapter_checkpoint,
        which settles before it restores anything)."""
        self._skipped_steps = int(count)
        self.consecutive_skips = 0
        self._guard_rec = None
        self._guard_record(torch.device(device))

    def state_dict(self):
        self.settle()
        return super().state_dict()

    def _max_grad_norm(self):
        vals = {float(g.get("max_grad_norm") or 0.0) for g in self.param_groups}
        if len(vals) > 1:
            raise ValueError(f"max_grad_norm differs between parameter groups ({sorted(vals)}): the "
                             f"norm is global, so it takes one value")
        v = vals.pop() if vals else 0.0
        if v < 0:
            raise ValueError(f"max_grad_norm must be >= 0, got {v}")
        return v

    # What a subclass states: the chunk-table layout of its step (None: AdamW's, by mode), the state key it
    # creates last, whether a nearest-mode bucket is split by step count (its kernels take the step), and
    # whether a step that finds no gradient still counts as an EMA step.
    _LAYOUT = None
    _LAST_STATE_KEY = "exp_avg_sq"
    _BUCKET_BY_STEP = True
    _EMPTY_STEP_TICKS = True

    @torch.no_grad()
    def step(self, closure=None):
        """The table step of both optimizers: guard, collect and validate, bucket by (param group, dtype or
        "sr", step) with the state created on the way, tables, the clip's launches when max_grad_norm is
        set, the EMA tick, the optimizer's own launches (_launch), bump_weight_generation."""
        if self._ema_swapped is not None:
            raise RuntimeError(f"{type(self).__name__}.step() while the EMA weights are swapped in: call "
                               f"ema_swap_out() first")
        guard = self._skip_nonfinite()
        if guard:
            self.settle()  # before any counter is read: the last step may not have happened
        max_norm = self._max_grad_norm()
        if self._step_without_tables(max_norm):
            return
        device = self._check_params(*self._names(max_norm))
        touched = []  # under the guard: the states this step increments
        ema, sr = self.ema, self.bf16_update == "stochastic"
        ordinals = self._ordinals() if sr else None
        last_key, by_step = self._LAST_STATE_KEY, self._BUCKET_BY_STEP
        launches = []
        for gi, group in enumerate(self.param_groups):
            buckets = {}  # (dtype or "sr", step) or, where the kernels take no step, dtype -> items, in order
            for p in group["params"]:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                st = self.state[p]
                kind = p.dtype
                mixed = sr and kind is torch.bfloat16
                if mixed:
                    self._mixed_state(g, st)
                    kind = "sr"
                if last_key not in st or (ema is not None and "ema" not in st):
                    self._make_state(p, st, mixed)
                st["step"] += 1
                if guard:
                    touched.append(st)
                # the step count is part of a mixed bucket's rounding counter
                key = (kind, st["step"]) if (by_step or mixed) else kind
                buckets.setdefault(key, []).append((p, g.contiguous(), st))
            seen = {}
            for key, items in buckets.items():
                kind, step = key if type(key) is tuple else (key, None)
                j = seen[kind] = seen.get(kind, -1) + 1
                layout = self._LAYOUT or ("sr" if kind == "sr" else "adamw" if ema is None else "ema")
                # slot (kind, 0, 0) is also the unclipped fast path's: the usual case (one group, one step
                # count) switches between the two without a rebuild
                dev, nrows = self._items_table(layout, (kind, gi, j), items, ordinals)
                # the norm kernel walks 6-field rows and reads the gradient, first element and count only
                norm = dev if layout == "adamw" else None
                if (max_norm > 0 or guard) and norm is None:
                    norm = self._items_table("adamw", (kind, gi, j), items)[0]
                launches.append(_Launch(dev, nrows, 2 if kind == "sr" else 1 if kind is torch.bfloat16 else 0, group,
                                        step, norm))
        if launches:
            self._ready(device)
        ema_before = (self.ema_steps, self.ema_decay) if ema is not None else None
        omd = self._ema_tick() if (launches or self._EMPTY_STEP_TICKS) else None
        if not launches:
            self.clip_sumsq = self.grad_norm = self.clip_coef = self.step_applied = None
            self.keys_scaled = self.avg_key_norm = self.max_key_norm = None
            return
        stream = ops._s()
        cap = self._scale_weight_norms()
        if not guard:
            self.step_applied = None
            coef = self._clip_pass(launches, max_norm, device, stream)
            self._launch(launches, coef, omd, device, stream)
            if cap > 0:
                self._max_norm_pass(cap, omd, device)
        else:
            coef, rec = self._guard_pass(launches, max_norm, device, stream)
            self._launch(launches, coef, omd, device, stream, ops._p(rec))
            if cap > 0:
                self._max_norm_pass(cap, omd, device, ops._p(rec))
            self._guard_outcome(rec, touched, ema_before)
        ops.bump_weight_generation()  # in-place kernel updates: invalidate weight-derived caches

    def _names(self, max_norm):
        """(what, kernels, sums) of _check_params' messages"""
        if max_norm > 0:
            return "FusedAdamW(max_grad_norm)", "clip kernels", "the global norm"
        if self._skip_nonfinite():
            return "FusedAdamW(skip_nonfinite)", "guard kernels", "the global norm"
        if self.ema is not None:
            return "FusedAdamW(ema)", "EMA kernels", "the global norm"
        if self._scale_weight_norms() > 0:
            return "FusedAdamW(scale_weight_norms)", "max-norm kernels", "the pairs' norms"
        return "FusedAdamW(bf16_update)", "stochastic-rounding kernels", "the global norm"

    def _check_params(self, what, kernels, sums=None):
        """Every parameter with a gradient is an f32 or bf16 ROCm device tensor, all on one device, which is
        returned. `sums` None (the swap): every parameter with a shadow instead, on any devices."""
        from . import _lib
        swap, device = sums is None, None
        for group in self.param_groups:
            for p in group["params"]:
                if ("ema" not in self.state.get(p, ())) if swap else (p.grad is None):
                    continue
                if not p.is_cuda:
                    raise _lib.LtxHipError(f"{what}: the {kernels} need ROCm device parameters, got one on {p.device}")
                if p.dtype not in (torch.float32, torch.bfloat16):
                    raise TypeError(f"{what}: expected f32 or bf16 parameters, got {p.dtype}")
                if device is None:
                    device = p.device
                elif p.device != device and not swap:
                    raise ValueError(f"{what}: parameters on {device} and {p.device}; the table kernels (and "
                                     f"{sums}) run on one device")
        return device

    def _make_state(self, p, st, mixed):
        """The lazy state of a parameter's first step (or what a restore left out): the moments in the
        parameter's dtype, f32 for a mixed step; the subclass's own (_extra_state); with the EMA the f32
        shadow, the value before the step."""
        if not st:
            mdtype = torch.float32 if mixed else p.dtype
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, dtype=mdtype)
            st["exp_avg_sq"] = torch.zeros_like(p, dtype=mdtype)
        self._extra_state(p, st, mixed)
        if self.ema is not None and "ema" not in st:
            # with the moments; later only where a restore brought moments without shadows
            st["ema"] = p.detach().float().clone()

    def _extra_state(self, p, st, mixed):
        pass

    def _ready(self, device):
        """Before the first launch of a step that has something to step."""

    def _ema_tick(self):
        """Count an EMA step; returns 1 - decay in double (the entry points take it as one f32), None
        without an EMA."""
        if self.ema is None:
            return None
        self.ema_steps += 1
        self.ema_decay = self.ema.decay_at(self.ema_steps)
        return 1.0 - self.ema_decay

    def _clip_pass(self, launches, max_norm, device, stream):
        """With max_norm > 0 the norm launches of all buckets and the coefficient launch; sets clip_sumsq /
        grad_norm / clip_coef and returns the coefficient's pointer. Otherwise clears the three and returns
        None."""
        if not max_norm > 0:
            self.clip_sumsq = self.grad_norm = self.clip_coef = None
            return None
        part, total = self._norm_partials(launches, device, stream)
        # the record {f64 sumsq, f32 norm, f32 coef}: a fresh one per step, so a norm somebody holds keeps
        # its value
        rec = torch.empty(2, dtype=torch.float64, device=device)
        tail = rec[1:].view(torch.float32)
        ops.call("ltx_grad_clip_coef", ops._p(part), total, float(max_norm), ops._p(rec), stream)
        self.clip_sumsq, self.grad_norm, self.clip_coef = rec[0], tail[0], tail[1]
        return ops._p(tail[1])

    def _norm_partials(self, launches, device, stream):
        """The norm launches of all buckets, each writing its per-row partials behind the previous bucket's;
        returns (the partials, how many)."""
        total = sum(l.nrows for l in launches)
        if self._clip_part is None or self._clip_part.numel() < total or self._clip_part.device != device:
            self._clip_part = torch.empty(total, dtype=torch.float64, device=device)
        part = self._clip_part
        off = 0
        for _, nrows, mode, _, _, norm_table in launches:
            ops.call("ltx_grad_sumsq_multi", ops._p(norm_table), nrows, 1 if mode else 0,
                     ctypes.c_void_p(part.data_ptr() + 8 * off), stream)
            off += nrows
        return part, total

    def _guard_pass(self, launches, max_norm, device, stream):
        """_clip_pass under the guard: the norm launches run with or without max_norm, and
        ltx_grad_guard_record in the coefficient launch's place writes the 32-byte guard record (the clip's
        record, then applied and the skipped count carried on from the last step's record). Sets clip_sumsq,
        grad_norm and step_applied, clip_coef when clipping, and returns (the coefficient's pointer or None,
        the record)."""
        part, total = self._norm_partials(launches, device, stream)
        prev = self._guard_record(device)
        # a fresh record per step, as the clip's: a norm or a flag somebody holds keeps its value
        rec = torch.empty(4, dtype=torch.float64, device=device)
        ops.call("ltx_grad_guard_record", ops._p(part), total, float(max_norm) if max_norm > 0 else 0.0,
                 ops._p(prev), ops._p(rec), stream)
        self._guard_rec = rec
        tail = rec[1:2].view(torch.float32)
        self.clip_sumsq, self.grad_norm = rec[0], tail[0]
        self.clip_coef = tail[1] if max_norm > 0 else None
        self.step_applied = rec[2:3].view(torch.int32)[0]
        return (ops._p(tail[1]) if max_norm > 0 else None), rec

    def _guard_outcome(self, rec, touched, ema_before):
        """Behind a guarded step's launches: the outcome (applied, the skipped count) on its way to the pinned
        slot, an event behind the copy, and what settle() rolls back if the step was skipped. settle() ran at
        the top of this step, so the slot is free."""
        if self._guard_slot is None:
            self._guard_slot = torch.zeros(2, dtype=torch.int64).pin_memory()
        self._guard_slot.copy_(rec[2:].view(torch.int64), non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self._guard_pending = (event, touched, ema_before)

    def _launch(self, launches, coef, omd, device, stream, guard=None):
        """One AdamW launch per bucket: ltx_adamw_multi_clip, with the EMA ltx_adamw_multi_ema (given the
        coefficient when clipping), for a mixed bucket ltx_adamw_multi_sr (the coefficient and the shadow
        as arguments), and for an f32 bucket of the stochastic mode without clip or EMA ltx_adamw_multi.
        `guard` (the guard record's pointer): ltx_adamw_multi_sr_guard for a mixed bucket, ltx_adamw_multi_guard
        (the coefficient and the EMA as arguments) for every other."""
        ema = self.ema is not None
        for table, nrows, mode, group, step, _ in launches:
            b1, b2 = group["betas"]
            hyper = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                     int(step))
            if guard is not None:
                tail = (coef, 1 if ema else 0, 0.0 if omd is None else omd)
                if mode == 2:
                    ops.call("ltx_adamw_multi_sr_guard", ops._p(table), nrows, *hyper, *tail, self.sr_seed, guard,
                             stream)
                else:
                    ops.call("ltx_adamw_multi_guard", ops._p(table), nrows, mode, *hyper, *tail, guard, stream)
            elif mode == 2:
                ops.call("ltx_adamw_multi_sr", ops._p(table), nrows, *hyper, coef, 1 if ema else 0,
                         0.0 if omd is None else omd, self.sr_seed, stream)
            elif ema:
                ops.call("ltx_adamw_multi_ema", ops._p(table), nrows, mode, *hyper, coef, omd, stream)
            elif coef is not None:
                ops.call("ltx_adamw_multi_clip", ops._p(table), nrows, mode, *hyper, coef, stream)
            else:
                ops.call("ltx_adamw_multi", ops._p(table), nrows, mode, *hyper, stream)

    def _max_norm_tables(self, device):
        """(pair table, pairs, Gram workgroups, workspace, factors, scale table, rows) on the device, built once
        per set of buffers and reused while every pair's A, B and their EMA shadows keep their storage. The
        workspace holds the Gram partials and, behind them, one f64 sum per pair. The pinned host copies stay
        alive in the cache entry until the next build, past their non-blocking uploads."""
        key, pairs, tensors = [], [], []
        for i, (_, A, B, s) in enumerate(self.norm_pairs):
            if A.device != device or B.device != device:
                raise ValueError(f"{type(self).__name__}(scale_weight_norms): pair {i} is on {A.device} / {B.device}, "
                                 f"the step on {device}")
            shadows = [(self.state.get(t) or {}).get("ema") for t in (A, B)]
            ptrs = [0 if sh is None else sh.data_ptr() for sh in shadows]
            key.append((A.data_ptr(), B.data_ptr(), ptrs[0], ptrs[1]))
            pairs.append((A.data_ptr(), B.data_ptr(), B.shape[0], A.shape[1], A.shape[0], s))
            tensors += [(A.numel(), A.data_ptr(), ptrs[0], i), (B.numel(), B.data_ptr(), ptrs[1], i)]
        hit = self._max_norm_cache
        if hit is not None and hit[0] == key:
            return hit[1]
        pair_rows, nwg, ws_f64 = max_norm_pair_rows(pairs)
        rows = max_norm_scale_rows(tensors, self.CHUNK)
        hosts = [torch.tensor(pair_rows, dtype=torch.int64).pin_memory(),
                 torch.tensor(rows, dtype=torch.int64).pin_memory()]
        table, scale = (h.to(device, non_blocking=True) for h in hosts)
        ws = torch.empty(ws_f64 + len(pairs), dtype=torch.float64, device=device)
        factor = torch.empty(len(pairs), dtype=torch.float32, device=device)
        out = (table, len(pairs), nwg, ws, factor, scale, len(rows))
        self._max_norm_cache = (key, out, hosts)
        return out

    def _max_norm_pass(self, cap, omd, device, guard=None):
        """The three max-norm entry points behind the update launches: the sums of squares of every pair, the
        factors and the record (a fresh one per step, so a value somebody holds keeps it), the stores. `omd`:
        this step's 1 - decay for the shadows' correction (None without an EMA); `guard`: the guard record's
        pointer, under which a skipped step scales nothing."""
        table, npairs, nwg, ws, factor, scale, nrows = self._max_norm_tables(device)
        sumsq = ws[ws.numel() - npairs:]
        ops.max_norm_sumsq(table, npairs, nwg, ws, sumsq)
        rec = torch.empty(4, dtype=torch.int32, device=device)
        ops.max_norm_finish(table, sumsq, npairs, cap, factor, rec, guard)
        ops.max_norm_scale_multi(scale, nrows, factor, 0.0 if omd is None else omd, guard)
        self.keys_scaled = rec[0]
        self.avg_key_norm, self.max_key_norm = rec[1:3].view(torch.float32)
        self.key_factors = factor  # f per pair, in norm_pairs' order: the pass's own buffer, rewritten every step

    def _step_without_tables(self, max_norm):
        """The unclipped, EMA-less, nearest step: ltx_adamw_multi per dtype group of more than one tensor,
        ltx_adamw_step otherwise, CPU parameters included. False when the step needs the table path."""
        if max_norm > 0 or self.ema is not None or self.bf16_update == "stochastic" or self._skip_nonfinite() \
                or self._scale_weight_norms() > 0:
            return False
        for group in self.param_groups:
            b1, b2 = group["betas"]
            todo = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                todo.append((p, p.grad.contiguous(), st))
            by_dtype = {}
            for item in todo:
                by_dtype.setdefault(item[0].dtype, []).append(item)
            for dtype, items in by_dtype.items():
                steps = {st["step"] for _, _, st in items}
                if self.multi_tensor and len(items) > 1 and len(steps) == 1 and items[0][0].is_cuda:
                    self._multi(items, dtype, group, b1, b2, steps.pop())
                    continue
                for p, g, st in items:
                    ops.adamw_step(p, g, st["exp_avg"], st["exp_avg_sq"], group["lr"], b1, b2,
                                   group["eps"], group["weight_decay"], st["step"])
        ops.bump_weight_generation()  # in-place kernel updates: invalidate weight-derived caches
        return True

    def _multi(self, items, dtype, group, b1, b2, step):
        """One ltx_adamw_multi launch for all tensors of a dtype (bitwise the per-tensor math)."""
        dev, nrows = self._items_table("adamw", (dtype, 0, 0), items)
        ops.call("ltx_adamw_multi", ops._p(dev), nrows, 1 if dtype == torch.bfloat16 else 0,
                 float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                 float(group["weight_decay"]), int(step), ops._s())

    def _items_table(self, layout, slot, items, ordinals=None):
        """(device chunk table, rows) of `items` in LAYOUTS[layout] (tensor_fields' items), cached in the
        entry (layout, slot)."""
        fields = tensor_fields(layout, items, self.ema is not None, ordinals)
        return self._chunk_table((layout, slot), fields, items)

    def _chunk_table(self, slot, fields, items):
        """(device table, rows) of the tensors `fields` (tensor_fields' tuples of `items`, on whose first
        tensor's device the table goes). A table (~10^4 rows at
        LTX-2B: milliseconds of host time) is built once per set of buffers and reused while the cache
        entry `slot` holds the same fields, that is while the parameter / gradient / state storages stay
        the same. The pinned host copy stays alive until its H2D copy has landed: the cache entry holds
        it, and so do the last two builds, for an entry that is rebuilt at once."""
        hit = self._table_cache.get(slot)
        if hit is not None and hit[0] == fields:
            return hit[1], hit[2]
        rows = table_rows(fields, self.CHUNK)
        host = torch.tensor(rows, dtype=torch.int64).pin_memory()
        dev = host.to(items[0][0].device, non_blocking=True)
        self._tables = (self._tables + [(host, dev)])[-2:]
        self._table_cache[slot] = (fields, dev, len(rows), host)
        return dev, len(rows)

    def _ordinals(self):
        """parameter -> its index in the concatenation of param_groups[*]["params"] (torch's state_dict
        index), the stream of its stochastic rounding"""
        out = {}
        for group in self.param_groups:
            for p in group["params"]:
                out[p] = len(out)
        return out

    def _mixed_state(self, grad, st):
        """The checks of a bf16 parameter's stochastic step: a bf16 gradient, f32 moments."""
        if grad.dtype != torch.bfloat16:
            raise TypeError(f"{type(self).__name__}(bf16_update='stochastic'): a bf16 parameter's gradient must "
                            f"be bf16, got {grad.dtype}")
        if st and st["exp_avg"].dtype != torch.float32:
            raise ValueError(f"{type(self).__name__}(bf16_update='stochastic'): a bf16 parameter's moments are "
                             f"{st['exp_avg'].dtype}, from a run in nearest mode; they are not converted")

    # ---- the averaged weights as the model's weights ---------------------------------------
    def _swap_tables(self):
        """[(device table, rows, is_bf16)] over every parameter that has a shadow, one per dtype: the
        EMA rows with (param, 0, 0, 0, first element, count, shadow, stash). The stashes are allocated
        on first use and kept; the tables are cached on the three pointers."""
        by_dtype = {}
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if not st or "ema" not in st or p.numel() == 0:
                    continue
                stash = self._ema_stash.get(p)
                if stash is None or stash.shape != p.shape or stash.dtype != p.dtype or stash.device != p.device:
                    stash = self._ema_stash[p] = torch.empty_like(p)
                by_dtype.setdefault(p.dtype, []).append((p, st["ema"], stash))
        return [self._items_table("swap", dtype, items) + (1 if dtype == torch.bfloat16 else 0,)
                for dtype, items in by_dtype.items()]

    @torch.no_grad()
    def ema_swap_in(self):
        """Stash the live value of every parameter that has a shadow and install the shadow in its
        place, rounded to the parameter's dtype (ltx_ema_load_multi, one launch per dtype); the
        weight-derived caches are invalidated. RuntimeError without an EMA or while swapped in."""
        if self.ema is None:
            raise RuntimeError("FusedAdamW.ema_swap_in(): this optimizer keeps no EMA (ema=None)")
        if self._ema_swapped is not None:
            raise RuntimeError("FusedAdamW.ema_swap_in(): the EMA weights are swapped in already")
        self.settle()
        self._check_params("FusedAdamW(ema)", "EMA kernels")
        launches = self._swap_tables()
        stream = ops._s()
        for dev, nrows, is_bf16 in launches:
            ops.call("ltx_ema_load_multi", ops._p(dev), nrows, is_bf16, stream)
        self._ema_swapped = launches
        ops.bump_weight_generation()

    @torch.no_grad()
    def ema_swap_out(self):
        """Put the stashed live values back (ltx_ema_restore_multi over the swap-in's tables).
        RuntimeError when nothing is swapped in."""
        if self._ema_swapped is None:
            raise RuntimeError("FusedAdamW.ema_swap_out(): the EMA weights are not swapped in")
        stream = ops._s()
        for dev, nrows, is_bf16 in self._ema_swapped:
            ops.call("ltx_ema_restore_multi", ops._p(dev), nrows, is_bf16, stream)
        self._ema_swapped = None
        ops.bump_weight_generation()

    @contextlib.contextmanager
    def ema_weights(self):
        """`with optimizer.ema_weights():` runs its body under the averaged weights."""
        self.ema_swap_in()
        try:
            yield self
        finally:
            self.ema_swap_out()


class FusedProdigy(FusedAdamW):
    """Prodigy (Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner"; the
    published prodigyopt.Prodigy for one parameter group with fsdp_in_use = False), the optimizer that
    estimates its own step size d: `lr` stays at 1.0 (times a schedule's factor). The statement is DESIGN.md's
    Prodigy section and tests/prodigy_utils.ProdigyStatement. d, d_max, d_numerator and the step count k live
    in `record`, a float64 device tensor (RECORD names its eight fields), and a step never reads it back:

      [ltx_grad_sumsq_multi per dtype, ltx_grad_clip_coef]      with max_grad_norm, as FusedAdamW
      ltx_prodigy_moments_multi per dtype   exp_avg, exp_avg_sq, s with the old d; f64 partials per row
      ltx_prodigy_d_update                  the f64 update of the record
      ltx_prodigy_apply_multi per dtype     the parameter step (a no-op where the sum of |s| was 0) and, with
                                            `ema`, the shadow update of FusedAdamW(ema)

    state[p] holds exp_avg, exp_avg_sq, s and p0 in the parameter's dtype (p0: the value before the first
    step) and "step", the steps this parameter took. Parameters without a gradient are skipped and keep
    everything. A step with lr == 0 launches nothing and changes nothing. The public surface is FusedAdamW's
    (max_grad_norm, grad_norm / clip_coef, ema, ema_swap_in / ema_swap_out / ema_weights) plus `record` and
    `d`, a 0-dim float64 device tensor that syncs only at float(). One parameter group only.

    `bf16_update="stochastic"` / `sr_seed`, as FusedAdamW's: a bf16 parameter keeps f32 exp_avg, exp_avg_sq
    and s (p0 stays a bf16 clone, which is exact), both passes run the f32 arithmetic on float(p), float(g)
    and float(p0) (ltx_prodigy_moments_multi in its mixed mode, ltx_prodigy_apply_multi_sr), and pass 2
    stores the parameter stochastically rounded (stochastic_round_bf16).

    `scale_weight_norms` / `norm_pairs`, as FusedAdamW's: the max-norm pass runs behind pass 2. The scaled
    weights move without p0 following, so d's numerator sees the scaling as distance travelled (as it would
    under kohya's loop around prodigyopt); s, p0 and the record are not touched.

    `skip_nonfinite`, as FusedAdamW's: pass 1 and the d update run behind the guard record
    (ltx_prodigy_moments_multi_guard, ltx_prodigy_d_update_guard). A skipped step leaves exp_avg, exp_avg_sq,
    s, p0 and the record's d, d_max, d_numerator, d_denom, d_hat, dlr and k, and sets the record's applied to
    0, under which pass 2 is the no-op it already is; k lives on the device and needs no rollback.

    Two departures from the published code: the factor (d / d0) dlr multiplies the summed numerator once
    instead of every tensor's dot product, and a bf16 tensor's dot product is not rounded to bf16 before it
    is added (products in f32, sums in f64, fixed order: bitwise reproducible, the same on every rank)."""

    RECORD = ("d", "d_max", "d_numerator", "d_denom", "d_hat", "dlr", "k", "applied")
    HYPER = ("betas", "beta3", "eps", "weight_decay", "decouple", "use_bias_correction", "safeguard_warmup",
             "d0", "d_coef", "growth_rate")
    ROW = 10  # int64 fields per row of the Prodigy chunk table

    def __init__(self, params, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0,
                 decouple=True, use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0,
                 growth_rate=float("inf"), max_grad_norm=None, ema=None, bf16_update="nearest", sr_seed=0,
                 skip_nonfinite=False, scale_weight_norms=None, norm_pairs=None):
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must be in [0, 1), got {betas}")
        if beta3 is not None and not 0.0 <= float(beta3) < 1.0:
            raise ValueError(f"beta3 must be in [0, 1), got {beta3}")
        if not float(eps) > 0.0:
            raise ValueError(f"eps must be > 0, got {eps}")
        if not float(weight_decay) >= 0.0:
            raise ValueError(f"weight_decay must be >= 0, got {weight_decay}")
        if not (float(d0) > 0.0 and math.isfinite(float(d0))):
            raise ValueError(f"d0 must be a finite value > 0, got {d0}")
        if not float(d_coef) > 0.0:
            raise ValueError(f"d_coef must be > 0, got {d_coef}")
        if not float(growth_rate) > 0.0:
            raise ValueError(f"growth_rate must be > 0, got {growth_rate}")
        super().__init__(params, lr=lr, betas=(b1, b2), eps=float(eps), weight_decay=float(weight_decay),
                         max_grad_norm=max_grad_norm, ema=ema, bf16_update=bf16_update, sr_seed=sr_seed,
                         skip_nonfinite=skip_nonfinite, scale_weight_norms=scale_weight_norms,
                         norm_pairs=norm_pairs)
        extra = dict(beta3=None if beta3 is None else float(beta3), decouple=bool(decouple),
                     use_bias_correction=bool(use_bias_correction), safeguard_warmup=bool(safeguard_warmup),
                     d0=float(d0), d_coef=float(d_coef), growth_rate=float(growth_rate))
        self.defaults.update(extra)
        for group in self.param_groups:
            for k, v in extra.items():
                group.setdefault(k, v)
        self._one_group()
        self.record = None  # the float64 device record, made with the first step (or a restore)
        self._prodigy_part = None  # f64 (num, den) partials per row

    def _one_group(self):
        if len(self.param_groups) != 1:
            raise ValueError(f"FusedProdigy takes one parameter group, got {len(self.param_groups)}: d is "
                             f"estimated over all parameters together")
        return self.param_groups[0]

    def hyper(self):
        """The hyper-parameters that shape the trajectory besides lr, as a JSON-able dict: floats as
        float.hex() strings (growth_rate is inf by default), flags as bools, beta3 None when derived."""
        group = self._one_group()
        out = {}
        for k in self.HYPER:
            v = group[k]
            if isinstance(v, tuple):
                out[k] = [float(x).hex() for x in v]
            elif isinstance(v, bool) or v is None:
                out[k] = v
            else:
                out[k] = float(v).hex()
        return out

    def ensure_record(self, device=None):
        """The record, created as {d0, d0, 0, ...} on the parameters' device when it does not exist yet."""
        if self.record is None:
            group = self._one_group()
            if device is None:
                device = next((p.device for p in group["params"]), torch.device("cpu"))
            d0 = float(group["d0"])
            self.record = torch.tensor([d0, d0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=device)
        return self.record

    @property
    def d(self):
        """The step-size estimate: a 0-dim float64 view of the device record (float() syncs)."""
        return self.ensure_record()[0]

    _LAYOUT = "prodigy"
    _LAST_STATE_KEY = "s"
    _BUCKET_BY_STEP = False  # the nearest-mode kernels take no step count: one bucket per dtype
    _EMPTY_STEP_TICKS = False  # a step without a gradient changes nothing

    def _max_grad_norm(self):
        self._one_group()
        return super()._max_grad_norm()

    def _names(self, max_norm):
        return "FusedProdigy", "Prodigy kernels", "the sums behind d"

    def _step_without_tables(self, max_norm):
        if float(self.param_groups[0]["lr"]) == 0.0:
            # the published code returns before any state moves; nothing is launched
            self.clip_sumsq = self.grad_norm = self.clip_coef = self.step_applied = None
            return True
        return False

    def _extra_state(self, p, st, mixed):
        if "s" not in st:  # with the moments, before anything moves
            st["s"] = torch.zeros_like(p, dtype=torch.float32 if mixed else p.dtype)
            st["p0"] = p.detach().clone()

    def _ready(self, device):
        rec = self.ensure_record(device)
        if rec.device != device:
            raise ValueError(f"FusedProdigy: the record is on {rec.device}, the parameters on {device}")

    def _launch(self, launches, coef, omd, device, stream, guard=None):
        """Pass 1 per bucket (each writes its (num, den) partials behind the previous bucket's), the d
        update, pass 2 per bucket -- ltx_prodigy_apply_multi_sr for a mixed bucket. `guard` (the guard
        record's pointer): pass 1 and the d update through their _guard entry points; pass 2 as it is, gated
        on the record's applied, which a skipped step's d update has set to 0."""
        gated = () if guard is None else (guard,)
        suffix = "" if guard is None else "_guard"
        group, rec = launches[0].group, self.record
        ema, omd = 1 if self.ema is not None else 0, 0.0 if omd is None else omd
        total = sum(l.nrows for l in launches)
        if self._prodigy_part is None or self._prodigy_part.numel() < 2 * total or self._prodigy_part.device != device:
            self._prodigy_part = torch.empty(2 * total, dtype=torch.float64, device=device)
        part = self._prodigy_part
        lr = float(group["lr"])
        b1, b2 = (float(b) for b in group["betas"])
        b3 = math.sqrt(b2) if group["beta3"] is None else float(group["beta3"])
        d0, wd = float(group["d0"]), float(group["weight_decay"])
        decouple, use_bc = bool(group["decouple"]), int(bool(group["use_bias_correction"]))
        off = 0
        for table, nrows, mode, _, _, _ in launches:
            ops.call("ltx_prodigy_moments_multi" + suffix, ops._p(table), nrows, mode, ops._p(rec), lr, b1, b2, b3, d0,
                     0.0 if decouple else wd, use_bc, int(bool(group["safeguard_warmup"])), coef,
                     ctypes.c_void_p(part.data_ptr() + 16 * off), *gated, stream)
            off += nrows
        ops.call("ltx_prodigy_d_update" + suffix, ops._p(part), total, ops._p(rec), lr, b1, b2, b3, d0,
                 float(group["d_coef"]), float(group["growth_rate"]), use_bc, *gated, stream)
        for table, nrows, mode, _, step, _ in launches:
            if mode == 2:
                ops.call("ltx_prodigy_apply_multi_sr", ops._p(table), nrows, ops._p(rec), float(group["eps"]),
                         wd if decouple else 0.0, ema, omd, self.sr_seed, int(step), stream)
                continue
            ops.call("ltx_prodigy_apply_multi", ops._p(table), nrows, mode, ops._p(rec), float(group["eps"]),
                     wd if decouple else 0.0, ema, omd, stream)


OPTIMIZERS = ("adamw", "prodigy")
_PRODIGY_KEYS = (("prodigy_d0", "d0", float), ("prodigy_d_coef", "d_coef", float),
                 ("prodigy_growth_rate", "growth_rate", float), ("prodigy_beta3", "beta3", float),
                 ("prodigy_use_bias_correction", "use_bias_correction", bool),
                 ("prodigy_safeguard_warmup", "safeguard_warmup", bool), ("prodigy_decouple", "decouple", bool))


class OptimizerSpec:
    """What optimizer_from_config decided: `kind` ("adamw" or "prodigy"), `lr` and the constructor's other
    keyword arguments -- only those the config names, so absent keys leave the class's defaults (and for
    AdamW today's constructor call). build() makes the optimizer."""

    def __init__(self, kind, lr, kwargs):
        self.kind, self.lr, self.kwargs = kind, lr, dict(kwargs)

    def build(self, params, max_grad_norm=None, ema=None, skip_nonfinite=False, scale_weight_norms=None,
              norm_pairs=None):
        cls = FusedProdigy if self.kind == "prodigy" else FusedAdamW  # the module's names at call time
        kwargs = dict(self.kwargs, skip_nonfinite=True) if skip_nonfinite else self.kwargs
        if scale_weight_norms:  # absent: today's call
            kwargs = dict(kwargs, scale_weight_norms=scale_weight_norms, norm_pairs=norm_pairs)
        return cls(params, lr=self.lr, max_grad_norm=max_grad_norm, ema=ema, **kwargs)


def optimizer_from_config(config):
    """OptimizerSpec from the optional config keys (setattr, or train.<key> in the YAML; not TrainConfig
    fields), validated here, before anything is built: `optimizer` ("adamw", also when absent, or
    "prodigy"), `weight_decay`, `adam_beta1`, `adam_beta2`, `adam_eps` (absent: the chosen optimizer's
    defaults) and, with Prodigy, `prodigy_d0`, `prodigy_d_coef`, `prodigy_growth_rate`, `prodigy_beta3`,
    `prodigy_use_bias_correction`, `prodigy_safeguard_warmup`, `prodigy_decouple`. The rate is
    config.learning_rate; with Prodigy None means 1.0. ValueError for another optimizer name, a value out
    of range, or a prodigy_* key without `optimizer: prodigy`; NotImplementedError for Prodigy outside
    train_mode 'lora_audio' or with use_deepspeed (the sharded Zero2AdamW step is its own path).

    `bf16_update` ("nearest", also when absent: today's constructor call; "stochastic") and `bf16_sr_seed`
    (an integer in [0, 2^64), 0 when absent) select the stochastically rounded bf16 step of either
    optimizer; they become the keyword arguments bf16_update / sr_seed in stochastic mode only. The seed
    comes from the config and never from a generator, so every data-parallel rank rounds alike and the
    replicas stay identical without a collective. ValueError for another mode, a seed out of range or a
    seed without `bf16_update: stochastic`; NotImplementedError outside train_mode 'lora_audio' or with
    use_deepspeed."""
    kind = getattr(config, "optimizer", None)
    kind = "adamw" if kind is None else kind
    if kind not in OPTIMIZERS:
        raise ValueError(f"optimizer {kind!r} is not one of {', '.join(OPTIMIZERS)}")
    kw = {}
    mode, seed = getattr(config, "bf16_update", None), getattr(config, "bf16_sr_seed", None)
    mode, seed = _check_bf16_update("nearest" if mode is None else mode, 0 if seed is None else seed)
    if mode == "stochastic":
        train_mode = getattr(config, "train_mode", "full")
        if train_mode != "lora_audio" or getattr(config, "use_deepspeed", False):
            raise NotImplementedError(f"bf16_update 'stochastic' with train_mode={train_mode!r}, use_deepspeed="
                                      f"{bool(getattr(config, 'use_deepspeed', False))}: the stochastically rounded "
                                      f"step exists in FusedAdamW and FusedProdigy, which step the lora_audio "
                                      f"trainable set; the sharded Zero2AdamW path has none")
        kw.update(bf16_update=mode, sr_seed=seed)
    elif getattr(config, "bf16_sr_seed", None) is not None:
        raise ValueError("bf16_sr_seed set without bf16_update: stochastic")
    b1, b2 = getattr(config, "adam_beta1", None), getattr(config, "adam_beta2", None)
    if b1 is not None or b2 is not None:
        betas = (0.9 if b1 is None else float(b1), 0.999 if b2 is None else float(b2))
        if not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"adam_beta1 / adam_beta2 must be in [0, 1), got {betas}")
        kw["betas"] = betas
    eps = getattr(config, "adam_eps", None)
    if eps is not None:
        if not float(eps) > 0.0:
            raise ValueError(f"adam_eps must be > 0, got {eps}")
        kw["eps"] = float(eps)
    wd = getattr(config, "weight_decay", None)
    if wd is not None:
        if not float(wd) >= 0.0:
            raise ValueError(f"weight_decay must be >= 0, got {wd}")
        kw["weight_decay"] = float(wd)
    named = [key for key, _, _ in _PRODIGY_KEYS if getattr(config, key, None) is not None]
    lr = config.learning_rate
    if kind == "adamw":
        if named:
            raise ValueError(f"{', '.join(named)} set without optimizer: prodigy")
        return OptimizerSpec(kind, lr, kw)
    train_mode = getattr(config, "train_mode", "full")
    if train_mode != "lora_audio" or getattr(config, "use_deepspeed", False):
        raise NotImplementedError(f"optimizer 'prodigy' with train_mode={train_mode!r}, use_deepspeed="
                                  f"{bool(getattr(config, 'use_deepspeed', False))}: FusedProdigy steps the "
                                  f"lora_audio trainable set only; the sharded Zero2AdamW path has no Prodigy")
    for key, arg, cast in _PRODIGY_KEYS:
        v = getattr(config, key, None)
        if v is not None:
            kw[arg] = cast(v)
    if not (kw.get("d0", 1e-6) > 0.0 and math.isfinite(kw.get("d0", 1e-6))):
        raise ValueError(f"prodigy_d0 must be a finite value > 0, got {kw['d0']}")
    if not kw.get("d_coef", 1.0) > 0.0:
        raise ValueError(f"prodigy_d_coef must be > 0, got {kw['d_coef']}")
    if not kw.get("growth_rate", 1.0) > 0.0:
        raise ValueError(f"prodigy_growth_rate must be > 0, got {kw['growth_rate']}")
    if not 0.0 <= kw.get("beta3", 0.5) < 1.0:
        raise ValueError(f"prodigy_beta3 must be in [0, 1), got {kw['beta3']}")
    lr = 1.0 if lr is None else float(lr)
    if not lr >= 0.0:
        raise ValueError(f"learning_rate must be >= 0, got {lr}")
    return OptimizerSpec(kind, lr, kw)


class OverlapHooks:
    """Readiness tracking shared by the reducers that overlap their collectives with the last
    micro-step's backward (GradAllReduce here, zero.Zero2AdamW): ``self.buckets`` is a list of
    dicts with a "params" list, ``self._where`` maps id(param) -> (bucket, index), and the subclass
    implements ``_launch(bi)`` (start bucket bi's collective, set ``self._launched = bi + 1``).

    ``install(model)`` hooks the model: each block reports, at the end of its backward, the grads
    its own kernels wrote into .grad (the attn1 / attn2 parameters: LoRA adapters, and in
    train_mode='full' the attention weights, biases and q/k norm weights); every other trainable
    parameter -- including a block's scale_shift_table, whose gradient autograd accumulates AFTER
    the block's backward returns (through _AdaModFn) -- reports through a post-accumulate-grad
    hook. ``arm()`` before the last backward of an accumulation cycle; from then on a bucket
    launches as soon as all of its grads are final, always in index order on every rank (a ready
    bucket waits for its predecessors), so the collectives match across ranks."""

    # test-only: launch the collectives (and take their stream waits) even at world size 1, so a
    # one-GPU box exercises RCCL's own stream and the armed bucket path (tests/test_dp_gpu.py)
    collectives_at_world1 = False

    def _collectives_on(self):
        return self._world() > 1 or self.collectives_at_world1

    def _init_hooks(self):
        self._armed = False
        self._pending = None   # per bucket: grads not yet final
        self._launched = 0     # buckets [0, _launched) have their collective in flight
        self._works = []
        self._hooks = []
        self._block_cbs = []  # (weakref to block, callback) appended to its _grad_ready_hooks

    def _world(self):
        if not (dist.is_available() and dist.is_initialized()):
            return 1
        return dist.get_world_size(self.group)

    def install(self, model):
        import weakref
        self.uninstall()
        me = weakref.ref(self)

        def block_cb(b, done=None, ps=None, ids=None):
            # done: the subset the block has finished (None: all it writes); only parameters the
            # block's kernels write are reported here
            red = me()
            if red is not None:
                red._ready(ps if done is None else [p for p in done if id(p) in ids])

        in_blocks = set()
        for blk in getattr(model, "transformer_blocks", ()):
            written = [p for name in ("attn1", "attn2") if name in blk._modules
                       for p in blk._modules[name].parameters() if id(p) in self._where]
            if written:
                in_blocks.update(id(p) for p in written)
                cb = functools.partial(block_cb, ps=written, ids={id(p) for p in written})
                blk.__dict__.setdefault("_grad_ready_hooks", []).append(cb)
                self._block_cbs.append((weakref.ref(blk), cb))
        for p in self.params:
            if id(p) not in in_blocks:
                self._hooks.append(p.register_post_accumulate_grad_hook(
                    lambda q: me() is not None and me()._ready([q])))
        return self

    def uninstall(self):
        """Remove this reducer's block callbacks and post-accumulate-grad hooks."""
        for h in self._hooks:
            h.remove()
        self._hooks = []
        for bref, cb in self._block_cbs:
            blk = bref()
            hooks = blk.__dict__.get("_grad_ready_hooks") if blk is not None else None
            if hooks is not None:
                hooks[:] = [h for h in hooks if h is not cb]
        self._block_cbs = []

    def _prepare_arm(self):
        """subclass hook: make the grads views of the buckets before an armed backward"""

    def arm(self):
        """The next backward is the last of the accumulation cycle: reduce during it."""
        if not self._collectives_on():
            return
        self._prepare_arm()
        self._armed = True
        self._pending = [set(id(p) for p in b["params"]) for b in self.buckets]
        self._launched = 0
        self._works = []

    def _ready(self, ps):
        if not self._armed:
            return
        for p in ps:  # (each grad must be final after one report: one accumulation per backward)
            bi, _ = self._where[id(p)]
            self._pending[bi].discard(id(p))
        while self._launched < len(self.buckets) and not self._pending[self._launched]:
            self._launch(self._launched)


class GradAllReduce(OverlapHooks):
    """Data-parallel averaging of the trainable gradients (LoRA f32 + caption projection bf16)
    over torch.distributed (RCCL on ROCm, gloo in the CPU tests), overlapped with the backward.

    * The gradients ARE views of per-dtype flat bucket buffers (``zero_grad`` installs them), so
      the backward's kernels accumulate straight into what gets reduced: no pack, no copy-back.
      f32 buckets are reduced in place; bf16 buckets (caption projection) through an f32 staging
      copy (one cast each way), so the sum is f32 and rounds to bf16 once.
    * Buckets (~bucket_mb of f32 each) follow ``order``: the order the backward completes the
      grads (``Transformer3DModel.grad_ready_order``: last block first).
    * ``arm()`` before the LAST micro-step's backward of an accumulation cycle: a bucket's async
      all-reduce (SUM) is launched as soon as all of its grads are final (OverlapHooks) while the
      remaining blocks' backward runs.
    * ``__call__()`` (before the optimizer step) launches whatever has not been launched, waits
      (a stream wait, no host sync) and divides by the world size. Unarmed, it is the plain
      post-backward reduction of the same buckets: the two paths are bitwise equal.
    """

    def __init__(self, params, bucket_mb=25.0, group=None, order=None):
        params = [p for p in params if p.requires_grad]
        if order is not None:
            ids = {id(p) for p in params}
            ordered = [p for p in order if id(p) in ids]
            rest = [p for p in reversed(params) if id(p) not in {id(q) for q in ordered}]
            params = ordered + rest
        else:
            params = list(reversed(params))  # registration order reversed
        self.params = params
        self.group = group
        self.buckets = []  # each: {"dtype", "params", "offsets", "n", "flat", "stage"}
        open_b = {}
        for p in params:
            b = open_b.get(p.dtype)
            if b is None:
                b = {"dtype": p.dtype, "params": [], "offsets": [], "n": 0, "flat": None,
                     "stage": None}
                open_b[p.dtype] = b
                self.buckets.append(b)
            b["params"].append(p)
            b["offsets"].append(b["n"])
            b["n"] += p.numel()
            if b["n"] * 4 >= bucket_mb * 1e6:
                del open_b[p.dtype]
        self._where = {id(p): (bi, j) for bi, b in enumerate(self.buckets)
                       for j, p in enumerate(b["params"])}
        self._init_hooks()

    # ---- buffers -------------------------------------------------------------------------
    def _alloc(self, b):
        if b["flat"] is None:
            dev = b["params"][0].device
            b["flat"] = torch.zeros(b["n"], dtype=b["dtype"], device=dev)
            if b["dtype"] != torch.float32:
                b["stage"] = torch.empty(b["n"], dtype=torch.float32, device=dev)

    def _view(self, b, j):
        p, off = b["params"][j], b["offsets"][j]
        return b["flat"][off:off + p.numel()].view_as(p)

    @torch.no_grad()
    def zero_grad(self):
        """Zero every bucket (one fill each) and make each p.grad the view of its slice (in place
        of optimizer.zero_grad(set_to_none=True), which would detach the grads from the buckets)."""
        for b in self.buckets:
            self._alloc(b)
            b["flat"].zero_()
            for j, p in enumerate(b["params"]):
                p.grad = self._view(b, j)

    @torch.no_grad()
    def _adopt_grads(self, b):
        """Make the bucket's grads views again if something replaced them (copy them in)."""
        self._alloc(b)
        for j, p in enumerate(b["params"]):
            v = self._view(b, j)
            g = p.grad
            if g is not None and g.data_ptr() == v.data_ptr() and g.dtype == v.dtype:
                continue
            if g is None:
                v.zero_()
            else:
                v.copy_(g)
            p.grad = v

    def _prepare_arm(self):
        for b in self.buckets:
            self._adopt_grads(b)

    @torch.no_grad()
    def _launch(self, bi):
        b = self.buckets[bi]
        buf = b["flat"]
        if b["stage"] is not None:
            b["stage"].copy_(buf)  # bf16 -> f32
            buf = b["stage"]
        self._works.append(dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group,
                                           async_op=True))
        self._launched = bi + 1

    @torch.no_grad()
    def __call__(self):
        world = self._world()
        if not self._collectives_on():
            self._armed = False
            return
        if not self._armed:
            for b in self.buckets:
                self._adopt_grads(b)
            self._launched = 0
            self._works = []
        while self._launched < len(self.buckets):
            self._launch(self._launched)
        for w in self._works:
            w.wait()
        for b in self.buckets:
            if b["stage"] is not None:
                b["stage"].div_(world)
                b["flat"].copy_(b["stage"])  # f32 -> bf16, one rounding
            else:
                b["flat"].div_(world)
        self._armed = False
        self._works = []


def train_one_epoch(model, dataloader, optimizer, scheduler, patchifier, device, config,
                    prompt_embeds, prompt_attention_mask, epoch, global_step, reducer=None,
                    log_fn=None, lr_schedule=None, max_consecutive_skips=None):
    """training.py:169-231: micro-steps with gradient accumulation, the optimizer step every
    `gradient_accumulation_steps` batches (after the DP gradient all-reduce when `reducer` is
    given), per-step logging of loss / rel_mse / nrmse / lr through `log_fn` (wandb.log in the
    reference). Returns (global_step, mean epoch loss). The loss values stay on the device until
    an optimizer step logs them (one host sync per optimizer step, as the reference's .item()).

    `lr_schedule` (an LRSchedule): every optimizer step runs at lr_schedule.at(global_step), the
    steps taken before it, and "train/lr" is the rate that step used. An optimizer that clips
    (FusedAdamW(max_grad_norm)) adds "train/grad_norm", the pre-clip global norm of the step's
    gradients -- under data parallelism the averaged ones, the same on every rank -- read at the
    same sync point as the loss. An optimizer that averages (FusedAdamW(ema)) adds "train/ema_decay",
    the decay that step's shadow update used. FusedProdigy adds "train/prodigy_d", its step-size
    estimate after the step, read from the device record there too.

    An optimizer that guards (FusedAdamW(skip_nonfinite=True)) adds "train/step_applied" (1, or 0 for a step
    skipped for non-finite gradients), "train/skipped_steps" (the running count) and "train/grad_norm" also
    without clipping, all read at that sync point. global_step and the schedule count attempts, skipped
    ones included. `max_consecutive_skips` (None or 0: no limit): FloatingPointError naming the step once
    more steps than that were skipped in a row -- the outcome of a step is known to the host at the log
    point when there is a log_fn, otherwise when the next step (or the end of the epoch) settles it.

    An optimizer that bounds the adapters (FusedAdamW(scale_weight_norms)) adds "train/keys_scaled",
    "train/avg_key_norm" and "train/max_key_norm", the step's max-norm record, read at that sync point too."""
    model.train()
    accum = max(1, int(config.gradient_accumulation_steps))
    guarded = hasattr(optimizer, "_skip_nonfinite") and optimizer._skip_nonfinite()

    def check_skips():
        # the newest settled step is global_step, or the one before while this step's outcome is in flight
        if max_consecutive_skips and optimizer.consecutive_skips > max_consecutive_skips:
            at = global_step - (1 if optimizer.outcome_pending else 0)
            raise FloatingPointError(f"optimizer step {at}: {optimizer.consecutive_skips} steps in a row skipped "
                                     f"for non-finite gradients (max_consecutive_skips = {max_consecutive_skips})")

    def zero():
        if reducer is not None:
            reducer.zero_grad()  # grads stay views of the reducer's buckets
        else:
            optimizer.zero_grad(set_to_none=True)
    zero()
    losses = []
    for batch_idx, batch in enumerate(dataloader):
        last = (batch_idx + 1) % accum == 0
        if last and reducer is not None:
            reducer.arm()  # the all-reduce overlaps this micro-step's backward
        loss, rel_mse, nrmse, loss_dict = train_step(model, batch, scheduler, patchifier, config,
                                                     prompt_embeds, prompt_attention_mask, device)
        losses.append(loss.detach().float())
        if last:
            if reducer is not None:
                reducer()
            if lr_schedule is not None:
                lr = lr_schedule.at(global_step)
                for group in optimizer.param_groups:
                    group["lr"] = lr
            optimizer.step()
            zero()
            global_step += 1
            if log_fn is not None:
                payload = {"train/loss": float(loss), "train/rel_mse": float(rel_mse),
                           "train/nrmse": float(nrmse), "train/epoch": epoch,
                           "train/lr": optimizer.param_groups[0]["lr"]}
                if getattr(optimizer, "grad_norm", None) is not None:
                    payload["train/grad_norm"] = float(optimizer.grad_norm)
                if guarded and optimizer.step_applied is not None:
                    payload["train/step_applied"] = int(optimizer.step_applied)
                    payload["train/skipped_steps"] = optimizer.skipped_steps  # settles: the device is past it
                if isinstance(optimizer, FusedProdigy):
                    payload["train/prodigy_d"] = float(optimizer.d)  # the device record, at the same sync point
                if getattr(optimizer, "ema", None) is not None:
                    payload["train/ema_decay"] = optimizer.ema_decay  # a host value: no sync
                if getattr(optimizer, "keys_scaled", None) is not None:  # the max-norm pass's record
                    payload["train/keys_scaled"] = int(optimizer.keys_scaled)
                    payload["train/avg_key_norm"] = float(optimizer.avg_key_norm)
                    payload["train/max_key_norm"] = float(optimizer.max_key_norm)
                for k, v in (loss_dict or {}).items():
                    if not k.startswith("_"):
                        payload[f"train/{k}"] = float(v)
                log_fn(payload, global_step)
            if guarded:
                check_skips()
    epoch_loss = float(torch.stack(losses).mean()) if losses else 0.0
    if guarded:
        optimizer.settle()  # behind the loss's sync: the last step's outcome is there
        check_skips()
    return global_step, epoch_loss


def train_loop(model, config, dataloader, prompt_embeds, prompt_attention_mask, device=None,
               log_fn=None, rank=0, val_dataloader=None, resume_from=None):
    """training.py:234-401 for precomputed prompt embeddings (the T5 encode of main() is out of
    scope): trainable set per config.train_mode, FusedAdamW(lr), per-epoch checkpoints every
    `save_every_n_epochs` (best_ prefix on a new best epoch loss) through
    io.save_training_checkpoint, DP gradient averaging when torch.distributed is initialised.

    `val_dataloader`: validation.validate_epoch after every epoch (training.py:341-353), logged as
    {"val/loss", "val/epoch"} at the current global_step. `config.save_adapters` (a bool, absent =
    False; setattr or train.save_adapters in the YAML, not a TrainConfig field): in lora_audio mode,
    wherever the merged checkpoint is written, io.save_adapter_checkpoint also writes
    <output_dir>/adapter_epoch_{E}/ (adapters, optimizer moments, RNG states), after that epoch's
    validation pass. `resume_from` (or config.resume_from / train.resume_from): such a directory, or
    "auto" for the highest complete adapter_epoch_* of output_dir (none: start from scratch); the
    run continues at epoch E + 1, bitwise as the uninterrupted run would. Resume is per epoch.

    The optimizer step's optional keys (schedule_from_config; absent = today's step, call for call):
    `max_grad_norm` clips the global gradient norm inside FusedAdamW and logs "train/grad_norm";
    `lr_scheduler` / `lr_warmup_steps` / `lr_total_steps` set every step's lr from global_step
    (LRSchedule), so a resumed run continues the schedule with no saved state of its own.

    `ema_decay` (ema_from_config; absent or 0 = today's run, call for call and file for file; with
    `ema_warmup`, `ema_inv_gamma`, `ema_power`, `ema_update_after_step`, `ema_min_decay`): FusedAdamW
    keeps an f32 exponential moving average of the trained weights inside its step and
    "train/ema_decay" is logged per step. With a val_dataloader a second validation pass runs under
    the averaged weights (optimizer.ema_weights()), logged as {"val/loss_ema", "val/epoch"}, after the
    normal one and before the adapter checkpoint is written. With save_adapters the directory gains
    ema_model.safetensors and an "ema" block in train_state.json, which a resumed run with the same
    schedule restores (bitwise the uninterrupted run, shadows included). The merged per-epoch
    checkpoints stay the raw weights'. The shadow update runs after the gradient all-reduce, inside
    step(), and needs no collective: every rank's shadows are identical by construction (run at world
    size 1 only, like the rest of data parallelism here).

    The optimizer itself comes from optimizer_from_config (absent keys = FusedAdamW(lr) with today's
    defaults, call for call): `optimizer: prodigy` builds FusedProdigy, which estimates its own step
    size on the device (`learning_rate` 1.0, also when null; the schedule multiplies it as it does
    AdamW's rate), logs "train/prodigy_d" per optimizer step, and with save_adapters adds s.<name> /
    p0.<name> to optimizer.safetensors and a "prodigy" block to train_state.json, from which a resumed
    run continues bitwise. `weight_decay`, `adam_beta1`, `adam_beta2`, `adam_eps` reach either optimizer.

    `skip_nonfinite` (guard_from_config; absent or false = today's run, call for call and file for file):
    either optimizer skips, on the device and without a host sync, every step whose gradients are not all
    finite -- parameters, moments, shadows, Prodigy's state and the step counts are then exactly those of a
    run in which that step was never called -- and "train/step_applied" / "train/skipped_steps" (and
    "train/grad_norm" also without clipping) are logged per step; `max_consecutive_skips` ends the run with
    FloatingPointError instead of skipping forever. With save_adapters train_state.json gains a "guard" block
    with the skipped count, from which a resumed run continues bitwise.

    `scale_weight_norms` (max_norm_from_config; absent, null or 0 = today's run, call for call and file for
    file): kohya's max-norm regularisation with that cap. The optimizer gets lora.adapter_pairs(model) and
    scales, inside every step and on the device, the A and B of every adapter whose |s| ||B A||_F exceeds the
    cap; "train/keys_scaled", "train/avg_key_norm" and "train/max_key_norm" are logged per step. The rule is a
    function of the weights, so a checkpoint holds nothing new but the value in the optimizer's param_groups,
    and a resumed run continues bitwise.

    `loss_face_weight`, `loss_face_pad`, `loss_frame0_weight`, `loss_timestep_weighting`
    (loss_weights_from_config, read by every train_step; absent or at their defaults = today's run, launch
    for launch): the velocity loss weighted by the clip's face box (the batches' "face_bbox", which a
    LatentPairDataset built with face_bbox_dir carries), the first latent frame and the timestep.
    "train/transformer_wmse" is then logged beside "train/transformer_mse", which stays the unweighted mse,
    as does "val/loss".

    `loss_type`, `huber_c`, `huber_schedule` (robust_loss_from_config, read by every train_step; absent or
    "l2" = today's run, launch for launch): the pseudo-Huber velocity loss with a threshold per sample from
    its timestep, with or without the weights above. "train/transformer_robust" is then logged beside
    "train/transformer_mse", which stays the unweighted squared error, as does "val/loss". Nothing about
    the loss enters a checkpoint: it is a function of the config alone."""
    import os

    from . import io
    from .scheduler import RectifiedFlowScheduler
    train_mode = getattr(config, "train_mode", "full")
    save_adapters = bool(getattr(config, "save_adapters", False))
    if resume_from is None:
        resume_from = getattr(config, "resume_from", None)
    if train_mode != "lora_audio" and (save_adapters or resume_from):
        raise NotImplementedError(f"save_adapters / resume_from with train_mode={train_mode!r}: adapter "
                                  f"checkpoints exist in lora_audio mode only (a full-mode checkpoint is the "
                                  f"whole model already, and its sharded optimizer state is not saved)")
    # the optional optimizer-step keys, validated before anything is built
    max_grad_norm, lr_schedule = schedule_from_config(config, dataloader)
    ema = ema_from_config(config)
    skip_nonfinite, max_consecutive_skips = guard_from_config(config)
    scale_weight_norms = max_norm_from_config(config)
    spec = optimizer_from_config(config)
    if spec.kind == "prodigy" and lr_schedule is not None:
        lr_schedule.base_lr = spec.lr  # learning_rate: null means 1.0 there
    device = device or model.device
    patchifier = model.patchifier or SymmetricPatchifier(1)
    if getattr(config, "gradient_checkpointing", False):
        model.gradient_checkpointing = True
    rf = RectifiedFlowScheduler(num_train_timesteps=config.rf_num_train_timesteps,
                                shifting=config.rf_shifting,
                                base_resolution=config.rf_base_resolution,
                                target_shift_terminal=config.rf_target_shift_terminal,
                                sampler=config.rf_sampler, shift=config.rf_shift)
    params = [p for p in model.parameters() if p.requires_grad]
    guard_kw = dict(skip_nonfinite=True) if skip_nonfinite else {}  # absent: today's call
    if scale_weight_norms is not None:
        from .lora import adapter_pairs
        guard_kw.update(scale_weight_norms=scale_weight_norms, norm_pairs=adapter_pairs(model))
    optimizer = spec.build(params, max_grad_norm=max_grad_norm, ema=ema, **guard_kw)
    reducer = None
    if dist.is_available() and dist.is_initialized():
        order = model.grad_ready_order() if hasattr(model, "grad_ready_order") else None
        reducer = GradAllReduce(params, order=order).install(model)
    best = float("inf")
    global_step = 0
    first_epoch = 0
    if resume_from == "auto":
        resume_from = io.latest_adapter_checkpoint(config.output_dir)
    if resume_from:
        # after the optimizer and the reducer exist: values land in place, their pointers stay valid
        st = io.load_adapter_checkpoint(model, resume_from, optimizer=optimizer, loader=dataloader)
        global_step, best, first_epoch = st["global_step"], st["best_loss"], st["epoch"]
    for epoch in range(first_epoch, config.num_epochs or 0):
        if hasattr(dataloader, "set_epoch"):
            dataloader.set_epoch(epoch)
        global_step, epoch_loss = train_one_epoch(model, dataloader, optimizer, rf, patchifier,
                                                  device, config, prompt_embeds,
                                                  prompt_attention_mask, epoch, global_step,
                                                  reducer, log_fn, lr_schedule,
                                                  **(dict(max_consecutive_skips=max_consecutive_skips)
                                                     if skip_nonfinite else {}))
        if val_dataloader is not None:
            from .validation import validate_epoch
            val_loss = validate_epoch(model, val_dataloader, rf, patchifier, config, prompt_embeds,
                                      prompt_attention_mask, device)
            if log_fn is not None:
                log_fn({"val/loss": val_loss, "val/epoch": epoch}, global_step)
            if ema is not None:
                with optimizer.ema_weights():
                    val_loss = validate_epoch(model, val_dataloader, rf, patchifier, config, prompt_embeds,
                                              prompt_attention_mask, device)
                if log_fn is not None:
                    log_fn({"val/loss_ema": val_loss, "val/epoch": epoch}, global_step)
        if log_fn is not None:
            log_fn({"train/epoch_loss": epoch_loss}, global_step)
        saving = config.output_dir and (epoch + 1) % config.save_every_n_epochs == 0
        if saving and save_adapters:
            # every rank calls (the RNG states are gathered), rank 0 writes; after the validation
            # pass, so the device generator's state is the one the next epoch starts from
            io.save_adapter_checkpoint(
                model, os.path.join(config.output_dir, f"adapter_epoch_{epoch + 1}"), optimizer=optimizer,
                train_state={"epoch": epoch + 1, "global_step": global_step, "best_loss": best},
                loader=dataloader, metadata={"base_model_name_or_path": config.checkpoint_path,
                                             "epoch": str(epoch + 1), "global_step": str(global_step)})
        if saving and rank == 0:
            os.makedirs(config.output_dir, exist_ok=True)
            path = os.path.join(config.output_dir, f"model_epoch_{epoch + 1}.safetensors")
            meta = {"epoch": str(epoch + 1), "global_step": str(global_step),
                    "source": "single_gpu_epoch",
                    "scheduler": {"num_train_timesteps": config.rf_num_train_timesteps,
                                  "shifting": config.rf_shifting,
                                  "base_resolution": config.rf_base_resolution,
                                  "target_shift_terminal": config.rf_target_shift_terminal,
                                  "sampler": config.rf_sampler, "shift": config.rf_shift},
                    "vae": {"timestep_conditioning": True}}
            # the reference never updates best_loss (training.py:315, 395): every finite epoch
            # loss is "best" and the file gets the best_ prefix -- kept for drop-in paths
            io.save_training_checkpoint(model, path, getattr(config, "train_mode", "full"),
                                        metadata=meta, is_best=epoch_loss < best)
    return model
