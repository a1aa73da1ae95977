"""What the stochastically rounded bf16 step (bf16_update="stochastic": f32 moments for the bf16 caption
projection, the parameter stored through stochastic rounding) costs per optimizer step on one MI355X beside
today's step ("nearest"), and what it changes in how the weights move.

Timing, at the trainable set of config A's LoRA run (LTX-2B, 28 layers, D = 2048: attn2 adapters of rank r in
f32 plus the bf16 caption projection; only those tensors are allocated): twelve conditions in one process,
each on its own copy of the parameters, the same gradients for all: {adamw, prodigy} x {plain, clip
(max_grad_norm 1.0), EMA (EMASchedule(0.9999))} x {nearest, stochastic}. The nearest conditions are the
parent commit's step; a stochastic row compares with the nearest row of the same run only. After --warmup
steps of each, every round times --steps steps of each condition in turn (host clock around the steps, a
device synchronize on both sides), --rounds times. --only NAME[,NAME] restricts the conditions (for a kernel
trace). The gradients are views into one flat buffer per dtype and change sign before every step, as in
tools/prodigy_bench.py (where the reason is written down); the two neg_ launches are timed alone as `neg`.

Behaviour (--behaviour, the tiny golden model of smoke(), one fixed batch): the share of caption-projection
elements whose bits differ from the start after 20 AdamW steps at lr 1e-4, and the Prodigy step at which d
first leaves d0 (default d0, up to --prodigy-steps steps), in both modes. Records, not thresholds.

    python tools/bf16_sr_bench.py [--rank 16] [--steps 50] [--warmup 5] [--rounds 5] [--behaviour] [--out FILE.json]

Prints one JSON document (also written to --out), with the bytes each bf16 launch has to move."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "video-generation-for-human-avatars_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402


def timing(a, device):
    from grad_clip_bench import trainable_shapes
    from ltx_amd.training import EMASchedule, FusedAdamW, FusedProdigy
    shapes = trainable_shapes(a.rank, {})
    g = torch.Generator(device=device).manual_seed(1234)
    values = [torch.empty(s, dtype=torch.float32, device=device).normal_(0, 0.02, generator=g).to(dt)
              for s, dt in shapes]
    flat = {dt: torch.empty(sum(torch.Size(s).numel() for s, d in shapes if d == dt), dtype=torch.float32,
                            device=device).normal_(0, 1e-3, generator=g).to(dt) for dt in (torch.float32, torch.bfloat16)}
    grads, used = [], {dt: 0 for dt in flat}
    for s, dt in shapes:
        n = torch.Size(s).numel()
        grads.append(flat[dt].narrow(0, used[dt], n).view(s))
        used[dt] += n

    def negate():
        for buf in flat.values():
            buf.neg_()
    conditions = {}
    for kind, cls, lr in (("adamw", FusedAdamW, 1e-4), ("prodigy", FusedProdigy, 1.0)):
        for variant in ("", "_clip", "_ema"):
            for mode in ("nearest", "stochastic"):
                conditions[f"{kind}{variant}_{mode}"] = (cls, lr, 1.0 if variant == "_clip" else None,
                                                         EMASchedule(0.9999) if variant == "_ema" else None, mode)
    if a.only:
        conditions = {k: conditions[k] for k in a.only.split(",")}
    opts, steppers = {}, {"neg": negate}

    def stepper(opt):
        def step():
            negate()
            opt.step()
        return step
    for name, (cls, lr, max_norm, ema, mode) in conditions.items():
        ps = [torch.nn.Parameter(v.clone()) for v in values]
        for p, x in zip(ps, grads):
            p.grad = x  # shared; only the negation above writes it
        opts[name] = cls(ps, lr=lr, max_grad_norm=max_norm, ema=ema, bf16_update=mode, sr_seed=1)
        steppers[name] = stepper(opts[name])

    def run(step, n):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        t1 = time.perf_counter()
        torch.cuda.synchronize(device)
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3 / n, (t1 - t0) * 1e3 / n
    for step in steppers.values():
        run(step, a.warmup + a.warmup % 2)  # an even count: every condition starts from +g
    ms = {name: [] for name in steppers}
    enqueue = {name: [] for name in steppers}
    assert a.steps % 2 == 0, "--steps must be even (the gradients' sign alternates)"
    for _ in range(a.rounds):
        for name, step in steppers.items():
            total, host = run(step, a.steps)
            ms[name].append(total)
            enqueue[name].append(host)
    f32 = sum(torch.Size(s).numel() for s, dt in shapes if dt == torch.float32)
    bf16 = sum(torch.Size(s).numel() for s, dt in shapes if dt == torch.bfloat16)
    # bytes per bf16 element. AdamW: p, g, m, v in and p, m, v out; nearest 6 x 2, mixed 2 + 2 + 4 + 4 in and
    # 2 + 4 + 4 out (+ 8 with the f32 shadow either way). Prodigy pass 1: p, g, p0, m, v, s in and m, v, s out;
    # pass 2: p, m, v in and p out.
    traffic = {"adamw_nearest": 12 * bf16, "adamw_stochastic": 22 * bf16, "adamw_ema_nearest": 20 * bf16,
               "adamw_ema_stochastic": 30 * bf16, "prodigy_pass1_nearest": 18 * bf16,
               "prodigy_pass1_stochastic": 30 * bf16, "prodigy_pass2_nearest": 8 * bf16,
               "prodigy_pass2_stochastic": 12 * bf16, "prodigy_pass2_ema_nearest": 16 * bf16,
               "prodigy_pass2_ema_stochastic": 20 * bf16}
    finite = all(bool(torch.isfinite(p).all()) for opt in opts.values() for p in opt.param_groups[0]["params"])
    return {"rank": a.rank, "tensors": len(shapes), "f32_elements": f32, "bf16_elements": bf16, "steps": a.steps,
            "warmup": a.warmup, "rounds": a.rounds, "bf16_traffic_bytes": traffic, "parameters_finite": finite,
            "ms_per_step": ms, "host_enqueue_ms_per_step": enqueue,
            "median_ms_per_step": {k: sorted(v)[len(v) // 2] for k, v in ms.items()}}


def behaviour(a, device):
    """The tiny golden model under one fixed batch, t and noise (smoke()'s inputs)."""
    from safetensors.torch import load_file
    for p in (os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from ltx_amd.config import TrainConfig
    from ltx_amd.scheduler import RectifiedFlowScheduler
    from ltx_amd.training import FusedAdamW, FusedProdigy, train_step
    from model_utils import build_model
    gold = os.path.join(REPO, "tests", "golden")
    d = load_file(os.path.join(gold, "tiny_train_step.safetensors"))
    with open(os.path.join(gold, "tiny_train_step.json")) as f:
        meta = json.load(f)
    params = {k[2:]: v for k, v in d.items() if k.startswith("w.")}
    dev = str(device)
    batch = {k: d["in." + k].to(dev) for k in ("latents", "ref_image_latents", "pose_latents")}

    def run(cls, steps, **kw):
        model = build_model(meta["config"], params, meta["lora_rank"], device=dev)
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        cap = [p for n, p in named if "caption_projection" in n and p.dtype == torch.bfloat16]
        start = [p.detach().clone() for p in cap]
        opt = cls([p for _, p in named], **kw)
        left = None
        for k in range(steps):
            opt.zero_grad(set_to_none=True)
            train_step(model, batch, RectifiedFlowScheduler(), model.patchifier, TrainConfig(checkpoint_path="-"),
                       d["in.prompt_embeds"].to(dev), d["in.prompt_attention_mask"].to(dev), t=d["out.t"].to(dev),
                       noise=d["out.noise"].to(dev))
            opt.step()
            if left is None and hasattr(opt, "RECORD") and float(opt.d) != kw.get("d0", 1e-6):
                left = k + 1
        changed = sum(int((p.detach().view(torch.int16) != s.view(torch.int16)).sum()) for p, s in zip(cap, start))
        return {"caption_projection_elements": sum(p.numel() for p in cap), "changed": changed,
                "share_changed": changed / max(1, sum(p.numel() for p in cap)),
                "prodigy_d_left_d0_at_step": left, "prodigy_d": float(opt.d) if hasattr(opt, "RECORD") else None}
    out = {}
    for mode in ("nearest", "stochastic"):
        out[f"adamw_lr1e-4_20_steps_{mode}"] = run(FusedAdamW, 20, lr=1e-4, bf16_update=mode, sr_seed=1)
        out[f"prodigy_{a.prodigy_steps}_steps_{mode}"] = run(FusedProdigy, a.prodigy_steps, bf16_update=mode, sr_seed=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--behaviour", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--prodigy-steps", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ltx_amd import _lib
    device = torch.device("cuda", 0)
    _lib.ensure_device(device)
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(device)}
    if not a.no_timing:
        res.update(timing(a, device))
    if a.behaviour:
        res["behaviour"] = behaviour(a, device)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
