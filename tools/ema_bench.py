"""What the EMA of the trained weights costs per optimizer step on one MI355X, at the trainable set of
config A's LoRA run (LTX-2B, 28 layers, D = 2048: attn2 adapters of rank r in f32 plus the bf16 caption
projection; only those tensors are allocated, the model itself stays on the meta device).

Three conditions in one process, each on its own copy of the parameters, the same gradients for all:
  off       FusedAdamW(ema=None): ltx_adamw_multi per dtype, the step as it is without the feature;
  fused     FusedAdamW(ema=EMASchedule(0.9999)): ltx_adamw_multi_ema per dtype, the shadow update inside;
  foreach   the `off` step followed by the same update of f32 shadows as torch._foreach_ ops (diffusers'
            EMAModel.step: sub, mul, sub_; the bf16 tensors are first cast to f32), the yardstick for what
            fusing buys.
After --warmup steps of each, every round times --steps steps of each condition in turn (host clock around
the steps, a device synchronize on both sides), --rounds times.

    python tools/ema_bench.py [--rank 32] [--steps 50] [--warmup 5] [--rounds 5] [--out FILE.json]

Prints one JSON document (also written to --out)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "video-generation-for-human-avatars_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from grad_clip_bench import trainable_shapes
    from ltx_amd import _lib
    from ltx_amd.training import EMASchedule, FusedAdamW
    device = torch.device("cuda", 0)
    _lib.ensure_device(device)
    shapes = trainable_shapes(a.rank, {})
    g = torch.Generator(device=device).manual_seed(1234)

    def tensors(std):
        return [torch.empty(s, dtype=torch.float32, device=device).normal_(0, std, generator=g).to(dt)
                for s, dt in shapes]
    values, grads = tensors(0.02), tensors(1e-3)
    sched = EMASchedule(0.9999)
    opts, params = {}, {}
    for name, ema in (("off", None), ("fused", sched), ("foreach", None)):
        ps = [torch.nn.Parameter(v.clone()) for v in values]
        for p, x in zip(ps, grads):
            p.grad = x  # shared, read-only
        opts[name], params[name] = FusedAdamW(ps, lr=1e-4, ema=ema), ps
    shadows = [p.detach().float().clone() for p in params["foreach"]]
    counter = [0]

    def foreach_step():
        opts["foreach"].step()
        counter[0] += 1
        omd = 1.0 - sched.decay_at(counter[0])
        pf = [p.detach() if p.dtype == torch.float32 else p.detach().float() for p in params["foreach"]]
        tmp = torch._foreach_sub(shadows, pf)
        torch._foreach_mul_(tmp, omd)
        torch._foreach_sub_(shadows, tmp)
    steppers = {"off": opts["off"].step, "fused": opts["fused"].step, "foreach": foreach_step}

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
        run(step, a.warmup)
    ms = {name: [] for name in steppers}
    enqueue = {name: [] for name in steppers}
    for _ in range(a.rounds):
        for name, step in steppers.items():
            total, host = run(step, a.steps)
            ms[name].append(total)
            enqueue[name].append(host)
    # the three conditions ran the same number of steps on the same gradients: the same weights, and the
    # fused shadows are the foreach ones (the same three f32 operations)
    same_params = all(torch.equal(x, y) and torch.equal(x, z)
                      for x, y, z in zip(params["off"], params["fused"], params["foreach"]))
    same_shadows = all(torch.equal(opts["fused"].state[p]["ema"], s) for p, s in zip(params["fused"], shadows))
    f32 = sum(torch.Size(s).numel() for s, dt in shapes if dt == torch.float32)
    bf16 = sum(torch.Size(s).numel() for s, dt in shapes if dt == torch.bfloat16)
    res = {"device": torch.cuda.get_device_name(device), "rank": a.rank, "tensors": len(shapes),
           "f32_elements": f32, "bf16_elements": bf16, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "params_bitwise_equal": same_params, "fused_shadows_equal_foreach": same_shadows,
           "ms_per_step": ms, "host_enqueue_ms_per_step": enqueue,
           "median_ms_per_step": {k: sorted(v)[len(v) // 2] for k, v in ms.items()}}
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
