"""What the Prodigy step costs per optimizer step on one MI355X beside FusedAdamW.step(), at the trainable
set of config A's LoRA run (LTX-2B, 28 layers, D = 2048: attn2 adapters of rank r in f32 plus the bf16
caption projection; only those tensors are allocated, the model itself stays on the meta device).

Eight conditions in one process, each on its own copy of the parameters, the same gradients for all:
{adamw, prodigy} x {plain, clip (max_grad_norm 1.0)} x {no EMA, EMA (EMASchedule(0.9999))}. FusedAdamW is
untouched by the Prodigy work, so its conditions are the parent commit's step. After --warmup steps of
each, every round times --steps steps of each condition in turn (host clock around the steps, a device
synchronize on both sides), --rounds times. --only NAME[,NAME] restricts the conditions (for a kernel
trace of one optimizer).

The gradients are views into one flat buffer per dtype (as under GradAllReduce) and change sign before
every step (one neg_ per flat buffer, two small launches that are part of every condition's step and are
timed alone as the condition `neg`; torch._foreach_neg_ over the 228 tensors is 228 launches here): under a gradient that never changes Prodigy's d
grows geometrically without end, which is the algorithm's answer to such a gradient and leaves inf and NaN
in the buffers after a few hundred steps; with the sign alternating the parameters move back and forth
around their start and d stays finite.

    python tools/prodigy_bench.py [--rank 16] [--steps 50] [--warmup 5] [--rounds 5] [--out FILE.json]

Prints one JSON document (also written to --out), with the bytes each Prodigy launch has to move."""
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
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from grad_clip_bench import trainable_shapes
    from ltx_amd import _lib
    from ltx_amd.training import EMASchedule, FusedAdamW, FusedProdigy
    device = torch.device("cuda", 0)
    _lib.ensure_device(device)
    shapes = trainable_shapes(a.rank, {})
    g = torch.Generator(device=device).manual_seed(1234)

    def tensors(std):
        return [torch.empty(s, dtype=torch.float32, device=device).normal_(0, std, generator=g).to(dt)
                for s, dt in shapes]
    values = tensors(0.02)
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
        for clip in (False, True):
            for ema in (False, True):
                name = kind + ("_clip" if clip else "") + ("_ema" if ema else "")
                conditions[name] = (cls, lr, 1.0 if clip else None, EMASchedule(0.9999) if ema else None)
    if a.only:
        conditions = {k: conditions[k] for k in a.only.split(",")}
    opts, steppers = {}, {"neg": negate}

    def stepper(opt):
        def step():
            negate()
            opt.step()
        return step
    for name, (cls, lr, max_norm, ema) in conditions.items():
        ps = [torch.nn.Parameter(v.clone()) for v in values]
        for p, x in zip(ps, grads):
            p.grad = x  # shared; only the negation above writes it
        opts[name] = cls(ps, lr=lr, max_grad_norm=max_norm, ema=ema)
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
    # bytes per element: pass 1 reads p, g, p0, m, v, s and writes m, v, s; pass 2 reads p, m, v and writes p
    # (with the EMA also reads and writes the f32 shadow)
    traffic = {"pass1_bytes": 9 * (4 * f32 + 2 * bf16), "pass2_bytes": 4 * (4 * f32 + 2 * bf16),
               "pass2_ema_bytes": 4 * (4 * f32 + 2 * bf16) + 8 * (f32 + bf16),
               "adamw_bytes": 7 * (4 * f32 + 2 * bf16)}
    records = {name: dict(zip(opt.RECORD, opt.record.tolist())) for name, opt in opts.items() if hasattr(opt, "RECORD")}
    finite = all(bool(torch.isfinite(p).all()) for opt in opts.values() for p in opt.param_groups[0]["params"])
    res = {"device": torch.cuda.get_device_name(device), "rank": a.rank, "tensors": len(shapes),
           "f32_elements": f32, "bf16_elements": bf16, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "traffic": traffic, "prodigy_records": records, "parameters_finite": finite,
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
