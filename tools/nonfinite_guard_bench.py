"""What the non-finite guard (`skip_nonfinite`: FusedAdamW / FusedProdigy skip, on the device, a step whose
gradients are not all finite) costs per optimizer step on one MI355X beside today's step, and what the host
waits for when it settles the previous step's outcome.

Timing, at the trainable set of config A's LoRA run (LTX-2B, 28 layers, D = 2048: attn2 adapters of rank r in
f32 plus the bf16 caption projection; only those tensors are allocated): eight conditions in one process, each
on its own copy of the parameters, the same finite gradients for all: {adamw, prodigy} x {plain, clip
(max_grad_norm 1.0)} x {off, guard}. The off conditions are the parent commit's step. Two figures per
condition, --rounds rounds of each, the conditions taken in turn within a round:

  back to back   --steps steps in a row, host clock around them with a device synchronize on both sides
                 (ms per step), and the time to enqueue them, before the closing synchronize. A guarded
                 step first waits for the previous step's outcome, so back to back the host runs one step
                 ahead of the device at the most: this is the worst case for the guard, not a training loop;
  device         one step at a time behind a device-side sleep long enough for the host to enqueue the whole
                 step, two events around the step's launches: the launches' time on the device with no host
                 gap between them (us per step, --device-steps of them).

The gradients are views into one flat buffer per dtype and change sign before every step, as in
tools/prodigy_bench.py (where the reason is written down); the two neg_ launches are outside the events and
timed alone back to back as `neg`.

--epoch: training.train_one_epoch on bench.py's model (config A, its synthetic batch), FusedAdamW with
max_grad_norm 1.0 and the guard, --epoch-steps optimizer steps of --accum micro-steps after one warm-up epoch,
with a log_fn (the loss is read after every optimizer step, as a training run does) and without one (nothing
reads anything: the host runs ahead until the guard's event stops it). Reports the wall time per optimizer
step and the host time inside the event wait of settle(), per step.

    python tools/nonfinite_guard_bench.py [--rank 16] [--steps 50] [--warmup 6] [--rounds 5] [--epoch] [--out FILE.json]

Prints one JSON document (also written to --out)."""
import argparse
import importlib.util
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
    from ltx_amd.training import FusedAdamW, FusedProdigy
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
        for variant in ("", "_clip"):
            for guard in ("off", "guard"):
                conditions[f"{kind}{variant}_{guard}"] = (cls, lr, 1.0 if variant else None, guard == "guard")
    if a.only:
        conditions = {k: conditions[k] for k in a.only.split(",")}
    opts = {}
    for name, (cls, lr, max_norm, guard) in conditions.items():
        ps = [torch.nn.Parameter(v.clone()) for v in values]
        for p, x in zip(ps, grads):
            p.grad = x  # shared; only the negation above writes it
        opts[name] = cls(ps, lr=lr, max_grad_norm=max_norm, **(dict(skip_nonfinite=True) if guard else {}))

    def stepper(opt):
        def step():
            negate()
            opt.step()
        return step
    steppers = dict({"neg": negate}, **{name: stepper(opt) for name, opt in opts.items()})

    def back_to_back(step, n):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        t1 = time.perf_counter()
        torch.cuda.synchronize(device)
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3 / n, (t1 - t0) * 1e3 / n

    # a device-side sleep of about 3 ms: calibrated once, in the sleep's own cycles, after its first launch
    cycles = 1_000_000
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(cycles)
    torch.cuda.synchronize(device)
    start.record()
    torch.cuda._sleep(cycles)
    end.record()
    torch.cuda.synchronize(device)
    cycles = int(cycles * 3.0 / max(start.elapsed_time(end), 1e-3))

    def on_device(opt, n):
        total = 0.0
        for _ in range(n):
            negate()
            torch.cuda.synchronize(device)  # the previous step's outcome is there: settle() does not wait
            torch.cuda._sleep(cycles)
            start.record()
            opt.step()
            end.record()
            torch.cuda.synchronize(device)
            total += start.elapsed_time(end)
        return total * 1e3 / n
    assert a.steps % 2 == 0 and a.device_steps % 2 == 0, "step counts must be even (the gradients' sign alternates)"
    for step in steppers.values():
        back_to_back(step, a.warmup + a.warmup % 2)  # an even count: every condition starts from +g
    ms = {name: [] for name in steppers}
    enqueue = {name: [] for name in steppers}
    device_us = {name: [] for name in opts}
    for _ in range(a.rounds):
        for name, step in steppers.items():
            total, host = back_to_back(step, a.steps)
            ms[name].append(total)
            enqueue[name].append(host)
        for name, opt in opts.items():
            device_us[name].append(on_device(opt, a.device_steps))
    f32 = sum(torch.Size(s).numel() for s, dt in shapes if dt == torch.float32)
    bf16 = sum(torch.Size(s).numel() for s, dt in shapes if dt == torch.bfloat16)
    finite = all(bool(torch.isfinite(p).all()) for opt in opts.values() for p in opt.param_groups[0]["params"])
    skipped = {name: opt.skipped_steps for name, opt in opts.items() if name.endswith("_guard")}
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return {"rank": a.rank, "tensors": len(shapes), "f32_elements": f32, "bf16_elements": bf16,
            "gradient_bytes": 4 * f32 + 2 * bf16, "steps": a.steps, "device_steps": a.device_steps, "warmup": a.warmup,
            "rounds": a.rounds, "sleep_cycles": cycles, "parameters_finite": finite, "skipped_steps": skipped,
            "ms_per_step": ms, "host_enqueue_ms_per_step": enqueue, "device_us_per_step": device_us,
            "median_ms_per_step": {k: med(v) for k, v in ms.items()},
            "median_device_us_per_step": {k: med(v) for k, v in device_us.items()}}


def epoch(a, device):
    """train_one_epoch on bench.py's model; the host time inside settle()'s event wait, per optimizer step."""
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from ltx_amd.config import TrainConfig
    from ltx_amd.scheduler import RectifiedFlowScheduler
    from ltx_amd.training import FusedAdamW, GradAllReduce, train_one_epoch
    model = bench.build_model(device)
    batch, prompt, mask = bench.synthetic_batch(device, 0)
    cfg = TrainConfig(checkpoint_path="-", batch_size=bench.B_PER_GPU, learning_rate=1e-4, lora_rank=bench.LORA_RANK,
                      lora_alpha=bench.LORA_RANK, gradient_accumulation_steps=a.accum, rf_log_normal_mu=-0.5,
                      rf_log_normal_sigma=1.0)
    sched = RectifiedFlowScheduler(num_train_timesteps=1000, shifting=None)
    waits = []

    class Timed(FusedAdamW):
        def settle(self):
            pending = self._guard_pending is not None
            t0 = time.perf_counter()
            super().settle()
            if pending:
                waits.append((time.perf_counter() - t0) * 1e6)
    opt = Timed([p for p in model.parameters() if p.requires_grad], lr=cfg.learning_rate, max_grad_norm=1.0,
                skip_nonfinite=True)
    # as bench.py: the gradients live in the reducer's buckets and zero_grad keeps them there, so the chunk
    # tables are built once (world size 1: no collective runs)
    reducer = GradAllReduce(opt.param_groups[0]["params"], order=model.grad_ready_order()).install(model)
    loader = [batch] * (a.accum * a.epoch_steps)
    torch.manual_seed(20251015)
    out, step = {}, 0
    for label, log_fn in (("warmup", None), ("with_log_fn", lambda payload, s: None), ("without_log_fn", None)):
        del waits[:]
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        step, _ = train_one_epoch(model, loader, opt, sched, model.patchifier, device, cfg, prompt, mask, 0, step,
                                  reducer=reducer, log_fn=log_fn)
        torch.cuda.synchronize(device)
        wall = (time.perf_counter() - t0) * 1e3 / a.epoch_steps
        if label != "warmup":
            out[label] = {"wall_ms_per_optimizer_step": wall, "settle_wait_us": list(waits),
                          "median_settle_wait_us": sorted(waits)[len(waits) // 2] if waits else None}
    out.update(optimizer_steps=a.epoch_steps, accum=a.accum, skipped_steps=opt.skipped_steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--device-steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--epoch", action="store_true")
    ap.add_argument("--epoch-steps", type=int, default=4)
    ap.add_argument("--accum", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ltx_amd import _lib
    device = torch.device("cuda", 0)
    _lib.ensure_device(device)
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(device)}
    if not a.no_timing:
        res.update(timing(a, device))
    if a.epoch:
        res["epoch"] = epoch(a, device)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
