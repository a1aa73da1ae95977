"""What the weighted velocity loss costs on one MI355X, at config A's shape (B = 8 samples of 7 x 16 x 16
latent tokens, C = 128: 14 336 tokens, 1 835 008 loss elements), written to profiles/loss_weight_bench.md.

Per call: ltx_mse_fwd_bwd (the unweighted loss pass, what the step launches today) beside the two launches
that take its place when a weight is configured -- ltx_loss_token_weights (face box, first-frame weight and
a per-sample factor given) and ltx_wmse_fwd_bwd -- and each of the two alone. Every call of a condition
works on the next of --sets operand pairs (32 pairs of out / v are 235 MB, with the seeds they write past
the 256 MiB Infinity Cache, so no call finds its inputs where the previous one left them). A batch of
--calls calls is enqueued behind a device-side sleep of about 3 ms, so the host is out of the picture, with
one device event on each side; the conditions take turns within a round.

Step: train_step (forward and backward, LTX-2B with the rank-16 attn2 adapters, the benchmark's model and
batch, t and noise drawn per step) with the weights off and on (loss_face_weight 4, loss_frame0_weight
0.25, cosmap, a face box per sample), --pairs interleaved pairs of --steps steps each, host clock around
the steps with a device synchronize on both sides.

    python tools/loss_weight_bench.py [--calls 16] [--rounds 7] [--pairs 5] [--steps 10] [--warmup 3]
                                      [--no-step] [--out profiles/loss_weight_bench.md]

Needs the GPU; nothing here falls back to the CPU."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "video-generation-for-human-avatars_amd"))

import torch  # noqa: E402

B, F, H, W, C = 8, 7, 16, 16, 128
ON_KEYS = dict(loss_face_weight=4.0, loss_frame0_weight=0.25, loss_timestep_weighting="cosmap")
NOISE_PCT = 1.5  # box-to-box noise of the step time


def face_boxes(device):
    i = torch.arange(B, dtype=torch.float32)
    x0, y0 = 0.21 + 0.03 * i, 0.13 + 0.02 * i
    return torch.stack([x0, y0, x0 + 0.37, y0 + 0.45], dim=1).to(device)


def per_call(a, device):
    from ltx_amd import ops
    N = F * H * W
    g = torch.Generator(device=device).manual_seed(7)
    outs = [torch.randn(B, N, C, generator=g, device=device).bfloat16() for _ in range(a.sets)]
    vs = [torch.randn(B, N, C, generator=g, device=device).bfloat16() for _ in range(a.sets)]
    bbox = face_boxes(device)
    frame_w = torch.ones(F, device=device)
    frame_w[0] = 0.25
    sample_w = torch.rand(B, generator=g, device=device) + 0.5
    wt0, _ = ops.loss_token_weights(B, F, H, W, device, bbox=bbox, frame_w=frame_w, sample_w=sample_w, face_weight=4.0)
    gs = 1.0 / 16

    def weights(k):
        return ops.loss_token_weights(B, F, H, W, device, bbox=bbox, frame_w=frame_w, sample_w=sample_w,
                                      face_weight=4.0)[0]
    conditions = {
        "mse_fwd_bwd": lambda k: ops.mse_fwd_bwd(outs[k], vs[k], grad_scale=gs),
        "token_weights + wmse_fwd_bwd": lambda k: ops.wmse_fwd_bwd(outs[k], vs[k], weights(k), gs, True),
        "wmse_fwd_bwd alone": lambda k: ops.wmse_fwd_bwd(outs[k], vs[k], wt0, gs, True),
        "token_weights alone": weights,
    }
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 1_000_000  # a device-side sleep of about 3 ms, calibrated in its own cycles after a first launch
    torch.cuda._sleep(cycles)
    torch.cuda.synchronize(device)
    start.record()
    torch.cuda._sleep(cycles)
    end.record()
    torch.cuda.synchronize(device)
    cycles = int(cycles * 3.0 / max(start.elapsed_time(end), 1e-3))
    nxt = {name: 0 for name in conditions}

    def batch(name, fn):
        torch.cuda.synchronize(device)
        torch.cuda._sleep(cycles)
        start.record()
        for _ in range(a.calls):
            fn(nxt[name] % a.sets)
            nxt[name] += 1
        end.record()
        torch.cuda.synchronize(device)
        return start.elapsed_time(end) * 1e3 / a.calls
    for name, fn in conditions.items():
        for _ in range(2):
            batch(name, fn)
    us = {name: [] for name in conditions}
    for _ in range(a.rounds):
        for name, fn in conditions.items():
            us[name].append(batch(name, fn))
    return us


def step_time(a, device):
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from ltx_amd.config import TrainConfig
    from ltx_amd.scheduler import RectifiedFlowScheduler
    from ltx_amd.training import train_step
    assert (bench.B_PER_GPU, bench.F_LAT, bench.H_LAT, bench.W_LAT) == (B, F, H, W)
    model = bench.build_model(device)
    batch, prompt, mask = bench.synthetic_batch(device, 0)
    sched = RectifiedFlowScheduler(num_train_timesteps=1000, shifting=None)

    def cfg(**extra):
        tc = TrainConfig(checkpoint_path="-", batch_size=B, learning_rate=1e-4, lora_rank=bench.LORA_RANK,
                         lora_alpha=bench.LORA_RANK, gradient_accumulation_steps=bench.ACCUM, rf_log_normal_mu=-0.5,
                         rf_log_normal_sigma=1.0)
        for k, v in extra.items():
            setattr(tc, k, v)
        return tc
    runs = {"off": (cfg(), batch), "on": (cfg(**ON_KEYS), dict(batch, face_bbox=face_boxes(device)))}
    torch.manual_seed(20251015)

    def run(name, n):
        tc, b = runs[name]
        for p in model.parameters():
            p.grad = None
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(n):
            train_step(model, b, sched, model.patchifier, tc, prompt, mask, device)
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) * 1e3 / n
    for name in runs:
        run(name, a.warmup)
    ms = {name: [] for name in runs}
    for i in range(a.pairs):
        for name in (("off", "on") if i % 2 == 0 else ("on", "off")):  # who goes first alternates
            ms[name].append(run(name, a.steps))
    return ms


def fmt(xs, digits):
    return " / ".join(f"{x:.{digits}f}" for x in xs)


def report(a, device, us, ms):
    n = B * F * H * W * C
    rows = B * F * H * W
    lines = [
        "# Face-box, frame and timestep weights in the fused velocity loss: measurements",
        "",
        "One MI355X (gfx950), one process, `python tools/loss_weight_bench.py`"  # ensure_device admits no other
        f" (--calls {a.calls} --rounds {a.rounds} --sets {a.sets} --pairs {a.pairs} --steps {a.steps}"
        f" --warmup {a.warmup}). Config A's loss shape: B = {B} samples of {F} x {H} x {W} latent tokens, C = {C}:"
        f" {rows} tokens, {n} elements. No number was fixed in advance. Algorithmic traffic of the loss pass:"
        f" out, v read and the seed written, {6 * n / 1e6:.1f} MB; the weights add {4 * rows / 1e3:.0f} KB.",
        "",
        "## Per call",
        "",
        f"A batch of {a.calls} calls behind a 3 ms device-side sleep, one device event on each side, every call"
        f" on the next of {a.sets} operand pairs ({a.sets * 4 * n / 1e6:.0f} MB of inputs, past the 256 MiB"
        " Infinity Cache with the seeds they write); the conditions in turn within a round; µs per call, the"
        " rounds, then the median. The events enclose the gaps between the launches of a batch as well as the"
        " kernels.",
        "",
        "| condition | launches per call | µs per call | median |",
        "|---|---|---|---|",
    ]
    launches = {"mse_fwd_bwd": 2, "token_weights + wmse_fwd_bwd": 3, "wmse_fwd_bwd alone": 2, "token_weights alone": 1}
    med = {k: statistics.median(v) for k, v in us.items()}
    for name, xs in us.items():
        lines.append(f"| {name} | {launches[name]} | {fmt(xs, 2)} | {med[name]:.2f} |")
    base, both = med["mse_fwd_bwd"], med["token_weights + wmse_fwd_bwd"]
    lines += [
        "",
        f"The two new launches together take {both:.2f} µs where ltx_mse_fwd_bwd takes {base:.2f} µs:"
        f" {both - base:+.2f} µs per call. ltx_wmse_fwd_bwd alone is {med['wmse_fwd_bwd alone'] - base:+.2f} µs"
        f" from ltx_mse_fwd_bwd, and the one-workgroup-per-sample weight kernel is {med['token_weights alone']:.2f} µs"
        " of its own. The spread of one condition's rounds is"
        f" {max(max(v) - min(v) for v in us.values()):.2f} µs at the most.",
    ]
    if ms is not None:
        m_off, m_on = statistics.median(ms["off"]), statistics.median(ms["on"])
        pct = (m_on - m_off) / m_off * 100.0
        spread = max((max(v) - min(v)) / statistics.median(v) * 100.0 for v in ms.values())
        verdict = (f"inside the ±{NOISE_PCT} % box-to-box noise of DESIGN §4: no difference is claimed"
                   if abs(pct) <= NOISE_PCT else f"outside the ±{NOISE_PCT} % box-to-box noise of DESIGN §4")
        lines += [
            "",
            "## Step",
            "",
            "train_step, forward and backward, the benchmark's LTX-2B model (rank-16 attn2 adapters) and batch,"
            " t and noise drawn per step, gradients accumulating. `off`: no key set, the step of the parent"
            " commit, launch for launch. `on`: loss_face_weight 4, loss_frame0_weight 0.25,"
            f" loss_timestep_weighting cosmap, a face box per sample. {a.pairs} interleaved pairs of {a.steps} steps"
            " (the order within a pair alternates), host clock with a device synchronize on both sides; ms per"
            " step, the pairs, then the median.",
            "",
            "| weights | ms per step | median |",
            "|---|---|---|",
            f"| off | {fmt(ms['off'], 2)} | {m_off:.2f} |",
            f"| on | {fmt(ms['on'], 2)} | {m_on:.2f} |",
            "",
            f"on − off = {m_on - m_off:+.3f} ms per step ({pct:+.2f} %), with the runs of one condition spread over"
            f" {spread:.2f} % of their median: {verdict}. The per-call figures above put the device cost of the"
            f" weighting at {both - base:+.2f} µs of a step of {m_off:.0f} ms; what the host adds is the weight"
            " kernel's launch and the handful of torch launches of the timestep factor.",
        ]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sets", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loss_weight_bench.md"))
    a = ap.parse_args()
    if a.pairs < 3:
        ap.error("--pairs must be at least 3")
    from ltx_amd import _lib
    device = torch.device("cuda", 0)
    _lib.ensure_device(device)
    torch.cuda.set_device(0)
    us = per_call(a, device)
    ms = None if a.no_step else step_time(a, device)
    doc = report(a, device, us, ms)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(doc)


if __name__ == "__main__":
    main()
