"""What the robust (pseudo-Huber) velocity loss costs on one MI355X, at config A's shape (B = 8 samples of
7 x 16 x 16 latent tokens, C = 128: out, v and the seed are (8, 1792, 128), 1 835 008 loss elements), written
to profiles/robust_loss_bench.md.

Per call: ltx_robust_loss_fwd_bwd (huber, thresholds per sample given; without and with token weights) beside
the two shipped loss passes, ltx_mse_fwd_bwd and ltx_wmse_fwd_bwd, in one process. Every call of a condition
works on the next of --sets operand pairs (32 pairs of out / v are 235 MB, with the seeds they write past
the 256 MiB Infinity Cache, so no call finds its inputs where the previous one left them). A batch of
--calls calls is enqueued behind a device-side sleep of about 3 ms, so the host is out of the picture, with
one device event on each side; the conditions take turns within a round.

Step: train_step (forward and backward, LTX-2B with the rank-16 attn2 adapters, the benchmark's model and
batch, t and noise drawn per step) without and with loss_type huber (huber_schedule snr, huber_c 0.1),
--pairs interleaved pairs of --steps steps each, host clock around the steps with a device synchronize on
both sides.

    python tools/robust_loss_bench.py [--calls 16] [--rounds 7] [--pairs 5] [--steps 10] [--warmup 3]
                                      [--no-step] [--out profiles/robust_loss_bench.md]

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
ON_KEYS = dict(loss_type="huber", huber_schedule="snr", huber_c=0.1)
NOISE_PCT = 1.5  # box-to-box noise of the step time
LAUNCHES = {"mse_fwd_bwd": 2, "wmse_fwd_bwd": 2, "robust_loss_fwd_bwd (huber)": 2,
            "robust_loss_fwd_bwd (huber, token weights)": 2}


def per_call(a, device):
    from ltx_amd import ops
    from ltx_amd.training import huber_threshold
    N = F * H * W
    g = torch.Generator(device=device).manual_seed(7)
    outs = [torch.randn(B, N, C, generator=g, device=device).bfloat16() for _ in range(a.sets)]
    vs = [torch.randn(B, N, C, generator=g, device=device).bfloat16() for _ in range(a.sets)]
    wt = torch.rand(B, N, generator=g, device=device) + 0.5
    c = huber_threshold(torch.rand(B, generator=g, device=device), "snr", 0.1)
    gs = 1.0 / 16
    conditions = {
        "mse_fwd_bwd": lambda k: ops.mse_fwd_bwd(outs[k], vs[k], grad_scale=gs),
        "wmse_fwd_bwd": lambda k: ops.wmse_fwd_bwd(outs[k], vs[k], wt, gs, True),
        "robust_loss_fwd_bwd (huber)": lambda k: ops.robust_loss_fwd_bwd(outs[k], vs[k], c, 1, grad_scale=gs),
        "robust_loss_fwd_bwd (huber, token weights)":
            lambda k: ops.robust_loss_fwd_bwd(outs[k], vs[k], c, 1, wt=wt, grad_scale=gs),
    }
    assert set(conditions) == set(LAUNCHES)
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
    runs = {"l2": cfg(), "huber": cfg(**ON_KEYS)}
    torch.manual_seed(20251015)

    def run(name, n):
        for p in model.parameters():
            p.grad = None
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(n):
            train_step(model, batch, sched, model.patchifier, runs[name], prompt, mask, device)
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) * 1e3 / n
    for name in runs:
        run(name, a.warmup)
    ms = {name: [] for name in runs}
    for i in range(a.pairs):
        for name in (("l2", "huber") if i % 2 == 0 else ("huber", "l2")):  # who goes first alternates
            ms[name].append(run(name, a.steps))
    return ms


def fmt(xs, digits):
    return " / ".join(f"{x:.{digits}f}" for x in xs)


def report(a, us, ms):
    n = B * F * H * W * C
    rows = B * F * H * W
    lines = [
        "# Huber and smooth-L1 velocity loss: measurements",
        "",
        "One MI355X (gfx950), one process, `python tools/robust_loss_bench.py`"
        f" (--calls {a.calls} --rounds {a.rounds} --sets {a.sets} --pairs {a.pairs} --steps {a.steps}"
        f" --warmup {a.warmup}). Config A's loss shape: out, v and the seed are ({B}, {F * H * W}, {C}), {n}"
        " elements. No number was fixed in advance. Algorithmic traffic of every loss pass here: out, v read and"
        f" the seed written, {6 * n / 1e6:.1f} MB; token weights add {4 * rows / 1e3:.0f} KB, the thresholds"
        f" {4 * B} bytes.",
        "",
        "## Per call",
        "",
        f"A batch of {a.calls} calls behind a 3 ms device-side sleep, one device event on each side, every call"
        f" on the next of {a.sets} operand pairs ({a.sets * 4 * n / 1e6:.0f} MB of inputs, past the 256 MiB"
        " Infinity Cache with the seeds they write); the conditions in turn within a round; µs per call, the"
        " rounds, then the median. The events enclose the gaps between the launches of a batch as well as the"
        " kernels. Each call is two launches: the pass over the elements and the one-workgroup finish.",
        "",
        "| condition | launches per call | µs per call | median | GB/s of the 11.0 MB |",
        "|---|---|---|---|---|",
    ]
    med = {k: statistics.median(v) for k, v in us.items()}
    for name, xs in us.items():
        lines.append(f"| {name} | {LAUNCHES[name]} | {fmt(xs, 2)} | {med[name]:.2f} | {6 * n / med[name] / 1e3:.0f} |")
    base = med["mse_fwd_bwd"]
    rob, robw = med["robust_loss_fwd_bwd (huber)"], med["robust_loss_fwd_bwd (huber, token weights)"]
    lines += [
        "",
        f"ltx_robust_loss_fwd_bwd takes {rob:.2f} µs where ltx_mse_fwd_bwd takes {base:.2f} µs ({rob - base:+.2f} µs),"
        f" and with token weights {robw:.2f} µs where ltx_wmse_fwd_bwd takes {med['wmse_fwd_bwd']:.2f} µs"
        f" ({robw - med['wmse_fwd_bwd']:+.2f} µs). The spread of one condition's rounds is"
        f" {max(max(v) - min(v) for v in us.values()):.2f} µs at the most. At the achievable HBM rate of about"
        f" 6.3 TB/s the 11.0 MB alone would take {6 * n / 6.3e6:.2f} µs.",
    ]
    if ms is not None:
        m_off, m_on = statistics.median(ms["l2"]), statistics.median(ms["huber"])
        pct = (m_on - m_off) / m_off * 100.0
        spread = max((max(v) - min(v)) / statistics.median(v) * 100.0 for v in ms.values())
        verdict = (f"inside the ±{NOISE_PCT} % box-to-box noise of DESIGN §4: no difference is claimed"
                   if abs(pct) <= NOISE_PCT else f"outside the ±{NOISE_PCT} % box-to-box noise of DESIGN §4")
        lines += [
            "",
            "## Step",
            "",
            "train_step, forward and backward, the benchmark's LTX-2B model (rank-16 attn2 adapters) and batch,"
            " t and noise drawn per step, gradients accumulating. `l2`: no key set, the step of the parent"
            " commit, launch for launch. `huber`: loss_type huber, huber_schedule snr, huber_c 0.1."
            f" {a.pairs} interleaved pairs of {a.steps} steps (the order within a pair alternates), host clock with"
            " a device synchronize on both sides; ms per step, the pairs, then the median.",
            "",
            "| loss_type | ms per step | median |",
            "|---|---|---|",
            f"| l2 | {fmt(ms['l2'], 2)} | {m_off:.2f} |",
            f"| huber | {fmt(ms['huber'], 2)} | {m_on:.2f} |",
            "",
            f"huber − l2 = {m_on - m_off:+.3f} ms per step ({pct:+.2f} %), with the runs of one condition spread"
            f" over {spread:.2f} % of their median: {verdict}. The per-call figures above put the device cost of"
            f" the robust loss at {rob - base:+.2f} µs of a step of {m_off:.0f} ms; what the host adds is the three"
            " torch launches of the snr threshold.",
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "robust_loss_bench.md"))
    a = ap.parse_args()
    if a.pairs < 3:
        ap.error("--pairs must be at least 3")
    from ltx_amd import _lib
    device = torch.device("cuda", 0)
    _lib.ensure_device(device)
    torch.cuda.set_device(0)
    us = per_call(a, device)
    ms = None if a.no_step else step_time(a, device)
    doc = report(a, us, ms)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(doc)


if __name__ == "__main__":
    main()
