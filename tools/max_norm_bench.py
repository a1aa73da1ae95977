"""What max-norm regularisation (FusedAdamW(scale_weight_norms=c)) costs per optimizer step on one MI355X, at
the trainable set of config A's LoRA run (LTX-2B, 28 layers, D = 2048; f32 adapters plus the bf16 caption
projection; only those tensors are allocated, the model itself stays on the meta device).

Per adapter set -- `attn2` (112 pairs) or `full` (attn1 + attn2 + the feed-forward linears, 280 pairs) at a rank --
four conditions in one process, each on its own copy of the parameters, the same gradients for all:
  off         FusedAdamW without the cap: the step as it is without the feature;
  fused_none  the cap far above every norm: the sums of squares and the finish run, nothing is stored;
  fused_some  the cap at the median of the initial norms: about half of the pairs are stored every step;
  torch_loop  the `off` step followed by the same rule as a loop of torch ops on the device, with its .item()
              per pair (kohya's apply_max_norm_regularization): what a user would write today.
After --warmup steps of each, every round times --steps steps of each condition in turn (host clock around the
steps, a device synchronize on both sides), --rounds times. Then, on the fused_some optimizer: the three entry
points' times from ops.LaunchTimer (HIP events around each launch), the stores' launch alone with every factor
forced under 1 (every row stores), the workspace's size and the host time to build and upload the two tables.

    python tools/max_norm_bench.py [--sets attn2:16,full:16,full:128] [--steps 20] [--warmup 3] [--rounds 5] [--out FILE.json]

Prints one JSON document (also written to --out)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "video-generation-for-human-avatars_amd"))

import torch  # noqa: E402

SETS = {"attn2": {}, "full": {"lora_targets": "attn1+attn2", "lora_ff": True}}


def meta_model(rank, extra):
    from ltx_amd.config import TrainConfig
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.transformer3d import OURS_TRANSFORMER_CONFIG, Transformer3DModel
    tc = TrainConfig(checkpoint_path="ltxv-2b.safetensors", lora_rank=rank, lora_alpha=rank)
    for k, v in extra.items():
        setattr(tc, k, v)
    with torch.device("meta"):
        model = Transformer3DModel.from_config(OURS_TRANSFORMER_CONFIG)
        apply_training_strategy(model, tc, "lora_audio")
    return model


def torch_loop(pairs, cap):
    """kohya's loop on the device tensors: a GEMM, a norm, two host reads and two multiplies per pair"""
    keys, norms = 0, []
    for _, down, up, scale in pairs:
        updown = (up @ down) * scale
        norm = updown.norm().clamp(min=cap / 2)
        desired = torch.clamp(norm, max=cap)
        ratio = desired.cpu() / norm.cpu()
        sqrt_ratio = ratio ** 0.5
        if ratio != 1:
            keys += 1
            up *= sqrt_ratio
            down *= sqrt_ratio
        norms.append((updown.norm() * ratio).item())
    return keys, sum(norms) / len(norms), max(norms)


def bench_set(name, rank, a, device):
    from ltx_amd import ops
    from ltx_amd.lora import adapter_pairs
    from ltx_amd.training import FusedAdamW
    model = meta_model(rank, SETS[name])
    named = [(n, p) for n, p in model.named_parameters() if ("lora_" in n) or ("caption_projection" in n)]
    index = {id(p): i for i, (_, p) in enumerate(named)}
    meta_pairs = adapter_pairs(model)
    g = torch.Generator(device=device).manual_seed(1234)

    def tensors(std):
        return [torch.empty(tuple(p.shape), dtype=torch.float32, device=device).normal_(0, std, generator=g)
                .to(torch.float32 if "lora_" in n else torch.bfloat16) for n, p in named]
    values, grads = tensors(0.02), tensors(1e-3)

    def make(cap):
        ps = [torch.nn.Parameter(v.clone()) for v in values]
        for p, x in zip(ps, grads):
            p.grad = x  # shared, read-only
        pairs = [(n, ps[index[id(A)]], ps[index[id(B)]], s) for n, A, B, s in meta_pairs]
        kw = dict(scale_weight_norms=cap, norm_pairs=pairs) if cap else {}
        return FusedAdamW(ps, lr=1e-4, **kw), pairs
    with torch.no_grad():
        first = [float(torch.linalg.matrix_norm((values[index[id(B)]].double() @ values[index[id(A)]].double())) * abs(s))
                 for _, A, B, s in meta_pairs]
    median = sorted(first)[len(first) // 2]
    opts = {"off": make(None), "fused_none": make(1e30), "fused_some": make(median), "torch_loop": make(None)}

    def loop_step():
        opts["torch_loop"][0].step()
        with torch.no_grad():
            torch_loop(opts["torch_loop"][1], median)
    steppers = {k: v[0].step for k, v in opts.items() if k != "torch_loop"}
    steppers["torch_loop"] = loop_step

    def run(step, n):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) * 1e3 / n
    # the first fused step builds and uploads the tables: timed on the host, with a synchronize behind it
    opt = opts["fused_some"][0]
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    tables = opt._max_norm_tables(device)
    torch.cuda.synchronize(device)
    build_ms = (time.perf_counter() - t0) * 1e3
    for step in steppers.values():
        run(step, a.warmup)
    ms = {k: [] for k in steppers}
    keys = []
    for _ in range(a.rounds):
        for k, step in steppers.items():
            ms[k].append(run(step, a.steps))
        keys.append(int(opt.keys_scaled))
    # per launch: HIP events around the three entry points over a few steps of fused_some
    timer = ops.LaunchTimer()
    ops.set_launch_timer(timer)
    try:
        run(opt.step, 10)
    finally:
        ops.set_launch_timer(None)
    launches = {e["kernel"]: round(1e3 * e["ms"] / e["launches"], 2) for e in timer.summary()}  # us per launch
    # the stores alone, every row storing (a factor just under 1; the weights shrink by 1e-6 per call)
    table, npairs, nwg, ws, factor, scale, nrows = tables
    factor.fill_(1.0 - 2.0 ** -20)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ops.max_norm_scale_multi(scale, nrows, factor)
    ev[0].record()
    for _ in range(10):
        ops.max_norm_scale_multi(scale, nrows, factor)
    ev[1].record()
    torch.cuda.synchronize(device)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    elements = sum(A.numel() + B.numel() for _, A, B, _ in meta_pairs)
    return {"set": name, "rank": rank, "pairs": len(meta_pairs), "paired_elements": elements,
            "cap_fused_some": median, "keys_scaled_after_each_round": keys,
            "ms_per_step": ms, "median_ms_per_step": med,
            "added_ms_per_step": {k: round(med[k] - med["off"], 4) for k in med if k != "off"},
            "us_per_launch": launches, "us_scale_launch_every_row_storing": round(100.0 * ev[0].elapsed_time(ev[1]), 2),
            "gram_workgroups": nwg, "scale_rows": nrows,
            "workspace_bytes": ws.numel() * 8 + factor.numel() * 4,
            "tables_bytes": table.numel() * 8 + scale.numel() * 8, "tables_host_build_ms": round(build_ms, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="attn2:16,full:16,full:128")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ltx_amd import _lib
    device = torch.device("cuda", 0)
    _lib.ensure_device(device)
    res = {"device": torch.cuda.get_device_name(device), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "sets": []}
    for item in a.sets.split(","):
        name, rank = item.split(":")
        res["sets"].append(bench_set(name, int(rank), a, device))
        torch.cuda.empty_cache()
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
