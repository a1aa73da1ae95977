"""LoRA dropout (config.lora_dropout) on one MI355X at config A (bench.py's workload: B = 8, N = 1792,
M = 14336, D = 2048, 28 layers):

  * the train step at p = 0.1 against p = 0 for the adapter sets 'attn2' (the default), 'attn1+attn2'
    and 'attn1+attn2' + lora_ff at r = 16, with bench.py's warm-up and step counts. One model per
    adapter set; p is flipped on its LoraLinear modules between measurements, so both rates run on the
    same weights, and each round times every (set, p) once (drift of the box hits all alike);
  * per-launch times of the two new kernels at config A's shapes against their HBM floor:
    ltx_lora_dropout_apply on [M, 2048] and [M, 8192], ltx_lora_up_masked_add at G = 1 and G = 3 on
    [M, 2048], with the GELU factor on [M, 8192], ranks 16 / 32 / 64 / 128;
  * xd recomputed in the backward (the default) against nothing else: keeping xd was not built.

    python tools/lora_dropout_bench.py [--steps 20] [--warmup 3] [--rounds 3] [--out FILE.json]

Prints one JSON document (also written to --out)."""
import argparse
import importlib.util
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "video-generation-for-human-avatars_amd"))

import torch  # noqa: E402

spec = importlib.util.spec_from_file_location("lora_ff_bench", os.path.join(REPO, "tools", "lora_ff_bench.py"))
ffb = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ffb)  # Runner (targets, rank, ff), base.per_launch_us

HBM_TBS = 8.0  # MI355X peak HBM bandwidth, TB/s (the floor below is bytes / this)


def set_rate(model, p):
    """flip lora_dropout on every adapter of the model (what LoraLinear(..., dropout=p) sets)"""
    from ltx_amd.transformer3d import LoraLinear
    for m in model.modules():
        if isinstance(m, LoraLinear):
            m.lora_dropout_p = float(p)
            m.lora_dropout["default"] = torch.nn.Dropout(p) if p > 0 else torch.nn.Identity()


def kernel_times(device):
    from ltx_amd import ops
    M, D, F = 14336, 2048, 8192
    gen = torch.Generator(device=device).manual_seed(0)
    key = 0x1234ABCD5678EF01
    T, c = ops.lora_dropout_threshold(0.1)
    out = {"hbm_peak_TBs": HBM_TBS}
    res = {}
    for K in (D, F):
        x = torch.randn(M, K, device=device, generator=gen).bfloat16()
        xd = torch.empty_like(x)
        us = [round(ffb.base.per_launch_us(lambda: ops.lora_dropout_apply(x, key, 5, T, out=xd)), 2) for _ in range(3)]
        nbytes = 4.0 * M * K
        res[f"[M, {K}]"] = {"us": us, "bytes": nbytes, "floor_us": round(nbytes / HBM_TBS / 1e6, 2)}
        del x, xd
    out["lora_dropout_apply"] = res
    res = {}
    for r in (16, 32, 64, 128):
        for tag, K, G, with_g in (("G=1 [M, 2048]", D, 1, False), ("G=3 [M, 2048]", D, 3, False),
                                  ("G=1 g [M, 8192]", F, 1, True)):
            dx = torch.randn(M, K, device=device, generator=gen).bfloat16()
            w = torch.randn(M, G * r, device=device, generator=gen)
            As = [torch.randn(r, K, device=device, generator=gen) / r ** 0.5 for _ in range(G)]
            g = ops.gelu_grad_q(torch.randn(M, K, device=device, generator=gen).bfloat16()) if with_g else None
            us = [round(ffb.base.per_launch_us(
                lambda: ops.lora_up_masked_add(dx, w, As, list(range(G)), key, T, c, g=g)), 2) for _ in range(3)]
            nbytes = 4.0 * M * K + 4.0 * G * r * (M + K) + (2.0 * M * K if with_g else 0.0)
            res[f"r={r} {tag}"] = {"us": us, "bytes": nbytes, "floor_us": round(nbytes / HBM_TBS / 1e6, 2),
                                   "flop": 2.0 * M * K * G * r}
            del dx, w, As, g
    out["lora_up_masked_add"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    from ltx_amd import _lib
    _lib.ensure_device(device)
    torch.manual_seed(20251019)
    doc = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "rank": 16, "p": 0.1}
    doc["kernels"] = kernel_times(device)
    print(json.dumps({"kernels": doc["kernels"]}), flush=True)
    sets = [("attn2", False), ("attn1+attn2", False), ("attn1+attn2", True)]
    name = lambda s: s[0] + ("+ff" if s[1] else "")
    ms, peak = {}, {}
    runners = {}
    for s in sets:
        runners[s] = ffb.Runner(device, s[0], 16, s[1])
        for p in (0.0, 0.1):
            set_rate(runners[s].model, p)
            for _ in range(args.warmup):
                runners[s].step()
    for _ in range(args.rounds):
        for s in sets:
            for p in (0.0, 0.1):
                set_rate(runners[s].model, p)
                runners[s].step()  # the first step after a flip (allocator, caches) is not timed
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                k = f"{name(s)} p={p}"
                ms.setdefault(k, []).append(round(runners[s].timed(args.steps), 3))
                peak.setdefault(k, []).append(round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1))
    doc["step_ms"] = ms
    doc["step_peak_above_resident_MiB"] = peak
    doc["last_lora_dropout_key"] = {name(s): runners[s].model.last_lora_dropout_key for s in sets}
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
