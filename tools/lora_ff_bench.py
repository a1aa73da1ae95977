"""LoRA adapters on the feed-forward linears (config.lora_ff) on one MI355X at config A (bench.py's
workload: B = 8, N = 1792, M = 14336, D = 2048, 28 layers):

  * the train step for 'attn2' (the default) and 'attn2' + lora_ff at r = 16 and r = 32, with
    bench.py's warm-up and step counts, the four models interleaved in one process (each round times
    every model once, so drift of the box hits all alike), and each model's peak allocated memory
    during its own steps;
  * per-launch times of the adapter backward at the feed-forward's shapes, the merged form
    (ltx_lora_dy_dA, for dY = d_f [M, 8192] the wide dA pass) against the LTX_LORA_DY_DA=0 route
    (ltx_lora_dy, then ltx_lora_wgrad for dA), both orientations, ranks 16 / 32 / 64;
  * the K = 8192 down-projection u2 = act . A2^T (ltx_lora_rows: column-split pass + finish) beside the
    K = 2048 one (whole-contraction kernel), and the norm pass that recomputes x2;
  * the same step with LTX_LORA_FF_DY_DA = 1 / 0 and with LTX_LORA_FF_KEEP_X2 = 0 / 1, interleaved
    (with each setting's peak memory);
  * what ops.gemm_kernel_name returns for the four GEMM forms the feed-forward adapters add.

    python tools/lora_ff_bench.py [--steps 20] [--warmup 3] [--rounds 3] [--out FILE.json]

Prints one JSON document (also written to --out)."""
import argparse
import importlib.util
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "video-generation-for-human-avatars_amd"))

import torch  # noqa: E402

spec = importlib.util.spec_from_file_location("lora_attn1_bench", os.path.join(REPO, "tools", "lora_attn1_bench.py"))
base = importlib.util.module_from_spec(spec)
spec.loader.exec_module(base)  # Runner, per_launch_us, bench


class Runner(base.Runner):
    """lora_attn1_bench.Runner with config.lora_ff: the model is built by its build_model with the
    switch set on the TrainConfig it creates"""

    def __init__(self, device, targets, rank, ff):
        from ltx_amd import lora
        apply = lora.apply_training_strategy

        def with_ff(model, config, mode):
            if ff:
                setattr(config, "lora_ff", True)
            return apply(model, config, mode)
        lora.apply_training_strategy = with_ff
        try:
            super().__init__(device, targets, rank)
        finally:
            lora.apply_training_strategy = apply
        n = sum(".ff." in k and "lora_" in k for k, _ in self.model.named_parameters())
        assert n == (4 * len(self.model.transformer_blocks) if ff else 0)


def kernel_times(device):
    from ltx_amd import ops
    M, D, F = 14336, 2048, 8192
    gen = torch.Generator(device=device).manual_seed(0)
    x2 = torch.randn(M, D, device=device, generator=gen).bfloat16()
    d_ffo = torch.randn(M, D, device=device, generator=gen).bfloat16()
    act = torch.randn(M, F, device=device, generator=gen).bfloat16()
    d_f = torch.randn(M, F, device=device, generator=gen).bfloat16()
    ops._gemm_workspace(x2.device)
    out = {}
    for r in (16, 32, 64):
        res = {}
        fns = []
        for tag, dy, x in (("d_f[M,8192] x2[M,2048]", d_f, x2), ("d_ffo[M,2048] act[M,8192]", d_ffo, act)):
            N, K = dy.shape[1], x.shape[1]
            u = torch.randn(M, r, device=device, generator=gen)
            pb = ops.lora_pieces(torch.randn(N, r, device=device, generator=gen) * 0.05, transposed=True)
            dB, dA = torch.zeros(N, r, device=device), torch.zeros(r, K, device=device)

            def merged(dy=dy, x=x, u=u, pb=pb, dB=dB, dA=dA):
                ops.lora_dy(dy, u, pb, r, 1.0, dB, x=x, dA_out=dA)

            def separate(dy=dy, x=x, u=u, pb=pb, dB=dB, dA=dA):
                w, _ = ops.lora_dy(dy, u, pb, r, 1.0, dB)
                ops.lora_wgrad(x, w, transpose_out=True, out=dA, accumulate=True)
            fns += [(f"{tag} merged_us", merged), (f"{tag} separate_us", separate)]
        for K, x in ((D, x2), (F, act)):
            pa = ops.lora_pieces(torch.randn(r, K, device=device, generator=gen) / K ** 0.5)
            fns.append((f"lora_rows K={K}_us", lambda x=x, pa=pa: ops.lora_rows(x, pa, r, split=True)))
        for _ in range(3):  # interleaved repeats; all three reported
            for name, fn in fns:
                res.setdefault(name, []).append(round(base.per_launch_us(fn), 2))
        out[f"r{r}"] = res
    B = 8
    mods = torch.randn(B, 6, D, device=device, generator=gen).bfloat16()
    onep = torch.randn(B, 6, D, device=device, generator=gen).bfloat16()
    out["rmsnorm_modulate_fwd_us"] = [round(base.per_launch_us(
        lambda: ops.rmsnorm_modulate_fwd(x2, mods[:, 3], onep[:, 4], mods.stride(0), M // B, 1e-6)), 2) for _ in range(3)]
    return out


def gemm_forms():
    from ltx_amd import ops
    M, D, F = 14336, 2048, 8192
    out = {}
    for r in (16, 32, 64, 128):
        K2 = ops.lora_k2(r)
        out[f"r{r}"] = {
            "K2": K2,
            "FF1 gelu + extension (4D x D, K2)": ops.gemm_kernel_name(M, F, D, K2, "gelu"),
            "FF2 gated_residual + extension (D x 4D, K2)": ops.gemm_kernel_name(M, D, F, K2, "gated_residual"),
            "d_f gelu_bwd + extension (4D x D, K2)": ops.gemm_kernel_name(M, F, D, K2, "gelu_bwd"),
            "dx2 store + extension (D x 4D, K2)": ops.gemm_kernel_name(M, D, F, K2, "store"),
        }
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
    doc = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "gemm_kernels": gemm_forms()}
    doc["kernels_us"] = kernel_times(device)
    print(json.dumps({"kernels_us": doc["kernels_us"]}), flush=True)
    cases = [("attn2", r, ff) for r in (16, 32) for ff in (False, True)]
    runners = {c: Runner(device, *c) for c in cases}
    for rn in runners.values():
        for _ in range(args.warmup):
            rn.step()
    ms = {c: [] for c in cases}
    peak = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c in cases:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            ms[c].append(round(runners[c].timed(args.steps), 3))
            peak[c].append(round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1))
    name = lambda c: f"{c[0]}{'+ff' if c[2] else ''} r={c[1]}"
    doc["step_ms"] = {name(c): v for c, v in ms.items()}
    # peak allocated during the model's own steps, above what was resident when they began (the four
    # models' weights and optimizer states): activations and workspaces of one micro-step
    doc["step_peak_above_resident_MiB"] = {name(c): v for c, v in peak.items()}
    print(json.dumps({"step_ms": doc["step_ms"], "peak": doc["step_peak_above_resident_MiB"]}), flush=True)
    ab = {}
    for var, flags in (("LTX_LORA_FF_DY_DA", ("1", "0")), ("LTX_LORA_FF_KEEP_X2", ("0", "1"))):
        for r in (16, 32):
            rn = runners[("attn2", r, True)]
            key = f"{var} r={r}"
            ab[key] = {f: [] for f in flags}
            for _ in range(args.rounds):
                for f in flags:
                    os.environ[var] = f
                    rn.step()
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    ab[key][f].append(round(rn.timed(args.steps), 3))
                    ab[key].setdefault(f + " peak_MiB", []).append(
                        round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1))
        os.environ.pop(var, None)
    doc["switch_step_ms"] = ab
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
