"""LoRA targets on one MI355X at config A (bench.py's workload: B = 8, N = 1792, 28 layers):

  * the train step for lora_targets 'attn2', 'attn1' and 'attn1+attn2' at r = 16 and r = 32, with
    bench.py's warm-up and step counts, the six models interleaved in one process (each round times
    every model once, so drift of the box hits all alike);
  * the per-launch times of the grouped adapter kernels (ltx_lora_rows_grouped,
    ltx_lora_dy_dA_grouped) against the three one-adapter calls they replace, at config A's shapes
    (M = 14336, D = 2048), ranks 16 / 32 / 64 / 128;
  * the same step with LTX_LORA_QKV_GROUPED = 1 and 0 ('attn1+attn2', r = 16 / 32), interleaved;
  * what ops.gemm_kernel_name returns for the four GEMM forms the attn1 adapters add.

    python tools/lora_attn1_bench.py [--steps 20] [--warmup 3] [--rounds 3] [--out FILE.json]

Prints one JSON document (also written to --out)."""
import argparse
import importlib.util
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "video-generation-for-human-avatars_amd"))

import torch  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def build_model(device, targets, rank, seed=1234):
    """bench.build_model with config.lora_targets and the rank as arguments"""
    import math
    from ltx_amd.config import TrainConfig
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.patchifier import SymmetricPatchifier
    from ltx_amd.transformer3d import OURS_TRANSFORMER_CONFIG, Transformer3DModel
    tc = TrainConfig(checkpoint_path="-", lora_rank=rank, lora_alpha=rank)
    setattr(tc, "lora_targets", targets)
    with torch.device("meta"):
        model = Transformer3DModel.from_config(OURS_TRANSFORMER_CONFIG)
        apply_training_strategy(model, tc, "lora_audio")
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, p in model.named_parameters():
        t = torch.empty(p.shape, dtype=torch.float32, device=device)
        if p.dim() == 2:
            t.normal_(0, 1.0 / math.sqrt(p.shape[1]), generator=g)
        elif "norm" in name:
            t.fill_(1.0)
        elif name.endswith("scale_shift_table"):
            t.normal_(0, 1.0 / math.sqrt(p.shape[-1]), generator=g)
        else:
            t.normal_(0, 0.02, generator=g)
        if "lora_B" in name:
            t.normal_(0, 0.01, generator=g)
        sd[name] = t.to(torch.float32 if "lora_" in name else torch.bfloat16)
    model.load_state_dict(sd, assign=True, strict=True)
    for n, p in model.named_parameters():
        p.requires_grad_(("lora_" in n) or ("caption_projection" in n))
    model.patchifier = SymmetricPatchifier(1)
    model.train()
    return model


class Runner:
    """bench.py's one_step for one model: micro-steps with the optimizer step every ACCUM-th"""

    def __init__(self, device, targets, rank):
        from ltx_amd.config import TrainConfig
        from ltx_amd.scheduler import RectifiedFlowScheduler
        from ltx_amd.training import FusedAdamW, GradAllReduce
        self.model = build_model(device, targets, rank)
        self.batch, self.prompt, self.mask = bench.synthetic_batch(device, 0)
        self.cfg = TrainConfig(checkpoint_path="-", batch_size=bench.B_PER_GPU, learning_rate=1e-4, lora_rank=rank,
                               lora_alpha=rank, gradient_accumulation_steps=bench.ACCUM, rf_log_normal_mu=-0.5,
                               rf_log_normal_sigma=1.0)
        self.sched = RectifiedFlowScheduler(num_train_timesteps=1000, shifting=None)
        trainable = [p for p in self.model.parameters() if p.requires_grad]
        self.opt = FusedAdamW(trainable, lr=self.cfg.learning_rate)
        self.reducer = GradAllReduce(trainable, order=self.model.grad_ready_order()).install(self.model)
        self.reducer.zero_grad()
        self.device, self.i = device, 0

    def step(self):
        from ltx_amd.training import train_step
        last = (self.i + 1) % bench.ACCUM == 0
        if last:
            self.reducer.arm()
        train_step(self.model, self.batch, self.sched, self.model.patchifier, self.cfg, self.prompt, self.mask,
                   self.device)
        if last:
            self.reducer()
            self.opt.step()
            self.reducer.zero_grad()
        self.i += 1

    def timed(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps


def per_launch_us(fn, it=30):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / it * 1e3


def kernel_times(device):
    """grouped against separate, config A's self-attention shapes; the separate forms are what the
    block calls with LTX_LORA_QKV_GROUPED=0 (outputs into the same side-by-side buffers)"""
    from ltx_amd import ops
    M, D, G = 14336, 2048, 3
    gen = torch.Generator(device=device).manual_seed(0)
    x = torch.randn(M, D, device=device, generator=gen).bfloat16()
    dy = torch.randn(M, G * D, device=device, generator=gen).bfloat16()
    ops._gemm_workspace(x.device)
    out = {}
    for r in (16, 32, 64, 128):
        K2 = ops.lora_k2(r)
        As = [torch.randn(r, D, device=device, generator=gen) / D ** 0.5 for _ in range(G)]
        Bs = [torch.randn(D, r, device=device, generator=gen) * 0.05 for _ in range(G)]
        pa = [ops.lora_pieces(A) for A in As]
        pb = [ops.lora_pieces(Bm, transposed=True) for Bm in Bs]
        u = torch.empty(M, G * r, device=device)
        su = torch.empty(M, G * K2, dtype=torch.bfloat16, device=device)

        def rows_sep():
            for g in range(G):
                ops.lora_rows(x, pa[g], r, out=u[:, g * r:(g + 1) * r], split=True, split_out=su[:, g * K2:(g + 1) * K2])

        def rows_grp():
            ops.lora_rows_grouped(x, pa, r, out=u[:, :r], split=True, split_out=su[:, :K2])
        us = [u[:, g * r:(g + 1) * r] for g in range(G)]
        dB = [torch.zeros(D, r, device=device) for _ in range(G)]
        dA = [torch.zeros(r, D, device=device) for _ in range(G)]
        w = torch.empty(M, G * r, device=device)
        sw = torch.empty(M, G * K2, dtype=torch.bfloat16, device=device)

        def dy_sep():
            for g in range(G):
                ops.lora_dy(dy[:, g * D:(g + 1) * D], us[g], pb[g], r, 1.0, dB[g], x=x, dA_out=dA[g],
                            w_out=w[:, g * r:(g + 1) * r], split_out=sw[:, g * K2:(g + 1) * K2])

        def dy_grp():
            ops.lora_dy_grouped(dy, us, pb, r, 1.0, dB, x, dA, w_out=w, split_out=sw)
        rows_sep()
        res = {}
        for _ in range(3):  # interleaved repeats; the median of each
            for name, fn in (("rows_separate_us", rows_sep), ("rows_grouped_us", rows_grp),
                             ("dy_dA_separate_us", dy_sep), ("dy_dA_grouped_us", dy_grp)):
                res.setdefault(name, []).append(per_launch_us(fn))
        out[f"r{r}"] = {k: round(sorted(v)[1], 2) for k, v in res.items()}
    return out


def gemm_forms():
    """the kernels the dispatcher picks for the four GEMM forms the attn1 adapters add (config A)"""
    from ltx_amd import ops
    M, D, d = 14336, 2048, 64
    out = {}
    for r in (16, 32, 64, 128):
        K2 = ops.lora_k2(r)
        out[f"r{r}"] = {
            "K2": K2,
            "qkv store, grouped extension (3D x D, K2)": ops.gemm_kernel_name(M, 3 * D, D, K2, "store"),
            "to_out gated_residual + extension (D x D, K2)": ops.gemm_kernel_name(M, D, D, K2, "gated_residual"),
            "do1 store_rowdot + extension (D x D, K2)": ops.gemm_kernel_name(M, D, D, K2, "store_rowdot", d),
            "dx1 dgrad + extension (D x 3D, 3 K2)": ops.gemm_kernel_name(M, D, 3 * D, 3 * K2, "store"),
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
    torch.manual_seed(20251015)
    doc = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "gemm_kernels": gemm_forms()}
    doc["kernels_us"] = kernel_times(device)
    print(json.dumps({"kernels_us": doc["kernels_us"]}), flush=True)
    cases = [(t, r) for r in (16, 32) for t in ("attn2", "attn1", "attn1+attn2")]
    runners = {c: Runner(device, *c) for c in cases}
    for rn in runners.values():
        for _ in range(args.warmup):
            rn.step()
    ms = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c in cases:
            ms[c].append(round(runners[c].timed(args.steps), 3))
    doc["step_ms"] = {f"{t} r={r}": v for (t, r), v in ms.items()}
    print(json.dumps({"step_ms": doc["step_ms"]}), flush=True)
    # grouped against separate q / k / v adapter kernels inside the step (bitwise the same results)
    ab = {}
    for r in (16, 32):
        rn = runners[("attn1+attn2", r)]
        ab[f"r={r}"] = {"grouped": [], "separate": []}
        for _ in range(args.rounds):
            for flag, key in (("1", "grouped"), ("0", "separate")):
                os.environ["LTX_LORA_QKV_GROUPED"] = flag
                rn.step()
                ab[f"r={r}"][key].append(round(rn.timed(args.steps), 3))
    os.environ.pop("LTX_LORA_QKV_GROUPED", None)
    doc["qkv_grouped_step_ms"] = ab
    doc["peak_mem_GiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
