"""DoRA (config.use_dora) on one MI355X at config A (bench.py's workload: B = 8, N = 1792, M = 14336,
D = 2048, 28 layers):

  * per-call times of the new kernels beside their algorithmic bytes: ltx_dora_fold at N = K = 2048
    (the kernel alone, and with the ltx_transpose_bf16 of W_eff that ops.dora_fold adds),
    ltx_dora_mag_grad at M = 14336 and on the 256 shared text rows, ltx_dora_rowscale_add, and the
    to_out.0 recompute GEMM (o2 . W_eff^T plus the K extension, no bias);
  * the refresh of one model's DoRA operands after an optimizer step (112 folds + transposes, the
    K | V concatenations, the splits and pieces of c (.) s B): what one accumulation cycle pays once;
  * the train step of three models on the same weights, interleaved (each round times every model
    once): plain LoRA on attn2 with the batched text side (the default), plain LoRA on the per-block
    text path (transformer3d._TEXT_BATCH off, what LTX_TEXT_BATCH=0 selects), and DoRA (which always
    takes the per-block path), with each one's peak allocated memory.

    python tools/lora_dora_bench.py [--rank 16] [--steps 20] [--warmup 3] [--rounds 3] [--out FILE.json]

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


class DoraRunner(base.Runner):
    """lora_attn1_bench.Runner with config.use_dora; W, A and B are copied from `like` (a plain runner's
    model) and the magnitudes set to norm * |1 + 0.2 randn|, so c differs from 1 as in a trained model"""

    def __init__(self, device, rank, like):
        from ltx_amd import lora
        from ltx_amd.transformer3d import LoraLinear
        apply = lora.apply_training_strategy

        def with_dora(model, config, mode):
            setattr(config, "use_dora", True)
            return apply(model, config, mode)
        lora.apply_training_strategy = with_dora
        try:
            super().__init__(device, "attn2", rank)
        finally:
            lora.apply_training_strategy = apply
        sd = like.state_dict()
        with torch.no_grad():
            for name, p in self.model.named_parameters():
                if name in sd:
                    p.copy_(sd[name])
            g = torch.Generator(device=device).manual_seed(7)
            n = 0
            for m in self.model.modules():
                if isinstance(m, LoraLinear):
                    norm = m.dora_operands()["norm"]
                    m.lora_magnitude_vector["default"].weight.copy_(
                        norm * (1 + 0.2 * torch.randn(norm.shape, device=device, generator=g)).abs())
                    n += 1
        assert n == 4 * len(self.model.transformer_blocks)


def kernel_times(device, rank):
    from ltx_amd import ops
    M, D, L = 14336, 2048, 256
    gen = torch.Generator(device=device).manual_seed(0)
    W = (torch.randn(D, D, device=device, generator=gen) / D ** 0.5).bfloat16()
    A = torch.randn(rank, D, device=device, generator=gen) / D ** 0.5
    B = 0.05 * torch.randn(D, rank, device=device, generator=gen)
    m = torch.rand(D, device=device, generator=gen) + 0.5
    dy = torch.randn(M, D, device=device, generator=gen).bfloat16()
    y = torch.randn(M, D, device=device, generator=gen).bfloat16()
    bias = (0.1 * torch.randn(D, device=device, generator=gen)).bfloat16()
    dm = torch.zeros(D, device=device)
    u = torch.randn(M, rank, device=device, generator=gen)
    ops._gemm_workspace(device)
    norm, c, w_eff, w_effT, sb = ops.dora_fold(W, A, B, m, 1.0)
    spl = ops.lora_split(sb, "weight", 1.0)
    dB, scratch = torch.zeros(D, rank, device=device), torch.randn(D, rank, device=device, generator=gen)
    fns = [
        ("dora_fold (kernel alone)", lambda: ops.dora_fold(W, A, B, m, 1.0, transposed=False),
         4.0 * D * D + 4.0 * rank * 2 * D),  # W read, W_eff written (the second W read is L2's), A, B
        ("dora_fold + transpose", lambda: ops.dora_fold(W, A, B, m, 1.0), 8.0 * D * D + 4.0 * rank * 2 * D),
        ("transpose [2048, 2048] alone", lambda: ops.transpose(w_eff, out=w_effT), 4.0 * D * D),
        ("lora_split + lora_pieces of c.sB", lambda: (ops.lora_split(sb, "weight", 1.0), ops.lora_pieces(sb, transposed=True)), 0.0),
        (f"dora_mag_grad M={M}", lambda: ops.dora_mag_grad(dy, y, bias, m, dm), 4.0 * M * D),
        (f"dora_mag_grad M={L} (shared text rows)", lambda: ops.dora_mag_grad(dy[:L], y[:L], bias, m, dm), 4.0 * L * D),
        ("dora_rowscale_add", lambda: ops.dora_rowscale_add(dB, scratch, c, 1.0), 12.0 * D * rank),
        ("to_out.0 recompute: lora_split(u_o)", lambda: ops.lora_split(u, "act"), 0.0),
        ("to_out.0 recompute: store GEMM + K extension", lambda: ops.gemm(y, w_eff, ext=(ops.lora_split(u, "act"), spl)), 0.0),
    ]
    res = {}
    for _ in range(3):  # interleaved repeats; all three reported
        for name, fn, nbytes in fns:
            e = res.setdefault(name, {"us": [], "bytes": nbytes})
            e["us"].append(round(base.per_launch_us(fn), 2))
    for e in res.values():
        if e["bytes"]:
            e["TBs_at_best"] = round(e["bytes"] / min(e["us"]) / 1e6, 2)
    return res


def refresh_ms(runner, rounds=3):
    """every DoRA operand of the model rebuilt, as the first forward after an optimizer step does"""
    from ltx_amd import ops
    from ltx_amd.transformer3d import LoraLinear, _kv_ext
    lins = [m for m in runner.model.modules() if isinstance(m, LoraLinear)]
    out = []
    for _ in range(rounds):
        ops.bump_weight_generation()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for blk in runner.model.transformer_blocks:
            blk.weights()
            _kv_ext(blk, blk.attn2.to_k, blk.attn2.to_v)
        for m in lins:
            m.weight_split("B"), m.weight_pieces("Bt"), m.weight_split("A"), m.weight_pieces("A")
        b.record()
        torch.cuda.synchronize()
        out.append(round(a.elapsed_time(b), 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    from ltx_amd import _lib
    import ltx_amd.transformer3d as T
    _lib.ensure_device(device)
    torch.manual_seed(20251019)
    doc = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "rank": args.rank,
           "accum": base.bench.ACCUM}
    doc["kernels"] = kernel_times(device, args.rank)
    print(json.dumps({"kernels": doc["kernels"]}), flush=True)
    text_batch = T._TEXT_BATCH
    plain = base.Runner(device, "attn2", args.rank)
    dora = DoraRunner(device, args.rank, plain.model)
    doc["refresh_ms"] = refresh_ms(dora)
    cases = [("plain, batched text side", plain, True), ("plain, per-block text path", plain, False),
             ("use_dora", dora, True)]
    ms, peak = {}, {}
    try:
        for name, rn, tb in cases:
            T._TEXT_BATCH = tb and text_batch
            for _ in range(args.warmup):
                rn.step()
        for _ in range(args.rounds):
            for name, rn, tb in cases:
                T._TEXT_BATCH = tb and text_batch
                rn.step()  # the first step after a flip (caches, allocator) is not timed
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                ms.setdefault(name, []).append(round(rn.timed(args.steps), 3))
                peak.setdefault(name, []).append(round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1))
    finally:
        T._TEXT_BATCH = text_batch
    doc["step_ms"] = ms
    doc["step_peak_above_resident_MiB"] = peak
    held = sum(t.numel() * t.element_size() for blk in dora.model.transformer_blocks
               for k, t in blk.weights().items() if k in ("q2_w", "q2_wT", "o2_w", "o2_wT", "kv2_w", "kv2_wT"))
    doc["dora_effective_weights_MiB"] = round(held / 2 ** 20, 1)
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
