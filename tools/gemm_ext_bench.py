"""Per-launch time of the attn2 projection GEMMs with a LoRA K extension (config A: M = 14336,
N = K = 2048), the default dispatch (the ring kernel) against gemm_nt_kernel_t (variant 15),
interleaved in one process: K2 = 64 / 128 / 192 / 384 (ranks 16 / 32 / 64 / 128), the plain store
(forward, with bias) and the accumulate epilogue (dgrad).
  python tools/gemm_ext_bench.py [rounds]
Each figure is the median over `rounds` (default 7) of the mean of 10 back-to-back launches on 4
rotating operand sets (3 x 58.7 MB + outputs per set: past the 256 MB MALL between reuses)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "video-generation-for-human-avatars_amd"))
import torch  # noqa: E402

from ltx_amd import _lib, ops  # noqa: E402

M, N, K = 14336, 2048, 2048
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
_lib.ensure_device()
lib = _lib.load()
g = torch.Generator(device="cuda").manual_seed(0)
sets = [dict(a=torch.randn(M, K, device="cuda", generator=g).bfloat16(),
             w=(torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).bfloat16(),
             b=torch.randn(N, device="cuda", generator=g).bfloat16(),
             c=torch.randn(M, N, device="cuda", generator=g).bfloat16(),
             a2=torch.randn(M, 384, device="cuda", generator=g).bfloat16(),
             w2=torch.randn(N, 384, device="cuda", generator=g).bfloat16()) for _ in range(4)]


def launch(s, K2, epi):
    ext = (s["a2"][:, :K2], s["w2"][:, :K2]) if K2 else None  # strided views of the 384-wide operands
    if epi == "store":
        ops.gemm(s["a"], s["w"], bias=s["b"], ext=ext)
    else:
        ops.gemm(s["a"], s["w"], epilogue="accum", aux0=s["c"], out=s["c"], ext=ext)


def timed(K2, epi, variant):
    lib.ltx_gemm_set_variant(variant)
    try:
        for s in sets:
            launch(s, K2, epi)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(10):
            launch(sets[i % 4], K2, epi)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 100.0  # us per launch
    finally:
        lib.ltx_gemm_set_variant(0)


for epi in ("store", "accum"):
    for K2 in (0, 64, 128, 192, 384):
        ops._GEMM_NAMES.clear()
        name = ops.gemm_kernel_name(M, N, K, K2, epi).split("(")[0]
        t = {0: [], 15: []}
        for _ in range(rounds):
            for v in (0, 15):
                t[v].append(timed(K2, epi, v))
        med = {v: sorted(x)[len(x) // 2] for v, x in t.items()}
        print(f"{epi:6s} K2 {K2:3d}  default {med[0]:7.1f} us ({name})   gemm_nt_kernel_t {med[15]:7.1f} us   "
              f"min {min(t[0]):.1f} / {min(t[15]):.1f}", flush=True)
