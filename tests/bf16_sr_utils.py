"""Helpers of tests/test_bf16_sr_cpu.py and tests/test_bf16_sr_gpu.py: a second, scalar statement of the
random numbers behind the stochastically rounded bf16 store (plain Python integers, written from the
Random123 description of Philox4x32-10 and the lane rule, independent of lora.philox4x32_10's numpy), and
the per-tensor model of the stochastic AdamW step: the project's f32 step on the widened values, then
training.stochastic_round_bf16."""
import torch

M32 = 0xFFFFFFFF
# bf16 tensors of one element, one short of a vector, a vector, one short of a chunk, one over, two chunks
# and a ragged tail (vector part and single elements in the last row); one f32 tensor beside them
BF16_SIZES = [1, 7, 8, 2047, 2049, 4096 + 13]
F32_SIZE = 2049


def philox_scalar(counter, key):
    """Philox4x32-10 on Python ints: ten rounds of two 32 x 32 -> 64 bit multiplies, the key bumped by the
    Weyl constants between rounds."""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def sr_bits_scalar(seed, ordinal, step, i):
    """The 16-bit r of element i: counter (lo32(i >> 3), hi32(i >> 3), ordinal, step mod 2^32), key
    (seed lo, seed hi), lane i & 7 -- the low half of word lane // 2 for an even lane, the high half for
    an odd one."""
    q = i >> 3
    words = philox_scalar((q & M32, q >> 32, ordinal, step & M32), (seed & M32, seed >> 32))
    lane = i & 7
    return (words[lane >> 1] >> (16 * (lane & 1))) & 0xFFFF


def sr_store(x_f32, seed, ordinal, step):
    """stochastic_round_bf16 of a device tensor, back on its device"""
    from ltx_amd.training import stochastic_round_bf16
    return stochastic_round_bf16(x_f32.detach().float().cpu(), seed, ordinal, step).to(x_f32.device)


def make_params(seed, device, scale=1.0, sizes=BF16_SIZES, f32_size=F32_SIZE):
    """bf16 parameters of `sizes` and one f32 parameter of `f32_size` behind them"""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((scale * torch.randn(n, generator=g)).to(torch.bfloat16).to(device)) for n in sizes]
    return ps + [torch.nn.Parameter((scale * torch.randn(f32_size, generator=g)).to(device))]


def make_grads(seed, device, scale=1.0, sizes=BF16_SIZES, f32_size=F32_SIZE):
    g = torch.Generator().manual_seed(seed)
    gs = [(scale * torch.randn(n, generator=g)).to(torch.bfloat16).to(device) for n in sizes]
    return gs + [(scale * torch.randn(f32_size, generator=g)).to(device)]


class AdamWModel:
    """The statement of FusedAdamW(bf16_update="stochastic") for bf16 tensors, one tensor at a time:
    ops.adamw_step (the f32 per-tensor kernel) on float(p), float(g) -- with `coef` on
    float(bf16(float(g) * coef)) -- and the carried f32 moments, then stochastic_round_bf16 under
    (seed, the tensor's ordinal, its step). `p`, `exp_avg`, `exp_avg_sq` are lists over the tensors."""

    def __init__(self, params, seed, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, ordinals=None):
        self.p = [p.detach().clone() for p in params]
        self.exp_avg = [torch.zeros_like(p, dtype=torch.float32) for p in params]
        self.exp_avg_sq = [torch.zeros_like(p, dtype=torch.float32) for p in params]
        self.seed, self.lr, self.wd, self.betas, self.eps = seed, lr, weight_decay, betas, eps
        self.ordinals = list(range(len(params))) if ordinals is None else ordinals
        self.steps = 0

    def step(self, grads, coef=None):
        from ltx_amd import ops
        self.steps += 1
        for i, g in enumerate(grads):
            P, G = self.p[i].float(), g.float()
            if coef is not None:
                G = (G * coef).to(torch.bfloat16).float()
            ops.adamw_step(P, G, self.exp_avg[i], self.exp_avg_sq[i], self.lr, self.betas[0], self.betas[1], self.eps,
                           self.wd, self.steps)
            self.p[i] = sr_store(P, self.seed, self.ordinals[i], self.steps)
