"""Helpers of tests/test_optim_guard_gpu.py: a small tensor set that reaches every branch of the chunk-table
row walks, the optimizer modes the guard is tested under, gradients with one non-finite element, bitwise
snapshots of everything a step may write, and a loader that poisons chosen batches of chosen epochs."""
import torch

BF16 = torch.bfloat16
# one element, one short of a vector, one short of a chunk, a chunk, one over (a one-element tail row), and
# two chunks with a ragged third
SIZES = [1, 7, 2047, 2048, 2049, 5000]
VIEW = 1000  # the two tensors whose gradients are views one element into a larger buffer
N_F32 = len(SIZES)
# index of: the first tensor, the 2049-element f32 tensor, the 5000-element bf16 tensor, the tensor without a
# gradient
FIRST, TAIL, IN_BF16, NO_GRAD = 0, SIZES.index(2049), N_F32 + SIZES.index(5000), 2 * N_F32 + 2
# (tensor, element, value): the first element of the first tensor, the last element of the 2049-element
# tensor (its one-element tail row), inside a bf16 tensor
POISONS = {"nan_first": (FIRST, 0, float("nan")), "inf_tail": (TAIL, 2048, float("inf")),
           "neginf_in_bf16": (IN_BF16, 2500, float("-inf"))}


def _ema():
    from ltx_amd.training import EMASchedule
    return EMASchedule(0.999)


# name -> (optimizer, constructor arguments); the EMA schedule is made per optimizer
MODES = {
    "adamw": ("adamw", {}),
    "adamw_clip": ("adamw", {"max_grad_norm": 0.5}),
    "adamw_ema": ("adamw", {"ema": True}),
    "adamw_clip_ema": ("adamw", {"max_grad_norm": 0.5, "ema": True}),
    "adamw_sr": ("adamw", {"bf16_update": "stochastic", "sr_seed": 0x5EED0123456789AB}),
    "adamw_sr_ema": ("adamw", {"bf16_update": "stochastic", "sr_seed": 0x5EED0123456789AB, "ema": True}),
    "prodigy": ("prodigy", {}),
    "prodigy_clip_ema": ("prodigy", {"max_grad_norm": 0.5, "ema": True}),
    "prodigy_sr": ("prodigy", {"bf16_update": "stochastic", "sr_seed": 0x5EED0123456789AB}),
}


def make_optimizer(mode, params, **more):
    from ltx_amd.training import FusedAdamW, FusedProdigy
    kind, kw = MODES[mode]
    kw = dict(kw, **more)
    if kw.get("ema"):
        kw["ema"] = _ema()
    if kind == "adamw":
        return FusedAdamW(params, lr=1e-2, weight_decay=1e-2, **kw)
    # d0 large enough that the first steps move bf16 weights too
    return FusedProdigy(params, d0=1e-3, weight_decay=1e-2, **kw)


def _dtypes():
    return [torch.float32] * N_F32 + [BF16] * N_F32 + [torch.float32, BF16, torch.float32]


def _numels():
    return SIZES + SIZES + [VIEW, VIEW, 16]


def make_params(device, seed=1):
    """f32 tensors of SIZES, bf16 tensors of SIZES, an f32 and a bf16 tensor of VIEW elements (their gradients
    are the unaligned views) and a 16-element tensor that never gets a gradient"""
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g).to(dt).to(device)) for n, dt in zip(_numels(), _dtypes())]


def clone_params(params):
    return [torch.nn.Parameter(p.detach().clone()) for p in params]


def make_grads(device, seed):
    """One finite gradient per parameter in its dtype (None for the last); the two VIEW gradients start one
    element into a buffer, 4 or 2 bytes past a 16-byte boundary."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for i, (n, dt) in enumerate(zip(_numels(), _dtypes())):
        if i == NO_GRAD:
            out.append(None)
            continue
        v = torch.randn(n, generator=g).to(dt).to(device)
        if n == VIEW:
            buf = torch.empty(n + 1, dtype=dt, device=device)
            v = buf[1:].copy_(v)
            assert v.data_ptr() % 16 == v.element_size()
        out.append(v)
    return out


def poisoned(grads, which):
    """`grads` with the one non-finite element of POISONS[which] (the other tensors shared, not copied)"""
    i, j, value = POISONS[which]
    out = list(grads)
    out[i] = grads[i].clone()
    out[i][j] = value
    return out


def set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = g


def snapshot(opt, params):
    """Clones of every device tensor a step may write -- parameters, exp_avg, exp_avg_sq, EMA shadows,
    Prodigy's s, p0 and record -- and the host's counters."""
    tensors, counters = {}, {"ema_steps": opt.ema_steps, "ema_decay": opt.ema_decay}
    for i, p in enumerate(params):
        tensors[f"param.{i}"] = p.detach().clone()
        for k, v in opt.state.get(p, {}).items():
            if torch.is_tensor(v):
                tensors[f"{k}.{i}"] = v.detach().clone()
            else:
                counters[f"{k}.{i}"] = v
    if getattr(opt, "record", None) is not None:
        tensors["record"] = opt.record.detach().clone()
    return tensors, counters


def assert_same(a, b, where=""):
    """bitwise: the same keys, dtypes and bit patterns (a NaN would compare equal to itself here)"""
    assert sorted(a) == sorted(b) and a, (where, sorted(set(a) ^ set(b)))
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (where, k)
        as_int = {4: torch.int32, 2: torch.int16, 8: torch.int64}[x.element_size()]
        assert torch.equal(x.contiguous().view(as_int), y.contiguous().view(as_int)), (where, k)


class PoisonLoader:
    """A LatentLoader whose batches number `poison[epoch]` (a set per epoch) carry NaN latents. The seed and
    set_epoch are the inner loader's, so a checkpoint saves and restores it as it would the loader itself."""

    def __init__(self, inner, poison):
        self.inner, self.poison, self.epoch = inner, poison, 0

    @property
    def seed(self):
        return self.inner.seed

    @seed.setter
    def seed(self, v):
        self.inner.seed = v

    def set_epoch(self, epoch):
        self.epoch = epoch
        self.inner.set_epoch(epoch)

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        bad = self.poison.get(self.epoch, ())
        for i, batch in enumerate(self.inner):
            if i in bad:
                batch = dict(batch, latents=torch.full_like(batch["latents"], float("nan")))
            yield batch
