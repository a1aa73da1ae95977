"""ProdigyStatement: the statement of the Prodigy step ("Prodigy") written with plain torch
eager ops, the yardstick of tests/test_prodigy_cpu.py and tests/test_prodigy_gpu.py.

It is the published prodigyopt.Prodigy for one parameter group with fsdp_in_use = False -- prodigyopt is
not a dependency and is not installed where the tests run, so the sequence of ops is written out here --
with the project's two departures: the factor (d / d0) dlr multiplies the summed numerator once, and a
bf16 tensor's dot product is formed in f32 and added in f64 instead of being rounded to bf16. State is kept
in the parameter's dtype; every torch op below rounds to it, which is the statement's R."""
import math

import torch


class ProdigyStatement:
    def __init__(self, params, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True,
                 use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf")):
        self.params = list(params)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.beta3 = math.sqrt(betas[1]) if beta3 is None else beta3
        self.decouple, self.use_bias_correction, self.safeguard_warmup = decouple, use_bias_correction, safeguard_warmup
        self.d0, self.d_coef, self.growth_rate = d0, d_coef, growth_rate
        self.d = self.d_max = d0
        self.d_numerator, self.k = 0.0, 0
        self.d_denom = self.d_hat = self.dlr = 0.0
        self.applied = False
        self.state = {}

    def _state(self, p):
        if p not in self.state:
            self.state[p] = {"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p),
                             "s": torch.zeros_like(p), "p0": p.detach().clone()}
        return self.state[p]

    @torch.no_grad()
    def step(self, grads, coef=None, override=None):
        """One step with `grads` (a list aligned with the parameters; None skips that parameter). `coef`:
        the clip coefficient (a 0-dim f32 tensor), g = grad * coef rounded to the gradient's dtype.
        `override` = (d_new, dlr): run the elementwise ops with this dlr and install this d after the
        d update, in place of the values computed here -- the sums have their own order on the device, so
        its d differs from this one's in the last bits, and with the device's d fed back every
        elementwise result can be compared bitwise."""
        lr, (beta1, beta2), beta3, d, d0 = self.lr, self.betas, self.beta3, self.d, self.d0
        if lr == 0:
            return
        bc = 1.0
        if self.use_bias_correction:
            bc = math.sqrt(1 - beta2 ** (self.k + 1)) / (1 - beta1 ** (self.k + 1))
        dlr = d * lr * bc if override is None else override[1]
        wd = self.weight_decay
        num = den = 0.0
        todo = []
        for p, grad in zip(self.params, grads):
            if grad is None:
                continue
            st = self._state(p)
            # R(grad * coef) with the f32 coefficient (grad * coef itself would first round coef to bf16)
            g = grad if coef is None else (grad.float() * coef.to(grad.device)).to(grad.dtype)
            assert g.dtype == p.dtype
            if wd != 0 and not self.decouple:
                g = g.add(p, alpha=wd)
            diff = st["p0"] - p
            # the f32 product of the two rounded factors, added in f64 (for f64 tensors, an f64 product)
            prod = diff.float() * g.float() if p.dtype == torch.bfloat16 else diff * g
            num += float(prod.double().sum())
            st["exp_avg"].mul_(beta1).add_(g, alpha=d * (1 - beta1))
            st["exp_avg_sq"].mul_(beta2).addcmul_(g, g, value=d * d * (1 - beta2))
            st["s"].mul_(beta3).add_(g, alpha=(d / d0) * (d if self.safeguard_warmup else dlr))
            den += float(st["s"].abs().double().sum())
            todo.append((p, st))
        self.dlr, self.d_denom = dlr, den
        if den == 0:
            self.applied = False
            return
        self.applied = True
        self.d_numerator = beta3 * self.d_numerator + (d / d0) * dlr * num
        self.d_hat = self.d_coef * self.d_numerator / den
        if d == d0:
            d = max(d, self.d_hat)
        self.d_max = max(self.d_max, self.d_hat)
        self.d = min(self.d_max, d * self.growth_rate)
        self.k += 1
        if override is not None:
            self.d = override[0]
        for p, st in todo:
            denom = st["exp_avg_sq"].sqrt().add_(self.d * self.eps)
            if wd != 0 and self.decouple:
                p.add_(p, alpha=-wd * dlr)
            p.addcdiv_(st["exp_avg"], denom, value=-dlr)
