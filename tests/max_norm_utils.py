"""The statement of the max-norm pass (FusedAdamW / FusedProdigy(scale_weight_norms=c)) in numpy, f64, and the
fixtures its tests share. This file is the specification; csrc/max_norm.hip and DESIGN.md "Max-norm
(scale_weight_norms)" follow it.

The rule is kohya's apply_max_norm_regularization (sd-scripts, networks/lora.py, --scale_weight_norms), restated
from the published code: for every adapter pair (A f32 [r, K], B f32 [N, r], s = lora_alpha / r) and one cap
c > 0

    norm  = |s| * ||B A||_F                        f64
    ratio = 1 if norm <= c else c / norm           f64
    f     = float32(sqrt(ratio))
    if ratio != 1:  A <- fl32(A * f),  B <- fl32(B * f)     one f32 multiply per element, as torch's `*=`
    scaled_norm = norm * ratio

and the step's record is (keys_scaled = the pairs with ratio != 1, the mean and the maximum of scaled_norm).
kohya's norm.clamp(min=c / 2) never changes the ratio (a norm under c / 2 gives 1 either way), so it is not
part of the statement; kohya_loop below keeps it and test_max_norm_cpu.py compares the two."""
import numpy as np
import torch


def norm_direct(A, B, s):
    """|s| ||B A||_F with the product formed, all in f64"""
    P = np.asarray(B, dtype=np.float64) @ np.asarray(A, dtype=np.float64)
    return abs(float(s)) * np.sqrt(np.sum(P * P))


def sumsq_direct(A, B):
    P = np.asarray(B, dtype=np.float64) @ np.asarray(A, dtype=np.float64)
    return np.sum(P * P)


def norm_gram(A, B, s, dtype=np.float64):
    """The same norm without the product: ||B A||_F^2 = sum_ij (B^T B)_ij (A A^T)_ij, the Gram matrices and
    their contraction in `dtype` (f64: what the device computes; f32: what it must not; a sum that cancels
    below zero counts as zero)"""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    ga, gb = A @ A.T, B.T @ B
    return abs(float(s)) * np.sqrt(max(np.float64(np.sum(ga * gb, dtype=dtype)), 0.0))


def statement(pairs, cap):
    """pairs: [(A f32 [r, K], B f32 [N, r], s)] as numpy arrays. Returns a dict of per-pair lists `norm`, `ratio`
    (f64), `f` (np.float32), `scaled_norm` (f64), `A`, `B` (the f32 arrays after the rule; the inputs themselves
    where ratio == 1) and the record `keys_scaled`, `avg_key_norm`, `max_key_norm` (f64)."""
    cap = float(cap)
    assert cap > 0
    out = {k: [] for k in ("norm", "ratio", "f", "scaled_norm", "A", "B")}
    for A, B, s in pairs:
        assert A.dtype == np.float32 and B.dtype == np.float32 and A.shape[0] == B.shape[1]
        norm = norm_direct(A, B, s)
        ratio = 1.0 if norm <= cap else cap / norm
        f = np.float32(np.sqrt(np.float64(ratio)))
        if ratio != 1.0:
            A, B = A * f, B * f  # f32 * f32 -> f32, one rounding per element
        out["norm"].append(norm)
        out["ratio"].append(ratio)
        out["f"].append(f)
        out["scaled_norm"].append(norm * ratio)
        out["A"].append(A)
        out["B"].append(B)
    out["keys_scaled"] = sum(r != 1.0 for r in out["ratio"])
    out["avg_key_norm"] = float(np.mean(np.asarray(out["scaled_norm"], dtype=np.float64)))
    out["max_key_norm"] = float(np.max(np.asarray(out["scaled_norm"], dtype=np.float64)))
    return out


def kohya_loop(pairs, max_norm_value):
    """A literal torch transcription of the linear branch of kohya's apply_max_norm_regularization over
    `pairs` = [(down f32 [r, K], up f32 [N, r], alpha)] (torch tensors, scaled in place), clamp included.
    The product and its norm are taken on f64 copies, so that the comparison with the statement is about the
    rule and not about an f32 matmul's error; the weights stay f32 and are scaled by torch's `*=` with the
    0-dim ratio ** 0.5, as there. Returns (keys_scaled, mean of the scaled norms, their maximum, the list of
    per-pair (scaled or not, float32(sqrt_ratio)))."""
    norms, decisions, keys_scaled = [], [], 0
    for down, up, alpha in pairs:
        dim = down.shape[0]
        scale = alpha / dim
        updown = up.double() @ down.double()
        updown *= scale
        norm = updown.norm().clamp(min=max_norm_value / 2)
        desired = torch.clamp(norm, max=max_norm_value)
        ratio = desired.cpu() / norm.cpu()
        sqrt_ratio = ratio ** 0.5
        if ratio != 1:
            keys_scaled += 1
            up *= sqrt_ratio
            down *= sqrt_ratio
        decisions.append((bool(ratio != 1), np.float32(float(sqrt_ratio))))
        scalednorm = updown.norm() * ratio
        norms.append(scalednorm.item())
    return keys_scaled, sum(norms) / len(norms), max(norms), decisions


# ---- fixtures ----------------------------------------------------------------------------------------
def random_pair(N, K, r, seed, scale=1.0):
    g = np.random.default_rng(seed)
    A = (g.standard_normal((r, K)) / np.sqrt(K)).astype(np.float32)
    B = (scale * g.standard_normal((N, r)) / np.sqrt(r)).astype(np.float32)
    return A, B


def adversarial_pair(N, K, r, seed):
    """The pair on which an f32 Gram form fails: every row of A is one vector a0 plus 1e-3 of noise, so A A^T
    is all but rank one, and the rows (over r) of B are mean-centred, so B^T B all but annihilates it: the
    contraction cancels to ~1e-6 of its terms."""
    g = np.random.default_rng(seed)
    a0 = g.standard_normal(K)
    A = (a0[None, :] + 1e-3 * g.standard_normal((r, K))).astype(np.float32)
    B = g.standard_normal((N, r))
    B = (B - B.mean(axis=1, keepdims=True)).astype(np.float32)
    return A, B


def exact_pair(N, K, r, seed):
    """Entries that are small integers times a power of two: A in {-3 .. 3} / 4, B in {-3 .. 3} / 2. Every Gram
    entry, every product of two and every partial sum of either form is then an integer multiple of 2^-6 below
    2^53 of them (up to N, K = 8192, r = 128: |G_A| <= 9 K / 16, |G_B| <= 9 N / 4, r^2 products, two of each
    off the diagonal), so any summation order gives the same f64 and the Gram form equals the direct one."""
    g = np.random.default_rng(seed)
    A = (g.integers(-3, 4, size=(r, K)) / 4.0).astype(np.float32)
    B = (g.integers(-3, 4, size=(N, r)) / 2.0).astype(np.float32)
    return A, B


def pair_with_norm(N, K, r, s, target, seed):
    """A random pair rescaled (B only) so that its statement norm is `target` to f32 rounding; target 0: B = 0."""
    A, B = random_pair(N, K, r, seed)
    if target == 0:
        return A, np.zeros_like(B)
    B = (B * (target / norm_direct(A, B, s))).astype(np.float32)
    return A, B


def ulps_f32(a, b):
    """distance in units in the last place between two positive finite float32 values"""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))
