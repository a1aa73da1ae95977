"""Shared by tests/test_norm_truth_cpu.py and tests/test_norm_truth_gpu.py: inputs whose f32 row
sums are exact in any order, float64 emulators of the row-normalisation kernels (csrc/norms.hip) and
of the train_mode='full' reductions (csrc/paramgrad.hip, batch_sum), the element-by-element
comparator and the case table of the GPU file.

An emulator computes in float64 and rounds to bf16 where the reference's eager bf16 op sequence
does (oracle/ltx_oracle.py; tests/test_norm_truth_cpu.py holds the emulators to those ops). A value
it rounds is an interval (Iv): the rounding of the float64 value, and the roundings of the value
moved down and up by the slack of the f32 arithmetic behind it (relative 2^-19 after rsqrtf, r^3,
dvar / D, expf; absolute 2^-21 on a cos / sin; none on products and sums of bf16 values, which f32
holds exactly). Rounding, adding and multiplying by an exact value are monotone, so the interval
is carried to the output: an element whose two ends agree there is closed and the kernel must
return it bit for bit; one whose ends differ is open and must lie within 2 bf16 ulps. At most 2 %
of an output may be open (build() refuses the case otherwise).
"""
import collections
import functools
import math
import types

import torch

S19 = 2.0 ** -19      # relative slack on a value behind rsqrtf / r^3 / dvar / D / expf (32 f32 ulps)
TRIG = 2.0 ** -21     # absolute slack on a cos / sin of the f32 phase
STAT = 2.0 ** -21     # rstd and mean against float64 (three f32 roundings and a 1-ulp rsqrtf)
OPEN_ULPS = 2
OPEN_CAP = 0.02
EXACT = 2.0 ** 24
# max_pos of the t axis is 21, not the model's 20: with 20 an integer t gives fractions that are
# multiples of 0.1, the frequencies theta^(k/20) pi/2 hold every decade, and 5 % of the phases land on
# a multiple of pi/2 up to the f32 rounding, where the absolute 2^-21 on a sin of 1e-7 opens the element
THETA, MAX_POS = 10000.0, (21, 2048, 2048)
BF16 = torch.bfloat16


def bf(t):
    """float64 -> f32 -> bf16 -> float64, the two roundings of a kernel's rbf(f32 expression)"""
    return t.float().bfloat16().double()


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


class Iv:
    """value v with the ends lo <= hi it may take in a correct kernel (float64 tensors)"""
    __slots__ = ("v", "lo", "hi")

    def __init__(self, v, lo=None, hi=None):
        self.v, self.lo, self.hi = v, v if lo is None else lo, v if hi is None else hi

    @property
    def open(self):
        return self.lo != self.hi

    def __getitem__(self, i):
        return Iv(self.v[i], self.lo[i], self.hi[i])

    def map(self, fn):
        return Iv(fn(self.v), fn(self.lo), fn(self.hi))


def iv(a):
    return a if isinstance(a, Iv) else Iv(a)


def mul(a, t):
    """a (Iv) times the exact tensor t"""
    a = iv(a)
    p, q = a.lo * t, a.hi * t
    return Iv(a.v * t, torch.minimum(p, q), torch.maximum(p, q))


def add(a, b):
    a, b = iv(a), iv(b)
    return Iv(a.v + b.v, a.lo + b.lo, a.hi + b.hi)


def neg(a):
    a = iv(a)
    return Iv(-a.v, -a.hi, -a.lo)


def rb(a, rel=0.0, ab=0.0):
    """round to bf16; rel / ab: the slack of the f32 value being rounded"""
    a = iv(a)
    return Iv(bf(a.v), bf(a.lo - (a.lo.abs() * rel + ab)), bf(a.hi + (a.hi.abs() * rel + ab)))


def colsum_iv(a, dim=0):
    return a.map(lambda t: t.sum(dim))


def spacing(t):
    """the weight of the lowest set bit of every element (inf for 0): what an exact f32 sum of such
    terms must resolve"""
    m, e = torch.frexp(t.double())
    mant = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mant & -mant).double()
    return torch.where(mant == 0, torch.full_like(low, float("inf")), torch.ldexp(low, e - 53))


def sum_steps(terms, dim=-1):
    """sum |term| / grid along dim, grid the smallest spacing of a term there: under 2^24 every
    partial sum, in any order, is an f32 value and the f32 sum is exact"""
    q = spacing(terms).amin(dim)
    s = terms.abs().sum(dim)
    return torch.where(s == 0, torch.zeros_like(s), s / q)


class Refused(AssertionError):
    pass


STRICT = [True]


class any_inputs:
    """with any_inputs(): the emulators run on inputs whose sums are not exact (randn): what the
    planted-fault table needs of them is a value, not a truth"""

    def __enter__(self):
        STRICT[0] = False

    def __exit__(self, *exc):
        STRICT[0] = True


def exact_sum(name, terms, dim=-1, log=None):
    """terms.sum(dim) after asserting that it is exact in f32 in any order"""
    steps = float(sum_steps(terms, dim).max())
    if log is not None:
        log[name] = max(log.get(name, 0.0), steps)
    if STRICT[0] and not steps < EXACT:
        raise Refused("%s: sum |term| / grid = 2^%.1f, not exact in f32" % (name, math.log2(steps)))
    return terms.sum(dim)


def graded_sum(name, terms, dim=-1, log=None):
    """a sum whose terms' spacing the inputs do not control (a bf16 product with a RoPE table entry
    or with bf16(x * rstd) can be arbitrarily small): (sum, absolute slack), the slack 0 where the
    sum is exact and 2^-19 sum |term| where it is not (a 64-lane tree over at most 32 serial adds is
    within 38 x 2^-24 of that)"""
    steps = sum_steps(terms, dim)
    if log is not None:
        log[name + " inexact share"] = max(log.get(name + " inexact share", 0.0), float((steps >= EXACT).double().mean()))
    return terms.sum(dim), torch.where(steps < EXACT, 0.0, S19) * terms.abs().sum(dim)


# ------------------------------------------------------------------------------------- emulators
def _batch_of(M, rpb, fault):
    m = torch.arange(M)
    if fault == "b_first_row":
        m = m // 4 * 4
    return m // (rpb if rpb > 0 else M)


def _ss(xd, fault, log):
    D = xd.shape[1]
    ss = exact_sum("sum x^2", xd * xd, log=log)
    if fault == "clamped_chunk":  # the chunks past D, clamped onto the last 8 elements, summed too
        ss = ss + (256 - D // 8) * (xd[:, D - 8:] ** 2).sum(-1)
    return ss


def rms_fwd(x, shift, onep, rpb, eps, fault=None, log=None):
    """y = bf16(bf16(n * onep[b]) + shift[b]), n = bf16(x * rstd): (y Iv, rstd float64)"""
    M, D = x.shape
    xd = x.double()
    r = (_ss(xd, fault, log) / D + f32(eps)).rsqrt()
    b = _batch_of(M, rpb, fault)
    n = Iv(xd * r[:, None]) if fault == "n_unrounded" else rb(Iv(xd * r[:, None]), S19)
    return rb(add(rb(mul(n, onep.double()[b])), shift.double()[b])), r


def _rms_bwd_core(g, xd, r, fault, log, graded=False):
    """dx1 + dx2 of the RMSNorm backward from the f32 gradient g at the norm output"""
    D = xd.shape[1]
    if graded:
        dr, slack = graded_sum("sum g x", g * xd, log=log)
    else:
        dr, slack = exact_sum("sum g x", g * xd, log=log), 0.0
    k = (-0.5 * r ** 3 / D)[:, None] * (2.0 * xd)
    p = dr[:, None] * k
    dx1 = rb(Iv(g * r[:, None]), S19)
    lo, hi = p - slack[:, None] * k.abs() if graded else p, p + slack[:, None] * k.abs() if graded else p
    dx2 = Iv(p) if fault == "dx2_unrounded" else rb(Iv(p, lo, hi), S19)
    return dx1, dx2


def rms_bwd(dy, x, r, onep, rpb, dres=None, gate=None, fault=None, log=None):
    """dx = bf16(dres + bf16(dx1 + dx2)) (dx, gout or None); r: the float64 rstd"""
    M, D = x.shape
    b = _batch_of(M, rpb, fault)
    g = bf(dy.double() * onep.double()[b])
    dx1, dx2 = _rms_bwd_core(g, x.double(), r, fault, log)
    d = rb(add(dx1, dx2))
    raw = add(dres.double(), d) if dres is not None else d
    dx = rb(raw)
    gout = None
    if gate is not None:
        gout = rb(mul(raw if fault == "gout_unrounded_dx" else dx, gate.double()[b]))
    return dx, gout


def ln_stats(x, eps, log=None):
    xd = x.double()
    D = xd.shape[1]
    mean = exact_sum("sum x", xd, log=log) / D
    xc = xd - mean[:, None]
    r = (exact_sum("sum (x-mean)^2", xc * xc, log=log) / D + f32(eps)).rsqrt()
    return mean, r, xc


def ln_fwd(x, shift, onep, rpb, eps, fault=None, log=None):
    """(y Iv, mean, rstd)"""
    M, D = x.shape
    mean, r, xc = ln_stats(x, eps, log)
    b = _batch_of(M, rpb, fault)
    xh = Iv(xc * r[:, None]) if fault == "n_unrounded" else rb(Iv(xc * r[:, None]), S19)
    return rb(add(rb(mul(xh, onep.double()[b])), shift.double()[b])), mean, r


def ln_bwd(dy, x, mean, r, onep, rpb, fault=None, log=None):
    """dx = bf16(r (g - mean(g) - xhat mean(g xhat))), one rounding. xhat and g xhat are f32 values
    with roundings of their own, so the slack is absolute: 2^-19 of the magnitudes that enter,
    r (|g| + |mean g| + |xhat| mean |g xhat|), not of the (cancelling) result."""
    M, D = x.shape
    b = _batch_of(M, rpb, fault)
    g = bf(dy.double() * onep.double()[b])
    xh = (x.double() - mean[:, None]) * r[:, None]
    mg = exact_sum("sum g", g, log=log) / D
    mgx = (g * xh).sum(-1) / D
    mag = (g * xh).abs().sum(-1) / D
    p = r[:, None] * (g - mg[:, None] - xh * mgx[:, None])
    return rb(Iv(p), ab=S19 * r[:, None] * (g.abs() + mg.abs()[:, None] + xh.abs() * mag[:, None]))


def rope_t(g, cos, sin):
    """RoPE^T of the bf16 gradient g (exact: products and sums of bf16 values):
    dn[2i] = bf16(bf16(g0 c) + bf16(g1 s)), dn[2i+1] = bf16(bf16(g1 c) - bf16(g0 s))"""
    da, dr = bf(g * cos), bf(g * sin)
    dn = torch.empty_like(g)
    dn[:, 0::2] = bf(da[:, 0::2] + dr[:, 1::2])
    dn[:, 1::2] = bf(da[:, 1::2] - dr[:, 0::2])
    return dn


def qk_fwd(x, w, cos=None, sin=None, eps=1e-5, fault=None, log=None):
    """out = rope(bf16(bf16(x rstd) w)); cos / sin: exact float64 [M, D] (the table the kernel
    reads) or None. (out Iv, rstd)"""
    M, D = x.shape
    xd = x.double()
    r = (_ss(xd, fault, log) / D + f32(eps)).rsqrt()
    n = Iv(xd * r[:, None]) if fault == "n_unrounded" else rb(Iv(xd * r[:, None]), S19)
    nw = rb(mul(n, w.double()[None]))
    if cos is None:
        return nw, r
    if fault == "pad_at_end":
        pad = D % 6
        cos, sin = torch.roll(cos, -pad, 1), torch.roll(sin, -pad, 1)
    if fault == "neighbour_row":
        cos, sin = torch.roll(cos, 1, 0), torch.roll(sin, 1, 0)

    def rot(t):
        o = torch.empty_like(t)
        o[:, 0::2], o[:, 1::2] = -t[:, 1::2], t[:, 0::2]
        return o
    rt = Iv(rot(nw.v), torch.minimum(rot(nw.lo), rot(nw.hi)), torch.maximum(rot(nw.lo), rot(nw.hi)))
    return rb(add(rb(mul(nw, cos)), rb(mul(rt, sin)))), r


def qk_bwd(g_in, x, w, r, cos=None, sin=None, fault=None, log=None):
    """dx of qk_fwd from the incoming gradient (bf16, or f32 rounded to bf16 first)"""
    g = bf(g_in.double())
    if cos is not None:
        if fault == "neighbour_row":
            cos, sin = torch.roll(cos, 1, 0), torch.roll(sin, 1, 0)
        g = rope_t(g, cos, sin)
    gx = bf(g * w.double()[None])
    dx1, dx2 = _rms_bwd_core(gx, x.double(), r, fault, log, graded=cos is not None)
    return rb(add(dx1, dx2))


def splits(rows, groups):
    """ops._splits"""
    return max(1, min(max(1, min(rows // 8, 512 // max(1, groups))), rows))


def finish(part, sum_groups, accumulate, out0, fault=None):
    """colsum_finish on part (Iv [G, D], the exact per-group sums): bf16 per group, then over the
    groups, then onto out0"""
    per = part if fault == "no_group_rbf" else rb(part)
    tot = rb(colsum_iv(per, 0)) if sum_groups else per
    return rb(add(out0.double(), tot)) if accumulate else tot


def _col_sums(name, t, G, rpg, log, drop_last=0):
    """Iv [G*rpg, D] -> Iv [G, D]; a column whose sum is not exact in f32 takes the absolute slack of
    graded_sum. drop_last: the split count of the planted fault that loses each split's last row."""
    D = t.v.shape[1]
    keep = torch.ones(rpg, dtype=torch.bool)
    if drop_last:
        keep[[(s + 1) * rpg // drop_last - 1 for s in range(drop_last)]] = False
    v3 = t.map(lambda u: u.view(G, rpg, D)[:, keep])
    _, slack = graded_sum(name, v3.v, 1, log)
    s = colsum_iv(v3, 1)
    return Iv(s.v, s.lo - slack, s.hi + slack)


def wgrad(g_in, x, r32, g0, cos=None, sin=None, fault=None, log=None):
    """gq = bf16(g0 + bf16(sum_rows bf16(dn bf16(x rstd)))); r32: the f32 rstd the kernel reads"""
    M, D = x.shape
    g = bf(g_in.double())
    dn = rope_t(g, cos, sin) if cos is not None else g
    n = rb(Iv(x.double() * r32.double()[:, None]), S19)
    S = splits(M, 1)
    part = _col_sums("wgrad rows", rb(mul(n, dn)), 1, M, log, S if fault == "split_drops_last_row" else 0)
    return finish(part, True, True, g0)


def colsum(a, b=None, r32=None, mean32=None, mode=0, rpg=None, sum_groups=True, accumulate=True, out0=None,
           fault=None, log=None):
    """ops.colsum_into"""
    M, D = a.shape
    rpg = M if rpg is None else rpg
    G = M // rpg
    ad = a.double()
    if mode == 0:
        t = Iv(ad)
    elif mode == 1:
        t = Iv(bf(ad * b.double()))
    else:
        c = b.double() - (mean32.double()[:, None] if mode == 3 else 0.0)
        t = rb(mul(rb(Iv(c * r32.double()[:, None]), S19), ad))
    part = _col_sums("colsum rows", t, G, rpg, log)
    return finish(part, sum_groups, accumulate, out0, fault)


def silu_bwd(x, dy, dres=None):
    xd, g = x.double(), dy.double()
    s = torch.sigmoid(xd)
    d = rb(Iv(g * (s * (1.0 + xd * (1.0 - s)))), S19)
    return rb(add(dres.double(), d)) if dres is not None else d


def batch_sum(x, B, log=None):
    rows = x.shape[0] // B
    return Iv(bf(exact_sum("batch sum", x.double().view(B, rows, -1), 0, log)))


def rope_omega(D):
    idx = THETA ** torch.linspace(math.log(1, THETA), math.log(THETA, THETA), D // 6, dtype=torch.float32)
    return idx.to(torch.float32) * math.pi / 2


def rope_table(grid, D):
    """(cos, sin) Iv [B*N, D] of the grid [B, 3, N] (int64 or f32): the phase in f32 exactly as
    RopeSpec / ltx_rope_table and the reference build it, its cos and sin in float64 +- 2^-21; the
    D % 6 leading elements are (1, 0)"""
    Bt, _, N = grid.shape
    pad = D % 6
    fr = torch.stack([(grid[:, a].to(torch.float32) / torch.tensor(float(MAX_POS[a]), dtype=torch.float32)) * 2.0
                      - 1.0 for a in range(3)], -1)                       # [B, N, 3] f32
    phi = (rope_omega(D)[None, None, :, None] * fr[:, :, None, :]).double().reshape(Bt * N, -1)
    c = torch.cat([torch.ones(Bt * N, pad // 2, dtype=torch.float64), phi.cos()], 1).repeat_interleave(2, 1)
    s = torch.cat([torch.zeros(Bt * N, pad // 2, dtype=torch.float64), phi.sin()], 1).repeat_interleave(2, 1)
    # no slack on the pad, nor where the phase is exactly 0 (a position in the middle of its axis):
    # cos 0 = 1 and sin 0 = 0 are exact in any sincosf
    slack = torch.cat([torch.zeros(Bt * N, pad // 2, dtype=torch.float64), torch.where(phi == 0, 0.0, TRIG)],
                      1).repeat_interleave(2, 1)
    return rb(Iv(c), ab=slack), rb(Iv(s), ab=slack)


def unpack_cs(cs, rows):
    """the packed table words (int32 [table rows, D/2]) as float64 (cos, sin) [len(rows), D]"""
    wds = cs.cpu()[rows].to(torch.int64) & 0xFFFFFFFF
    one = lambda u: (u - ((u & 0x8000) << 1)).to(torch.int16).view(BF16).double().repeat_interleave(2, 1)  # noqa: E731
    return one(wds & 0xFFFF), one(wds >> 16)


def pack_words(cos, sin):
    """bf16 [rows, D] (cos, sin), each value repeated for its pair -> the int64 words of the table"""
    u = lambda t: t[:, 0::2].contiguous().view(torch.int16).to(torch.int64) & 0xFFFF  # noqa: E731
    return u(cos) | (u(sin) << 16)


# ------------------------------------------------------------------------------------ comparator
def _ordered(t16):
    i = t16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulp_dist(a16, b16):
    return (_ordered(a16) - _ordered(b16)).abs()


def open_share(want):
    return float(want.open.double().mean())


def assert_truth(name, got, want, cap=OPEN_CAP):
    """got (bf16) against the emulator's Iv: closed elements bit for bit (the sign of zero ignored),
    open ones within 2 bf16 ulps, at most cap of them open. Returns (open share, open elements that
    differ, the largest ulp distance)."""
    got = got.detach().cpu()
    assert got.dtype == BF16 and got.shape == want.v.shape, (name, got.dtype, got.shape, want.v.shape)
    opn = want.open
    share = float(opn.double().mean())
    assert share <= cap, "%s: %.2f %% of the elements are open (cap %.0f %%)" % (name, 100 * share, 100 * cap)
    dist = ulp_dist(got, want.v.bfloat16())
    bad = torch.where(opn, dist > OPEN_ULPS, ~(got.double() == want.v))
    if bad.any():
        idx = bad.nonzero()
        vals = ["%s got %r want %r%s" % (tuple(int(v) for v in i), float(got[tuple(i)]), float(want.v[tuple(i)]),
                                         " (open)" if bool(opn[tuple(i)]) else "") for i in idx[:6]]
        raise AssertionError("%s: %d of %d elements differ from the emulator (%d closed); rows %s; first: %s"
                             % (name, len(idx), bad.numel(), int((bad & ~opn).sum()),
                                sorted(set(idx[:, 0].tolist()))[:12], "; ".join(vals)))
    return share, int((opn & (dist > 0)).sum()), int(dist.max())


def stat_err(got, want64):
    """largest |got - want| / |want| of an f32 statistic (0 must be returned as 0)"""
    g, w = got.detach().cpu().double().reshape(-1), want64.reshape(-1)
    assert bool((g[w == 0] == 0).all())
    nz = w != 0
    return float(((g[nz] - w[nz]).abs() / w[nz].abs()).max()) if nz.any() else 0.0


def assert_stat(name, got, want64, bound=STAT):
    e = stat_err(got, want64)
    assert e <= bound, "%s: relative error %.3g (2^%.1f) over %.3g" % (name, e, math.log2(max(e, 1e-300)), bound)
    return e


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def ulps_bad(a, b, max_ulp=1):
    """tests/test_kernels_gpu.py's criterion: the fraction of bf16 entries more than max_ulp apart"""
    ai = a.contiguous().view(torch.int16).to(torch.int32)
    bi = b.contiguous().view(torch.int16).to(torch.int32)
    return float(((ai - bi).abs() > max_ulp).float().mean())


# --------------------------------------------------------------------------------------- builder
ROW_A, ROW_B = 5, 10          # in every (3, 7) case: batch 0 and batch 1, both inside a 4-row block


def known_rows(M):
    return (ROW_A, ROW_B) if M > ROW_B else (1, 2)


def twins(D):
    """column pairs (e, e + 2) that share a RoPE (cos, sin) on a token whose h and w coordinates
    are equal: the pairs of axes 1 and 2 of every frequency. Row B's construction lives on them."""
    pad = D % 6
    e = torch.arange(D // 6)[:, None] * 6 + pad + 2 + torch.arange(2)[None]
    return e.reshape(-1)


def grid_vals(shape, gen, nonzero):
    t = torch.randint(-7, 8, shape, generator=gen).double() / 4
    return torch.where(t == 0, torch.full_like(t, 0.25), t) if nonzero else t


def generic_bf16(shape, gen):
    """bf16 values with a random 8-bit significand, magnitude in [0.5, 2), random sign"""
    m = (128 + torch.randint(0, 128, shape, generator=gen)).double() / 128
    e = torch.randint(-1, 1, shape, generator=gen).double()
    s = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (s * m * 2.0 ** e).bfloat16()


def _known_rows(x, g, M, D, gen, dup, mean0=False):
    """rows A and B into x and the gradient g (float64, in place). A: x = +-1. B: x = +-1 and the
    gradient only on the twin columns, equal on a column and its twin where x is opposite: with the
    per-column factor (onep, the norm weight, the RoPE table entry) duplicated on the twins (dup
    does that) the sum of g x cancels pair by pair. mean0: as many +1 as -1 (LayerNorm)."""
    a, b_ = known_rows(M)
    tw = twins(D)
    for row in (a, b_):
        s = (torch.randint(0, 2, (D,), generator=gen) * 2 - 1).double()
        if mean0:
            s = torch.ones(D, dtype=torch.float64)
            s[torch.randperm(D, generator=gen)[:D // 2]] = -1.0
        x[row] = s
    x[b_, tw + 2] = -x[b_, tw]
    if mean0:  # the twins cancel; balance the remaining columns
        rest = torch.ones(D, dtype=torch.bool)
        rest[tw], rest[tw + 2] = False, False
        idx = rest.nonzero()[:, 0]
        x[b_, idx] = 1.0
        x[b_, idx[torch.randperm(len(idx), generator=gen)[:len(idx) // 2]]] = -1.0
    g[b_] = 0.0
    g[b_, tw] = grid_vals((len(tw),), gen, True)
    g[b_, tw + 2] = g[b_, tw]
    dup(tw)
    return a, b_


def _balance(x):
    """LayerNorm rows: move elements by 1/4 until the row sum is a multiple of D/4 (the mean is then
    on the 1/4 grid and x - mean is exact)"""
    D = x.shape[1]
    for row in x:
        k = int(round(float(row.sum() * 4))) % D
        step, need = (-0.25, k) if k <= D // 2 else (0.25, D - k)
        while need:
            ok = ((row + step).abs() <= 1.75) & ((row + step) != 0)
            idx = ok.nonzero()[:need, 0]
            assert len(idx)
            row[idx] += step
            need -= len(idx)
    assert bool(((x.sum(1) * 4) % D == 0).all())


def _seeded(fn):
    """fn(seed) with the first of 8 seeds whose case is not refused (an inexact sum, over 2 % open)"""
    @functools.lru_cache(maxsize=None)
    def build(*key):
        err = None
        for seed in range(8):
            try:
                c = fn(*key, seed=1000 * seed + 7)
                c.seed = seed
                return c
            except Refused as e:
                err = e
        raise err
    return build


def _cap(c, **outs):
    c.open = {n: open_share(w) for n, w in outs.items()}
    for n, s in c.open.items():
        if s > OPEN_CAP:
            raise Refused("%s: %.2f %% open" % (n, 100 * s))


@_seeded
def mod_case(kind, D, B, N, rpb, seed=0):
    """RMSNorm / LayerNorm + modulate (kind 'rms' / 'ln'): x, dy, dres [M, D] on the grid, mod
    [Bm, 6, D] generic bf16 whose rows 0, 1 and 5 are shift, 1 + scale and the gate (views with
    ld_mod = 6 D), and the emulated outputs. rpb = 0: one modulation row for all M rows."""
    gen = torch.Generator().manual_seed(seed + D)
    M, Bm = B * N, (B if rpb > 0 else 1)
    c = types.SimpleNamespace(kind=kind, D=D, B=B, N=N, M=M, rpb=rpb, eps=1e-6, log={})
    x, dy = grid_vals((M, D), gen, True), grid_vals((M, D), gen, False)
    mod = generic_bf16((Bm, 6, D), gen)

    def dup(tw):
        mod[:, :, tw + 2] = mod[:, :, tw]
    if kind == "ln":  # means of -1/2 ... 1/2, one per row
        x += ((torch.arange(M) % 5 - 2).double() / 4)[:, None]
        x.clamp_(-1.75, 1.75)
        x[x == 0] = 0.25
        _balance(x)
    c.row_a, c.row_b = _known_rows(x, dy, M, D, gen, dup, mean0=kind == "ln")
    c.x, c.dy, c.mod = x.bfloat16(), dy.bfloat16(), mod
    c.dres = grid_vals((M, D), gen, False).bfloat16()
    assert torch.equal(c.x.double(), x) and torch.equal(c.dy.double(), dy)
    shift, onep, gate = mod[:, 0], mod[:, 1], mod[:, 5]
    if kind == "rms":
        c.y, c.r = rms_fwd(c.x, shift, onep, rpb, c.eps, log=c.log)
        c.dx, _ = rms_bwd(c.dy, c.x, c.r, onep, rpb, dres=c.dres, log=c.log)
        c.dx_g, c.gout = rms_bwd(c.dy, c.x, c.r, onep, rpb, gate=gate, log=c.log)
        _cap(c, y=c.y, dx=c.dx, dx_g=c.dx_g, gout=c.gout)
    else:
        c.y, c.mean, c.r = ln_fwd(c.x, shift, onep, rpb, c.eps, log=c.log)
        c.dx = ln_bwd(c.dy, c.x, c.mean, c.r, onep, rpb, log=c.log)
        _cap(c, y=c.y, dx=c.dx)
    check_known_rows(c)
    return c


def check_known_rows(c):
    """rows A and B are what section 4 says: sum x^2 / D = 1, n = x, nothing of row A's forward
    open; on row B sum g x = 0 and (RMSNorm) dx2 = 0, so dx = bf16(g rstd) [+ dres]"""
    xa, xb = c.x.double()[c.row_a], c.x.double()[c.row_b]
    assert float((xa * xa).mean()) == 1.0 and float((xb * xb).mean()) == 1.0
    assert abs(float(c.r[c.row_a]) - (1 - 0.5 * c.eps)) < 1e-9
    assert bf(xa * c.r[c.row_a]).equal(xa)
    assert not bool(c.y.open[c.row_a].any()) and not bool(c.y.open[c.row_b].any())
    b = int(_batch_of(c.M, c.rpb, None)[c.row_b]) if hasattr(c, "rpb") else None
    if c.kind in ("rms", "ln"):
        g = bf(c.dy.double()[c.row_b] * c.mod[b, 1].double())
        assert float((g * xb).sum()) == 0.0 and float((g * xb).abs().sum()) > 0
    if c.kind == "rms":
        want = bf(c.dres.double()[c.row_b] + bf(bf(g * c.r[c.row_b])))
        assert c.dx.v[c.row_b].equal(want)


def coords(B, N, gen, is_float, shared):
    """[B, 3, N] (t, h, w) positions over the whole of max_pos, so that the phases spread and few
    cos / sin are small enough for the absolute 2^-21 to span a bf16 boundary; row B's token has h = w. is_float: fractional pixel-space
    positions; shared: a batch-broadcast view of one batch"""
    Bt = 1 if shared else B
    g = torch.stack([torch.randint(0, MAX_POS[0], (Bt, N), generator=gen), torch.randint(0, MAX_POS[1], (Bt, N), generator=gen),
                     torch.randint(0, MAX_POS[2], (Bt, N), generator=gen)], 1)
    tok = known_rows(B * N)[1] % N
    g[:, 2, tok] = g[:, 1, tok]
    if is_float:
        g = g.float() * torch.tensor([8.0, 32.0, 32.0]).view(1, 3, 1) / 25.0
    return g.expand(B, -1, -1) if shared else g


@_seeded
def qk_case(D, B, N, has_k, rope, is_float, shared, seed=0):
    """q (and k) [M, D] on the grid, generic norm weights, incoming gradients on the grid and the
    position grid. The emulated outputs need the table the kernels read: emulate(c, cos, sin)."""
    gen = torch.Generator().manual_seed(seed + 3 * D)
    M = B * N
    c = types.SimpleNamespace(kind="qk", D=D, B=B, N=N, M=M, has_k=has_k, rope=rope, eps=1e-5, log={})
    c.grid = coords(B, N, gen, is_float, shared) if rope else None
    c.x, c.g, c.w = [], [], []
    for _ in range(2 if has_k else 1):
        x, g = grid_vals((M, D), gen, True), grid_vals((M, D), gen, False)
        w = generic_bf16((D,), gen)

        def dup(tw):
            w[tw + 2] = w[tw]
        c.row_a, c.row_b = _known_rows(x, g, M, D, gen, dup)
        c.x.append(x.bfloat16()), c.g.append(g.bfloat16()), c.w.append(w)
    # the cap, on the emulated table (the launch is emulated again under the table words it read)
    tab = ()
    if rope:
        bt = 1 if shared else B
        c.table = rope_table(c.grid[:bt].contiguous(), D)
        _cap(c, cos=c.table[0], sin=c.table[1])
        tab = tuple(t.v[table_rows(c, 0 if shared else N)] for t in c.table)
    c.em = qk_emulate(c, *tab)
    return c


def qk_emulate(c, cos=None, sin=None):
    """(out, rstd, dx) per operand of a qk_case under the exact table (cos, sin) [M, D]; checks the
    cap and rows A and B"""
    res = []
    for x, g, w in zip(c.x, c.g, c.w):
        out, r = qk_fwd(x, w, cos, sin, c.eps, log=c.log)
        dx = qk_bwd(g, x, w, r, cos, sin, log=c.log)
        o = types.SimpleNamespace(kind="qk", x=x, y=out, r=r, dx=dx, row_a=c.row_a, row_b=c.row_b, eps=c.eps, M=c.M)
        _cap(o, out=out, dx=dx)
        o.log = dict(c.log)
        check_known_rows(o)
        gb = g.double() if cos is None else rope_t(g.double(), cos, sin)
        gxb = bf(gb * w.double()[None])[c.row_b]
        assert float((gxb * x.double()[c.row_b]).sum()) == 0.0 and float(gxb.abs().sum()) > 0
        assert dx.v[c.row_b].equal(bf(bf(gxb * r[c.row_b])))
        res.append(o)
    return res


@_seeded
def wgrad_case(D, B, N, has_k, rope, seed=0):
    """the qk_case of the shape with f32 rstd rows of their own (an input of the weight-gradient
    kernel) and nonzero bf16 [D] accumulators; .want(tab) emulates under a table and holds the cap"""
    c = qk_case(D, B, N, has_k, rope, False, False)
    gen = torch.Generator().manual_seed(seed + c.M + D)
    w = types.SimpleNamespace(c=c, log={})
    w.rs = [(0.5 + torch.rand(c.M, generator=gen)).float() for _ in c.x]
    w.g0 = [grid_vals((D,), gen, True).bfloat16() for _ in c.x]

    def want(tab):
        out = [wgrad(g, x, r, g0, *tab, log=w.log) for g, x, r, g0 in zip(c.g, c.x, w.rs, w.g0)]
        _cap(w, **{"g" + n: o for n, o in zip("qk", out)})
        return out
    w.want = want
    want(tuple(t.v[table_rows(c, N)] for t in c.table) if rope else ())
    return w


@_seeded
def colsum_case(mode, rpg, G, D, seed=0):
    """a on the grid (zeros included), b on it without zeros, f32 rstd in [0.5, 1.5) and means on the
    1/8 grid as the modes need them, nonzero accumulators, and the emulated outputs of the four
    (sum_groups, accumulate) settings under the cap"""
    gen = torch.Generator().manual_seed(seed + mode * 1000 + rpg + D + G)
    M = G * rpg
    c = types.SimpleNamespace(mode=mode, rpg=rpg, G=G, D=D, M=M, log={})
    c.a = grid_vals((M, D), gen, False).bfloat16()
    c.b = grid_vals((M, D), gen, True).bfloat16() if mode else None
    c.r32 = (0.5 + torch.rand(M, generator=gen)).float() if mode >= 2 else None
    c.mean32 = (torch.randint(-4, 5, (M,), generator=gen).float() / 8) if mode == 3 else None
    c.out0, c.want = {}, {}
    for sg in (True, False):
        for acc in (True, False):
            c.out0[sg, acc] = grid_vals((D,) if sg else (G, D), gen, True).bfloat16()
            c.want[sg, acc] = colsum(c.a, c.b, c.r32, c.mean32, mode, rpg, sg, acc, c.out0[sg, acc], log=c.log)
    _cap(c, **{"sg%d_acc%d" % k: v for k, v in c.want.items()})
    return c


def table_rows(c, cs_batch_rows):
    m = torch.arange(c.M)
    return (m // c.N) * cs_batch_rows + m % c.N


# ------------------------------------------------------------------------------------ the case table
Row = collections.namedtuple("Row", "entry id p")
WIDTHS_MOD = (8, 64, 96, 520, 1024, 1536, 2040, 2048)
WIDTHS_QK = (8, 64, 96, 128, 1024, 2048)
ENTRIES = ("ltx_rmsnorm_modulate_fwd", "ltx_rmsnorm_modulate_bwd", "ltx_rmsnorm_modulate_bwd_gated",
           "ltx_layernorm_modulate_fwd", "ltx_layernorm_modulate_bwd", "ltx_rope_table", "ltx_rope_pack_bf16",
           "ltx_qk_norm_rope_fwd", "ltx_qk_norm_rope_bwd", "ltx_qk_norm_fwd_grouped", "ltx_qk_norm_bwd_grouped",
           "ltx_qk_norm_wgrad", "ltx_group_colsum", "ltx_colsum_finish", "ltx_silu_bwd_bf16", "ltx_batch_sum_bf16",
           "ltx_ada_modulation", "ltx_gate_mul_bf16")


def _table():
    rows = []

    def add(entries, ident, **p):
        for e in entries.split():
            rows.append(Row("ltx_" + e, ident, p))

    for kind, ents in (("rms", "rmsnorm_modulate_fwd rmsnorm_modulate_bwd rmsnorm_modulate_bwd_gated"),
                       ("ln", "layernorm_modulate_fwd layernorm_modulate_bwd")):
        for D in WIDTHS_MOD:
            for B, N, rpb in ((3, 7, 7), (2, 4, 4), (3, 7, 0)):
                add(ents, "%s-D%d-%dx%d-rpb%d" % (kind, D, B, N, rpb), kind=kind, D=D, B=B, N=N, rpb=rpb,
                    ld_mod=6 * D, dres=(True, False), out_given=True)
    for D in WIDTHS_QK:
        pad = D % 6
        # q + k, per-batch int64 grid: inputs as views of one [M, 3D] buffer, outputs into strided views
        add("qk_norm_rope_fwd qk_norm_rope_bwd rope_table", "qk-D%d-int64" % D, D=D, pad=pad, B=3, N=7, has_k=True, rope="spec",
            grid="int64", shared=False, dq="bf16", dk="f32", fused_in=True, strided_out=True)
        add("qk_norm_rope_fwd qk_norm_rope_bwd rope_table", "qk-D%d-float-shared" % D, D=D, pad=pad, B=3, N=7, has_k=True,
            rope="spec", grid="float", shared=True, dq="f32", dk="bf16", fused_in=False, strided_out=False)
        add("qk_norm_rope_fwd qk_norm_rope_bwd rope_pack_bf16", "q-D%d-pair" % D, D=D, pad=pad, B=3, N=7, has_k=False,
            rope="pair", grid="int64", shared=False, dq="bf16", dk=None, fused_in=False, strided_out=False)
        add("qk_norm_rope_fwd qk_norm_rope_bwd", "q-D%d-plain" % D, D=D, pad=pad, B=3, N=7, has_k=False, rope=None,
            grid=None, shared=False, dq="f32", dk=None, fused_in=False, strided_out=False)
    for D in (64, 2048):
        add("qk_norm_fwd_grouped qk_norm_bwd_grouped", "grouped-D%d" % D, D=D, G=3, rows=5, strided=True, in_place=True)
    for B, N in ((3, 7), (4, 25)):
        for D in (96, 2048):
            for has_k, rope, dt in ((True, True, "f32"), (True, False, "bf16"), (False, True, "bf16"), (False, False, "f32")):
                add("qk_norm_wgrad colsum_finish", "wgrad-M%d-D%d-%s-%s-%s" % (B * N, D, "qk" if has_k else "q",
                                                                             "rope" if rope else "plain", dt),
                    B=B, N=N, D=D, has_k=has_k, rope=rope, dtype=dt, accumulate_nonzero=True)
    for mode in range(4):
        for rpg in (7, 50, 136):
            for G in (1, 3):
                for D in (8, 24, 2056):
                    add("group_colsum colsum_finish", "colsum-m%d-r%d-G%d-D%d" % (mode, rpg, G, D), mode=mode, rpg=rpg,
                        G=G, D=D, S=splits(rpg, G), sum_groups=(True, False), accumulate=(True, False))
    for n in (37, 4096 * 256 + 40):
        add("silu_bwd_bf16", "silu-%d" % n, n=n, dres=(True, False))
    for cols in (8, 136):
        add("batch_sum_bf16", "batchsum-%d" % cols, B=3, rows=5, cols=cols, strided=True)
    for D in (8, 520):
        for bc in (False, True):
            add("ada_modulation gate_mul_bf16", "ada-D%d-bc%d" % (D, bc), D=D, B=3, N=7, broadcast=bc)
    return rows


CASES = _table()


def rows_of(entry):
    seen, out = set(), []
    for r in CASES:
        if r.entry == entry and r.id not in seen:
            seen.add(r.id)
            out.append(r)
    return out
