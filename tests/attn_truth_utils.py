"""Shared by tests/test_attn_truth_cpu.py and tests/test_attn_truth_gpu.py: attention inputs whose
exact answer is known (DESIGN "Attention truth tests"), the element-by-element comparator and the
case table of the GPU file.

One (batch, head) of a case: the head dim is split into L "code" columns (a different subset per
head) and d - L free columns. Kept keys form groups of m tied keys (m in 1, 2, 4; members j % G, so
a group spans tiles and blocks) that share one +-1 code x AK in the code columns and carry their own
small integers in the free columns; a query carries AQ x the code of its target group and zeros in
the free columns. Its score is then bitwise equal on the m keys of its group (an integer dot
product) and lower by >= 160 log2 units on every other kept key, so P = 1/m on the group and
exactly 0 elsewhere in f32, O is the mean of m integer rows, and with +-1 / 0 dO every quantity a
kernel rounds to bf16 on its way (P, dS, O, dQ, dK, dV) lies on the bf16 grid: a correct kernel
returns the float64 reference bit for bit in any summation order. Masked keys (bias -10000) are
decoys: the code of a group at twice the amplitude, which would win its rows without the mask.
"""
import collections
import functools
import math
import types

import torch

LOG2E = 1.0 / math.log(2.0)
AQ, AK = 8.0, 4.0
MASK = -10000.0
# head dim -> (code columns L, scale, largest positive cross-correlation of two codes): the gap
# between a query's group and any other kept key is (L - corr) * AQ * AK * scale >= 112 natural units
CODE = {64: (48, 2.0 ** -3, 20), 32: (24, 2.0 ** -2, 10)}
MIN_GAP_LOG2 = 160.0
GRID_TOL = 2.0 ** -20
LSE_TOL = 2.0 ** -12   # ~3 f32 roundings of a value in [256, 512) (ulp 2^-15) are 1e-4: twice that
DQ32_TOL = 2.0 ** -10  # exact MFMA operands; P's f32 error is ~2e-4: five times that
KEEP_SETS = ("a", "b", "c", "d1", "d2", "e", "f", "g")


def _codes(n, L, cmax, gen):
    """n +-1 codes of length L, drawn greedily: a candidate whose correlation with an accepted code
    exceeds cmax is rejected."""
    C = torch.empty(n, L)
    have = 0
    while have < n:
        cand = (torch.randint(0, 2, (256, L), generator=gen) * 2 - 1).float()
        for c in cand:
            if have == 0 or float((C[:have] @ c).max()) <= cmax:
                C[have] = c
                have += 1
                if have == n:
                    break
    return C


def keep_mask(keep, Bk, Nk, gen):
    """bool [Bk, Nk] of the named keep set (32-key blocks are the one-pass backward's, 64-key tiles
    the forward's); the batches differ. a: a short prefix (config A's caption keeps 16); b: a
    scattered subset of block 3; c: the tail of the last, ragged block; d1: blocks {1, 2}; d2: blocks
    {0, 5}; e: a scattered half; f: batch 0 fully masked, the others keep a prefix; g: the batches keep
    different blocks, {6} and {2, 7} (reading the other batch's mask then skips a kept block)."""
    assert keep in KEEP_SETS, keep
    kk = torch.zeros(Bk, Nk, dtype=torch.bool)

    def scatter(b, lo, hi, n):
        kk[b, lo + torch.randperm(hi - lo, generator=gen)[:n]] = True

    for b in range(Bk):
        if keep == "a":
            kk[b, :min(16, Nk // 2) - 3 * b] = True
        elif keep == "b":
            scatter(b, 96, 128, 11 + 6 * b)
        elif keep == "c":
            assert Nk % 32 != 0
            kk[b, (Nk - 1) // 32 * 32 + b:] = True
        elif keep == "d1":
            if b == 0:
                kk[b, 32:96] = True
            else:
                scatter(b, 32, 64, 9)
                scatter(b, 64, 96, 14)
        elif keep == "d2":
            if b == 0:
                kk[b, 0:32] = True
                kk[b, 160:192] = True
            else:
                scatter(b, 0, 32, 12)
                scatter(b, 160, 192, 7)
        elif keep == "e":
            scatter(b, 0, Nk, Nk // 2)
        elif keep == "f":
            assert Bk > 1
            if b > 0:
                kk[b, :16] = True
        elif keep == "g":
            if b % 2 == 0:
                scatter(b, 192, 224, 10)
            else:
                scatter(b, 64, 96, 9)
                scatter(b, 224, 256, 13)
    return kk


def reference64(q, k, v, do, bias, B, Bk, H, d, scale, row_bias=None):
    """Plain float64 softmax attention and its gradients, written out: q/do [B*Nq, H*d], k/v
    [Bk*Nk, H*d] (Bk = 1: shared by every batch), bias [Bk, Nk] or None. row_bias [B, H, Nq, Nk] is
    added to the scores (planted faults). Returns a
    dict of o, dq [B*Nq, H*d], dk, dv [B*Nk, H*d] (per batch), lse (log2 units), delta [B, H, Nq]
    and p, ds [B, H, Nq, Nk]. Magnitudes under 1e-12 are 0: float64 keeps the 2^-160 tails f32 does
    not, and its own rounding of P (1/m to 1e-16) leaves 1e-15 where tied keys cancel exactly; the
    smallest nonzero magnitude of an exact case is 1/(8 m^2) >= 2^-7."""
    Nq, Nk = q.shape[0] // B, k.shape[0] // Bk
    qh = q.double().view(B, Nq, H, d).transpose(1, 2)
    doh = do.double().view(B, Nq, H, d).transpose(1, 2)
    kh = k.double().view(Bk, Nk, H, d).transpose(1, 2).expand(B, H, Nk, d)
    vh = v.double().view(Bk, Nk, H, d).transpose(1, 2).expand(B, H, Nk, d)
    s = (qh @ kh.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.double().view(Bk, 1, 1, Nk)
    if row_bias is not None:
        s = s + row_bias
    lse_n = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse_n)
    o = p @ vh
    delta = (doh * o).sum(-1, keepdim=True)
    ds = p * (doh @ vh.transpose(-1, -2) - delta)
    out = dict(o=o, dq=(ds @ kh) * scale, dk=(ds.transpose(-1, -2) @ qh) * scale, dv=p.transpose(-1, -2) @ doh,
               lse=lse_n[..., 0] * LOG2E, delta=delta[..., 0], p=p, ds=ds, s2=s * LOG2E)
    for n in ("o", "dq", "dk", "dv"):
        out[n] = out[n].transpose(1, 2).reshape(-1, H * d)
    return {n: torch.where(t.abs() < 1e-12, torch.zeros_like(t), t) for n, t in out.items()}


def off_grid(t):
    """largest |x - bf16(x)| / |x| over the nonzero elements"""
    t = t.double()
    return float(((t - t.float().bfloat16().double()).abs() / t.abs().clamp(min=1e-300)).max())


@functools.lru_cache(maxsize=None)
def make_case(B, Bk, H, Nq, Nk, d, m, keep, seed):
    """The bf16 inputs q, do [B*Nq, H*d], k, v [Bk*Nk, H*d], key_bias f32 [Bk, Nk] or None (keep
    None: every key kept, no bias; else a name of KEEP_SETS), scale, and .ref: the float64 o, lse
    (log2 units), delta, dq, dk, dv (reference64). Every (batch, head) has its own codes, code
    columns, targets and values. .noisy names the batches with no kept key: their reference is the
    uniform softmax over all Nk keys (their keys are 0 in the code columns and the queries in the
    free ones: all scores 0), O exact, dS off the bf16 grid. Asserts what makes "exact" well defined: the
    score gap, and P, dS and every output on the bf16 grid (only P and O in a noisy batch)."""
    assert Bk in (1, B) and m in (1, 2, 4) and keep in (None,) + KEEP_SETS
    L, scale, cmax = CODE[d]
    gen = torch.Generator().manual_seed(seed)
    kk = torch.ones(Bk, Nk, dtype=torch.bool) if keep is None else keep_mask(keep, Bk, Nk, gen)
    q = torch.zeros(B, Nq, H, d)
    k = torch.randint(-2, 3, (Bk, Nk, H, d), generator=gen).float()
    v = torch.randint(-2, 3, (Bk, Nk, H, d), generator=gen).float()
    group = torch.zeros(Bk, H, Nk, dtype=torch.long)  # of a kept key: its group; of a decoy: the group it mimics
    target = torch.zeros(B, H, Nq, dtype=torch.long)
    built = {}
    for bk in range(Bk):
        kept, masked = kk[bk].nonzero()[:, 0], (~kk[bk]).nonzero()[:, 0]
        n = len(kept)
        G, r = n // m, n % m  # G groups of m tied keys, the r kept keys left over are groups of one
        ng = max(G + r, 1)
        for h in range(H):
            cols = torch.randperm(d, generator=gen)[:L].sort().values
            C = _codes(ng, L, cmax, gen)
            j = torch.arange(n)
            group[bk, h, kept] = torch.where(j < G * m, j % max(G, 1), G + j - G * m)
            group[bk, h, masked] = torch.arange(len(masked)) % ng
            amp = torch.where(kk[bk], AK, 2 * AK) if n else torch.zeros(Nk)
            k[bk, :, h][:, cols] = amp[:, None] * C[group[bk, h]]
            built[bk, h] = (cols, C, ng, n == 0)
    for b in range(B):
        for h in range(H):
            cols, C, ng, uniform = built[b % Bk, h]
            if uniform:  # random codes against keys that are 0 in the code columns: every score is 0
                q[b, :, h][:, cols] = AQ * (torch.randint(0, 2, (Nq, L), generator=gen) * 2 - 1).float()
                continue
            # every group is a target when Nq allows; the last kept key's group (always ng - 1) is
            # the last query row's, so ragged last tiles meet
            t = (ng - 1 - torch.arange(Nq) % ng)[torch.randperm(Nq, generator=gen)]
            at = int((t == ng - 1).nonzero()[0])
            t[at], t[Nq - 1] = t[Nq - 1].clone(), t[at].clone()
            target[b, h] = t
            q[b, :, h][:, cols] = AQ * C[t]
    do = torch.zeros(B, Nq, H, d)
    do.scatter_(3, torch.rand(B, Nq, H, d, generator=gen).topk(4).indices,
                (torch.randint(0, 2, (B, Nq, H, 4), generator=gen) * 2 - 1).float())
    c = types.SimpleNamespace(B=B, Bk=Bk, H=H, Nq=Nq, Nk=Nk, d=d, m=m, keep=keep, scale=scale, shared=Bk == 1 and B > 1,
                              kept=kk, group=group, target=target,
                              noisy=[b for b in range(B) if not kk[b % Bk].any()])
    c.q, c.do = q.reshape(B * Nq, H * d).bfloat16(), do.reshape(B * Nq, H * d).bfloat16()
    c.k, c.v = k.reshape(Bk * Nk, H * d).bfloat16(), v.reshape(Bk * Nk, H * d).bfloat16()
    for t, t16 in ((q, c.q), (k, c.k), (v, c.v), (do, c.do)):
        assert torch.equal(t.reshape(t16.shape), t16.float())
    c.key_bias = None if keep is None else torch.where(kk, 0.0, MASK).float().contiguous()
    ref = reference64(c.q, c.k, c.v, c.do, c.key_bias, B, Bk, H, d, scale)
    c.ref = types.SimpleNamespace(**ref)
    exact = [b for b in range(B) if b not in c.noisy]
    s2 = ref["s2"][exact]
    gap = s2.amax(-1, keepdim=True) - s2
    ties = (gap < 1e-9).sum(-1)
    assert float(gap[gap >= 1e-9].min()) >= MIN_GAP_LOG2, float(gap[gap >= 1e-9].min())
    assert set(ties.unique().tolist()) <= {1, m}, ties.unique()
    if c.noisy:
        assert float((ref["p"][c.noisy] * Nk - 1).abs().max()) <= 1e-12
    rows = lambda t, n: t.view(B, n, H * d)  # noqa: E731
    grids = dict(p=ref["p"], o=rows(ref["o"], Nq), ds=ref["ds"][exact], dq=rows(ref["dq"], Nq)[exact],
                 dk=rows(ref["dk"], Nk)[exact], dv=rows(ref["dv"], Nk)[exact])
    for n, t in grids.items():
        assert off_grid(t) <= GRID_TOL, (n, off_grid(t))
    return c


def describe(bad, shape, d):
    """the count and the first positions of a bool mismatch map, (row, head, column) for [rows, H*d]"""
    idx = bad.nonzero()
    if len(shape) == 2:
        pos = [(int(r), int(c) // d, int(c) % d) for r, c in idx[:6]]
        where = "rows %s heads %s" % (sorted(set(idx[:, 0].tolist()))[:12], sorted(set((idx[:, 1] // d).tolist())))
    else:
        pos = [tuple(int(x) for x in i) for i in idx[:6]]
        where = "batches %s heads %s" % (sorted(set(idx[:, 0].tolist())), sorted(set(idx[:, 1].tolist())))
    return idx, pos, where


def assert_truth(name, out, ref64, d=64, neighbour=False):
    """out against the float64 reference, element by element. bf16: bf16(ref64) bit for bit, the sign
    of zero ignored (neighbour=True, one documented output of one kernel: a differing element must
    be a bf16 neighbour of a nonzero reference). f32 "lse": |out - ref| <= 2^-12. Any other f32 (dQ
    with dq_f32): exactly 0 where the reference is, else |out - ref| <= 2^-10 |ref|. Returns the
    largest absolute error. The failure names the count, the first (row, head, column) positions
    with both values (in a [rows, H*d] operand a row is batch * N + query or key) and the rows and
    heads affected."""
    got = out.detach().cpu()
    ref = ref64.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if got.dtype == torch.bfloat16:
        want = ref.float().bfloat16()
        bad = ~(got.float() == want.float())
        if neighbour:
            step = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs()
            bad &= ~((step == 1) & (ref != 0))
        want = want.double()
    elif name == "lse":
        want = ref
        bad = ~((got.double() - ref).abs() <= LSE_TOL)
    else:
        want = ref
        bad = torch.where(ref == 0, got != 0, ~((got.double() - ref).abs() <= DQ32_TOL * ref.abs()))
    if bad.any():
        idx, pos, where = describe(bad, got.shape, d)
        vals = ["%s got %r want %r" % (p_, float(got[tuple(i)]), float(want[tuple(i)])) for p_, i in zip(pos, idx)]
        raise AssertionError("%s: %d of %d elements differ from the exact reference; %s; first: %s"
                             % (name, len(idx), bad.numel(), where, "; ".join(vals)))
    return float((got.double() - want).abs().max())


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _noise_refs(B, Bk, H, Nq, Nk, d, m, keep, seed):
    """fp32 and bf16 torch SDPA with autograd on a case: (o, dq, dk, dv) each, dk / dv per batch"""
    import torch.nn.functional as F
    c = make_case(B, Bk, H, Nq, Nk, d, m, keep, seed)
    outs = []
    for dt in (torch.float32, torch.bfloat16):
        q, k, v = (t.to(dt).clone().requires_grad_(True) for t in (c.q, c.k.repeat(B // Bk, 1), c.v.repeat(B // Bk, 1)))
        heads = lambda t, n: t.view(B, n, H, d).transpose(1, 2)  # noqa: E731
        mask = None if c.key_bias is None else c.key_bias.repeat(B // Bk, 1).view(B, 1, 1, Nk).to(dt)
        o = F.scaled_dot_product_attention(heads(q, Nq), heads(k, Nk), heads(v, Nk), attn_mask=mask, scale=c.scale)
        o = o.transpose(1, 2).reshape(B * Nq, H * d)
        o.backward(c.do.to(dt))
        outs.append(dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad))
    return outs


def check_outputs(c, seed, outs, neighbour=()):
    """assert_truth on every output of outs (a dict of o, lse, dq, dk, dv as the kernels return
    them; a subset is fine). In a batch with no kept key (c.noisy) dS is off the bf16 grid: there
    dq, dk and dv take the suite's noise criterion against fp32 for that batch alone, rel-Frobenius
    within 1.25 x torch's own bf16 SDPA error + 1e-3; O and lse stay exact. Returns the largest
    absolute error per output."""
    B, H, d = c.B, c.H, c.d
    errs = {}
    for n, t in outs.items():
        t = t.detach().cpu()
        ref = getattr(c.ref, n)
        if n in ("o", "lse") or not c.noisy:
            errs[n] = assert_truth(n, t, ref, d, neighbour=n in neighbour)
            continue
        r32, r16 = _noise_refs(c.B, c.Bk, H, c.Nq, c.Nk, d, c.m, c.keep, seed)
        per = lambda x: x.reshape(B, -1, H * d)  # noqa: E731
        for b in range(B):
            if b in c.noisy:
                e, e16 = rel(per(t)[b], per(r32[n])[b]), rel(per(r16[n])[b], per(r32[n])[b])
                assert e <= 1.25 * e16 + 1e-3, (n, "batch", b, e, e16)
            else:
                errs[n] = assert_truth("%s batch %d" % (n, b) if t.dtype == torch.bfloat16 else n, per(t)[b],
                                       per(ref)[b], d, neighbour=n in neighbour)
    return errs


def labelled(fn, *args, **kw):
    """fn(*args, **kw) and the labels its attention launches recorded under a LaunchTimer: the
    kernels the dispatcher planned (ltx_attn_describe)."""
    from ltx_amd import ops
    saved, timer = ops._timer, ops.LaunchTimer()
    ops.set_launch_timer(timer)
    try:
        out = fn(*args, **kw)
    finally:
        ops.set_launch_timer(saved)
    return out, tuple(r[0] for r in timer.records)


# ------------------------------------------------------------------------------------ the case table
# One row of the GPU file: the LTX_ATTN_* switches it sets (names without the prefix), the shape, the
# construction, and the kernels its forward / backward label must name. B = 2 throughout.
Case = collections.namedtuple("Case", "id env H Nq Nk d m keep fwd bwd shared fused dq_f32")
B = 2
SEED = 20
MASKS_256 = ("a", "b", "d1", "d2", "e", "f", "g")


def _table():
    rows, ms = [], [1, 2, 4]

    def add(tag, env, shape, keep=None, fwd=(), bwd=(), d=64, m=None, shared=False, fused=False, dq_f32=False):
        H, Nq, Nk = shape
        m = ms[len(rows) % 3] if m is None else m
        if keep == "c" and m == 4:  # 8 kept keys are 2 groups: hundreds of queries per key sum dK off the grid
            m = 2
        ident = "%s-%dx%dx%d-m%d%s%s" % (tag, H, Nq, Nk, m, "-" + keep if keep else "",
                                         "".join("-%s%s" % (k_.lower(), v_) for k_, v_ in sorted(env.items())))
        rows.append(Case(ident, env, H, Nq, Nk, d, m, keep, tuple(fwd), tuple(bwd), shared, fused, dq_f32))

    f1 = {"1": "attn_fwd1_kernel<64, %s, true>", "0": "attn_fwd1_kernel<64, %s, false>"}
    b1, fin = "attn_bwd1_kernel<64, %s>", "attn_bwd1_finish_kernel<64>"
    delta = "attn_delta_kernel<64>"
    for rws in ("1", "0"):  # the one-pass forward, both O stores; 520 queries: two workgroups per head
        env = {"FWD1_ROWS": rws}
        for shape in ((2, 300, 256), (2, 520, 256)):
            add("fwd1", env, shape, fwd=[f1[rws] % "false"], bwd=[delta, b1 % "false, false", fin])
        for shape, keep in (((3, 300, 200), None), ((2, 64, 33), None), ((3, 300, 200), "c")):
            add("fwd1", env, shape, keep, fwd=[f1[rws] % "true"], bwd=[b1 % "true, false"])
        for keep in MASKS_256:
            add("fwd1", env, (2, 300, 256), keep, fwd=[f1[rws] % "true"], bwd=[b1 % "true, false", fin])
    w1p = ["attn_dq_w1p_kernel<0>", "attn_dkdv_w1p_kernel<0>"]
    long_ = ((2, 200, 320), (3, 520, 768))
    for f32sum in ("1", "0"):  # the pipelined forward, and the persistent backward pair behind it
        for shape in long_:
            add("pipe", {"FWD_F32SUM": f32sum}, shape, fwd=["attn_fwd_pipe_kernel<%s>" % ("true" if f32sum == "1" else "false")],
                bwd=[delta] + w1p)
    add("tiled8", {"FWD_PIPE": "0"}, (2, 200, 320), fwd=["attn_q_kernel<64, 0, false, 8>"], bwd=w1p)
    for nbuf in ("4", "3"):  # biased tiled forward; the biased split pair
        for shape, keep in (((2, 200, 520), None), ((2, 300, 320), "e")):
            add("tiled8b", {"DKDV_NBUF": nbuf}, shape, keep, fwd=["attn_q_kernel<64, 0, true, 8>"],
                bwd=["attn_q_kernel<64, 1, true, 4>", "attn_dkdv_pipe_kernel<true, %s>" % nbuf])
    add("tiled4", {"W8": "0", "FWD_PIPE": "0"}, (2, 200, 320), fwd=["attn_q_kernel<64, 0, false, 4>"], bwd=w1p)
    add("tiled4", {"W8": "0", "FWD_PIPE": "0", "FWD1": "0"}, (2, 100, 77), "e", fwd=["attn_q_kernel<64, 0, true, 4>"],
        bwd=[b1 % "true, false"])
    for m in (1, 2):  # head dim 32
        add("d32", {}, (4, 200, 128), d=32, m=m, fwd=["attn_q_kernel<32, 0, false, 4>"],
            bwd=["attn_delta_kernel<32>", "attn_q_kernel<32, 1, false, 4>", "attn_dkdv_kernel<32, false, 4>"])
        add("d32", {}, (3, 100, 77), "e", d=32, m=m, fwd=["attn_q_kernel<32, 0, true, 4>"],
            bwd=["attn_q_kernel<32, 1, true, 4>", "attn_dkdv_kernel<32, true, 4>"])
    for m in (1, 2, 4):  # the unbiased one-pass backward, split over the queries and not
        add("bwd1", {}, (2, 300, 256), m=m, bwd=[b1 % "false, false", fin])
        add("bwd1", {"QSPLIT": "0"}, (2, 300, 256), m=m, bwd=[b1 % "false, false"])
    # the biased one-pass backward: 100 queries run unsplit (bwd1_few_keys where one block is
    # active: a, b, c), 300 split over the queries
    for env in ({}, {"BWD1_FEW": "0"}, {"SKIP": "0"}):
        for Nq in (300, 100):
            for keep in MASKS_256 + ("c",):
                add("bwd1b", env, (2, Nq, 200 if keep == "c" else 256), keep, fwd=["attn_fwd1_kernel<64, true, true>"],
                    bwd=[b1 % "true, false"] + ([fin] if Nq == 300 else []))
    for Nq in (300, 100):  # its query-split form: taken behind a leading masked block, not over a hole
        for keep in ("a", "d1", "d2"):
            add("bwd1qs", {"BWD1_QS": "1", "QSPLIT": "0"}, (2, Nq, 256), keep, bwd=[b1 % "true, true"])
    for shape in long_:
        add("w1", {"DQ_W1": "1", "DKDV_W1": "1"}, shape, bwd=["attn_dq_w1_kernel<0>", "attn_dkdv_w1_kernel<0>"])
        add("w1", {}, shape, bwd=["attn_dq_w1_kernel<0>", "attn_dkdv_w1p_kernel<0>"], dq_f32=True)
        for nbuf in ("3", "4"):
            add("bpipe", {"DQ_W1": "0", "DKDV_W1": "0", "DQ_NBUF": nbuf, "DKDV_NBUF": nbuf}, shape,
                bwd=["attn_dq_pipe_kernel<%s>" % nbuf, "attn_dkdv_pipe_kernel<false, %s>" % nbuf])
    add("bplain", {"DQ_W1": "0", "DKDV_W1": "0", "DQ_PIPE": "0"}, (2, 200, 320),
        bwd=["attn_q_kernel<64, 1, false, 4>", "attn_dkdv_pipe_kernel<false, 4>"])
    for w8, waves in ((None, 4), ("3", 8)):  # the plain pair, 4-wave and 8-wave dK / dV
        env = {"DKDV_PIPE": "0"} if w8 is None else {"DKDV_PIPE": "0", "W8": w8}
        for shape, b in (((2, 200, 320), "false"), ((2, 200, 520), "true")):
            add("bplain", env, shape, bwd=["attn_q_kernel<64, 1, %s, 4>" % b, "attn_dkdv_kernel<64, %s, %d>" % (b, waves)])
    add("short", {"BWD1": "0"}, (2, 300, 256), bwd=w1p)
    add("short", {"BWD1": "0"}, (3, 300, 200), bwd=["attn_q_kernel<64, 1, true, 4>", "attn_dkdv_pipe_kernel<true, 4>"])
    for shape in ((2, 300, 256), (2, 200, 320)):  # shared keys; Q, K and V views of one fused buffer
        short = shape[2] == 256
        fwd = ["attn_fwd1_kernel<64, false, true>" if short else "attn_fwd_pipe_kernel<true>"]
        add("shared", {}, shape, m=2, shared=True, fwd=fwd, bwd=[b1 % "false, false", fin] if short else w1p)
        add("fused", {}, shape, m=2, fused=True, fwd=fwd, bwd=[b1 % "false, false", fin] if short else w1p)
    add("shared", {}, (2, 300, 256), "a", m=2, shared=True, fwd=[f1["1"] % "true"], bwd=[b1 % "true, false", fin])
    add("shared", {}, (2, 100, 256), "b", m=2, shared=True, fwd=[f1["1"] % "true"], bwd=[b1 % "true, false"])
    assert len({r.id for r in rows}) == len(rows)
    return rows


CASES = _table()
# the forward rows that rerun under the RESCALE_TAU = 0 build where it exists
TAU0_TAGS = ("fwd1-", "pipe-", "tiled8-", "tiled8b-")


def case_inputs(row):
    return make_case(B, 1 if row.shared else B, row.H, row.Nq, row.Nk, row.d, row.m, row.keep, SEED)
