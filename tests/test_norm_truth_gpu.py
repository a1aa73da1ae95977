"""Norm, RoPE and column-sum truth tests on the MI355X: every entry point of csrc/norms.hip, the
train_mode='full' reductions of csrc/paramgrad.hip and ltx_batch_sum_bf16 on inputs whose f32 sums
are exact, every output element against the float64 emulators of tests/norm_truth_utils.py (held to
the oracle's eager bf16 ops by tests/test_norm_truth_cpu.py): closed elements bit for bit, open
ones (an f32 rounding of rsqrtf, r^3, sincosf, expf could move them) within 2 bf16 ulps and at most
2 % of an output, rstd and mean within 2^-21 of float64. The table is norm_truth_utils.CASES;
`pytest -s` prints the measured errors of profiles/norm_truth.md."""
import math

import pytest
import torch

import ltx_oracle as O
import norm_truth_utils as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = 3.0


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from ltx_amd import _lib as L
    L.ensure_device()
    return L


def ids(entry):
    rows = U.rows_of(entry)
    return pytest.mark.parametrize("row", rows, ids=[r.id for r in rows])


def dev(t):
    return None if t is None else t.to(DEV)


def report(row, **kw):
    print("\n%s: %s" % (row.id, ", ".join("%s %s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in kw.items())))


def framed(M, D, left=8, right=8):
    """a [M, D] view inside a wider buffer of sentinels: (buffer, view)"""
    buf = torch.full((M, left + D + right), SENTINEL, dtype=BF16, device=DEV)
    return buf, buf[:, left:left + D]


def assert_frame(buf, D, left=8):
    assert bool((buf[:, :left] == SENTINEL).all()) and bool((buf[:, left + D:] == SENTINEL).all()), "wrote outside its view"


# ------------------------------------------------------------------------- RMSNorm / LayerNorm
@ids("ltx_rmsnorm_modulate_fwd")
def test_rmsnorm_modulate(row):
    from ltx_amd import ops
    p = row.p
    c = U.mod_case("rms", p["D"], p["B"], p["N"], p["rpb"])
    M, D = c.M, c.D
    mod = dev(c.mod)
    shift, onep, gate = mod[:, 0], mod[:, 1], mod[:, 5]   # views, ld_mod = 6 D
    assert mod.stride(0) == p["ld_mod"]
    x, dy, dres = dev(c.x), dev(c.dy), dev(c.dres)
    y, rstd = ops.rmsnorm_modulate_fwd(x, shift, onep, mod.stride(0), c.rpb, c.eps)
    e_r = U.assert_stat("rstd", rstd, c.r)
    U.assert_truth("y", y, c.y)
    out = torch.full((M + 1, D), SENTINEL, dtype=BF16, device=DEV)
    y2, _ = ops.rmsnorm_modulate_fwd(x, shift, onep, mod.stride(0), c.rpb, c.eps, out=out[:M])
    assert torch.equal(out[:M], y) and bool((out[M] == SENTINEL).all())
    dx = ops.rmsnorm_modulate_bwd(dy, x, rstd, onep, mod.stride(0), c.rpb, dres=dres)
    U.assert_truth("dx", dx, c.dx)
    out.fill_(SENTINEL)
    ops.rmsnorm_modulate_bwd(dy, x, rstd, onep, mod.stride(0), c.rpb, dres=dres, out=out[:M])
    assert torch.equal(out[:M], dx) and bool((out[M] == SENTINEL).all())
    dx0 = ops.rmsnorm_modulate_bwd(dy, x, rstd, onep, mod.stride(0), c.rpb)
    U.assert_truth("dx without dres", dx0, c.dx_g)
    dxg, gout = ops.rmsnorm_modulate_bwd(dy, x, rstd, onep, mod.stride(0), c.rpb, gate=gate)
    assert torch.equal(dxg, dx0)
    U.assert_truth("gout", gout, c.gout)
    assert torch.equal(gout, ops.gate_mul(dx0, gate, c.rpb if c.rpb else M))
    report(row, rstd_err=e_r, open=c.open)


@ids("ltx_layernorm_modulate_fwd")
def test_layernorm_modulate(row):
    from ltx_amd import ops
    p = row.p
    c = U.mod_case("ln", p["D"], p["B"], p["N"], p["rpb"])
    mod = dev(c.mod)
    shift, onep = mod[:, 0], mod[:, 1]
    x, dy = dev(c.x), dev(c.dy)
    y, mean, rstd = ops.layernorm_modulate_fwd(x, shift, onep, mod.stride(0), c.rpb, c.eps)
    e_m = U.assert_stat("mean", mean, c.mean)
    e_r = U.assert_stat("rstd", rstd, c.r)
    U.assert_truth("y", y, c.y)
    dx = ops.layernorm_modulate_bwd(dy, x, mean, rstd, onep, mod.stride(0), c.rpb)
    U.assert_truth("dx", dx, c.dx)
    report(row, mean_err=e_m, rstd_err=e_r, open=c.open)


# --------------------------------------------------------------------------- q/k norm + RoPE
def _rope(c, p):
    """the RoPE state of the row (RopeSpec on the int64 / float grid, or RopePair on the reference's
    own pair), after checking its table words against the emulator"""
    from ltx_amd import ops
    if p["rope"] is None:
        return None
    shared = p["shared"]
    if p["rope"] == "pair":
        cos, sin = O.rope_freqs(c.grid, c.D, U.THETA, list(U.MAX_POS), BF16)
        rope = ops.RopePair(dev(cos), dev(sin))
        want = U.pack_words(cos.reshape(c.M, c.D), sin.reshape(c.M, c.D))
        assert torch.equal(rope.cs.cpu().to(torch.int64) & 0xFFFFFFFF, want), "rope_pack: table words differ"
        assert rope.cs_batch_rows == c.N
        return rope
    grid = dev(c.grid[:1]).expand(c.B, -1, -1) if shared else dev(c.grid)
    rope = ops.RopeSpec(grid, c.D, U.THETA, list(U.MAX_POS))
    assert rope.cs_batch_rows == (0 if shared else c.N) and rope.cs.shape[0] == (c.N if shared else c.M)
    assert rope.is_float == (1 if p["grid"] == "float" else 0)
    assert torch.equal(rope.omega.cpu(), U.rope_omega(c.D))
    rows = torch.arange(rope.cs.shape[0])
    cos, sin = U.unpack_cs(rope.cs, rows)
    U.assert_truth("table cos", cos.bfloat16(), c.table[0])
    U.assert_truth("table sin", sin.bfloat16(), c.table[1])
    return rope


@ids("ltx_qk_norm_rope_fwd")
def test_qk_norm_rope(row):
    from ltx_amd import ops
    p = row.p
    c = U.qk_case(p["D"], p["B"], p["N"], p["has_k"], p["rope"] is not None, p["grid"] == "float", p["shared"])
    M, D = c.M, c.D
    rope = _rope(c, p)
    tab = ()
    if rope is not None:
        tab = U.unpack_cs(rope.cs, U.table_rows(c, rope.cs_batch_rows))
    em = U.qk_emulate(c, *tab)   # under the table words the kernels read
    if p["fused_in"]:
        qkv = torch.full((M, 3 * D), SENTINEL, dtype=BF16, device=DEV)
        qkv[:, :D], qkv[:, D:2 * D] = dev(c.x[0]), dev(c.x[1])
        xin = [qkv[:, :D], qkv[:, D:2 * D]]
    else:
        xin = [dev(x) for x in c.x]
    ws = [dev(w) for w in c.w]
    frames = [framed(M, D) for _ in xin] if p["strided_out"] else None
    outs = [f[1] for f in frames] if frames else [None, None]
    k_in = xin[1] if c.has_k else None
    q_out, k_out, rq, rk = ops.qk_norm_rope_fwd(xin[0], k_in, ws[0], ws[1] if c.has_k else None, rope, B=c.B, N=c.N,
                                                eps=c.eps, q_out=outs[0], k_out=outs[1] if c.has_k else None)
    got, rs = [q_out, k_out][:len(em)], [rq, rk][:len(em)]
    errs = []
    for name, o, r, e in zip("qk", got, rs, em):
        errs.append(U.assert_stat("rstd_" + name, r, e.r))
        U.assert_truth(name + "_out", o, e.y)
    if frames:
        for buf, _ in frames:
            assert_frame(buf, D)
    # backward: dq / dk in the row's dtypes, outputs into framed views where the row says so
    gin = [dev(g).float() if dt == "f32" else dev(g) for g, dt in zip(c.g, (p["dq"], p["dk"]))]
    frames = [framed(M, D) for _ in xin] if p["strided_out"] else None
    outs = [f[1] for f in frames] if frames else [None, None]
    dq_out, dk_out = ops.qk_norm_rope_bwd(gin[0], xin[0], ws[0], rq, gin[1] if c.has_k else None, k_in,
                                          ws[1] if c.has_k else None, rk, rope, B=c.B, N=c.N, dq_out=outs[0],
                                          dk_out=outs[1] if c.has_k else None)
    for name, o, e in zip("qk", [dq_out, dk_out][:len(em)], em):
        U.assert_truth("d%s_raw" % name, o, e.dx)
    if frames:
        for buf, _ in frames:
            assert_frame(buf, D)
    if p["fused_in"]:
        assert bool((qkv[:, 2 * D:] == SENTINEL).all())
    report(row, rstd_err=max(errs), open=[e.open for e in em], table_open=c.open if rope is not None else None,
           sums={k: round(math.log2(v), 1) if v > 1 else v for k, v in c.log.items()})


@ids("ltx_qk_norm_fwd_grouped")
def test_qk_norm_grouped(row):
    from ltx_amd import ops
    p = row.p
    G, rows, D = p["G"], p["rows"], p["D"]
    c = U.qk_case(D, 1, rows, False, False, False, False)
    # group g: the case's rows rolled by g (other rows under another weight), in [k_g | v_g] columns
    gen = torch.Generator().manual_seed(D)
    w = torch.stack([c.w[0]] + [U.generic_bf16((D,), gen) for _ in range(G - 1)])
    kv = torch.full((rows, 2 * G * D), SENTINEL, dtype=BF16, device=DEV)
    dkv = torch.full((rows, 2 * G * D), SENTINEL, dtype=BF16, device=DEV)
    xs, gs = [], []
    for g in range(G):
        xs.append(torch.roll(c.x[0], g, 0)), gs.append(torch.roll(c.g[0], g, 0))
        kv[:, 2 * g * D:(2 * g + 1) * D], dkv[:, 2 * g * D:(2 * g + 1) * D] = dev(xs[g]), dev(gs[g])
    y, rstd = ops.qk_norm_fwd_grouped(kv, 2 * D, dev(w))
    dy = torch.stack([dev(g_) for g_ in gs]).view(G * rows, D)
    dx = torch.full((rows, 2 * G * D), SENTINEL, dtype=BF16, device=DEV)
    ops.qk_norm_bwd_grouped(dy, rows * D, kv, 2 * D, dev(w), rstd, dx, 2 * D)
    ops.qk_norm_bwd_grouped(dkv, 2 * D, kv, 2 * D, dev(w), rstd, dkv, 2 * D)   # in place, strided
    assert torch.equal(dkv, dx)
    errs = []
    for g in range(G):  # (the emulators refuse a group whose sums are not exact)
        out, r = U.qk_fwd(xs[g], w[g], eps=1e-5)
        errs.append(U.assert_stat("rstd", rstd[g], r))
        U.assert_truth("y[%d]" % g, y[g], out)
        U.assert_truth("dx[%d]" % g, dx[:, 2 * g * D:(2 * g + 1) * D], U.qk_bwd(gs[g], xs[g], w[g], r))
        assert bool((dx[:, (2 * g + 1) * D:(2 * g + 2) * D] == SENTINEL).all())  # v columns untouched
    report(row, rstd_err=max(errs))


@ids("ltx_qk_norm_wgrad")
def test_qk_norm_wgrad(row):
    from ltx_amd import ops
    p = row.p
    w = U.wgrad_case(p["D"], p["B"], p["N"], p["has_k"], p["rope"])
    c = w.c
    M, D, k = c.M, c.D, c.has_k
    assert ops._splits(M, D, 2 if k else 1) == U.splits(M, 2 if k else 1)
    rope, tab = None, ()
    if p["rope"]:
        rope = ops.RopeSpec(dev(c.grid), D, U.THETA, list(U.MAX_POS))
        tab = U.unpack_cs(rope.cs, U.table_rows(c, rope.cs_batch_rows))
    xin = [dev(x) for x in c.x]
    gin = [dev(g).float() if p["dtype"] == "f32" else dev(g) for g in c.g]
    acc = [dev(g).clone() for g in w.g0]   # nonzero: the kernel accumulates
    rs = [dev(r) for r in w.rs]
    ops.qk_norm_wgrad_into(gin[0], xin[0], rs[0], acc[0], gin[1] if k else None, xin[1] if k else None,
                           rs[1] if k else None, acc[1] if k else None, rope, B=c.B, N=c.N)
    want = w.want(tab)   # under the table words the kernel read
    for name, got, e in zip("qk", acc, want):
        U.assert_truth("g" + name, got, e)
    report(row, open=w.open, **w.log)


# ------------------------------------------------------------------------------- column sums
@ids("ltx_group_colsum")
def test_group_colsum(row):
    from ltx_amd import ops
    p = row.p
    mode, rpg, G, D = p["mode"], p["rpg"], p["G"], p["D"]
    assert ops._splits(rpg, D, G) == p["S"]
    c = U.colsum_case(mode, rpg, G, D)
    # strided row views: a and b are column ranges of one buffer
    buf = torch.full((c.M, 2 * D + 8), SENTINEL, dtype=BF16, device=DEV)
    buf[:, :D] = dev(c.a)
    if mode:
        buf[:, D + 8:] = dev(c.b)
    av, bv = buf[:, :D], (buf[:, D + 8:] if mode else None)
    r32, mean32 = dev(c.r32), dev(c.mean32)
    for sum_groups in p["sum_groups"]:
        for accumulate in p["accumulate"]:
            out = dev(c.out0[sum_groups, accumulate]).clone()
            ops.colsum_into(out, av, bv, r32, mean32, mode, rpg, sum_groups=sum_groups, accumulate=accumulate)
            U.assert_truth("sum_groups=%s accumulate=%s" % (sum_groups, accumulate), out, c.want[sum_groups, accumulate])
    U.assert_truth("group_colsum", ops.group_colsum(av, bv, r32, mean32, mode, rpg), c.want[False, False])
    report(row, open=max(c.open.values()), **c.log)


@ids("ltx_silu_bwd_bf16")
def test_silu_bwd(row):
    from ltx_amd import ops
    n = row.p["n"]
    gen = torch.Generator().manual_seed(n)
    x = (torch.randint(-48, 49, (n,), generator=gen).double() / 4).bfloat16()
    dy, dres = U.grid_vals((n,), gen, False).bfloat16(), U.grid_vals((n,), gen, False).bfloat16()
    assert float(x.min()) == -12.0 and float(x.max()) == 12.0 or n < 100
    shares = []
    for res in row.p["dres"]:
        want = U.silu_bwd(x, dy, dres if res else None)
        got = ops.silu_bwd(dev(x), dev(dy), dev(dres) if res else None)
        shares.append(U.assert_truth("dres=%s" % res, got, want)[0])
    report(row, open=max(shares))


@ids("ltx_batch_sum_bf16")
def test_batch_sum(row):
    from ltx_amd import ops
    p = row.p
    B, rows, cols = p["B"], p["rows"], p["cols"]
    gen = torch.Generator().manual_seed(cols)
    x = U.grid_vals((B * rows, cols), gen, False).bfloat16()
    buf = torch.full((B * rows, cols + 16), SENTINEL, dtype=BF16, device=DEV)
    buf[:, 8:8 + cols] = dev(x)
    want = U.batch_sum(x, B)
    U.assert_truth("contiguous", ops.batch_sum(dev(x), B), want)
    obuf, out = framed(rows, cols)
    ops.batch_sum(buf[:, 8:8 + cols], B, out=out)    # a strided source into a strided view
    U.assert_truth("strided", out, want)
    assert_frame(obuf, cols)


@ids("ltx_ada_modulation")
def test_ada_modulation_and_gate_mul(row):
    from ltx_amd import ops
    p = row.p
    D, B, N, bc = p["D"], p["B"], p["N"], p["broadcast"]
    P = 2 if bc else 6
    gen = torch.Generator().manual_seed(D + bc)
    sst = dev(U.generic_bf16((P, D), gen))
    tmod = dev(U.generic_bf16((B, D) if bc else (B, P * D), gen))
    mask = (1 << 1) if bc else (1 << 1) | (1 << 4)
    mod, onep = ops.ada_modulation(sst, tmod, scale_mask=mask, broadcast=bc)
    ada = sst[None] + (tmod[:, None] if bc else tmod.view(B, P, D))
    assert torch.equal(mod, ada)
    for j in range(P):
        if mask >> j & 1:
            assert torch.equal(onep[:, j], 1 + ada[:, j])
    dy = dev(U.grid_vals((B * N, D), gen, False).bfloat16())
    gate = mod[:, P - 1]
    want = (dy.double().view(B, N, D) * gate.double()[:, None]).view(B * N, D)
    U.assert_truth("gate_mul", ops.gate_mul(dy, gate, N), U.Iv(U.bf(want.cpu())))
