"""The norm truth tests' own checks, without a GPU (tests/norm_truth_utils.py): the float64
emulators against the oracle's eager bf16 torch ops with autograd on the builder's inputs, the
builder's assertions (exact sums, the 2 % cap, rows A and B), the comparator against nine planted
faults (and what today's criteria of tests/test_kernels_gpu.py say of them on randn inputs), and the
coverage of the GPU table. `pytest -s` prints the tables of profiles/norm_truth.md."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

import ltx_oracle as O
import norm_truth_utils as U

BF16 = torch.bfloat16


def _mods(c):
    return c.mod[:, 0], c.mod[:, 1], c.mod[:, 5]


def _rows(t, c):
    """[Bm, D] modulation rows -> [M, D], as the reference's [B, 1, D] broadcast"""
    return t[U._batch_of(c.M, c.rpb, None)]


# --------------------------------------------------------------------- the oracle arbitrates
@pytest.mark.parametrize("D", U.WIDTHS_MOD)
@pytest.mark.parametrize("B,N,rpb", [(3, 7, 7), (3, 7, 0)])
def test_rmsnorm_emulator_is_the_oracle(D, B, N, rpb):
    c = U.mod_case("rms", D, B, N, rpb)
    shift, onep, gate = (_rows(t, c) for t in _mods(c))
    x = c.x.clone().requires_grad_(True)
    y = O.rmsnorm(x, c.eps) * onep + shift
    U.assert_truth("y", y.detach(), c.y)
    var = c.x.float().pow(2).mean(-1)
    U.assert_stat("rstd", torch.rsqrt(var + c.eps), c.r)
    y.backward(c.dy)
    U.assert_truth("dx", x.grad + c.dres, c.dx)
    U.assert_truth("dx gated", x.grad, c.dx_g)
    U.assert_truth("gout", x.grad * gate, c.gout)


def _layer_norm(x, eps):
    """F.layer_norm with the f32 statistics the reference's device kernels keep: ATen's CPU kernel
    saves mean and rstd in the input's dtype (bf16) for the backward unless the affine parameters
    are f32, so it gets an f32 weight of ones and bias of zeros (x 1 + 0 is exact)"""
    D = x.shape[-1]
    return F.layer_norm(x, (D,), torch.ones(D), torch.zeros(D), eps)


@pytest.mark.parametrize("D", U.WIDTHS_MOD)
@pytest.mark.parametrize("B,N,rpb", [(3, 7, 7), (2, 4, 4)])
def test_layernorm_emulator_is_the_oracle(D, B, N, rpb):
    c = U.mod_case("ln", D, B, N, rpb)
    shift, onep, _ = (_rows(t, c) for t in _mods(c))
    x = c.x.clone().requires_grad_(True)
    y = _layer_norm(x, c.eps) * onep + shift
    U.assert_truth("y", y.detach(), c.y)
    y.backward(c.dy)
    U.assert_truth("dx", x.grad, c.dx)


def _oracle_table(c):
    cos, sin = O.rope_freqs(c.grid, c.D, U.THETA, list(U.MAX_POS), BF16)
    return cos.reshape(c.M, c.D), sin.reshape(c.M, c.D)


@pytest.mark.parametrize("D", U.WIDTHS_QK)
@pytest.mark.parametrize("is_float,shared", [(False, False), (True, True)])
def test_rope_table_emulator_is_the_oracle(D, is_float, shared):
    c = U.qk_case(D, 3, 7, True, True, is_float, shared)
    cos, sin = _oracle_table(c)
    ec, es = (t[U.table_rows(c, 0 if shared else c.N)] for t in c.table)
    U.assert_truth("cos", cos, ec)
    U.assert_truth("sin", sin, es)
    tb = U.ROW_B
    assert torch.equal(cos[tb, U.twins(D)], cos[tb, U.twins(D) + 2])  # h = w on row B's token
    # the packed words and back
    words = U.pack_words(cos, sin)
    c2, s2 = U.unpack_cs(words.to(torch.int32), torch.arange(c.M))
    assert torch.equal(c2, cos.double()) and torch.equal(s2, sin.double())


@pytest.mark.parametrize("D", U.WIDTHS_QK)
@pytest.mark.parametrize("rope", [True, False])
def test_qk_emulator_is_the_oracle(D, rope):
    c = U.qk_case(D, 3, 7, True, rope, False, False)
    cos = sin = None
    if rope:
        cos, sin = _oracle_table(c)
    em = U.qk_emulate(c, *((cos.double(), sin.double()) if rope else ()))
    for x0, g, w0, e in zip(c.x, c.g, c.w, em):
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        out = O.rmsnorm(x, c.eps, w)
        if rope:
            out = O.apply_rotary_emb(out, cos, sin)
        U.assert_truth("out", out.detach(), e.y)
        out.backward(g)
        U.assert_truth("dx", x.grad, e.dx)
        # the f32 incoming gradient of the kernels is rounded to bf16 first: the same answer
        assert U.qk_bwd(g.float(), x0, w0, e.r, *((cos.double(), sin.double()) if rope else ())).v.equal(e.dx.v)
        gw = U.wgrad(g, x0, e.r.float(), torch.zeros(D, dtype=BF16), *((cos.double(), sin.double()) if rope else ()))
        U.assert_truth("dw", w.grad, gw, cap=1.0)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("rpg,G,D", [(7, 3, 24), (50, 3, 8), (136, 1, 24)])
def test_colsum_emulator_is_autograd(mode, rpg, G, D):
    """autograd's broadcast reductions: a [G, 1, D] parameter used by the rpg rows of its group (the
    AdaLN shift, scale and gate rows), then sst[None] + tmod summing the groups"""
    gen = torch.Generator().manual_seed(mode * 100 + rpg)
    M = G * rpg
    a = U.grid_vals((M, D), gen, False).bfloat16()
    b = U.grid_vals((M, D), gen, True).bfloat16()
    if mode == 3:
        bd = b.double()
        U._balance(bd)
        b = bd.bfloat16()
    sst = torch.zeros(D, dtype=BF16, requires_grad=True)
    tmod = torch.zeros(G, D, dtype=BF16, requires_grad=True)
    p = (sst[None] + tmod)[:, None]                               # [G, 1, D]
    p.retain_grad()
    r32 = mean32 = None
    if mode == 0:
        y = torch.zeros(G, rpg, D, dtype=BF16) + p
    elif mode == 1:
        y = b.view(G, rpg, D) * p
    elif mode == 2:
        r32 = torch.rsqrt(b.float().pow(2).mean(-1) + 1e-6)
        y = O.rmsnorm(b, 1e-6).view(G, rpg, D) * p
    else:
        mean32 = b.float().mean(-1)
        r32 = torch.rsqrt((b.float() - mean32[:, None]).pow(2).mean(-1) + 1e-6)
        y = _layer_norm(b, 1e-6).view(G, rpg, D) * p
    y.backward(a.view(G, rpg, D))
    per = U.colsum(a, b, r32, mean32, mode, rpg, sum_groups=False, accumulate=False)
    U.assert_truth("per group", tmod.grad, per, cap=1.0)
    tot = U.colsum(a, b, r32, mean32, mode, rpg, sum_groups=True, accumulate=False)
    U.assert_truth("summed", sst.grad, tot, cap=1.0)
    acc = U.colsum(a, b, r32, mean32, mode, rpg, sum_groups=True, accumulate=True, out0=sst.grad)
    U.assert_truth("accumulated", sst.grad + sst.grad, acc, cap=1.0)


def test_silu_and_batch_sum_emulators_are_torch():
    gen = torch.Generator().manual_seed(5)
    x = (torch.randint(-48, 49, (4096,), generator=gen).double() / 4).bfloat16().requires_grad_(True)
    dy, dres = U.grid_vals((4096,), gen, False).bfloat16(), U.grid_vals((4096,), gen, False).bfloat16()
    F.silu(x).backward(dy)
    U.assert_truth("silu_bwd", x.grad, U.silu_bwd(x.detach(), dy))
    U.assert_truth("silu_bwd + dres", x.grad + dres, U.silu_bwd(x.detach(), dy, dres))
    t = U.grid_vals((15, 136), gen, False).bfloat16()
    U.assert_truth("batch_sum", t.view(3, 5, 136).sum(0), U.batch_sum(t, 3))


# ------------------------------------------------------------------------------- builder checks
def test_builder_refuses_inexact_sums_and_open_cases():
    log = {}
    c = U.mod_case("rms", 2048, 3, 7, 7)
    assert max(c.log.values()) < U.EXACT
    print("\nD = 2048 sum |term| / grid: " + ", ".join("%s 2^%.1f" % (k, math.log2(v)) for k, v in sorted(c.log.items())))
    U.exact_sum("grid", U.grid_vals((4, 2048), torch.Generator().manual_seed(0), True) ** 2, log=log)
    with pytest.raises(U.Refused):  # generic f32 terms: no common grid
        U.exact_sum("randn", torch.randn(4, 2048, generator=torch.Generator().manual_seed(0)).float().double())
    with pytest.raises(U.Refused):  # 5 % of an output open
        v = torch.zeros(100)
        U._cap(types.SimpleNamespace(), y=U.Iv(v, v, torch.cat([torch.ones(5), torch.zeros(95)])))
    with pytest.raises(AssertionError):  # the comparator holds a launch to the cap as well
        U.assert_truth("y", v.bfloat16(), U.Iv(v, v, torch.cat([torch.ones(5), torch.zeros(95)])))


@pytest.mark.parametrize("kind", ["rms", "ln"])
def test_every_mod_case_builds_under_the_cap_with_rows_a_and_b(kind):
    worst = {}
    for r in U.rows_of("ltx_rmsnorm_modulate_fwd" if kind == "rms" else "ltx_layernorm_modulate_fwd"):
        c = U.mod_case(kind, r.p["D"], r.p["B"], r.p["N"], r.p["rpb"])  # runs check_known_rows and the cap
        assert max(c.log.values()) < U.EXACT
        for n, s in c.open.items():
            worst[n] = max(worst.get(n, (0, 0)), (s, r.p["D"]))
    print("\n%s: largest open share per output (share, D): %s" % (kind, worst))
    assert all(s <= U.OPEN_CAP for s, _ in worst.values())


# ------------------------------------------------------------------------------- planted faults
def _plant(name):
    """(output name, faulty emulator output, emulator output) on a builder case"""
    c = U.mod_case("rms", 520, 3, 7, 7)
    shift, onep, gate = _mods(c)
    if name in ("n_unrounded", "b_first_row", "clamped_chunk"):
        return "y", U.rms_fwd(c.x, shift, onep, 7, c.eps, fault=name)[0], c.y
    if name == "dx2_unrounded":
        return "dx", U.rms_bwd(c.dy, c.x, c.r, onep, 7, dres=c.dres, fault=name)[0], c.dx
    if name == "gout_unrounded_dx":
        ok = U.rms_bwd(c.dy, c.x, c.r, onep, 7, dres=c.dres, gate=gate)[1]
        return "gout", U.rms_bwd(c.dy, c.x, c.r, onep, 7, dres=c.dres, gate=gate, fault=name)[1], ok
    if name in ("pad_at_end", "neighbour_row"):
        q = U.qk_case(128, 3, 7, True, True, False, False)
        cos, sin = (t.double() for t in _oracle_table(q))
        return "q_out", U.qk_fwd(q.x[0], q.w[0], cos, sin, q.eps, fault=name)[0], U.qk_fwd(q.x[0], q.w[0], cos, sin, q.eps)[0]
    gen = torch.Generator().manual_seed(3)
    if name == "split_drops_last_row":
        q = U.qk_case(96, 4, 25, False, False, False, False)
        r32 = U.qk_fwd(q.x[0], q.w[0])[1].float()
        g0 = torch.zeros(96, dtype=BF16)
        return "gq", U.wgrad(q.g[0], q.x[0], r32, g0, fault=name), U.wgrad(q.g[0], q.x[0], r32, g0)
    assert name == "no_group_rbf"
    a = U.generic_bf16((3 * 50, 24), gen)
    return "sum", U.colsum(a, rpg=50, accumulate=False, fault=name), U.colsum(a, rpg=50, accumulate=False)


FAULTS = ("n_unrounded", "b_first_row", "clamped_chunk", "dx2_unrounded", "pad_at_end", "neighbour_row",
          "split_drops_last_row", "no_group_rbf", "gout_unrounded_dx")


def _old_criteria(name):
    """what tests/test_kernels_gpu.py's criteria say of the fault on randn inputs at its shapes:
    (criterion, value, threshold)"""
    with U.any_inputs():
        return _old_criteria_any(name)


def _old_criteria_any(name):
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).bfloat16()  # noqa: E731
    B, N, D = 2, 96, 2048
    x, dy, dres = rn(B * N, D), rn(B * N, D), rn(B * N, D)
    mod = rn(B, 6, D, scale=D ** -0.5) + rn(B, 6, D)
    shift, onep, gate = mod[:, 0], 1 + mod[:, 1], mod[:, 5]
    if name in ("n_unrounded", "b_first_row", "clamped_chunk"):
        Dd = 520 if name == "clamped_chunk" else D  # D = 2048 has no partial pass: the shape cannot show it
        args = (x[:, :Dd].contiguous(), shift[:, :Dd], onep[:, :Dd], N, 1e-6)
        bad, ok = U.rms_fwd(*args, fault=name)[0].v, U.rms_fwd(*args)[0].v
        return "ulps_bad(y, ref, 1) < 1e-3", U.ulps_bad(bad.bfloat16(), ok.bfloat16()), 1e-3
    if name in ("dx2_unrounded", "gout_unrounded_dx"):
        r = U.rms_fwd(x, shift, onep, N, 1e-6)[1]
        i = 0 if name == "dx2_unrounded" else 1
        bad = U.rms_bwd(dy, x, r, onep, N, dres=dres, gate=gate, fault=name)[i].v
        ok = U.rms_bwd(dy, x, r, onep, N, dres=dres, gate=gate)[i].v
        return ("rel(dx, ref) < 5e-3", U.rel(bad, ok), 5e-3) if i == 0 else \
            ("torch.equal(gout, gate_mul(dx))", float((bad != ok).double().mean()), 0.0)
    if name in ("pad_at_end", "neighbour_row"):
        B, N = 2, 60
        grid = O.latent_coords(3, 4, 5, B)
        cos, sin = (t.reshape(B * N, D).double() for t in O.rope_freqs(grid, D, U.THETA, list(U.MAX_POS), BF16))
        q, w = rn(B * N, D), rn(D, scale=0.1) + 1
        bad, ok = U.qk_fwd(q, w, cos, sin, fault=name)[0].v, U.qk_fwd(q, w, cos, sin)[0].v
        return "rel(q_out, ref) < 5e-3", U.rel(bad, ok), 5e-3
    return "e_b <= 1.25 e_r + 1e-2 (whole-model gradients)", float("nan"), 1e-2


def test_comparator_fails_planted_faults_and_what_the_old_criteria_say():
    lines = []
    for name in FAULTS:
        out, bad, ok = _plant(name)
        with pytest.raises(AssertionError, match="differ from the emulator"):
            U.assert_truth(out, bad.v.bfloat16(), ok)
        n = int((bad.v.bfloat16().double() != ok.v).sum())
        crit, val, thr = _old_criteria(name)
        verdict = "no kernel test" if val != val else ("catches" if val > thr or (thr == 0 and val > 0) else "passes")
        lines.append("| %s | %s: %d of %d elements | %s | %.2e | %s |" % (name, out, n, ok.v.numel(), crit, val, verdict))
    print("\n| planted fault | truth comparator (builder inputs) | old criterion (randn, today's shape) | value | old verdict |")
    print("|---|---|---|---|---|")
    print("\n".join(lines))


# ------------------------------------------------------------------------------------- coverage
def test_the_gpu_table_covers_every_entry_point_and_variant():
    have = {r.entry for r in U.CASES}
    assert have == set(U.ENTRIES), set(U.ENTRIES) ^ have
    mod = U.rows_of("ltx_rmsnorm_modulate_fwd") + U.rows_of("ltx_layernorm_modulate_bwd")
    for kind in ("rms", "ln"):
        assert {r.p["D"] for r in mod if r.p["kind"] == kind} == set(U.WIDTHS_MOD)
        assert {(r.p["B"], r.p["N"], r.p["rpb"]) for r in mod if r.p["kind"] == kind} == {(3, 7, 7), (2, 4, 4), (3, 7, 0)}
    assert all(r.p["ld_mod"] == 6 * r.p["D"] and r.p["dres"] == (True, False) and r.p["out_given"] for r in mod)
    for entry in ("ltx_qk_norm_rope_fwd", "ltx_qk_norm_rope_bwd"):
        qk = U.rows_of(entry)
        assert {r.p["D"] for r in qk} == set(U.WIDTHS_QK) and {r.p["pad"] for r in qk} == {0, 2, 4}
        for pad in (0, 2, 4):
            rs = [r for r in qk if r.p["pad"] == pad]
            assert {r.p["rope"] for r in rs} == {"spec", "pair", None}
            assert {r.p["grid"] for r in rs} == {"int64", "float", None}
            assert {r.p["shared"] for r in rs} == {True, False} and {r.p["has_k"] for r in rs} == {True, False}
            assert {(r.p["dq"], bool(r.p["rope"])) for r in rs} >= {("bf16", True), ("f32", True), ("f32", False)}
            assert {r.p["dk"] for r in rs} == {"bf16", "f32", None}
            assert any(r.p["fused_in"] for r in rs) and any(r.p["strided_out"] for r in rs)
    assert {r.p["pad"] for r in U.rows_of("ltx_rope_table")} == {0, 2, 4}
    assert {r.p["pad"] for r in U.rows_of("ltx_rope_pack_bf16")} == {0, 2, 4}
    gr = U.rows_of("ltx_qk_norm_bwd_grouped")
    assert {r.p["D"] for r in gr} == {64, 2048} and all(r.p["G"] == 3 and r.p["rows"] == 5 and r.p["strided"]
                                                        and r.p["in_place"] for r in gr)
    wg = U.rows_of("ltx_qk_norm_wgrad")
    assert {r.p["B"] * r.p["N"] for r in wg} == {21, 100}
    assert {(r.p["has_k"], r.p["rope"]) for r in wg} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {r.p["dtype"] for r in wg} == {"f32", "bf16"} and all(r.p["accumulate_nonzero"] for r in wg)
    assert U.splits(100, 2) == 12 and 100 % 12 != 0  # uneven splits
    cs = U.rows_of("ltx_group_colsum")
    assert {(r.p["mode"], r.p["rpg"], r.p["G"], r.p["D"]) for r in cs} == \
        {(m, r, g, d) for m in range(4) for r in (7, 50, 136) for g in (1, 3) for d in (8, 24, 2056)}
    assert {r.p["S"] for r in cs if r.p["G"] == 1} == {1, 6, 17}
    assert all(r.p["sum_groups"] == (True, False) and r.p["accumulate"] == (True, False) for r in cs)
    assert {r.p["n"] for r in U.rows_of("ltx_silu_bwd_bf16")} == {37, 4096 * 256 + 40}
    assert {r.p["cols"] for r in U.rows_of("ltx_batch_sum_bf16")} == {8, 136}
    assert {(r.p["D"], r.p["broadcast"]) for r in U.rows_of("ltx_ada_modulation")} == \
        {(d, b) for d in (8, 520) for b in (True, False)}


def test_every_qk_case_builds_under_the_cap_with_rows_a_and_b():
    worst, sums = {}, {}
    for r in U.rows_of("ltx_qk_norm_rope_fwd"):
        p = r.p
        c = U.qk_case(p["D"], p["B"], p["N"], p["has_k"], p["rope"] is not None, p["grid"] == "float", p["shared"])
        for e in c.em:  # qk_emulate: the cap, rows A and B, the exact sums
            for n, s in e.open.items():
                worst[n] = max(worst.get(n, (0, 0)), (s, p["D"]))
        for n, s in getattr(c, "open", {}).items():
            worst[n] = max(worst.get(n, (0, 0)), (s, p["D"]))
        for n, v in c.log.items():
            sums[n] = max(sums.get(n, 0), v)
    print("\nqk: largest open share per output (share, D): %s\nsums: %s" % (worst, sums))
    assert all(s <= U.OPEN_CAP for s, _ in worst.values())
    assert sums["sum x^2"] < U.EXACT
