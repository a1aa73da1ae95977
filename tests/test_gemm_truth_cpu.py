"""CPU half of the GEMM truth tests (DESIGN "GEMM truth tests"): the float64 reference of every
epilogue against an independent integer evaluation, every row of the GPU table constructed with its
conditions met (so no row can be refused for the first time on the GPU machine), the comparator
against ten planted faults, and what the suite's older criteria say of the same faults."""
import types

import pytest
import torch

import gemm_truth_utils as U
from gemm_truth_utils import ROWS, Row, assert_truth, build, rbf

BY_ID = {r.id: r for r in ROWS}


# ------------------------------------------------------------- an independent evaluation, tiny cases
def rne_bf16(x):
    """round to nearest even by hand, on the f32 bit pattern (x: float64 holding f32 values)"""
    assert torch.equal(x.float().double(), x)
    b = x.float().view(torch.int32).long() & 0xFFFFFFFF
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b)
    return b.to(torch.int32).view(torch.float32).double()


def integer_reference(row):
    """The outputs of a row from an int64 matmul (in units of the case's grid), Python loops over the
    batches and rne_bf16: shares no rounding and no product with gemm_truth_utils.build."""
    b = build(row)
    c, kw = b.case, b.kw
    unit = int(round(1.0 / c.scale))
    ints = lambda t: (t.double() * unit).round().long()  # noqa: E731
    P = c.A.long() @ ints(c.W).t()
    if c.ext is not None:
        P += c.ext[0].long() @ ints(c.ext[1]).t()
    if kw["bias"] is not None:
        P += ints(kw["bias"])
    y = rne_bf16(P.double() / unit)
    M, N, rpb = row.M, row.N, row.rpb
    out = {}
    if row.epi == "store":
        out["C"] = y
    elif row.epi == "gelu":
        out["y"] = y
    elif row.epi == "gated_residual":
        C = torch.empty(M, N, dtype=torch.float64)
        for bi in range(M // rpb):
            rows = slice(bi * rpb, (bi + 1) * rpb)
            C[rows] = rne_bf16(kw["aux0"][rows].double() + rne_bf16(kw["aux1"][bi].double() * y[rows]))
        out["C"] = C
        if "aux2" in row.opt:
            out["aux2"] = y
    elif row.epi == "gelu_bwd":
        prod = y * kw["aux0"].double()                          # exact: under 2^24
        f32 = (prod * float(torch.tensor(2.0 / 32767.0, dtype=torch.float32))).float().double()  # one f32 rounding
        out["C"] = rne_bf16(f32)
    elif row.epi == "accum":
        out["C"] = rne_bf16(kw["aux0"].double() + y)
        if "gate" in row.opt:
            out["aux2"] = torch.cat([rne_bf16(out["C"][bi * rpb:(bi + 1) * rpb] * kw["aux1"][bi].double())
                                     for bi in range(M // rpb)])
    elif row.epi == "store_rowdot":
        hd = kw["rank"]
        out["C"] = y
        d = torch.zeros(M // rpb, N // hd, rpb, dtype=torch.float64)
        yo = (y * kw["aux0"].double())
        for m in range(M):
            for h in range(N // hd):
                d[m // rpb, h, m % rpb] = yo[m, h * hd:(h + 1) * hd].sum()
        out["delta"] = d
    elif row.epi in ("lora", "lora_residual"):
        s = kw["aux1"].long() @ kw["aux2"].long().t()
        t = rne_bf16(y + s.double() / 2)
        out["C"] = rne_bf16(kw["aux0"].double() + t) if row.epi == "lora_residual" else t
    elif row.epi == "lora_dgrad_accum":
        s = kw["aux1"].long() @ kw["aux2"].long()
        t = rne_bf16(y + rne_bf16(s.double() / 2))
        out["C"] = rne_bf16(kw["aux0"].double() + t) if "res" in row.opt else t
    return b, out


def _tiny_rows():
    rows = []
    for epi, opt in U.EPILOGUES + (("store_rowdot", ("hd32",)), ("lora", ("bias", "r8")), ("lora_residual", ("bias", "r16")),
                                   ("lora_dgrad_accum", ("r32",)), ("lora_dgrad_accum", ("r8", "res"))):
        N = 64 if epi == "store_rowdot" else 40
        rows.append(Row("tiny-%s%s" % (epi, "".join("-" + o for o in opt)), "tiny", 36, N, 192, 64, epi, tuple(opt),
                        0, 12, "", False, (128, 128)))
    return rows


@pytest.mark.parametrize("row", _tiny_rows(), ids=lambda r: r.id)
def test_reference_against_integer_evaluation(row):
    b, out = integer_reference(row)
    assert set(out) == set(b.want)
    for name, t in out.items():
        assert torch.equal(t, b.want[name]), (name, int((t != b.want[name]).sum()))


def test_float64_to_bf16_rounds_ties_to_even():
    """what the reference relies on: .to(bfloat16) of a float64 rounds ties to even and agrees with
    float64 -> f32 -> bf16 and with the hand-written rounding on the values the cases produce"""
    x = torch.cat([torch.arange(-1200, 1201, dtype=torch.float64) / 2, torch.arange(-600, 601, dtype=torch.float64) / 16,
                   torch.tensor([257.0, 259.0, 261.0, 263.0, 129.5, 130.5, 200.5, 201.5], dtype=torch.float64)])
    assert torch.equal(rbf(x), rne_bf16(x))
    assert torch.equal(rbf(x), x.float().to(torch.bfloat16).double())
    assert float(rbf(torch.tensor([261.0], dtype=torch.float64))) == 260.0
    assert float(rbf(torch.tensor([263.0], dtype=torch.float64))) == 264.0
    ties = dict(up=0, down=0)
    rbf(torch.tensor([129.5, 130.5, -129.5, 3.0, 128.25], dtype=torch.float64), ties)
    assert ties == dict(up=1, down=2)


def test_gelu_reference_keeps_the_negative_tail():
    """the float64 GELU of the GPU file: the textbook form where that is accurate, and in the tail
    the small negative values that 1 + tanh u loses (a first version of this reference returned -0
    from y = -6.6 down and refused a kernel that was right)"""
    y = torch.arange(-255, 256, dtype=torch.float64) / 16.0
    u = U.GELU_K * (y + 0.044715 * y ** 3)
    mid = y.abs() <= 4
    naive = 0.5 * y * (1.0 + torch.tanh(u))
    assert float(((U.gelu_tanh64(y) - naive)[mid]).abs().max()) < 1e-14
    tail = U.gelu_tanh64(torch.tensor([-7.25], dtype=torch.float64))
    assert -1.1e-16 < float(tail) < -1.0e-16
    yy = y.clone().requires_grad_(True)
    U.gelu_tanh64(yy).sum().backward()
    assert float((yy.grad - U.gelu_tanh_grad64(y)).abs().max()) < 1e-14
    aten = torch.ops.aten.gelu_backward(torch.ones_like(y), y, approximate="tanh")
    assert float((aten - U.gelu_tanh_grad64(y))[mid].abs().max()) < 1e-13


# -------------------------------------------------------------------------- every table row constructs
SHAPES = sorted({(r.M, r.N) for r in ROWS})


@pytest.mark.parametrize("M,N", SHAPES)
def test_every_row_of_the_shape_constructs(M, N):
    """build() asserts the three conditions; rows that share operands, epilogue and options (the
    same case on another route) are built once. The caches are dropped per shape."""
    seen = set()
    try:
        for row in ROWS:
            key = (row.K, row.K2, row.epi, row.opt, row.rpb)
            if (row.M, row.N) != (M, N) or key in seen:
                continue
            seen.add(key)
            b = build(row)
            assert b.case.max_acc <= 255.0 and b.case.bound < 2.0 ** 24
            assert b.want
    finally:
        for f in (U.operands, U.aux_operands, U.lora_operands):
            f.cache_clear()
    assert seen


def test_table_names_every_family():
    have = {U.family(r) for r in ROWS}
    assert set(U.FAMILIES) <= have, set(U.FAMILIES) - have
    for r in ROWS:
        if r.epi in ("gated_residual", "store_rowdot") or "gate" in r.opt:
            assert r.M % r.rpb == 0 and (r.M <= 256 or r.tile[0] % r.rpb != 0), r.id


# ----------------------------------------------------------------------------------- planted faults
def model_of(row, randn=False):
    """The operands of a row as float64, from the row's exact case or, randn, as dense random bf16
    values of the same shapes (what the older tests feed the kernels)."""
    b = build(row)
    c, kw = b.case, b.kw
    m = types.SimpleNamespace(row=row, exact=not randn, want=b.want)
    names = dict(A=c.A, W=c.W, bias=kw["bias"], R=kw.get("aux0"), gate=kw.get("aux1"),
                 A2=None if c.ext is None else c.ext[0], W2=None if c.ext is None else c.ext[1])
    if row.epi == "store_rowdot":
        names.update(O=kw["aux0"], R=None)
    gen = torch.Generator().manual_seed(row.M + row.N)
    for n, t in names.items():
        if t is not None and randn:
            t = torch.randn(t.shape, generator=gen) / (t.shape[1] ** 0.5 if n in ("W", "W2") else 1.0)
            t = t.to(torch.bfloat16)
        setattr(m, n, None if t is None else t.double())
    if m.bias is None:
        m.bias = torch.zeros(row.N, dtype=torch.float64)
    m.P = m.A @ m.W.t()
    if m.A2 is not None:
        if c.ext_group is None:
            m.P += m.A2 @ m.W2.t()
        else:
            for g in range(2):
                m.P[:, g * 256:(g + 1) * 256] += m.A2[:, _gcols(row, g)] @ m.W2[g * 256:(g + 1) * 256].t()
    return m


def _gcols(row, g):
    return slice(g * (row.K2 + 8), g * (row.K2 + 8) + row.K2)


def evaluate(m, P=None, bias=None, gate_rows=None, rnd=rbf):
    """the row's outputs from the model's operands, with the pieces a fault replaces"""
    row = m.row
    y = rnd((m.P if P is None else P) + (m.bias if bias is None else bias))
    if gate_rows is None and m.gate is not None:
        gate_rows = m.gate[torch.arange(row.M) // row.rpb]
    if row.epi == "store":
        return dict(C=y)
    if row.epi == "gated_residual":
        out = dict(C=rnd(m.R + rnd(gate_rows * y)))
        if "aux2" in row.opt:
            out["aux2"] = y
        return out
    if row.epi == "accum":
        out = dict(C=rnd(m.R + y))
        if "gate" in row.opt:
            out["aux2"] = rnd(out["C"] * gate_rows)
        return out
    if row.epi == "store_rowdot":
        return dict(C=y, delta=U.rowdot64(y, m.O, row.rpb, 64))
    raise ValueError(row.epi)


def truncate(x):
    """f64 -> bf16 by dropping the low 16 bits of the f32 pattern"""
    b = x.float().view(torch.int32) & -65536
    return b.view(torch.float32).double()


def _last_k_tile(m):
    P = m.P.clone()
    P[128:256, :128] -= m.A[128:256, -64:] @ m.W[:128, -64:].t()
    return "C", evaluate(m, P=P)["C"]


def _extension_group(m):
    P = m.P.clone()
    P[:, 256:] -= m.A2[:, _gcols(m.row, 1)] @ m.W2[256:].t()
    return "C", evaluate(m, P=P)["C"]


def _rows_swapped(m):
    C = evaluate(m)["C"]
    C[[3, 77]] = C[[77, 3]]
    return "C", C


def _ragged_tile_neighbour(m):
    C = evaluate(m)["C"]
    C[256:300] = C[128:172].clone()
    return "C", C


def _gate_of_previous_batch(m):
    g = m.gate[torch.arange(m.row.M) // m.row.rpb]
    g[100:128] = m.gate[0]  # tile 0 holds rows 0..127, the batch changes at row 100
    return "C", evaluate(m, gate_rows=g)["C"]


def _bias_shifted(m):
    return "C", evaluate(m, bias=torch.roll(m.bias, 8))["C"]


def _truncation(m):
    return "C", evaluate(m, rnd=truncate)["C"]


def _split_slice(m):
    P = m.P.clone()
    P[:128, :128] -= m.A[:128, 256:] @ m.W[:128, 256:].t()  # the second of two 256-deep slices
    return "C", evaluate(m, P=P)["C"]


def _delta_index(m):
    d = evaluate(m)["delta"]
    f = d.clone()
    f[1, 1:] = d[1, :-1]  # m in place of m % rows_per_batch: every head of batch 1 lands one head on
    f[1, 0] = float("nan") if m.exact else 0.0
    return "delta", f


def _aux2_unwritten(m):
    a = evaluate(m)["aux2"]
    a[256:300, 128:136] = float(torch.tensor([U.SENT16], dtype=torch.int16).view(torch.bfloat16)) if m.exact else 0.0
    return "aux2", a


FAULTS = [
    ("the last 64-wide K tile dropped for one output tile", "small3-300x136x128-store-bias", _last_k_tile),
    ("the K extension dropped for one 256-column group", "small3-300x512x128+64-store-bias-group", _extension_group),
    ("two rows swapped inside one tile", "small3-300x136x128-store-bias", _rows_swapped),
    ("the ragged last row tile holds its neighbour's rows", "small3-300x136x128-store-bias", _ragged_tile_neighbour),
    ("the gate row of batch b-1 after a batch boundary inside a tile", "small3-300x136x128-gated_residual-bias",
     _gate_of_previous_batch),
    ("bias shifted by 8 columns", "small3-300x136x128-store-bias", _bias_shifted),
    ("truncation instead of round-to-nearest-even", "small3-300x136x128-accum", _truncation),
    ("one split-K slice omitted for one tile", "small-splitk-200x136x512-store-bias", _split_slice),
    ("delta stored at m instead of m % rows_per_batch in the second batch", "small3-300x192x128-store_rowdot", _delta_index),
    ("aux2 left unwritten in the last tile", "small3-300x136x128-gated_residual-bias-aux2", _aux2_unwritten),
]


@pytest.mark.parametrize("what,rid,fault", FAULTS, ids=[f[2].__name__.strip("_") for f in FAULTS])
def test_comparator_fails_planted_faults(what, rid, fault):
    m = model_of(BY_ID[rid])
    clean = evaluate(m)
    for name, t in clean.items():  # the model's own evaluation is the table's reference
        assert torch.equal(t, m.want[name]), name
    name, faulty = fault(m)
    dtype = torch.float32 if name == "delta" else torch.bfloat16
    assert assert_truth(clean[name].to(dtype), m.want[name], what)
    with pytest.raises(AssertionError, match="differ"):
        assert_truth(faulty.to(dtype), m.want[name], what)


def test_guard_notices_a_write_outside_the_view():
    g = U.Guarded((10, 16), torch.bfloat16, "cpu")
    assert g.untouched() and g.view.shape == (10, 16) and g.view.stride(0) == 32
    g.view.fill_(1.0)
    assert g.untouched()
    g.bits[12, 8] = 0  # the row after the last
    assert not g.untouched()
    d = U.Guarded((2, 3, 5), torch.float32, "cpu", dense=True)
    d.view.fill_(2.0)
    assert d.untouched() and d.view.is_contiguous()
    d.bits[64 + 30] = 0
    assert not d.untouched()


def test_present_criteria_on_random_inputs(capsys):
    """What the criteria of tests/test_kernels_gpu.py (rel-Frobenius < 1e-2, ulps_bad(., ., 2) < 1e-3)
    say of the ten faults on dense random inputs of the same shapes, the faulty output against the
    clean one. Printed for profiles/gemm_truth.md; nothing is asserted about the content."""
    lines = ["| planted fault on randn inputs | shape (M, N, K) | rel-Frobenius (< 1e-2) | share > 2 ulp (< 1e-3) |",
             "|---|---|---|---|"]
    for what, rid, fault in FAULTS:
        row = BY_ID[rid]
        m = model_of(row, randn=True)
        clean = evaluate(m)
        name, faulty = fault(m)
        a, b = faulty, clean[name]
        r = float((a - b).norm() / b.norm())
        cell = "n/a (f32)"
        if name != "delta":
            ai, bi = (t.to(torch.bfloat16).view(torch.int16).int() for t in (a, b))
            u = float(((ai - bi).abs() > 2).float().mean())
            cell = "%.2e %s" % (u, "passes" if u < 1e-3 else "catches")
        lines.append("| %s | (%d, %d, %d%s) | %.2e %s | %s |" % (what, row.M, row.N, row.K, " + %d" % row.K2 if row.K2 else "",
                                                                  r, "passes" if r < 1e-2 else "catches", cell))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert len(lines) == 12
