"""GEMM truth tests (DESIGN "GEMM truth tests"): every route of plan_gemm and every fused epilogue
on inputs whose answer is known exactly (tests/gemm_truth_utils.py). One launch per row; every output
is a view inside a sentinel-filled buffer and must equal the float64 reference bit for bit (the
GELU rows: every element within one bf16 value, every code within 1), with the sentinel around it
untouched and the split-K workspace NaN before the call. tests/test_gemm_truth_cpu.py constructs
the same cases without a GPU and shows the comparator failing ten planted faults."""
import pytest
import torch

import gemm_truth_utils as U
from gemm_truth_utils import ROWS, Guarded, assert_gelu, assert_truth, build

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _label(row):
    """the dispatcher's kernel for the row under its variant (the name cache does not key on it)"""
    from ltx_amd import _lib, ops
    _lib.load().ltx_gemm_set_variant(row.variant)
    ops._GEMM_NAMES.clear()
    try:
        rank = row_rank(row)
        return ops.gemm_kernel_name(row.M, row.N, row.K, row.K2, row.epi, rank)
    finally:
        _lib.load().ltx_gemm_set_variant(0)
        ops._GEMM_NAMES.clear()


def row_rank(row):
    r = [int(o[1:]) for o in row.opt if o[0] == "r" and o[1:].isdigit()]
    return r[0] if r else (32 if "hd32" in row.opt else 64 if row.epi == "store_rowdot" else 0)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_gemm_truth(row):
    from ltx_amd import _lib, ops
    assert {k: ops.EPI[k] for k in U.EPI} == U.EPI
    assert _label(row) == row.label
    b = build(row, DEV)
    kw, want, M, N = dict(b.kw), b.want, row.M, row.N
    a, w = kw.pop("a"), kw.pop("w")
    guards = {"C": Guarded((M, N), torch.bfloat16, DEV)}
    if b.alias:  # C aliases R: the accumulator is updated in place
        guards["C"].view.copy_(kw["aux0"])
        kw["aux0"] = guards["C"].view
    if "aux2" in want:
        guards["aux2"] = Guarded((M, N), torch.bfloat16, DEV)
        kw["aux2"] = guards["aux2"].view
    if "code" in row.opt:
        guards["code"] = Guarded((M, N), torch.int16, DEV)
        kw["aux0"] = guards["code"].view
    if "delta" in want:
        guards["delta"] = Guarded(tuple(want["delta"].shape), torch.float32, DEV, dense=True)
        kw["aux1"] = guards["delta"].view
    ws = ops._gemm_workspace(a.device)
    ws.fill_(float("nan"))  # a split-K tail that reads a slice nobody wrote cannot match
    _lib.load().ltx_gemm_set_variant(row.variant)
    try:
        out = ops.gemm(a, w, out=guards["C"].view, **kw)
        torch.cuda.synchronize()
    finally:
        _lib.load().ltx_gemm_set_variant(0)
    assert out.data_ptr() == guards["C"].view.data_ptr()
    # the partials of a split-K row are in the workspace; any other row left it alone
    assert bool(torch.isnan(ws[:M * N]).any()) != row.split, "split-K " + ("did not run" if row.split else "ran")
    if row.epi == "gelu":
        code = guards["code"] if "code" in guards else None
        worst = assert_gelu(out, None if code is None else code.view, want["y"], row.id, guards["C"], code)
        print("\nGEMM_TRUTH_GELU | %s | %s | %d | %d | %s |" % (row.id, row.label, worst[0], worst[1],
                                                              worst[2] if code is not None else "-"))
        return
    for name in ("C", "aux2", "delta"):
        if name in want:
            assert_truth(guards[name].view, want[name], "%s %s" % (row.id, name), guards[name], row.tile)


def test_case_table_names_every_route():
    """No launch: the dispatcher's plan for every row. Together the rows name the 128 x 128 kernel with
    2 and 3 LDS stages and with split-K, the 256-row split-K kernel, gemm_nt_kernel_t at 224 and 256 rows and
    the ring kernel at both heights with every K-extension length: a dispatcher change that drops
    a route from the table fails here."""
    ran = set()
    for row in ROWS:
        assert _label(row) == row.label, row.id
        ran.add(U.family(row))
    assert set(U.FAMILIES) <= ran, set(U.FAMILIES) - ran
    names = {r.label.split("<")[0] + "<.., " + ", ".join(r.label.split("(")[0].rstrip(">").split(", ")[2:]) + ">" for r in ROWS}
    for need in ["ltx::gemm_nt_kernel<.., 3>", "ltx::gemm_nt_kernel<.., 2>", "ltx::gemm_nt_kernel_t<.., 256, 8, 1>",
                 "ltx::gemm_nt_kernel_t<.., 224, 4, 0>", "ltx::gemm_nt_kernel_t<.., 256, 8, 0>"] + \
                ["ltx::gemm_ring_kernel<.., %d, %d>" % (h, t2) for h in (7, 8) for t2 in U.RING_T2]:
        assert need in names, (need, sorted(names))
