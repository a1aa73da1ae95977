"""Every attention kernel of the default build against inputs whose exact answer is known
(tests/attn_truth_utils.py, DESIGN "Attention truth tests"): O, dQ, dK and dV must equal the float64
reference bit for bit, lse within 2^-12, on the kernel each row of the case table names in its
launch label. The backward runs twice: on the kernel's own o and lse (end to end) and on the
reference o, lse and a ready delta, so a backward fault is neither masked nor caused by a forward
one. profiles/attn_truth.md records the table with the labels it ran and the measured lse errors.
"""
import contextlib
import json
import os

import pytest
import torch

import attn_truth_utils as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
TAU0_LIB = os.path.join(os.path.dirname(HERE), "video-generation-for-human-avatars_amd", "ltx_amd",
                        "libltxhip_tau0.so")

# every kernel of LTX_ATTN_KERNELS_MAIN and LTX_ATTN_KERNELS_PIPE (csrc/attn_plan.h) and both delta
# kernels, written out: a kernel added to the dispatch later fails the coverage test until the case
# table has a row for it
KERNELS = [
    "attn_fwd1_kernel<64, false, false>", "attn_fwd1_kernel<64, false, true>",
    "attn_fwd1_kernel<64, true, false>", "attn_fwd1_kernel<64, true, true>",
    "attn_q_kernel<32, 0, false, 4>", "attn_q_kernel<32, 0, true, 4>",
    "attn_q_kernel<32, 1, false, 4>", "attn_q_kernel<32, 1, true, 4>",
    "attn_q_kernel<64, 0, false, 4>", "attn_q_kernel<64, 0, true, 4>",
    "attn_q_kernel<64, 1, false, 4>", "attn_q_kernel<64, 1, true, 4>",
    "attn_q_kernel<64, 0, false, 8>", "attn_q_kernel<64, 0, true, 8>",
    "attn_dkdv_kernel<32, false, 4>", "attn_dkdv_kernel<32, true, 4>",
    "attn_dkdv_kernel<64, false, 4>", "attn_dkdv_kernel<64, true, 4>",
    "attn_dkdv_kernel<64, false, 8>", "attn_dkdv_kernel<64, true, 8>",
    "attn_bwd1_kernel<64, false, false>", "attn_bwd1_kernel<64, true, false>",
    "attn_bwd1_kernel<64, true, true>", "attn_bwd1_finish_kernel<64>",
    "attn_fwd_pipe_kernel<false>", "attn_fwd_pipe_kernel<true>",
    "attn_dkdv_pipe_kernel<false, 3>", "attn_dkdv_pipe_kernel<false, 4>",
    "attn_dkdv_pipe_kernel<true, 3>", "attn_dkdv_pipe_kernel<true, 4>",
    "attn_dq_pipe_kernel<3>", "attn_dq_pipe_kernel<4>",
    "attn_dkdv_w1_kernel<0>", "attn_dkdv_w1p_kernel<0>", "attn_dq_w1_kernel<0>", "attn_dq_w1p_kernel<0>",
    "attn_delta_kernel<64>", "attn_delta_kernel<32>",
]


@pytest.fixture(scope="module", autouse=True)
def _dev():
    from ltx_amd import _lib as L
    L.ensure_device()


@contextlib.contextmanager
def library(path):
    """Route ltx_amd.ops through another build of the library for the duration."""
    from ltx_amd import _lib as L
    saved = L._lib
    L._lib = None
    try:
        L.load(path)
        yield
    finally:
        L._lib = saved


def _switches(row, monkeypatch):
    """the row's switches and no other: one left in the caller's environment would pick another kernel"""
    from ltx_amd import ops
    for name in ops._ATTN_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in row.env.items():
        assert "LTX_ATTN_" + name in ops._ATTN_ENV, name
        monkeypatch.setenv("LTX_ATTN_" + name, value)


def _names(label):
    return [n.replace("ltx::", "") for n in label.split(": ", 1)[1].split(" + ")]


def _device_inputs(row):
    c = U.case_inputs(row)
    D = row.H * row.d
    if row.fused:  # Q, K and V read in place from one fused [M, 3 * H * d] projection buffer
        buf = torch.full((max(c.q.shape[0], c.k.shape[0]), 3 * D), 3.0, dtype=torch.bfloat16, device=DEV)
        q, k, v = buf[:c.q.shape[0], :D], buf[:c.k.shape[0], D:2 * D], buf[:c.k.shape[0], 2 * D:]
        for view, t in ((q, c.q), (k, c.k), (v, c.v)):
            view.copy_(t)
    else:
        q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
    bias = None if c.key_bias is None else c.key_bias.to(DEV)
    return c, q, k, v, c.do.to(DEV), bias


def _forward(row, c, q, k, v, bias):
    from ltx_amd import ops
    (o, lse), lab = U.labelled(ops.attn_fwd, q, k, v, c.B, c.H, c.d, c.scale, key_bias=bias, kv_shared=c.shared)
    assert len(lab) == 1 and all(n in _names(lab[0]) for n in row.fwd), (row.fwd, lab)
    return o, lse, lab[0]


def _report(**line):
    path = os.environ.get("LTX_ATTN_TRUTH_REPORT")  # one JSON line per case, for profiles/attn_truth.md
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


@pytest.mark.parametrize("row", U.CASES, ids=[r.id for r in U.CASES])
def test_attention_truth(row, monkeypatch):
    from ltx_amd import ops
    _switches(row, monkeypatch)
    c, q, k, v, do, bias = _device_inputs(row)
    o, lse, lab_f = _forward(row, c, q, k, v, bias)
    errs = U.check_outputs(c, U.SEED, dict(o=o, lse=lse))
    kw = dict(key_bias=bias, kv_shared=c.shared, dq_f32=row.dq_f32)
    # end to end: the backward on the kernel's own o and lse, the delta pass included
    grads, lab_b = U.labelled(ops.attn_bwd, q, k, v, o, do, lse, c.B, c.H, c.d, c.scale, **kw)
    assert len(lab_b) == 1 and "attn_delta_kernel<%d>" % c.d in _names(lab_b[0]), lab_b
    assert all(n in _names(lab_b[0]) for n in row.bwd), (row.bwd, lab_b)
    U.check_outputs(c, U.SEED, dict(zip(("dq", "dk", "dv"), grads)))
    # the backward alone: the reference o and lse and its delta, ready
    o_ref, lse_ref = c.ref.o.float().bfloat16().to(DEV), c.ref.lse.float().to(DEV)
    grads, lab_r = U.labelled(ops.attn_bwd, q, k, v, o_ref, do, lse_ref, c.B, c.H, c.d, c.scale,
                              delta=c.ref.delta.float().contiguous().to(DEV), **kw)
    assert len(lab_r) == 1 and _names(lab_r[0]) == [n for n in _names(lab_b[0]) if "attn_delta_kernel" not in n], (lab_r, lab_b)
    U.check_outputs(c, U.SEED, dict(zip(("dq", "dk", "dv"), grads)))
    _report(id=row.id, fwd=_names(lab_f), bwd=_names(lab_b[0]), lse_err=errs["lse"],
            lse_err_exact_batches=float((lse.cpu().double() - c.ref.lse)[[b for b in range(c.B) if b not in c.noisy]].abs().max()))


def test_case_table_names_every_kernel(monkeypatch):
    """No launch: the dispatcher's own plan (ltx_attn_describe) for every row of the table, with
    and without a ready delta; together the rows name every kernel of the default build."""
    from ltx_amd import ops
    ops._gemm_workspace(torch.device(DEV, torch.cuda.current_device()))  # the query-split plans ask for it
    seen = set()
    for row in U.CASES:
        with monkeypatch.context() as mp:
            _switches(row, mp)
            ld = (3 if row.fused else 1) * row.H * row.d
            args = (U.B, row.H, row.Nq, row.Nk, row.d, row.keep is not None)
            seen.update(_names(ops.attn_kernel_label(False, *args)))
            for ready in (False, True):
                seen.update(_names(ops.attn_kernel_label(True, *args, row.dq_f32, ready, ld, ld, ld, row.H * row.d)))
            for n in row.fwd + row.bwd:
                assert n in KERNELS, (row.id, n)
    assert sorted(set(KERNELS) - seen) == [], "kernels without a case"
    assert sorted(seen - set(KERNELS)) == [], "kernels the list does not know"


TAU0_ROWS = [r for r in U.CASES if r.id.startswith(U.TAU0_TAGS)]


@pytest.mark.parametrize("row", TAU0_ROWS, ids=[r.id for r in TAU0_ROWS])
def test_attention_truth_forward_tau0_build(row, monkeypatch):
    """The forward rows under the RESCALE_TAU = 0 build (every growth of the running max rescales):
    the answers are exact, so both builds return the same bits."""
    if not os.path.exists(TAU0_LIB):
        return  # a test-only build: nothing to compare without it
    _switches(row, monkeypatch)
    c, q, k, v, _, bias = _device_inputs(row)
    o, lse, _ = _forward(row, c, q, k, v, bias)
    with library(TAU0_LIB):
        o0, lse0, _ = _forward(row, c, q, k, v, bias)
    U.check_outputs(c, U.SEED, dict(o=o0, lse=lse0))
    assert torch.equal(o, o0) and torch.equal(lse, lse0)
