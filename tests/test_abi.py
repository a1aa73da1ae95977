"""The C-ABI library loads on the host (no GPU needed) and exports every symbol declared in
include/ltx_hip.h; the Python binding table matches the header. No compute calls here."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ltx_hip.h")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(ltx_\w+)\s*\(", src, flags=re.M)))


def test_header_declares_entry_points():
    names = header_functions()
    assert "ltx_gemm_bf16_nt" in names and "ltx_attn_fwd" in names and len(names) >= 25


def test_library_exports_every_declared_symbol():
    from ltx_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build() first")
    lib = _lib.load()
    for name in header_functions():
        assert hasattr(lib, name), name
    assert set(header_functions()) == set(_lib.exported_symbols())
    assert lib.ltx_abi_version() == 1


def test_ops_refuse_cpu_tensors():
    import torch
    from ltx_amd import ops, _lib
    x = torch.zeros(128, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.LtxHipError):
        ops.gemm(x, x)


def test_gemm_describe_names_the_dispatched_kernel():
    """ltx_gemm_describe (host-only: the dispatcher's plan, no launch) names the kernel rocprof
    reports for the config-A shapes, which is what bench.py's roofline attributes timings to."""
    import ctypes
    from ltx_amd import _lib
    lib = _lib.load()

    def name(M, N, K, K2=0, epi="store", rank=0):
        buf = ctypes.create_string_buffer(256)
        assert lib.ltx_gemm_describe(M, N, K, K2, _lib.EPI[epi], rank, None, buf, 256) == 0
        return buf.value.decode()
    M = 8 * 1792
    # N = 2048 tiles: 64 x 8 = 512 of 224 rows fill two rounds exactly; the ring kernel by default
    assert name(M, 2048, 8192) == "ltx::gemm_ring_kernel<0, 0, 7, 0>(ltx::GemmParams)"
    assert name(M, 8192, 2048, epi="gelu") == "ltx::gemm_ring_kernel<1, 0, 8, 0>(ltx::GemmParams)"
    assert name(M, 2048, 2048, K2=64) == "ltx::gemm_ring_kernel<0, 0, 7, 1>(ltx::GemmParams)"
    # K % 128 != 0 keeps gemm_nt_kernel_t; variant 15 selects it everywhere
    assert name(M, 2048, 2112) == "ltx::gemm_nt_kernel_t<0, 0, 224, 4, 0>(ltx::GemmParams)"
    assert lib.ltx_gemm_set_variant(15) == 0
    try:
        assert name(M, 2048, 8192) == "ltx::gemm_nt_kernel_t<0, 0, 224, 4, 0>(ltx::GemmParams)"
        assert name(M, 8192, 2048, epi="gelu") == "ltx::gemm_nt_kernel_t<1, 0, 256, 8, 0>(ltx::GemmParams)"
    finally:
        lib.ltx_gemm_set_variant(0)
    # the text side (M = 256 rows) runs the 128x128 kernel with three LDS stages
    assert name(256, 4096, 2048, K2=128).startswith("ltx::gemm_nt_kernel<0, 0, 3>")


def test_gemm_set_variant_rejects_removed_schedules():
    """Only the kernel / tile-height knobs remain (0 / 13 / 14 / 15 / 20); the not-adopted
    schedules are no longer in the library (tools/experiments/)."""
    from ltx_amd import _lib
    lib = _lib.load()
    assert lib.ltx_gemm_set_variant(13) == 0
    assert lib.ltx_gemm_set_variant(0) == 0
    assert lib.ltx_gemm_set_variant(15) == 0
    assert lib.ltx_gemm_set_variant(20) == 0
    for v in (21, 22, 30, 40, 50, 60):
        assert lib.ltx_gemm_set_variant(v) != 0
    assert lib.ltx_gemm_set_variant(0) == 0


def test_bench_traffic_lookup_reads_newest_profile():
    """bench.py's roofline.traffic comes from the newest committed profiles/r*_traffic.json, with
    kernel names compared after dropping the argument list and trailing default (0) template
    arguments, and names the file it used."""
    import glob
    import importlib.util
    import json
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(repo, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench._kernel_key("void ltx::gemm_nt_kernel_t<0, 0, 224, 4, 0>(ltx::GemmParams)") == \
        "ltx::gemm_nt_kernel_t<0,0,224,4>"
    newest = sorted(glob.glob(os.path.join(repo, "profiles", "r*_traffic.json")))[-1]
    table = json.load(open(newest))["bytes_per_launch"]
    name, val = max(((k, v) for k, v in table.items() if k.startswith("ltx::gemm_")),
                    key=lambda kv: kv[1])
    got, src = bench.load_traffic(name + "(ltx::GemmParams)")
    assert src == os.path.basename(newest) and got == val
    got, why = bench.load_traffic("ltx::no_such_kernel<1>")
    assert got is None and "no entry" in why


def test_bench_dump_sample_is_fixed_and_bounded(tmp_path):
    """bench.py --dump-outputs: small outputs are written whole, in order, as float32; beyond
    DUMP_MAX_ELEMS every tensor gives its share at the same seeded positions in every call, so two
    runs' files line up element for element and stay under the size cap."""
    import importlib.util
    import os

    import numpy as np
    import torch
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(repo, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = torch.arange(6, dtype=torch.bfloat16).view(2, 3)
    b = torch.tensor(7.0)
    whole = bench._sampled_f32([a, b])
    assert whole.dtype == np.float32 and whole.tolist() == [0, 1, 2, 3, 4, 5, 7]
    cap = bench.DUMP_MAX_ELEMS
    big = [torch.arange(cap, dtype=torch.float32), torch.arange(3 * cap, dtype=torch.float32), torch.ones(1)]
    s1, s2 = bench._sampled_f32(big), bench._sampled_f32([t.clone() for t in big])
    assert np.array_equal(s1, s2)
    n0, n1 = cap * cap // (4 * cap + 1), 3 * cap * cap // (4 * cap + 1)
    assert s1.size == n0 + n1 + 1 and s1.nbytes <= 16 * 2 ** 20 + 4 * len(big)
    # positions ascend within each tensor's share, and the values are the sampled elements themselves
    assert (np.diff(s1[:n0]) >= 0).all() and s1[:n0].max() < cap
    assert (np.diff(s1[n0:n0 + n1]) >= 0).all() and s1[n0:n0 + n1].max() >= cap
    bench.dump_outputs(str(tmp_path / "d"), {"x": whole})
    assert np.array_equal(np.load(tmp_path / "d" / "x.npy"), whole)


@pytest.fixture
def attn_switches():
    """set(**{name without LTX_ATTN_: value}): exactly these switches in the environment, then
    ltx_attn_reload_switches(). Afterwards the environment is restored and the library reads it
    again, so later tests find the table their environment describes."""
    from ltx_amd import _lib, ops
    lib = _lib.load()
    with pytest.MonkeyPatch.context() as mp:
        def set_(**kw):
            for name in ops._ATTN_ENV:
                mp.delenv(name, raising=False)
            for k, v in kw.items():
                mp.setenv("LTX_ATTN_" + k, str(v))
            assert lib.ltx_attn_reload_switches() == 0
        yield set_
    assert lib.ltx_attn_reload_switches() == 0


def test_attn_switch_table_is_the_librarys():
    """ops._ATTN_ENV (whose changes make ops reload the switches) is the library's own table."""
    from ltx_amd import _lib, ops
    lib = _lib.load()
    names = []
    while (n := lib.ltx_attn_switch_name(len(names))) is not None:
        names.append(n.decode())
    assert lib.ltx_attn_switch_name(-1) is None
    assert tuple(names) == ops._ATTN_ENV and len(names) == 18 and len(set(names)) == 18
    assert all(n.startswith("LTX_ATTN_") for n in names)


# (switches, (B, H, Nq, Nk), call options, forward kernel or None, backward kernels or None), each
# "ltx::" + the name; "ws": "big" a 128-MiB workspace on the call's stream, "small" 1 MiB, None none
_W1P = "attn_dkdv_w1p_kernel<0> + attn_dq_w1p_kernel<0>"
_SELF, _CROSS, _FEWBH = (2, 3, 1000, 512), (8, 32, 1792, 256), (2, 4, 1792, 256)
_ATTN_DESCRIBE = [
    # head dim 32 (the tiny config): the 4-wave tiled kernels, biased when Nk % 64 != 0
    ({}, (1, 3, 100, 128), dict(d=32), "attn_q_kernel<32, 0, false, 4>",
     "attn_dkdv_kernel<32, false, 4> + attn_q_kernel<32, 1, false, 4>"),
    ({}, (1, 3, 100, 77), dict(d=32), "attn_q_kernel<32, 0, true, 4>",
     "attn_dkdv_kernel<32, true, 4> + attn_q_kernel<32, 1, true, 4>"),
    ({"W8": 3}, (1, 3, 100, 128), dict(d=32, bias=True), "attn_q_kernel<32, 0, true, 4>",
     "attn_dkdv_kernel<32, true, 4> + attn_q_kernel<32, 1, true, 4>"),
    # Nk <= 256: the one-pass kernels; H * B >= 128 is one workgroup per (batch, head)
    ({}, _CROSS, {}, "attn_fwd1_kernel<64, false, true>", "attn_bwd1_kernel<64, false, false>"),
    ({}, _CROSS, dict(bias=True), "attn_fwd1_kernel<64, true, true>", "attn_bwd1_kernel<64, true, false>"),
    ({}, _CROSS, dict(ready=False), None, "attn_delta_kernel<64> + attn_bwd1_kernel<64, false, false>"),
    ({"FWD1_ROWS": 0}, _CROSS, {}, "attn_fwd1_kernel<64, false, false>", None),
    ({"FWD1_ROWS": 0}, _CROSS, dict(bias=True), "attn_fwd1_kernel<64, true, false>", None),
    # H * B < 128 and >= 4 query tiles: split over the queries when the partials fit the workspace
    ({}, _FEWBH, {}, "attn_fwd1_kernel<64, false, true>",
     "attn_bwd1_kernel<64, false, false> + attn_bwd1_finish_kernel<64>"),
    ({}, _FEWBH, dict(bias=True), "attn_fwd1_kernel<64, true, true>",
     "attn_bwd1_kernel<64, true, false> + attn_bwd1_finish_kernel<64>"),
    ({}, _FEWBH, dict(ws=None), None, "attn_bwd1_kernel<64, false, false>"),
    ({}, _FEWBH, dict(ws=None, bias=True), None, "attn_bwd1_kernel<64, true, false>"),
    ({}, _FEWBH, dict(ws="small"), None, "attn_bwd1_kernel<64, false, false>"),  # S = 14: 14.7 MB
    ({}, (2, 4, 192, 256), {}, None, "attn_bwd1_kernel<64, false, false>"),      # 3 query tiles
    ({"QSPLIT": 0}, _FEWBH, {}, None, "attn_bwd1_kernel<64, false, false>"),
    ({"BWD1_QS": 1}, _CROSS, dict(bias=True), None, "attn_bwd1_kernel<64, true, true>"),
    ({"BWD1_QS": 1}, _CROSS, {}, None, "attn_bwd1_kernel<64, false, false>"),
    ({"BWD1_QS": 1}, _FEWBH, dict(bias=True), None,
     "attn_bwd1_kernel<64, true, false> + attn_bwd1_finish_kernel<64>"),
    ({"BWD1_QS": 1}, _FEWBH, dict(bias=True, ws=None), None, "attn_bwd1_kernel<64, true, true>"),
    # ragged Nk = 200 and Nk = 128: biased instantiations without a key bias
    ({}, (1, 2, 300, 200), dict(ws=None), "attn_fwd1_kernel<64, true, true>", "attn_bwd1_kernel<64, true, false>"),
    ({}, (8, 32, 1792, 128), {}, "attn_fwd1_kernel<64, false, true>", "attn_bwd1_kernel<64, true, false>"),
    # the one-pass paths off: the tiled / pipelined kernels at Nk = 256
    ({"FWD1": 0}, _CROSS, {}, "attn_fwd_pipe_kernel<true>", None),
    ({"FWD1": 0}, _CROSS, dict(bias=True), "attn_q_kernel<64, 0, true, 8>", None),
    ({"BWD1": 0}, _CROSS, {}, None, _W1P),
    ({"BWD1": 0}, _CROSS, dict(bias=True), None, "attn_dkdv_pipe_kernel<true, 4> + attn_q_kernel<64, 1, true, 4>"),
    ({"BWD1": 0}, (1, 2, 300, 200), {}, None, "attn_dkdv_pipe_kernel<true, 4> + attn_q_kernel<64, 1, true, 4>"),
    # Nk = 512 without bias: forward pipe; backward pipe / w1 / w1p per LTX_ATTN_{DKDV,DQ}_W1 0 / 1 / 2
    ({}, _SELF, {}, "attn_fwd_pipe_kernel<true>", _W1P),
    ({}, _SELF, dict(ready=False), None, "attn_delta_kernel<64> + " + _W1P),
    ({"FWD_F32SUM": 0}, _SELF, {}, "attn_fwd_pipe_kernel<false>", None),
    ({"FWD_PIPE": 0}, _SELF, {}, "attn_q_kernel<64, 0, false, 8>", None),
    ({"FWD_PIPE": 0, "W8": 0}, _SELF, {}, "attn_q_kernel<64, 0, false, 4>", None),
    ({"FWD_W1": 1}, _SELF, {}, "attn_fwd_pipe_kernel<true>", None),  # not a fwdw1 build
    ({}, _SELF, dict(bias=True), "attn_q_kernel<64, 0, true, 8>",
     "attn_dkdv_pipe_kernel<true, 4> + attn_q_kernel<64, 1, true, 4>"),
    ({"DKDV_W1": 1}, _SELF, {}, None, "attn_dkdv_w1_kernel<0> + attn_dq_w1p_kernel<0>"),
    ({"DKDV_W1": 0}, _SELF, {}, None, "attn_dkdv_pipe_kernel<false, 4> + attn_dq_w1p_kernel<0>"),
    ({"DQ_W1": 1}, _SELF, {}, None, "attn_dkdv_w1p_kernel<0> + attn_dq_w1_kernel<0>"),
    ({"DQ_W1": 0}, _SELF, {}, None, "attn_dkdv_w1p_kernel<0> + attn_dq_pipe_kernel<4>"),
    ({"DQ_W1": "02"}, _SELF, {}, None, _W1P),  # atoi, not a string prefix
    ({"DQ_W1": 0, "DQ_PIPE": 0}, _SELF, {}, None, "attn_dkdv_w1p_kernel<0> + attn_q_kernel<64, 1, false, 4>"),
    ({"DQ_W1": 0, "DQ_NBUF": 3}, _SELF, {}, None, "attn_dkdv_w1p_kernel<0> + attn_dq_pipe_kernel<3>"),
    ({"DKDV_W1": 0, "DKDV_NBUF": 3}, _SELF, {}, None, "attn_dkdv_pipe_kernel<false, 3> + attn_dq_w1p_kernel<0>"),
    ({"DKDV_NBUF": 3}, _SELF, dict(bias=True), None, "attn_dkdv_pipe_kernel<true, 3> + attn_q_kernel<64, 1, true, 4>"),
    # the stamped variants 12 / 13 / 22 exist in diag builds only: here the kernels they time
    ({"DKDV_W1": 12, "DQ_W1": 13}, _SELF, {}, None, "attn_dkdv_w1_kernel<0> + attn_dq_w1_kernel<0>"),
    ({"DKDV_W1": 22, "DQ_W1": 22}, _SELF, {}, None, _W1P),
    # the persistent kernels' limits: f32 dQ, 63 items per workgroup (x 256 CUs), 4-GiB descriptors
    ({}, _SELF, dict(f32=True), None, "attn_dkdv_w1p_kernel<0> + attn_dq_w1_kernel<0>"),
    ({}, (8, 32, 16384, 512), {}, None, "attn_dkdv_w1p_kernel<0> + attn_dq_w1_kernel<0>"),
    ({}, (8, 32, 512, 16384), {}, None, "attn_dkdv_w1_kernel<0> + attn_dq_w1p_kernel<0>"),
    ({}, (1, 2, 512, 2048), dict(ldk=1 << 20), None, "attn_dkdv_w1p_kernel<0> + attn_dq_w1_kernel<0>"),
    ({}, (1, 2, 2048, 512), dict(lddo=1 << 20), None, "attn_dkdv_w1_kernel<0> + attn_dq_w1p_kernel<0>"),
    # LTX_ATTN_W8: bit 0 the 8-wave tiled forward, bit 1 the 8-wave dK/dV (with the plain dQ)
    ({"W8": 0}, _SELF, dict(bias=True), "attn_q_kernel<64, 0, true, 4>",
     "attn_dkdv_pipe_kernel<true, 4> + attn_q_kernel<64, 1, true, 4>"),
    ({"W8": 1}, _SELF, {}, "attn_fwd_pipe_kernel<true>", _W1P),
    ({"W8": 2}, _SELF, {}, "attn_fwd_pipe_kernel<true>", "attn_dkdv_kernel<64, false, 8> + attn_q_kernel<64, 1, false, 4>"),
    ({"W8": 2}, _SELF, dict(bias=True), "attn_q_kernel<64, 0, true, 4>",
     "attn_dkdv_kernel<64, true, 8> + attn_q_kernel<64, 1, true, 4>"),
    ({"W8": 3}, _SELF, dict(bias=True), "attn_q_kernel<64, 0, true, 8>",
     "attn_dkdv_kernel<64, true, 8> + attn_q_kernel<64, 1, true, 4>"),
    ({"DKDV_PIPE": 0}, _SELF, {}, None, "attn_dkdv_kernel<64, false, 4> + attn_q_kernel<64, 1, false, 4>"),
    ({"DKDV_PIPE": 0}, _SELF, dict(bias=True), None, "attn_dkdv_kernel<64, true, 4> + attn_q_kernel<64, 1, true, 4>"),
    # switches that change a kernel's arguments, not the kernel
    ({"XCD": 0, "SKIP": 0, "BWD1_FEW": 0}, _CROSS, dict(bias=True), "attn_fwd1_kernel<64, true, true>",
     "attn_bwd1_kernel<64, true, false>"),
]


def test_attn_describe_names_the_dispatched_kernels(attn_switches):
    """ltx_attn_describe (host only: the plan ltx_attn_fwd / ltx_attn_bwd_ex launch from) over a
    table that reaches every branch of both planners. Without a device the CU count the persistent
    kernels' item limit uses falls back to 256, the MI355X's own. The workspace is a never
    dereferenced address registered under made-up stream handles; the default one is not touched."""
    import ctypes
    from ltx_amd import _lib
    lib = _lib.load()
    streams = {"big": (0x51A0, 128 << 20), "small": (0x51B0, 1 << 20), None: (0x51C0, 0)}
    for handle, nbytes in streams.values():
        assert lib.ltx_gemm_set_stream_workspace(ctypes.c_void_p(handle), ctypes.c_void_p(0x10000 if nbytes else 0),
                                                 nbytes) == 0

    def describe(backward, shape, d=64, bias=False, f32=False, ready=True, ws="big", ldk=0, lddo=0):
        B, H, Nq, Nk = shape
        buf = ctypes.create_string_buffer(512)
        assert lib.ltx_attn_describe(backward, B, H, Nq, Nk, d, int(bias), int(f32), int(ready), H * d, ldk or H * d,
                                     H * d, lddo or H * d, ctypes.c_void_p(streams[ws][0]), buf, 512) == 0
        return buf.value.decode()

    def named(kernels):
        return " + ".join("ltx::" + k for k in kernels.split(" + "))
    try:
        for sw, shape, opts, fwd, bwd in _ATTN_DESCRIBE:
            attn_switches(**sw)
            if fwd is not None:
                assert describe(0, shape, **opts) == named(fwd), (sw, shape, opts)
            if bwd is not None:
                assert describe(1, shape, **opts) == named(bwd), (sw, shape, opts)
        buf = ctypes.create_string_buffer(8)
        assert lib.ltx_attn_describe(0, 1, 1, 64, 64, 48, 0, 0, 1, 48, 48, 48, 48, None, buf, 8) != 0  # head dim
    finally:
        for handle, _ in streams.values():
            lib.ltx_gemm_set_stream_workspace(ctypes.c_void_p(handle), None, 0)


# ---- the LoRA adapter dispatch plan (csrc/lora_plan.h) through ltx_lora_describe, host only. The expected
# kernels are written from the dispatch code of the commit before the plan existed; {R} is the rank.
# (op, M, N, K, options, kernels): options groups (0: the one-adapter entry), ws ("big" 128 MiB on the call's
# stream, "small" 64 KiB, "huge" 1 GiB, None none)
_FULL, _DY1 = "lora_rows_full_kernel<{R}, 2, %d, 5>", "lora_dy_kernel<{R}, 1> + lora_dy_finish_kernel<{R}>"
_ROWS, _WG = "lora_rows_kernel<{R}, 4, 4>", "lora_wgrad_kernel<{R}>"
_LORA_ROUTES = [
    # ltx_lora_rows: the whole contraction per block at token-sized M and K = 512 / 1024 / 2048
    ("rows", 2048, 0, 512, {}, _FULL % 1),
    ("rows", 2048, 0, 1024, {}, _FULL % 2),
    ("rows", 2048, 0, 2048, {}, _FULL % 4),
    # any other K % 512 == 0: the column-split pass + finish while its partials (3 x 2048 x max(r, 16) f32:
    # 384 KiB at r = 16) fit the stream's workspace
    ("rows", 2048, 0, 1536, {}, _DY1),
    ("rows", 2048, 0, 1536, dict(ws="small"), _ROWS),
    ("rows", 2048, 0, 1536, dict(ws=None), _ROWS),
    # M < 2048, K % 512 != 0, M % 32 != 0
    ("rows", 2016, 0, 512, {}, _ROWS),
    ("rows", 2048, 0, 256, {}, _ROWS),
    ("rows", 2050, 0, 512, {}, _ROWS),
    # ltx_lora_rows_grouped: one launch on the whole-contraction route, else the one-adapter plan per group
    ("rows", 2048, 0, 512, dict(groups=3), "lora_rows_full_grouped_kernel<{R}, 2, 1, 5>"),
    ("rows", 2016, 0, 512, dict(groups=3), " + ".join([_ROWS] * 3)),
    # ltx_lora_wgrad: the dB product of lora_dy_kernel at token-sized M; below it row splits + finish (2016 rows:
    # 8 splits of 256) while the partials fit the workspace, else one split; 200 rows are one split anyway
    ("wgrad", 2048, 512, 0, {}, "lora_dy_kernel<{R}, 2> + lora_dy_finish_kernel<{R}>"),
    ("wgrad", 2016, 512, 0, {}, _WG + " + lora_wgrad_finish_kernel"),
    ("wgrad", 2016, 512, 0, dict(ws=None), _WG),
    ("wgrad", 200, 128, 0, {}, _WG),
    ("wgrad", 2048, 512, 0, dict(ws=None), _WG),
    ("wgrad", 2048, 512, 0, dict(groups=2), _WG + " + lora_wgrad_finish_kernel"),  # grouped: never the dY route
    # ltx_lora_down: <R, RG, KW>, RG = 2 from M = 8192 on, KW = 8 where K % 256 == 0
    ("down", 48, 0, 128, {}, "lora_down_kernel<{R}, 1, 4>"),
    ("down", 48, 0, 256, {}, "lora_down_kernel<{R}, 1, 8>"),
    ("down", 8192, 0, 128, {}, "lora_down_kernel<{R}, 2, 4>"),
    ("down", 8192, 0, 256, {}, "lora_down_kernel<{R}, 2, 8>"),
    ("down", 8192, 0, 256, dict(groups=3), "lora_down_kernel<{R}, 2, 8>"),
    # the dY family: the dY pass, the x pass from its partials (MODE 6 up to N = 2048, 14 beyond), one finish
    ("dy", 32, 512, 0, {}, "lora_dy_kernel<{R}, 3> + lora_dy_finish_kernel<{R}>"),
    ("dy_dA", 2048, 512, 512, {}, "lora_dy_kernel<{R}, 3> + lora_dy_kernel<{R}, 6> + lora_dy_finish_kernel<{R}>"),
    ("dy_dA", 2048, 2560, 512, {}, "lora_dy_kernel<{R}, 3> + lora_dy_kernel<{R}, 14> + lora_dy_finish_kernel<{R}>"),
    ("dy_dA", 2048, 512, 512, dict(groups=3),
     "lora_dy_grouped_kernel<{R}, 3> + lora_dy_grouped_kernel<{R}, 6> + lora_dy_finish_grouped_kernel<{R}>"),
]
_LORA_ALL_RANKS = {"rows": 0, "wgrad": 11, "down": 17, "dy": 22, "dy_dA": 23}  # row of _LORA_ROUTES run at every rank
_LORA_WS = {"big": (0x10A0, 128 << 20), "small": (0x10B0, 64 << 10), None: (0x10C0, 0), "huge": (0x10D0, 1 << 30)}


def _lora_describe(lib, op, M, N, K, r, groups=0, ws="big", split=False):
    """(return code, the kernels with "ltx::" taken off each)"""
    import ctypes
    from ltx_amd import _lib
    buf = ctypes.create_string_buffer(512)
    rc = lib.ltx_lora_describe(_lib.LORA_OP[op], M, N, K, 0, 0, 0, r, groups, int(split),
                               ctypes.c_void_p(_LORA_WS[ws][0]), buf, 512)
    names = buf.value.decode().split(" + ")
    assert rc != 0 or all(n.startswith("ltx::") for n in names)
    return rc, " + ".join(n[5:] for n in names)


@pytest.fixture
def lora_lib():
    """the library with never dereferenced workspaces registered under made-up stream handles (the default
    workspace, which GPU tests of the same process rely on, is not touched)"""
    import ctypes
    from ltx_amd import _lib
    lib = _lib.load()
    try:
        for handle, nbytes in _LORA_WS.values():
            assert lib.ltx_gemm_set_stream_workspace(ctypes.c_void_p(handle), ctypes.c_void_p(0x10000 if nbytes else 0),
                                                     nbytes) == 0
        yield lib
    finally:
        for handle, _ in _LORA_WS.values():
            lib.ltx_gemm_set_stream_workspace(ctypes.c_void_p(handle), None, 0)


def test_lora_describe_names_the_dispatched_kernels(lora_lib):
    """ltx_lora_describe (host only: the plan every ltx_lora_* launcher launches from) over a table with a row for
    every branch of every route at the smallest shape that takes it, at r = 16 and r = 64, and every rank on one
    row per operation. With and without the split operand the kernels are the same."""
    from ltx_amd import ops
    for i, (op, M, N, K, opts, want) in enumerate(_LORA_ROUTES):
        ranks = ops.LORA_RANKS if i == _LORA_ALL_RANKS[op] else (16, 64)
        for r in ranks:
            for split in ((False, True) if op in ("rows", "down") else (False,)):
                assert _lora_describe(lora_lib, op, M, N, K, r, split=split, **opts) == (0, want.replace("{R}", str(r))), \
                    (op, M, N, K, opts, r, split)
    # r = 64 at (2048, 1536): the partials are 1.5 MiB, the 64-KiB workspace is too small for r = 8 too
    assert _lora_describe(lora_lib, "rows", 2048, 0, 1536, 8, ws="small")[1] == "lora_rows_kernel<8, 4, 4>"
    assert _lora_describe(lora_lib, "dy", 2048, 500, 0, 16)[0] != 0  # N % 512
    assert _lora_describe(lora_lib, "rows", 2048, 0, 384, 16)[0] != 0                    # ltx_lora_rows wants K % 256
    assert _lora_describe(lora_lib, "dy_dA", 2048, 2560, 512, 16, groups=3)[0] != 0       # grouped: N <= 2048
    assert _lora_describe(lora_lib, "rows", 2048, 0, 512, 16, groups=5)[0] != 0


def test_lora_ranks_are_the_librarys(lora_lib):
    """ops.LORA_RANKS is exactly the set of ranks ltx_lora_describe accepts, for every operation; a rank outside
    it is rejected by every *_workspace entry as well."""
    import ctypes
    from ltx_amd import ops
    shapes = {"down": (48, 0, 128), "rows": (2048, 0, 512), "wgrad": (2048, 512, 0), "dy": (32, 512, 0),
              "dy_dA": (2048, 512, 512)}
    n = ctypes.c_int64(0)
    for op, (M, N, K) in shapes.items():
        assert tuple(r for r in range(0, 260) if _lora_describe(lora_lib, op, M, N, K, r)[0] == 0) == ops.LORA_RANKS
    for r in list(range(0, 260)):
        ok = r in ops.LORA_RANKS
        assert (lora_lib.ltx_lora_dy_workspace(2048, 512, r, ctypes.byref(n)) == 0) == ok
        assert (lora_lib.ltx_lora_dy_dA_workspace(2048, 512, 512, r, ctypes.byref(n)) == 0) == ok
        assert (lora_lib.ltx_lora_dy_dA_grouped_workspace(2048, 512, 512, r, 3, ctypes.byref(n)) == 0) == ok


def test_lora_dy_workspace_sizes(lora_lib):
    """The three *_workspace entries against the formula written out: CS M RP + RS N RP (+ RS K RP) floats per
    group, RP = max(r, 16), CS = N / 512, RS = ceil(M / (32 G)), G = 7 up to r = 16 and 4 above."""
    import ctypes
    from ltx_amd import ops
    n = ctypes.c_int64(0)
    cols = (512, 2048, 2560, 8192)
    for r in ops.LORA_RANKS:
        RP, G = max(r, 16), 7 if r <= 16 else 4
        for M in (32, 2016, 2048, 14336):
            RS = -(-M // (32 * G))
            for N in cols:
                dy = (N // 512) * M * RP + RS * N * RP
                assert lora_lib.ltx_lora_dy_workspace(M, N, r, ctypes.byref(n)) == 0 and n.value == dy, (M, N, r)
                for K in cols:
                    assert lora_lib.ltx_lora_dy_dA_workspace(M, N, K, r, ctypes.byref(n)) == 0
                    assert n.value == dy + RS * K * RP, (M, N, K, r)
                    for groups in (1, 3, 4):
                        assert lora_lib.ltx_lora_dy_dA_grouped_workspace(M, N, K, r, groups, ctypes.byref(n)) == 0
                        assert n.value == groups * (dy + RS * K * RP), (M, N, K, r, groups)
    assert lora_lib.ltx_lora_dy_dA_grouped_workspace(2048, 512, 512, 16, 5, ctypes.byref(n)) != 0


def test_lora_python_gates_follow_the_plan(lora_lib, monkeypatch):
    """The gates ops decides per call without asking the library, against the plan: lora_dy_da_fits(y, x, r) holds
    exactly where ltx_lora_wgrad(x, w), given its workspace, takes the lora_dy_kernel<R, 2> route (so the merged
    call is bitwise the separate ones), and lora_rows_gate only where ltx_lora_rows accepts the call."""
    import torch
    from ltx_amd import ops
    monkeypatch.delenv("LTX_LORA_DY_DA", raising=False)
    cols = (512, 2048, 2560, 8192)
    for r in ops.LORA_RANKS:
        for M in (2016, 2048, 8160, 8192):
            for K in cols:
                x = torch.empty(M, K, dtype=torch.bfloat16, device="meta")
                # a workspace that holds the partials of every row (256 MiB at M = 8192, K = 8192, r = 128)
                rc, names = _lora_describe(lora_lib, "wgrad", M, K, 0, r, ws="huge")
                dy_route = rc == 0 and names == f"lora_dy_kernel<{r}, 2> + lora_dy_finish_kernel<{r}>"
                for N in cols:
                    y = torch.empty(M, N, dtype=torch.bfloat16, device="meta")
                    assert ops.lora_dy_da_fits(y, x, r) == dy_route, (M, N, K, r)
            for K in cols + (128, 384, 640):
                assert ops.lora_rows_gate(M, K) == (M >= 8192 and K % 256 == 0)
                if ops.lora_rows_gate(M, K):
                    assert _lora_describe(lora_lib, "rows", M, 0, K, r)[0] == 0, (M, K, r)
    assert not ops.lora_dy_da_fits(torch.empty(2048, 512, device="meta"), torch.empty(2048, 512, device="meta"), 24)
    assert (ops.LORA_ROWS_MIN_M, ops.LORA_TOKEN_ROWS, ops.LORA_DY_COLS) == (8192, 2048, 512)


_LORA_SWITCH_CHILD = """
import ctypes, sys
from ltx_amd import _lib
lib = _lib.load()
assert lib.ltx_gemm_set_workspace(ctypes.c_void_p(0x10000), 128 << 20) == 0
buf = ctypes.create_string_buffer(512)
op, M, N, K = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
assert lib.ltx_lora_describe(_lib.LORA_OP[op], M, N, K, 0, 0, 0, 16, 0, 0, None, buf, 512) == 0
print(buf.value.decode())
"""


@pytest.mark.parametrize("env,call,want", [
    ({}, ("wgrad", 2048, 512, 0), "ltx::lora_dy_kernel<16, 2> + ltx::lora_dy_finish_kernel<16>"),
    ({"LTX_LORA_WGRAD_ROWS": "0"}, ("wgrad", 2048, 512, 0), "ltx::lora_wgrad_kernel<16> + ltx::lora_wgrad_finish_kernel"),
    ({"LTX_LORA_ROWS_DY": "0"}, ("rows", 2048, 0, 512), "ltx::lora_rows_kernel<16, 4, 4>"),
    ({"LTX_LORA_ROWS_FULL": "0"}, ("rows", 2048, 0, 512), "ltx::lora_dy_kernel<16, 1> + ltx::lora_dy_finish_kernel<16>"),
])
def test_lora_library_switches(env, call, want):
    """LTX_LORA_WGRAD_ROWS / LTX_LORA_ROWS_DY / LTX_LORA_ROWS_FULL are read once per process, so each is asked in a
    fresh one (host only)."""
    import subprocess
    import sys
    names = ("LTX_LORA_WGRAD_ROWS", "LTX_LORA_ROWS_DY", "LTX_LORA_ROWS_FULL")
    child_env = {k: v for k, v in os.environ.items() if k not in names}
    child_env.update(env, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    out = subprocess.run([sys.executable, "-c", _LORA_SWITCH_CHILD, *map(str, call)], env=child_env, check=True,
                         capture_output=True, text=True, timeout=120)
    assert out.stdout.strip().splitlines()[-1] == want
