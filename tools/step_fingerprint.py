"""Fingerprint of one step per model configuration (and, group `optim`, of three optimizer steps per
optimizer condition; group `attn`, of direct attention calls per shape and LTX_ATTN_* switch; group `lora`, of
direct adapter calls per route of csrc/lora_plan.h), to hold a refactor to equality.

    python tools/step_fingerprint.py run --pkg <dir that holds ltx_amd/> --group <name> --out fp.json
    python tools/step_fingerprint.py compare old.json new.json [--md table.md]

`run` imports ltx_amd from --pkg (another commit's Python sources beside the same built library:
set LTX_HIP_LIB to the library) in a fresh process, sets the group's environment switches before the
import (several are read at import), and for every configuration of the group runs one step under
ops.LaunchTimer. It writes the ordered kernel names, SHA-256 of the loss, of the model output and of
every gradient of grads_by_canonical, and torch.cuda.max_memory_allocated() of the step. Training
steps here are bitwise reproducible (fixed-order sums), so two commits that compute the same thing
give identical files. `compare` merges the per-group files of two commits into one verdict per
configuration: identical kernel lists and hashes, and a peak no higher than the old one.

The models come from the test helpers (tests/model_utils.py, lora_attn1_utils.py, lora_ff_utils.py,
lora_dora_utils.py); the tiny configurations use the inputs of tests/golden/tiny_lora_ff_step.
"""
import argparse
import gc
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
R_TINY, R_2B = 8, 16

TINY = ["fwd", "fwd_AttentionSkip", "fwd_AttentionValues", "fwd_Residual", "fwd_TransformerBlock",
        "attn2_shared", "attn2_per_sample", "attn1", "attn1+attn2", "attn2+ff", "all3", "all3_dropout",
        "dora_shared", "dora_per_sample", "full", "all3_ckpt"]
# group -> (environment set before the import, configurations)
GROUPS = {
    "tiny": ({}, TINY),
    "text_batch0": ({"LTX_TEXT_BATCH": "0"}, ["attn2_shared"]),
    "qkv_grouped0": ({"LTX_LORA_QKV_GROUPED": "0"}, ["all3"]),
    "ff_keep_x2_0": ({"LTX_LORA_FF_KEEP_X2": "0"}, ["all3"]),
    "ff_dy_da1": ({"LTX_LORA_FF_DY_DA": "1"}, ["all3"]),
    "delta_fused0": ({"LTX_DELTA_FUSED": "0"}, ["all3"]),
    "lora_dy0": ({"LTX_LORA_DY": "0"}, ["all3"]),
    # one LTX-2B-width block, B = 8, N = 1024 (M = 8192: past the token-sized gates), r = 16, 256 text tokens
    "2b": ({}, ["2b_all3", "2b_dora"]),
    # the optimizer step alone, no model: the twelve conditions of tools/bf16_sr_bench.py, and AdamW with
    # clip + EMA followed by ema_swap_in / ema_swap_out
    "optim": ({}, [f"{kind}{variant}_{mode}" for kind in ("adamw", "prodigy") for variant in ("", "_clip", "_ema")
                   for mode in ("nearest", "stochastic")] + ["adamw_clip_ema_swap"]),
}
# group `attn`: ops.attn_fwd + ops.attn_bwd alone, one small shape per branch of the attention planners
# (csrc/attn_plan.h; B, H, Nq, Nk, head dim, key bias, f32 dQ), at default switches and at each single
# non-default LTX_ATTN_* switch (set per configuration: ops reloads the library's table when one changes)
ATTN_SHAPES = [(1, 3, 100, 128, 32, False, False), (1, 3, 100, 77, 32, True, False), (2, 4, 100, 256, 64, False, False),
               (2, 4, 100, 200, 64, True, False), (2, 4, 256, 256, 64, False, False), (1, 2, 256, 256, 64, True, False),
               (2, 3, 300, 512, 64, False, False), (2, 3, 300, 512, 64, False, True), (1, 2, 300, 512, 64, True, False),
               (1, 2, 129, 300, 64, False, False)]
ATTN_SWITCHES = ["default", "XCD=0", "BWD1=0", "W8=0", "SKIP=0", "FWD1=0", "FWD1_ROWS=0", "BWD1_QS=1", "BWD1_FEW=0",
                 "QSPLIT=0", "DKDV_W1=1", "DKDV_W1=0", "DQ_W1=1", "DQ_W1=0", "DQ_PIPE=0", "DQ_NBUF=3", "FWD_W1=1",
                 "FWD_PIPE=0", "FWD_F32SUM=0", "DKDV_PIPE=0", "DKDV_NBUF=3"]
GROUPS["attn"] = ({}, [f"{'x'.join(str(int(v)) for v in shape)}/{sw}" for shape in ATTN_SHAPES for sw in ATTN_SWITCHES])


def _lora_configs():
    """group `lora`: one configuration per row of the adapter route table of tests/test_abi.py and rank it runs at"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from test_abi import _LORA_ALL_RANKS, _LORA_ROUTES
    names = []
    for i, (op, M, N, K, opts, _) in enumerate(_LORA_ROUTES):
        for r in ((8, 16, 32, 64, 128) if i == _LORA_ALL_RANKS[op] else (16, 64)):
            names.append(f"{i:02d}_{op}_{M}x{N}x{K}_g{opts.get('groups', 0)}_ws{opts.get('ws', 'big')}_r{r}")
    return names


GROUPS["lora"] = ({}, _lora_configs())


def _sha(t):
    import torch
    t = t.detach().contiguous().cpu().reshape(-1)
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _tiny_case():
    from safetensors.torch import load_file
    from lora_ff_utils import ff_params
    with open(os.path.join(GOLD, "tiny_lora_ff_step.json")) as f:
        meta = json.load(f)
    raw = load_file(os.path.join(GOLD, "tiny_lora_ff_step.safetensors"))
    d = {k: v.cuda() for k, v in raw.items() if k.startswith("in.") or k in ("out.t", "out.noise")}
    d["out.noise"] = d["out.noise"].bfloat16()
    cfg = meta["config"]
    return cfg, ff_params(cfg, meta["param_seed"], R_TINY, targets=("attn1", "attn2")), d


def _2b_case():
    from lora_ff_utils import ff_params
    from ltx_amd.transformer3d import OURS_TRANSFORMER_CONFIG
    from model_utils import synth_inputs
    cfg = dict(OURS_TRANSFORMER_CONFIG, num_layers=1)
    return cfg, ff_params(cfg, 300 + R_2B, R_2B, targets=("attn1", "attn2")), synth_inputs(8, 4, 16, 16, 256, 16, seed=33)


def _per_sample(d):
    B = d["in.latents"].shape[0]
    return dict(d, **{"in.prompt_embeds": d["in.prompt_embeds"].repeat(B, 1, 1),
                      "in.prompt_attention_mask": d["in.prompt_attention_mask"].repeat(B, 1)})


def _build(name, cfg, params, r):
    """The model of a configuration, through the tests' builders."""
    from lora_attn1_utils import build_targets_model
    from lora_dora_utils import build_dora_model
    from lora_ff_utils import build_ff_model, train_config
    from model_utils import build_full_model, build_model
    name = name[3:] if name.startswith("2b_") else name
    if name.startswith("fwd"):
        return build_model(cfg, params, 0)
    if name.startswith("attn2_"):
        return build_model(cfg, params, r)
    if name in ("attn1", "attn1+attn2"):
        return build_targets_model(cfg, params, r, name)
    if name == "attn2+ff":
        return build_ff_model(cfg, params, r, "attn2")
    if name in ("all3", "all3_ckpt"):
        return build_ff_model(cfg, params, r, "attn1+attn2")
    if name == "all3_dropout":
        import torch
        from ltx_amd.lora import apply_training_strategy
        from ltx_amd.patchifier import SymmetricPatchifier
        from ltx_amd.transformer3d import Transformer3DModel
        from params import canonical_name
        tc = train_config(r, "attn1+attn2", True)
        setattr(tc, "lora_dropout", 0.1)
        with torch.device("meta"):
            m = Transformer3DModel.from_config(cfg)
            apply_training_strategy(m, tc, "lora_audio")
        m.load_state_dict({n: params[canonical_name(n)].detach().cuda().clone() for n, _ in m.named_parameters()},
                          assign=True, strict=True)
        for n, q in m.named_parameters():
            q.requires_grad_(("lora_" in n) or ("caption_projection" in n))
        m.patchifier = SymmetricPatchifier(1)
        m.lora_dropout_key = 0x5EED5EED
        return m
    if name.startswith("dora"):
        return build_dora_model(cfg, params, r)
    if name == "full":
        return build_full_model(cfg, params)
    raise KeyError(name)


def _forward_only(model, d, strategy, torch):
    import ltx_oracle as O
    B = d["in.latents"].shape[0]
    tok, coords = O.patchify(d["in.latents"].bfloat16())
    x = O.add_noise(tok, d["out.noise"], d["out.t"]).bfloat16()
    nl = len(model.transformer_blocks)
    skip = (torch.arange(nl * B, device="cuda").view(nl, B) % 2).float() if strategy else None
    model.eval()
    with torch.no_grad():
        return model(hidden_states=x, indices_grid=coords.cuda(),
                     ref_image_hidden_states=d["in.ref_image_latents"].bfloat16(),
                     pose_hidden_states=d["in.pose_latents"].bfloat16(),
                     encoder_hidden_states=d["in.prompt_embeds"].bfloat16().expand(B, -1, -1), timestep=d["out.t"],
                     encoder_attention_mask=d["in.prompt_attention_mask"].expand(B, -1), skip_layer_mask=skip,
                     skip_layer_strategy=strategy or None).sample


def _one(name, case, torch):
    from ltx_amd import ops
    from model_utils import build_step, grads_by_canonical
    cfg, params, d = case
    model = _build(name, cfg, params, R_2B if name.startswith("2b_") else R_TINY)
    if name.endswith("per_sample"):
        d = _per_sample(d)
    outs = []
    if not name.startswith("fwd"):
        model.train()
        model.gradient_checkpointing = name.endswith("_ckpt")
        inner = model._forward_tokens
        model._forward_tokens = lambda *a, **k: (outs.append(inner(*a, **k)), outs[-1])[1]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    timer = ops.LaunchTimer()
    ops.set_launch_timer(timer)
    try:
        if name.startswith("fwd"):
            outs.append(_forward_only(model, d, name[4:], torch))
            loss = None
        else:
            loss = build_step(model, d)
    finally:
        ops.set_launch_timer(None)
    torch.cuda.synchronize()
    rec = {"kernels": [r[0] for r in timer.records], "peak_bytes": torch.cuda.max_memory_allocated(),
           "output": _sha(outs[0]), "loss": None if loss is None else _sha(torch.tensor(loss, dtype=torch.float64)),
           "grads": {}}
    if loss is not None:
        for k, g in sorted(grads_by_canonical(model).items()):
            rec["grads"][k] = None if g is None else _sha(g)
    return rec


def _optim_one(name, torch):
    """Three steps of one optimizer condition on the tensors of tests/bf16_sr_utils.py (BF16_SIZES bf16
    tensors and one f32 tensor of F32_SIZE) with seeded gradients. In the record's shape: "kernels" are the
    launch timer's names and the entry points called, in order, "output" is the
    hash of the last clip record, "loss" of the Prodigy record, "grads" holds every parameter, state
    tensor and shadow (and, for the swap, the weights while swapped in)."""
    from bf16_sr_utils import make_grads, make_params
    from ltx_amd import ops
    from ltx_amd.training import EMASchedule, FusedAdamW, FusedProdigy
    swap = name == "adamw_clip_ema_swap"
    kind, mode = name.split("_")[0], "stochastic" if name.endswith("_stochastic") else "nearest"
    cls, lr = (FusedProdigy, 1.0) if kind == "prodigy" else (FusedAdamW, 1e-3)
    ps = make_params(1, "cuda")
    opt = cls(ps, lr=lr, max_grad_norm=0.5 if "_clip" in name else None,
              ema=EMASchedule(0.999) if "_ema" in name else None, bf16_update=mode, sr_seed=0x5EED0123456789AB)
    grads = [make_grads(10 + k, "cuda") for k in range(3)]
    hashes = {}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    timer = ops.LaunchTimer()
    ops.set_launch_timer(timer)
    # the launch timer labels GEMM and attention launches only: the optimizer's sequence is the entry points
    # ops.call is given
    calls, inner = [], ops.call
    ops.call = lambda fn, *args: (calls.append(fn), inner(fn, *args))[1]
    try:
        for gs in grads:
            for p, g in zip(ps, gs):
                p.grad = g
            opt.step()
        if swap:
            opt.ema_swap_in()
            hashes.update({f"swapped_in.{i}": _sha(p) for i, p in enumerate(ps)})
            opt.ema_swap_out()
    finally:
        ops.call = inner
        ops.set_launch_timer(None)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    for i, p in enumerate(ps):
        hashes[f"param.{i}"] = _sha(p)
        for key, v in sorted(opt.state[p].items()):
            hashes[f"state.{i}.{key}"] = _sha(v if torch.is_tensor(v) else torch.tensor(v, dtype=torch.float64))
    clip = None if opt.clip_sumsq is None else _sha(torch.stack([opt.clip_sumsq, opt.grad_norm.double(),
                                                                 opt.clip_coef.double()]))
    record = getattr(opt, "record", None)
    return {"kernels": [r[0] for r in timer.records] + calls, "peak_bytes": peak, "output": clip,
            "loss": None if record is None else _sha(record), "grads": hashes}


def _attn_one(name, torch):
    """One forward + backward of the configuration's shape under its switch: "kernels" the two labels,
    "output" / "loss" the hashes of O / lse, "grads" those of dQ, dK and dV."""
    from ltx_amd import ops
    shape, sw = name.split("/")
    B, H, Nq, Nk, d, masked, f32 = (int(v) for v in shape.split("x"))
    gen = torch.Generator(device="cpu").manual_seed(Nq * 1000 + Nk)
    q, do, k, v = (torch.randn(B * n, H * d, generator=gen).bfloat16().cuda() for n in (Nq, Nq, Nk, Nk))
    bias = None
    if masked:  # caption-style padding: batch b keeps its first Nk - 5 - 3 b keys
        keep = torch.arange(Nk)[None, :] < (Nk - 5 - 3 * torch.arange(B)[:, None])
        bias = ((1 - keep.float()) * -10000.0).cuda().contiguous()
    env = dict([sw.split("=")]) if sw != "default" else {}
    for key, val in env.items():
        os.environ["LTX_ATTN_" + key] = val
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    timer = ops.LaunchTimer()
    ops.set_launch_timer(timer)
    try:
        o, lse = ops.attn_fwd(q, k, v, B, H, d, d ** -0.5, key_bias=bias)
        dq, dk, dv = ops.attn_bwd(q, k, v, o, do, lse, B, H, d, d ** -0.5, key_bias=bias, dq_f32=bool(f32))
    finally:
        ops.set_launch_timer(None)
        for key in env:
            del os.environ["LTX_ATTN_" + key]
    torch.cuda.synchronize()
    return {"kernels": [r[0] for r in timer.records], "peak_bytes": torch.cuda.max_memory_allocated(),
            "output": _sha(o), "loss": _sha(lse), "grads": {"dq": _sha(dq), "dk": _sha(dk), "dv": _sha(dv)}}


def _lora_one(name, torch):
    """The ops.lora_* calls of one route row on seeded inputs: "grads" holds the hash of every output (u, split, w,
    dB, dA; overwriting and accumulating; the grouped rows into column views of wider buffers), "labels" what
    ops.lora_kernel_label says each call launches, in call order (commits that have it; not compared)."""
    from ltx_amd import ops
    op, shape, g, ws, r = name.split("_", 1)[1].rsplit("_", 4)
    (M, N, K), G, r = (int(v) for v in shape.split("x")), int(g[1:]), int(r[1:])
    gen = torch.Generator(device="cpu").manual_seed(M * 7 + N + K + r)
    bf = lambda *sh: torch.randn(*sh, generator=gen).bfloat16().cuda()  # noqa: E731
    f32 = lambda *sh, scale=1.0: (torch.randn(*sh, generator=gen) * scale).cuda()  # noqa: E731
    K2, n = ops.lora_k2(r), max(G, 1)
    out, labels = {}, []
    buf = ops._gemm_workspace("cuda:0")  # then the row's workspace on the stream: whole, 64 KiB of it, or none
    nbytes = {"wsbig": ops.GEMM_WS_BYTES, "wssmall": 64 << 10, "wsNone": 0}[ws]
    ops.call("ltx_gemm_set_stream_workspace", ops._s(), ops._p(buf) if nbytes else None, nbytes)

    def label(*a, **k):
        if hasattr(ops, "lora_kernel_label"):
            labels.append(ops.lora_kernel_label(*a, **k))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    try:
        if op == "rows":
            x, As = bf(M, K), [f32(r, K, scale=K ** -0.5) for _ in range(n)]
            pieces = [ops.lora_pieces(A) for A in As]
            if G:
                ub, sb = torch.full((M, 2 * G * r), 3.0, device="cuda"), torch.full((M, 2 * G * K2), 7.0).bfloat16().cuda()
                ops.lora_rows_grouped(x, pieces, r, alpha=0.5, out=ub[:, r:2 * r], split=True, split_out=sb[:, K2:2 * K2],
                                      group_strides=(2 * r, 2 * K2))
                label("rows", M, K=K, r=r, groups=G, split=True, ld_out=2 * G * r)
                out.update(u=ub, split=sb, u_nosplit=ops.lora_rows_grouped(x, pieces, r, alpha=0.5))
                label("rows", M, K=K, r=r, groups=G)
            else:
                out["u"], out["split"] = ops.lora_rows(x, pieces[0], r, alpha=0.5, split=True)
                label("rows", M, K=K, r=r, split=True)
                out["u_nosplit"] = ops.lora_rows(x, pieces[0], r, alpha=0.5)
                label("rows", M, K=K, r=r)
        elif op == "down":
            x, A, Bm = bf(M, K), f32(n, r, K, scale=K ** -0.5), f32(K, r, scale=K ** -0.5)
            out["u"], out["split"] = torch.zeros(n, M, r, device="cuda"), torch.zeros(n, M, K2).bfloat16().cuda()
            ops.lora_down(x, A[0], alpha=0.5, out=out["u"][0], split=True, split_out=out["split"][0], groups=n,
                          group_strides=(0, r * K, M * r, M * K2))
            label("down", M, K=K, r=r, groups=G, split=True)
            out["w_t"] = ops.lora_down(x, Bm, alpha=0.5, transposed=True)
            label("down", M, K=K, r=r)
        elif op == "wgrad":
            y, u = bf(M, n * N), f32(M, n * r)
            for key, tr in (("dw", False), ("dw_t", True)):
                out[key] = ops.lora_wgrad(y[:, :N], u[:, :r], alpha=0.5, transpose_out=tr, groups=n, group_strides=(N, r))
                acc = f32(*out[key].shape)
                out[key + "_acc"] = ops.lora_wgrad(y[:, :N], u[:, :r], alpha=0.5, transpose_out=tr, out=acc,
                                                   accumulate=True, groups=n, group_strides=(N, r))
                for _ in range(2):
                    label("wgrad", M, N=N, r=r, groups=G, ld_in=n * N, ld_w=n * r)
        else:
            y, x = bf(M, n * N), bf(M, K) if K else None
            us, Bs = [f32(M, r) for _ in range(n)], [f32(N, r, scale=0.05) for _ in range(n)]
            pieces = [ops.lora_pieces(Bm, transposed=True) for Bm in Bs]
            for acc in (False, True):
                dB, dA = [f32(N, r) for _ in range(n)], [f32(r, K) for _ in range(n)] if K else None
                if G:
                    w, sp = ops.lora_dy_grouped(y, us, pieces, r, 0.5, dB, x, dA, accumulate=acc, dA_accumulate=acc)
                elif K:
                    w, sp = ops.lora_dy(y, us[0], pieces[0], r, 0.5, dB[0], accumulate=acc, x=x, dA_out=dA[0],
                                        dA_accumulate=acc)
                else:
                    w, sp = ops.lora_dy(y, us[0], pieces[0], r, 0.5, dB[0], accumulate=acc)
                label(op, M, N=N, K=K, r=r, groups=G)
                out.update({f"w{int(acc)}": w, f"split{int(acc)}": sp})
                out.update({f"dB{int(acc)}.{i}": t for i, t in enumerate(dB)})
                out.update({f"dA{int(acc)}.{i}": t for i, t in enumerate(dA or [])})
        torch.cuda.synchronize()
    finally:
        ops.call("ltx_gemm_set_stream_workspace", ops._s(), ops._p(buf), ops.GEMM_WS_BYTES)
    return {"kernels": [], "labels": labels, "peak_bytes": torch.cuda.max_memory_allocated(), "output": None,
            "loss": None, "grads": {k: _sha(v) for k, v in sorted(out.items())}}


def run(args):
    env, names = GROUPS[args.group]
    os.environ.update(env)
    for p in (os.path.abspath(args.pkg), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    import torch
    import ltx_amd
    from ltx_amd import _lib
    _lib.ensure_device("cuda:0")
    torch.cuda.set_device(0)
    case = None if args.group in ("optim", "attn", "lora") else _2b_case() if args.group == "2b" else _tiny_case()
    out = {"pkg": os.path.dirname(os.path.abspath(ltx_amd.__file__)), "env": env, "configs": {}}
    for name in names:
        rec = (_attn_one(name, torch) if args.group == "attn" else _lora_one(name, torch) if args.group == "lora"
               else _optim_one(name, torch) if case is None
               else _one(name, case, torch))
        out["configs"][f"{args.group}/{name}"] = rec
        gc.collect()
        torch.cuda.empty_cache()
        print(f"{args.group}/{name}: {len(out['configs'][f'{args.group}/{name}']['kernels'])} launches", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def _load(paths):
    cfgs = {}
    for p in paths:
        with open(p) as f:
            cfgs.update(json.load(f)["configs"])
    return cfgs


def compare(args):
    old, new = _load(args.old.split(",")), _load(args.new.split(","))
    rows, bad = [], 0
    for name in sorted(set(old) | set(new)):
        a, b = old.get(name), new.get(name)
        if a is None or b is None:
            rows.append((name, "-", "-", "-", "-", "-", "-", "MISSING"))
            bad += 1
            continue
        why = []
        if a["kernels"] != b["kernels"]:
            why.append("kernel list differs")
        if (a["output"], a["loss"]) != (b["output"], b["loss"]):
            why.append("output / loss differs")
        diff = [k for k in set(a["grads"]) | set(b["grads"]) if a["grads"].get(k, 0) != b["grads"].get(k, 1)]
        if diff:
            why.append(f"{len(diff)} gradients differ")
        if b["peak_bytes"] > a["peak_bytes"]:
            why.append("peak above the old one")
        bad += bool(why)
        n = lambda c: len(c["grads"]) + 1 + (c["loss"] is not None)  # noqa: E731
        rows.append((name, len(a["kernels"]), len(b["kernels"]), n(a), n(b), a["peak_bytes"], b["peak_bytes"],
                     "identical" if not why else "; ".join(why)))
    head = ("configuration", "launches old", "launches new", "tensors old", "tensors new", "peak bytes old",
            "peak bytes new", "verdict")
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    lines += ["| " + " | ".join(str(c) for c in r) + " |" for r in rows]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.md:
        with open(args.md, "w") as f:
            f.write(text)
    sys.exit(1 if bad else 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--pkg", default=os.path.join(REPO, "video-generation-for-human-avatars_amd"))
    r.add_argument("--group", required=True, choices=sorted(GROUPS))
    r.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("old", help="comma-separated fingerprint files of the old commit")
    c.add_argument("new", help="... of the new commit")
    c.add_argument("--md")
    args = ap.parse_args()
    run(args) if args.cmd == "run" else compare(args)


if __name__ == "__main__":
    main()
