"""The max-norm pass of the LoRA optimizer step on the MI355X (FusedAdamW / FusedProdigy(scale_weight_norms=c);
csrc/max_norm.hip) against its statement, tests/max_norm_utils.py:

  * the grouped sums of squares and the finish on exact inputs (small integers times powers of two, every
    summation order the same f64): bitwise the statement's, over every tile size, two tiles per side, ragged
    slabs and row blocks, the smallest and the largest rank;
  * random and adversarial pairs: the norm within 1e-6 of the f64 direct form (1000 x what the f64 Gram form
    reaches on the CPU, 3000 x tighter than the f32 Gram form's error);
  * decisions and stores: pairs at norm 0, 0.3 c, 0.9 c, 1.1 c and 5 c; a second pass scales nothing;
  * the tiny model through FusedAdamW: three steps against the parent path's steps with the statement applied;
    the cap absent or 0 launches exactly today's kernels; no host sync; the guard; the EMA's correction;
    Prodigy, DoRA and the stochastic bf16 mode; train_loop with the log keys and a bitwise resume.

The model is the tiny config of test_adapter_ckpt_gpu (2 layers, D = 128, r = 8, adapters on every target with
non-zero B); gradients are seeded random tensors: it is the optimizer that is under test."""
import numpy as np
import pytest
import torch

from max_norm_utils import adversarial_pair, exact_pair, norm_direct, pair_with_norm, random_pair, statement, sumsq_direct
from test_adapter_ckpt_gpu import _build, _config, _fixed_inputs, _forward_and_grads, _same, tiny  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
# the norm's tolerance (1000 x the f64 Gram form's own error on the CPU); a decision may differ from the statement's only where the
# statement's norm is that close to the cap
NORM_RTOL = 1e-6


# ---------------------------------------------------------------------------------------------
# the three entry points on hand-made pairs
# ---------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _device_pass(pairs, cap, scale=False, shadows=None, omd=0.0, guard=None, passes=1):
    """`pairs` = [(A, B, s)] numpy: the pair table and the scale table as FusedAdamW builds them, then
    ltx_max_norm_sumsq, ltx_max_norm_finish and, with `scale`, ltx_max_norm_scale_multi, `passes` times.
    Returns the f64 sums of squares, the factors, the record (keys, avg, max), the tensors after the pass and
    the shadows ([(A's, B's)] or None), all on the host."""
    from ltx_amd import ops, training
    dev = [(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)) for A, B, _ in pairs]
    sh = None if shadows is None else [(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)) for a, b in shadows]
    rows, nwg, ws_f64 = training.max_norm_pair_rows(
        [(a.data_ptr(), b.data_ptr(), b.shape[0], a.shape[1], a.shape[0], s) for (a, b), (_, _, s) in zip(dev, pairs)])
    tensors = []
    for i, (a, b) in enumerate(dev):
        sa, sb = (0, 0) if sh is None else (sh[i][0].data_ptr(), sh[i][1].data_ptr())
        tensors += [(a.numel(), a.data_ptr(), sa, i), (b.numel(), b.data_ptr(), sb, i)]
    srows = training.max_norm_scale_rows(tensors, training.FusedAdamW.CHUNK)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    stable = torch.tensor(srows, dtype=torch.int64, device=DEV)
    n = len(pairs)
    ws = torch.full((ws_f64 + n,), float("nan"), dtype=torch.float64, device=DEV)  # every partial read is written
    sumsq = ws[ws_f64:]
    factor = torch.empty(n, dtype=torch.float32, device=DEV)
    rec = torch.empty(4, dtype=torch.int32, device=DEV)
    out = []
    for _ in range(passes):
        ops.max_norm_sumsq(table, n, nwg, ws, sumsq)
        ops.max_norm_finish(table, sumsq, n, cap, factor, rec, guard)
        if scale:
            ops.max_norm_scale_multi(stable, len(srows), factor, omd, guard)
        out.append({"sumsq": sumsq.cpu().numpy().copy(), "f": factor.cpu().numpy().copy(),
                    "keys": int(rec[0]), "avg": float(rec[1:2].view(torch.float32)), "max": float(rec[2:3].view(torch.float32)),
                    "pairs": [(a.cpu().numpy().copy(), b.cpu().numpy().copy()) for a, b in dev],
                    "shadows": None if sh is None else [(a.cpu().numpy().copy(), b.cpu().numpy().copy()) for a, b in sh]})
    return out if passes > 1 else out[0]


# (N, K, r), s: tiles of 8, 16, 32 and 64, two tiles per side at r = 128; N = 40 and 72 end inside a 64-row
# stage, K = 136, 200 and 264 are no multiple of a stage's 64; 2048 rows at r = 16 and 8192 columns at r = 128 are
# two and four slabs, 1100 rows a full slab and a ragged one
EXACT = [((16, 128, 8), 1.0), ((40, 136, 8), 0.5), ((2048, 64, 16), 2.0), ((64, 8192, 128), 0.125),
         ((1100, 72, 16), 0.75), ((72, 200, 32), 0.25), ((100, 264, 64), 1.5)]


def test_grouped_sumsq_and_finish_on_exact_inputs_are_bitwise_the_statement():
    pairs = [exact_pair(*shape, seed=10 + i) + (s,) for i, (shape, s) in enumerate(EXACT)]
    want_sumsq = np.array([sumsq_direct(A, B) for A, B, _ in pairs])
    norms = np.array([norm_direct(A, B, s) for A, B, s in pairs])
    # no pair scales: the record holds the norms themselves
    got = _device_pass(pairs, cap=2.0 * norms.max())
    assert np.array_equal(got["sumsq"].view(np.int64), want_sumsq.view(np.int64)), (got["sumsq"], want_sumsq)
    assert np.array_equal(got["f"], np.ones(len(pairs), np.float32)) and got["keys"] == 0
    assert np.float32(got["max"]) == np.float32(norms.max())
    assert abs(got["avg"] - norms.mean()) <= 2.0 ** -23 * norms.mean()
    # every pair scales: f = float32(sqrt(cap / norm)) from the exact norm, bit for bit
    cap = 0.5 * norms.min()
    st = statement(pairs, cap)
    got = _device_pass(pairs, cap=cap)
    assert np.array_equal(got["f"].view(np.int32), np.asarray(st["f"], np.float32).view(np.int32)), (got["f"], st["f"])
    assert got["keys"] == len(pairs) == st["keys_scaled"]
    assert abs(got["avg"] - cap) <= 2.0 ** -22 * cap and abs(got["max"] - cap) <= 2.0 ** -22 * cap


@pytest.mark.parametrize("shape", [(2048, 2048, 16), (40, 136, 8)])
def test_random_and_adversarial_norms_are_the_f64_direct_norms(shape):
    N, K, r = shape
    pairs = [random_pair(N, K, r, seed=1) + (0.5,), adversarial_pair(N, K, r, seed=2) + (1.0,),
             random_pair(N, K, r, seed=3, scale=30.0) + (2.0,), adversarial_pair(N, K, r, seed=4) + (0.25,)]
    got = _device_pass(pairs, cap=1e30)
    for i, (A, B, s) in enumerate(pairs):
        want = norm_direct(A, B, s)
        dev = abs(s) * np.sqrt(got["sumsq"][i])
        print(f"pair {i} {shape}: device {dev!r} direct {want!r} rel {abs(dev - want) / want:.3e}")
        assert abs(dev - want) <= NORM_RTOL * want, (i, dev, want)


def _decision_pairs(c):
    targets = [0.0, 0.3, 0.9, 1.1, 5.0, 1.1, 0.9]
    shapes = [(40, 136, 8), (2048, 64, 16), (72, 200, 32), (2500, 72, 16), (64, 4200, 8), (100, 264, 64), (200, 8192, 128)]
    scal = [1.0, 0.5, 2.0, 1.0, 0.25, 1.0, 0.125]
    return [pair_with_norm(N, K, r, s, t * c, seed=40 + i) + (s,)
            for i, (t, (N, K, r), s) in enumerate(zip(targets, shapes, scal))]


def test_decisions_and_stores():
    """Norms of 0 (B = 0), 0.3 c, 0.9 c, 1.1 c and 5 c: pairs at or under the cap are bitwise untouched, the
    others are fl32(p * f_dev) element for element with f_dev within 1e-6 of the statement's f, the record is
    the statement's, and a second pass right after scales nothing the statement does not."""
    c = 0.7
    pairs = _decision_pairs(c)
    st = statement(pairs, c)
    assert [r != 1.0 for r in st["ratio"]] == [False, False, False, True, True, True, False]
    first, second = _device_pass(pairs, c, scale=True, passes=2)
    assert first["keys"] == st["keys_scaled"] == 3
    assert abs(first["avg"] - st["avg_key_norm"]) <= NORM_RTOL * st["avg_key_norm"]
    assert abs(first["max"] - st["max_key_norm"]) <= NORM_RTOL * st["max_key_norm"]
    for i, (A, B, _) in enumerate(pairs):
        f_dev, (a, b) = first["f"][i], first["pairs"][i]
        if st["ratio"][i] == 1.0:
            assert f_dev == np.float32(1.0)
            assert np.array_equal(a.view(np.int32), A.view(np.int32)) and np.array_equal(b.view(np.int32), B.view(np.int32))
        else:
            assert abs(float(f_dev) - float(st["f"][i])) <= NORM_RTOL * float(st["f"][i]), (i, f_dev, st["f"][i])
            assert np.array_equal(a.view(np.int32), (A * f_dev).view(np.int32)), i
            assert np.array_equal(b.view(np.int32), (B * f_dev).view(np.int32)), i
    # the second pass: the statement on the stored weights. A scaled pair sits on the cap to f32 rounding of its
    # elements, so its decision may go either way there; where the statement's norm is further than the norm's
    # tolerance from the cap the decisions agree, and nothing is scaled by more than that rounding
    st2 = statement([(a, b, s) for (a, b), (_, _, s) in zip(first["pairs"], pairs)], c)
    for i in range(len(pairs)):
        if abs(st2["norm"][i] - c) > NORM_RTOL * c:
            assert (second["f"][i] != 1.0) == (st2["ratio"][i] != 1.0), i
        assert abs(float(second["f"][i]) - float(st2["f"][i])) <= NORM_RTOL
        if second["f"][i] == 1.0:
            for x, y in zip(second["pairs"][i], first["pairs"][i]):
                assert np.array_equal(x.view(np.int32), y.view(np.int32)), i
    assert all(second["f"][i] == 1.0 for i in range(len(pairs)) if st["ratio"][i] == 1.0)


def test_scale_rows_with_shadows_and_a_skipped_guard():
    """The scale launch alone: a shadow takes the three-operation correction, a row without one is only scaled,
    and under a guard record whose applied is 0 the finish reports no key and nothing is stored."""
    c = 0.7
    pairs = _decision_pairs(c)[2:5]  # 0.9 c, 1.1 c, 5 c
    g = np.random.default_rng(7)
    shadows = [(g.standard_normal(A.shape).astype(np.float32), g.standard_normal(B.shape).astype(np.float32))
               for A, B, _ in pairs]
    omd = np.float32(1.0 - 0.99)
    got = _device_pass(pairs, c, scale=True, shadows=shadows, omd=float(omd))
    for i, (A, B, _) in enumerate(pairs):
        f = got["f"][i]
        for p, sh, sh_dev in zip((A, B), shadows[i], got["shadows"][i]):
            if f == 1.0:
                want = sh
            else:
                want = sh - omd * (p - p * f)  # numpy f32: one rounding per operation
            assert want.dtype == np.float32 and np.array_equal(sh_dev.view(np.int32), want.view(np.int32)), i
    assert got["keys"] == 2
    skipped = torch.zeros(4, dtype=torch.float64, device=DEV)  # a guard record: applied = 0
    from ltx_amd import ops
    got = _device_pass(pairs, c, scale=True, shadows=shadows, omd=float(omd), guard=ops._p(skipped))
    assert got["keys"] == 0 and np.array_equal(got["f"], np.ones(3, np.float32))
    for i, (A, B, _) in enumerate(pairs):
        assert np.array_equal(got["pairs"][i][0], A) and np.array_equal(got["pairs"][i][1], B)
        assert np.array_equal(got["shadows"][i][0], shadows[i][0]) and np.array_equal(got["shadows"][i][1], shadows[i][1])
    norms = statement(pairs, 1e30)["norm"]  # the record of a skipped step: the norms as they stand
    assert abs(got["max"] - max(norms)) <= NORM_RTOL * max(norms)
    applied = skipped.clone()
    applied[2:3].view(torch.int32)[0] = 1
    assert _device_pass(pairs, c, scale=True, guard=ops._p(applied))["keys"] == 2


# ---------------------------------------------------------------------------------------------
# the tiny model through the optimizers
# ---------------------------------------------------------------------------------------------
ALL = {"lora_targets": "attn1+attn2", "lora_ff": True}
# AdamW moves every element by about the rate per step: at 1e-4 the pairs' norms move by less than the widest gap
# of the fixture's norms (1.2 %), so a cap inside that gap leaves some pairs over it and some under at every step
LR = 1e-4


def _trainable(model):
    return [p for p in model.parameters() if p.requires_grad]


def _np_pairs(pairs):
    return [(A.detach().cpu().numpy().copy(), B.detach().cpu().numpy().copy(), s) for _, A, B, s in pairs]


def _cap_between(norms):
    """A cap in the widest gap between two neighbouring norms of the middle half: some pairs over, some under,
    none close."""
    n = np.sort(np.asarray(norms))
    lo, hi = len(n) // 4, 3 * len(n) // 4
    i = lo + int(np.argmax(n[lo + 1:hi + 1] / n[lo:hi]))
    return float(np.sqrt(n[i] * n[i + 1]))


def _set_grads(params, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = (scale * torch.randn(p.shape, generator=g)).to(p.dtype).to(DEV)


def _check_against_statement(opt, before, pairs, cap, where):
    """`before`: the np pairs the statement is applied to (the parent path's stepped weights); the live pairs
    must be them with the statement applied, compared as in test_decisions_and_stores. Returns the statement."""
    st = statement(before, cap)
    f_dev = opt.key_factors.cpu().numpy()
    keys = 0
    for i, ((A0, B0, _), (_, A, B, _)) in enumerate(zip(before, pairs)):
        a, b = A.detach().cpu().numpy(), B.detach().cpu().numpy()
        near = abs(st["norm"][i] - cap) <= NORM_RTOL * cap
        assert near or (f_dev[i] != 1.0) == (st["ratio"][i] != 1.0), (where, i)
        if f_dev[i] == 1.0:
            assert np.array_equal(a.view(np.int32), A0.view(np.int32)) and np.array_equal(b.view(np.int32), B0.view(np.int32))
        else:
            keys += 1
            assert abs(float(f_dev[i]) - float(st["f"][i])) <= NORM_RTOL * float(st["f"][i]), (where, i)
            assert np.array_equal(a.view(np.int32), (A0 * f_dev[i]).view(np.int32)), (where, i)
            assert np.array_equal(b.view(np.int32), (B0 * f_dev[i]).view(np.int32)), (where, i)
    assert int(opt.keys_scaled) == keys
    assert opt.keys_scaled.dim() == 0 and opt.keys_scaled.is_cuda and opt.keys_scaled.dtype == torch.int32
    for t in (opt.avg_key_norm, opt.max_key_norm):
        assert t.dim() == 0 and t.is_cuda and t.dtype == torch.float32
    assert abs(float(opt.avg_key_norm) - st["avg_key_norm"]) <= NORM_RTOL * st["avg_key_norm"], where
    assert abs(float(opt.max_key_norm) - st["max_key_norm"]) <= NORM_RTOL * st["max_key_norm"], where
    return st


def test_three_adamw_steps_are_the_parent_steps_with_the_statement_applied(tiny):
    """Model X steps with the cap, model Y without; before every step Y takes X's weights (AdamW's moments
    depend on the gradients alone, so they stay equal), and after it X must be Y with the statement applied:
    adapters as in test_decisions_and_stores, the caption projection bit for bit."""
    from ltx_amd.lora import adapter_pairs
    from ltx_amd.training import FusedAdamW
    x, y = _build(tiny, ALL), _build(tiny, ALL)
    px, py = _trainable(x), _trainable(y)
    pairs_x, pairs_y = adapter_pairs(x), adapter_pairs(y)
    assert len(pairs_x) == 20
    cap = _cap_between(statement(_np_pairs(pairs_x), 1e30)["norm"])  # from the fixture weights, on the CPU
    opt_x = FusedAdamW(px, lr=LR, scale_weight_norms=cap, norm_pairs=pairs_x)
    opt_y = FusedAdamW(py, lr=LR)
    held = None
    for k in range(3):
        with torch.no_grad():
            for a, b in zip(px, py):
                b.copy_(a)
        _set_grads(px, 300 + k)
        _set_grads(py, 300 + k)
        opt_x.step()
        opt_y.step()
        st = _check_against_statement(opt_x, _np_pairs(pairs_y), pairs_x, cap, k)
        assert 0 < st["keys_scaled"] < len(pairs_x), (k, st["keys_scaled"])
        paired = {id(t) for _, A, B, _ in pairs_x for t in (A, B)}
        rest = [(a, b) for a, b in zip(px, py) if id(a) not in paired]
        assert rest and all(torch.equal(_bits(a.detach()), _bits(b.detach())) for a, b in rest)  # caption_projection
        for a, b in zip(px, py):  # the moments are not touched
            assert torch.equal(opt_x.state[a]["exp_avg"], opt_y.state[b]["exp_avg"])
            assert torch.equal(opt_x.state[a]["exp_avg_sq"], opt_y.state[b]["exp_avg_sq"])
        if held is None:
            held = (opt_x.keys_scaled, int(opt_x.keys_scaled))
    assert int(held[0]) == held[1] and held[0] is not opt_x.keys_scaled  # a fresh record per step


def _recorded_step(model, opt, seed):
    """One optimizer step with every ops.call and every LaunchTimer label recorded, in order."""
    from ltx_amd import ops
    calls = []
    real = ops.call
    timer = ops.LaunchTimer()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        ops.set_launch_timer(timer)
        try:
            _set_grads(_trainable(model), seed)
            opt.step()
        finally:
            ops.set_launch_timer(None)
    return calls, [rec[0] for rec in timer.records]


def test_cap_absent_or_zero_launches_exactly_todays_kernels(tiny):
    from ltx_amd.lora import adapter_pairs
    from ltx_amd.training import FusedAdamW
    runs = []
    for kw in ({}, {"scale_weight_norms": None}, {"scale_weight_norms": 0, "norm_pairs": "pairs"},
               {"scale_weight_norms": 1e-3, "norm_pairs": "pairs"}):
        m = _build(tiny, ALL)
        if "norm_pairs" in kw:
            kw = dict(kw, norm_pairs=adapter_pairs(m))
        opt = FusedAdamW(_trainable(m), lr=1e-2, **kw)
        calls, labels = _recorded_step(m, opt, 11)
        runs.append((calls, labels, [p.detach().clone() for p in _trainable(m)], opt))
    today = runs[0]
    assert today[0] and all(n.startswith("ltx_adamw") for n in today[0]) and today[1] == []
    for calls, labels, weights, opt in runs[1:3]:
        assert calls == today[0] and labels == today[1]
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(weights, today[2]))
        assert opt.keys_scaled is None and "scale_weight_norms" not in opt.param_groups[0]
    calls, labels, weights, opt = runs[3]
    assert calls.count("ltx_max_norm_plan") == 20  # host only, once per pair while the tables are built
    calls = [n for n in calls if n != "ltx_max_norm_plan"]
    assert calls[-3:] == ["ltx_max_norm_sumsq", "ltx_max_norm_finish", "ltx_max_norm_scale_multi"]
    assert not any("max_norm" in n for n in calls[:-3]) and "ltx_adamw_multi" in calls[:-3]  # the table path
    assert labels == ["ltx::gram_partials_kernel + ltx::gram_contract_kernel", "ltx::max_norm_finish_kernel",
                      "ltx::max_norm_scale_multi_kernel"]
    assert int(opt.keys_scaled) == 20 and not all(torch.equal(a, b) for a, b in zip(weights, today[2]))


def _nan_grads(params):
    for p in params:
        p.grad = p.grad.clone()
    params[3].grad.view(-1)[1] = float("nan")


def test_the_pass_does_not_sync_with_the_host(tiny):
    """Cap, clip, EMA and guard all on: steps, a skipped one among them, run under torch's sync debug mode."""
    from ltx_amd.lora import adapter_pairs
    from ltx_amd.training import EMASchedule, FusedAdamW
    m = _build(tiny, ALL)
    ps = _trainable(m)
    opt = FusedAdamW(ps, lr=1e-2, max_grad_norm=0.5, ema=EMASchedule(0.99), skip_nonfinite=True,
                     scale_weight_norms=1e-2, norm_pairs=adapter_pairs(m))
    _set_grads(ps, 1)
    opt.step()  # tables, workspace, partials and the pinned slot warm
    fresh = []
    for k in (2, 3, 4):
        _set_grads(ps, k)
        if k == 3:
            _nan_grads(ps)
        fresh.append([p.grad.clone() for p in ps])  # copies: p.grad itself is written below
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gs in fresh:
            for p, g in zip(ps, gs):
                p.grad.copy_(g)  # the same buffers: the cached tables stay valid, as in a training loop
            opt.step()
        keys = opt.keys_scaled
        with pytest.raises(RuntimeError):
            int(keys)  # reading it is the sync
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(opt.keys_scaled) > 0 and opt.skipped_steps == 1 and opt.ema_steps == 3


def _snapshot(opt, params):
    out = {}
    for i, p in enumerate(params):
        out[f"p{i}"] = p.detach().clone()
        for k, v in opt.state.get(p, {}).items():
            if torch.is_tensor(v):
                out[f"{k}{i}"] = v.clone()
    return out


def test_a_skipped_step_scales_nothing_and_the_next_finite_step_scales(tiny):
    from ltx_amd.lora import adapter_pairs
    from ltx_amd.training import EMASchedule, FusedAdamW
    m = _build(tiny, ALL)
    ps = _trainable(m)
    pairs = adapter_pairs(m)
    cap = 0.5 * min(statement(_np_pairs(pairs), 1e30)["norm"])  # every pair is over the cap
    opt = FusedAdamW(ps, lr=1e-3, ema=EMASchedule(0.99), skip_nonfinite=True, scale_weight_norms=cap, norm_pairs=pairs)
    _set_grads(ps, 1)
    opt.step()
    assert int(opt.keys_scaled) == len(pairs) and int(opt.step_applied) == 1
    before = _snapshot(opt, ps)
    _set_grads(ps, 2)
    _nan_grads(ps)
    opt.step()
    assert int(opt.step_applied) == 0 and int(opt.keys_scaled) == 0
    assert np.array_equal(opt.key_factors.cpu().numpy(), np.ones(len(pairs), np.float32))
    after = _snapshot(opt, ps)
    assert sorted(after) == sorted(before)
    for k in before:
        assert torch.equal(_bits(before[k]), _bits(after[k])), k  # weights, moments and shadows
    # the record of the skipped step: the norms as they stand, on the cap since the last step
    assert abs(float(opt.max_key_norm) - cap) <= 1e-5 * cap
    _set_grads(ps, 3, scale=10.0)
    opt.step()
    assert int(opt.step_applied) == 1 and int(opt.keys_scaled) > 0 and opt.skipped_steps == 1


def test_the_shadows_take_the_stated_correction(tiny):
    """X with cap and EMA, Y with the EMA alone from the same weights and gradients: X's shadows are Y's with
    s <- s - omd (p_before - p_after), three f32 operations, bit for bit; and within f32 rounding of the EMA of
    the weights as stored."""
    from ltx_amd.lora import adapter_pairs
    from ltx_amd.training import EMASchedule, FusedAdamW
    x, y = _build(tiny, ALL), _build(tiny, ALL)
    px, py = _trainable(x), _trainable(y)
    pairs = adapter_pairs(x)
    cap = _cap_between(statement(_np_pairs(pairs), 1e30)["norm"])
    opt_x = FusedAdamW(px, lr=LR, ema=EMASchedule(0.9), scale_weight_norms=cap, norm_pairs=pairs)
    opt_y = FusedAdamW(py, lr=LR, ema=EMASchedule(0.9))
    # two steps: the schedule's decay is 0 at the first (the shadow becomes the weight) and 2 / 11 at the second
    for k in range(2):
        with torch.no_grad():  # Y takes X's weights and shadows: its step is X's without the pass
            for a, b in zip(px, py):
                b.copy_(a)
                if k:
                    opt_y.state[b]["ema"].copy_(opt_x.state[a]["ema"])
        before = [p.detach().clone() if k == 0 else opt_x.state[p]["ema"].clone() for p in px]
        _set_grads(px, 300 + k)
        _set_grads(py, 300 + k)
        opt_x.step()
        opt_y.step()
        assert 0 < int(opt_x.keys_scaled) < len(pairs)
        assert opt_x.ema_decay == opt_y.ema_decay == (0.0, 2 / 11)[k]
        omd = torch.tensor(1.0 - opt_x.ema_decay, dtype=torch.float32, device=DEV)
        changed = 0
        for a, b, s0 in zip(px, py, before):
            sx, sy = opt_x.state[a]["ema"], opt_y.state[b]["ema"]
            if a.dtype != torch.float32:
                assert torch.equal(sx, sy)
                continue
            moved = b.detach() - a.detach()  # p_before - p_after: Y holds the unscaled step
            want = sy - omd * moved
            assert torch.equal(_bits(sx), _bits(want)), k
            changed += int(not torch.equal(sx, sy))
            # the EMA of the stored weight from the shadow before the step, in f64: six f32 roundings (two
            # differences, two products, two subtractions from the shadow) of values no larger than |s0| + |p|
            ideal = s0.double() - (1.0 - opt_x.ema_decay) * (s0.double() - a.detach().double())
            tol = 6 * 2.0 ** -24 * (s0.abs().max().item() + a.detach().abs().max().item())
            assert float((sx.double() - ideal).abs().max()) <= tol, k
        assert changed == 2 * int(opt_x.keys_scaled)


def test_one_prodigy_step(tiny):
    """Prodigy's own step is untouched (s, p0, the moments and the record are those of the run without the cap);
    the weights are that run's with the statement applied."""
    from ltx_amd.lora import adapter_pairs
    from ltx_amd.training import FusedProdigy
    x, y = _build(tiny, ALL), _build(tiny, ALL)
    px, py = _trainable(x), _trainable(y)
    pairs_x, pairs_y = adapter_pairs(x), adapter_pairs(y)
    cap = _cap_between(statement(_np_pairs(pairs_x), 1e30)["norm"])
    opt_x = FusedProdigy(px, d0=3e-5, scale_weight_norms=cap, norm_pairs=pairs_x)  # a first step of ~1e-4
    opt_y = FusedProdigy(py, d0=3e-5)
    _set_grads(px, 8)
    _set_grads(py, 8)
    opt_x.step()
    opt_y.step()
    st = _check_against_statement(opt_x, _np_pairs(pairs_y), pairs_x, cap, "prodigy")
    assert 0 < st["keys_scaled"] < len(pairs_x)
    assert torch.equal(opt_x.record, opt_y.record)
    for a, b in zip(px, py):
        for k in ("exp_avg", "exp_avg_sq", "s", "p0"):
            assert torch.equal(_bits(opt_x.state[a][k]), _bits(opt_y.state[b][k])), k


def test_one_dora_step_and_the_forward_after_it(tiny):
    """The pairs of a DoRA model are A and B alone; the magnitudes are stepped and not scaled, and the forward
    after the step folds the scaled weights: it is the forward of a fresh model given the same tensors."""
    from ltx_amd.lora import adapter_pairs
    from ltx_amd.training import FusedAdamW
    extra = {"use_dora": True}
    x, y = _build(tiny, extra), _build(tiny, extra)
    px, py = _trainable(x), _trainable(y)
    pairs_x, pairs_y = adapter_pairs(x), adapter_pairs(y)
    assert len(pairs_x) == 8
    batch, t, noise = _fixed_inputs(tiny)
    warm = _forward_and_grads(tiny, x, batch, t, noise)  # W_eff and the packs are built from the old weights
    cap = 0.5 * min(statement(_np_pairs(pairs_x), 1e30)["norm"])
    opt_x = FusedAdamW(px, lr=1e-2, scale_weight_norms=cap, norm_pairs=pairs_x)
    opt_y = FusedAdamW(py, lr=1e-2)
    for a, b in zip(px, py):
        b.grad = a.grad.clone()
    opt_x.step()
    opt_y.step()
    _check_against_statement(opt_x, _np_pairs(pairs_y), pairs_x, cap, "dora")
    assert int(opt_x.keys_scaled) == 8
    mags = [(n, p) for n, p in x.named_parameters() if "lora_magnitude_vector" in n]
    named_y = dict(y.named_parameters())
    assert len(mags) == 8 and all(torch.equal(p.detach(), named_y[n].detach()) for n, p in mags)
    got = _forward_and_grads(tiny, x, batch, t, noise)
    fresh = _build(tiny, extra)
    fresh.load_state_dict({k: v.detach().clone() for k, v in x.state_dict().items()}, strict=True)
    want = _forward_and_grads(tiny, fresh, batch, t, noise)
    assert torch.equal(got[0], want[0]) and not torch.equal(got[0], warm[0])
    assert torch.equal(got[1], want[1])
    _same(got[2], want[2])


def test_one_stochastic_bf16_step_leaves_the_adapters_as_without_it(tiny):
    """bf16_update: stochastic concerns the bf16 caption projection, which is not paired: the f32 adapters are
    bitwise those of the nearest mode, the projection bitwise that of the stochastic run without the cap."""
    from ltx_amd.lora import adapter_pairs
    from ltx_amd.training import FusedAdamW
    sr = {"bf16_update": "stochastic", "sr_seed": 1234}
    models = [_build(tiny, ALL) for _ in range(3)]
    pairs = [adapter_pairs(m) for m in models]
    cap = _cap_between(statement(_np_pairs(pairs[0]), 1e30)["norm"])
    opts = [FusedAdamW(_trainable(models[0]), lr=LR, scale_weight_norms=cap, norm_pairs=pairs[0], **sr),
            FusedAdamW(_trainable(models[1]), lr=LR, scale_weight_norms=cap, norm_pairs=pairs[1]),
            FusedAdamW(_trainable(models[2]), lr=LR, **sr)]
    for m, opt in zip(models, opts):
        _set_grads(_trainable(m), 21)
        opt.step()
    assert 0 < int(opts[0].keys_scaled) == int(opts[1].keys_scaled) < len(pairs[0])
    bf16 = 0
    for a, b, c in zip(*[_trainable(m) for m in models]):
        if a.dtype == torch.float32:
            assert torch.equal(_bits(a.detach()), _bits(b.detach()))
        else:
            bf16 += 1
            assert torch.equal(a.detach(), c.detach())
    assert bf16 > 0


# ---------------------------------------------------------------------------------------------
# train_loop
# ---------------------------------------------------------------------------------------------
def _loop(tiny, out, epochs, extra, save=False, resume=None):
    from ltx_amd import io, training
    made = []

    class Recording(training.FusedAdamW):  # train_loop keeps its optimizer to itself
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(training, "FusedAdamW", Recording)
        model = _build(tiny, ALL)
        loader = io.LatentLoader(tiny["ds"]["train"], 2, DEV, shuffle=True, seed=1)
        tc = _config(dict(ALL, **extra), learning_rate=1e-3, num_epochs=epochs, output_dir=str(out), save_every_n_epochs=1)
        if save:
            tc.save_adapters = True
        logs = []
        torch.manual_seed(77)
        training.train_loop(model, tc, loader, tiny["prompt"], tiny["mask"], log_fn=lambda p, s: logs.append((s, p)),
                            resume_from=resume)
    return model, made[0], logs


def test_train_loop_logs_the_record_and_resumes_bitwise(tiny, tmp_path):
    import json
    import shutil
    from ltx_amd.lora import adapter_pairs
    KEYS = ("train/keys_scaled", "train/avg_key_norm", "train/max_key_norm")
    cap = _cap_between(statement(_np_pairs(adapter_pairs(_build(tiny, ALL))), 1e30)["norm"])
    extra = {"scale_weight_norms": cap, "ema_decay": 0.99}
    model_a, opt_a, logs_a = _loop(tiny, tmp_path / "a", 2, extra)
    steps = [p for _, p in logs_a if "train/loss" in p]
    assert len(steps) == 4 and all(all(k in p for k in KEYS) for p in steps)
    assert all(0 <= p["train/keys_scaled"] <= 20 and isinstance(p["train/keys_scaled"], int) for p in steps)
    assert steps[0]["train/keys_scaled"] >= 2  # two of the fixture's pairs are at twice the cap
    assert all(p["train/max_key_norm"] <= cap * (1 + 1e-5) and 0 < p["train/avg_key_norm"] <= p["train/max_key_norm"]
               for p in steps)
    assert opt_a.param_groups[0]["scale_weight_norms"] == cap and len(opt_a.norm_pairs) == 20
    # without the key: none of the three, and the optimizer is today's
    _, opt_off, logs_off = _loop(tiny, tmp_path / "off", 1, {})
    assert not any(k in p for _, p in logs_off for k in KEYS) and opt_off.norm_pairs is None
    assert "scale_weight_norms" not in opt_off.param_groups[0]
    # one epoch, save, resume, one epoch
    _loop(tiny, tmp_path / "b", 1, extra, save=True)
    with open(tmp_path / "b" / "adapter_epoch_1" / "train_state.json") as f:
        state = json.load(f)
    assert state["optimizer"]["param_groups"][0]["scale_weight_norms"] == cap
    assert not any("norm" in k for k in state if k != "optimizer")  # the rule is a function of the weights
    shutil.copytree(tmp_path / "b", tmp_path / "c")
    model_c, opt_c, logs_c = _loop(tiny, tmp_path / "c", 2, extra, resume="auto")

    def everything(model, opt):
        names = {id(p): n for n, p in model.named_parameters()}
        out = {n: p.detach() for n, p in model.named_parameters() if p.requires_grad}
        for p, st in opt.state.items():
            for k in ("exp_avg", "exp_avg_sq", "ema"):
                out[f"{k}.{names[id(p)]}"] = st[k]
        return out
    _same(everything(model_a, opt_a), everything(model_c, opt_c))
    second = lambda logs: [(s, [p[k] for k in KEYS], p["train/loss"]) for s, p in logs if p.get("train/epoch") == 1]
    assert second(logs_a) == second(logs_c) and len(second(logs_c)) == 2
