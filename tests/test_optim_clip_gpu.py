"""Global gradient-norm clipping and the learning-rate schedule of the LoRA optimizer step on the MI355X.

The yardstick of the norm is float64 (math.fsum of the exactly squared elements), not
torch.nn.utils.clip_grad_norm_, which rounds each bf16 tensor's norm to bf16 before combining them
(INTEGRATION.md section D). Everything else is bitwise: the clipped AdamW kernel against the unclipped
one fed (g.float() * coef).to(g.dtype), the off switch against today's calls, a huge max_grad_norm
against no clipping, a resumed run against the uninterrupted one, bucket-view gradients against plain ones.

Tensor sizes [1, 2047, 2048, 2049, 5000], alternating f32 and bf16: one element, one short of a chunk
(2048 elements, one block), exactly a chunk, one over, several chunks with a ragged tail -- the places
where a row's bounds can go wrong. The model runs use the tiny config and the construction of
tests/test_adapter_ckpt_gpu.py (2 layers, D = 128, 4 clips, batch 2)."""
import math
import shutil

import numpy as np
import pytest
import torch

from test_adapter_ckpt_gpu import _build, _config, _same, _state, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 77
SIZES = [1, 2047, 2048, 2049, 5000]
DTYPES = [torch.float32, torch.bfloat16, torch.float32, torch.bfloat16, torch.float32]
N = sum(SIZES)


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g).to(dt).to(DEV)) for n, dt in zip(SIZES, DTYPES)]


def _int_grads(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-3, 4, (n,), generator=g).to(dt).to(DEV) for n, dt in zip(SIZES, DTYPES)]


def _rand_grads(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(scale * torch.randn(n, generator=g)).to(dt).to(DEV) for n, dt in zip(SIZES, DTYPES)]


def _sumsq64(grads):
    """The correctly rounded float64 sum of squares: every square of an f32 / bf16 value is exact in
    float64, and math.fsum rounds their exact sum once."""
    sq = []
    for g in grads:
        if g is not None:
            sq.extend((g.detach().double().cpu().flatten() ** 2).tolist())
    return math.fsum(sq)


def _record(opt):
    """(sumsq float64, norm float32, coef float32) of the last clipped step, as numpy scalars."""
    assert opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda and opt.grad_norm.dtype == torch.float32
    assert opt.clip_coef.dim() == 0 and opt.clip_coef.is_cuda and opt.clip_coef.dtype == torch.float32
    return (np.float64(opt.clip_sumsq.item()), np.float32(opt.grad_norm.item()), np.float32(opt.clip_coef.item()))


def _within_one_f32_ulp(got, want64):
    want = np.float32(want64)
    return abs(np.float64(got) - np.float64(want64)) <= np.float64(np.spacing(np.abs(want)))


def _step(opt, ps, grads):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.clone()
    opt.step()


# ---------------------------------------------------------------------------------------------
# the record: sumsq, norm, coef
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [1.0, 2.5, 1e4])
def test_exact_inputs_give_the_exact_record(max_norm):
    """Integer gradients in [-3, 3]: every square and every partial sum is an integer below 2^53, so
    any order gives the same float64; the norm and the coefficient are pinned from there."""
    from ltx_amd.training import FusedAdamW
    ps, grads = _params(), _int_grads(1)
    want = float(sum(int((g.double() ** 2).sum().item()) for g in grads))
    assert want == _sumsq64(grads) and want > 1e4
    opt = FusedAdamW(ps, lr=1e-3, max_grad_norm=max_norm)
    _step(opt, ps, grads)
    sumsq, norm, coef = _record(opt)
    assert sumsq.tobytes() == np.float64(want).tobytes()
    assert _within_one_f32_ulp(norm, np.sqrt(np.float64(want)))
    want_coef = np.minimum(np.float32(1.0), np.float32(max_norm) / (norm + np.float32(1e-6)))
    assert want_coef.dtype == np.float32 and coef.tobytes() == want_coef.tobytes()
    assert (coef == 1.0) == (max_norm == 1e4)
    for p, g in zip(ps, grads):
        assert torch.equal(p.grad, g)  # .grad is left unscaled


def test_random_inputs_sumsq_error_bound():
    """|sumsq - exact| / exact <= N 2^-53: the worst case of any summation order of N exact,
    non-negative float64 terms (each of at most N - 1 additions errs by at most 2^-53 relative to a
    partial sum that never exceeds the total)."""
    from ltx_amd.training import FusedAdamW
    ps = _params()
    opt = FusedAdamW(ps, lr=1e-3, max_grad_norm=1.0)
    for seed, scale in ((2, 1.0), (3, 1e-3), (4, 300.0)):
        grads = _rand_grads(seed, scale)
        _step(opt, ps, grads)
        sumsq, norm, coef = _record(opt)
        want = _sumsq64(grads)
        err = abs(float(sumsq) - want) / want
        print(f"scale {scale}: sumsq {float(sumsq)!r} exact {want!r} rel err {err:.3e} bound {N * 2.0 ** -53:.3e}")
        assert err <= N * 2.0 ** -53
        assert _within_one_f32_ulp(norm, math.sqrt(want))
        assert (coef < 1.0) == (float(norm) > 1.0)


def test_two_calls_give_the_same_record_bitwise():
    from ltx_amd.training import FusedAdamW
    ps, grads = _params(), _rand_grads(5)
    opt = FusedAdamW(ps, lr=1e-3, max_grad_norm=1.0)
    _step(opt, ps, grads)
    first, held = _record(opt), opt.grad_norm
    _step(opt, ps, grads)
    second = _record(opt)
    assert [v.tobytes() for v in first] == [v.tobytes() for v in second]
    # a fresh optimizer (other table and partial buffers) as well
    ps2 = _params()
    opt2 = FusedAdamW(ps2, lr=1e-3, max_grad_norm=1.0)
    _step(opt2, ps2, grads)
    assert [v.tobytes() for v in _record(opt2)] == [v.tobytes() for v in first]
    # a norm somebody holds keeps its value when the next step has other gradients
    _step(opt, ps, _rand_grads(6))
    assert np.float32(held.item()).tobytes() == first[1].tobytes() and _record(opt)[1] != first[1]


# ---------------------------------------------------------------------------------------------
# the AdamW kernel
# ---------------------------------------------------------------------------------------------
def _raw_state(ps):
    return [{"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)} for p in ps]


@pytest.mark.parametrize("coef", [0.37, 1.0])
def test_adamw_multi_clip_is_adamw_multi_on_the_scaled_gradient(coef):
    """ltx_adamw_multi_clip with a device coefficient == ltx_adamw_multi fed (g.float() * coef).to(dtype):
    parameters and both moments bitwise, both dtypes, three steps. With coef = 1 that is ltx_adamw_multi
    on the raw gradients."""
    from ltx_amd import ops
    from ltx_amd.training import FusedAdamW
    c = torch.tensor(coef, dtype=torch.float32, device=DEV)
    pa, pb = _params(7), _params(7)
    sa, sb = _raw_state(pa), _raw_state(pb)
    ta, tb = FusedAdamW(pa), FusedAdamW(pb)  # for their chunk tables only
    hyper = (1e-2, 0.9, 0.999, 1e-8, 1e-2)
    for step in (1, 2, 3):
        grads = _rand_grads(10 + step)
        fed = grads if coef == 1.0 else [(g.float() * c).to(g.dtype) for g in grads]
        for dt in (torch.float32, torch.bfloat16):
            idx = [i for i, d in enumerate(DTYPES) if d == dt]
            bf = 1 if dt == torch.bfloat16 else 0
            dev, rows = ta._items_table("adamw", dt, [(pa[i], grads[i], sa[i]) for i in idx])
            assert rows == sum(-(-SIZES[i] // 2048) for i in idx)
            ops.call("ltx_adamw_multi_clip", ops._p(dev), rows, bf, *hyper, step, ops._p(c), ops._s())
            dev, rows = tb._items_table("adamw", dt, [(pb[i], fed[i], sb[i]) for i in idx])
            ops.call("ltx_adamw_multi", ops._p(dev), rows, bf, *hyper, step, ops._s())
        for i in range(len(SIZES)):
            assert torch.equal(pa[i], pb[i]) and not torch.equal(pa[i], _params(7)[i]), (step, i)
            assert torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]), (step, i)
            assert torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"]), (step, i)
    torch.cuda.synchronize()


def test_none_gradients_single_tensor_groups_and_mixed_steps():
    """A gradient set to None is left out of the norm and of the step; a dtype group of one tensor goes
    through the table kernels; tensors at different step counts are grouped by (dtype, step). The
    reference is the unclipped optimizer fed the gradients scaled by the coefficient read back."""
    from ltx_amd.training import FusedAdamW
    pc, pu = _params(8), _params(8)
    clip, plain = FusedAdamW(pc, lr=1e-2, max_grad_norm=0.5), FusedAdamW(pu, lr=1e-2)
    # step 1: bf16 has one tensor, f32 two; step 2: everything (f32 then holds steps 2, 2 and 1)
    masks = [(True, True, False, False, True), (True,) * 5, (False, False, True, True, False)]
    for k, mask in enumerate(masks):
        full = _rand_grads(20 + k)
        grads = [g if m else None for g, m in zip(full, mask)]
        before = [p.detach().clone() for p in pc]
        _step(clip, pc, grads)
        sumsq, norm, coef = _record(clip)
        want = _sumsq64(grads)
        assert abs(float(sumsq) - want) / want <= N * 2.0 ** -53
        if not all(mask):
            assert abs(float(sumsq) - _sumsq64(full)) / want > 1e-3
        assert coef < 1.0
        for p, b, m in zip(pc, before, mask):
            assert torch.equal(p, b) != m
        _step(plain, pu, [None if g is None else (g.float() * clip.clip_coef).to(g.dtype) for g in grads])
        for i, (a, b) in enumerate(zip(pc, pu)):
            assert torch.equal(a, b), (k, i)
            assert (a in clip.state) == (b in plain.state)
            if a in clip.state:
                assert clip.state[a]["step"] == plain.state[b]["step"]
                assert torch.equal(clip.state[a]["exp_avg"], plain.state[b]["exp_avg"]), (k, i)
                assert torch.equal(clip.state[a]["exp_avg_sq"], plain.state[b]["exp_avg_sq"]), (k, i)
    assert [clip.state[p]["step"] for p in pc] == [2, 2, 2, 2, 2]
    # no gradient at all: nothing is launched
    _step(clip, pc, [None] * 5)
    assert clip.grad_norm is None and clip.clip_coef is None


def test_off_switch_issues_todays_calls(monkeypatch):
    """max_grad_norm absent, None or 0: FusedAdamW.step passes ops.call exactly the entry points it
    passes today (one ltx_adamw_multi for the three f32 tensors, ltx_adamw_step for the single bf16 one)
    and none of the new ones; the results are bitwise the same. With clipping on, the launch order is the
    norm launches, the coefficient, then the clipped AdamW launches."""
    from ltx_amd import ops
    from ltx_amd.training import FusedAdamW
    names = []
    real = ops.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(ops, "call", call)
    grads = [[g if i != 3 else None for i, g in enumerate(_rand_grads(30 + k))] for k in range(2)]
    results = []
    for kw in ({}, {"max_grad_norm": None}, {"max_grad_norm": 0}, {"max_grad_norm": 0.0}):
        ps = _params(9)
        opt = FusedAdamW(ps, lr=1e-2, **kw)
        del names[:]
        for gs in grads:
            _step(opt, ps, gs)
        assert names == ["ltx_adamw_multi", "ltx_adamw_step"] * 2, kw
        assert opt.grad_norm is None
        results.append([p.detach().clone() for p in ps])
    for r in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, results[0]))
    ps = _params(9)
    opt = FusedAdamW(ps, lr=1e-2, max_grad_norm=1e30)
    del names[:]
    for gs in grads:
        _step(opt, ps, gs)
    assert names == (["ltx_grad_sumsq_multi"] * 2 + ["ltx_grad_clip_coef"] + ["ltx_adamw_multi_clip"] * 2) * 2
    # ... and a clip that never bites changes nothing
    assert float(opt.clip_coef) == 1.0
    assert all(torch.equal(a, b) for a, b in zip(ps, results[0]))


# ---------------------------------------------------------------------------------------------
# the tiny model through train_loop
# ---------------------------------------------------------------------------------------------
def _run(tiny, out, epochs, extra=None, accum=2, save=False, resume=None):
    """train_loop on fresh model / loader objects under torch.manual_seed(SEED): (model, the optimizer
    train_loop built, logs). The optimizer records the gradients every step() was called on."""
    from ltx_amd import io, training
    made = []

    class Recording(training.FusedAdamW):  # train_loop keeps its optimizer to itself
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.seen = []
            made.append(self)

        def step(self, closure=None):
            self.seen.append([p.grad.detach().clone() for g in self.param_groups for p in g["params"]
                              if p.grad is not None])
            return super().step(closure)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(training, "FusedAdamW", Recording)
        model = _build(tiny, {})
        loader = io.LatentLoader(tiny["ds"]["train"], 2, DEV, shuffle=True, seed=1)
        tc = _config(extra or {}, learning_rate=1e-3, num_epochs=epochs, gradient_accumulation_steps=accum,
                     output_dir=str(out), save_every_n_epochs=1)
        if save:
            tc.save_adapters = True
        logs = []
        torch.manual_seed(SEED)
        training.train_loop(model, tc, loader, tiny["prompt"], tiny["mask"], log_fn=lambda p, s: logs.append((s, p)),
                            resume_from=resume)
    return model, made[0], logs


_SHARED = {}


def _baseline(tiny, tmp_path_factory):
    """Two epochs with accumulation 2 (two optimizer steps) without the keys and with max_grad_norm =
    1e30, run once and left unchanged."""
    if not _SHARED:
        _SHARED["plain"] = _run(tiny, tmp_path_factory.mktemp("plain") / "out", 2)
        _SHARED["huge"] = _run(tiny, tmp_path_factory.mktemp("huge") / "out", 2, {"max_grad_norm": 1e30})
    return _SHARED["plain"], _SHARED["huge"]


def _steps(logs):
    return [(s, p) for s, p in logs if "train/loss" in p]


def test_huge_max_grad_norm_is_the_unclipped_run(tiny, tmp_path_factory):
    (model_a, opt_a, logs_a), (model_b, opt_b, logs_b) = _baseline(tiny, tmp_path_factory)
    assert [s for s, _ in _steps(logs_a)] == [s for s, _ in _steps(logs_b)] == [1, 2]
    assert not any("train/grad_norm" in p for _, p in logs_a)  # without the key the payload is today's
    assert all("train/grad_norm" in p for _, p in _steps(logs_b))
    for (_, pa), (_, pb) in zip(_steps(logs_a), _steps(logs_b)):
        assert {k: v for k, v in pb.items() if k != "train/grad_norm"} == pa and pa["train/lr"] == 1e-3
    for x, y in zip(_state(model_a, opt_a)[:2], _state(model_b, opt_b)[:2]):
        _same(x, y)
    assert opt_a.param_groups[0]["max_grad_norm"] is None and opt_b.param_groups[0]["max_grad_norm"] == 1e30


def test_logged_grad_norm_is_the_float64_norm_of_the_steps_gradients(tiny, tmp_path_factory):
    _, (_, opt, logs) = _baseline(tiny, tmp_path_factory)
    assert len(opt.seen) == 2
    assert {g.dtype for g in opt.seen[0]} == {torch.float32, torch.bfloat16}
    for (_, p), grads in zip(_steps(logs), opt.seen):
        want = math.sqrt(_sumsq64(grads))
        got = p["train/grad_norm"]
        print(f"logged {got!r} float64 {want!r}")
        assert isinstance(got, float) and got > 0 and _within_one_f32_ulp(np.float32(got), want)


def test_a_norm_below_the_first_steps_norm_changes_the_run(tiny, tmp_path_factory, tmp_path):
    (model_a, opt_a, _), (_, _, logs_b) = _baseline(tiny, tmp_path_factory)
    first = _steps(logs_b)[0][1]["train/grad_norm"]
    model_c, opt_c, logs_c = _run(tiny, tmp_path / "out", 2, {"max_grad_norm": 0.5 * first})
    assert _steps(logs_c)[0][1]["train/grad_norm"] == first  # the pre-clip norm of the same first gradients
    assert float(opt_c.clip_coef) < 1.0
    pa, pc = _state(model_a, opt_a)[0], _state(model_c, opt_c)[0]
    assert sorted(pa) == sorted(pc) and any(not torch.equal(pa[k], pc[k]) for k in pa)


def test_logged_lr_follows_the_cosine_schedule(tiny, tmp_path):
    """cosine with two warm-up steps over the default total (4 epochs x (2 batches // 2) = 4 steps)"""
    from ltx_amd.training import LRSchedule
    model, opt, logs = _run(tiny, tmp_path / "out", 4, {"lr_scheduler": "cosine", "lr_warmup_steps": 2,
                                                         "max_grad_norm": 1e30})
    sched = LRSchedule("cosine", 1e-3, 2, 4)
    got = [(s, p["train/lr"]) for s, p in _steps(logs)]
    assert got == [(s + 1, sched.at(s)) for s in range(4)]
    assert [lr for _, lr in got] == [0.0, 5e-4, 1e-3, 1e-3 * (0.5 * (1.0 + math.cos(math.pi * 0.5)))]
    assert all(p["train/grad_norm"] > 0 for _, p in _steps(logs))


def test_resumed_run_with_clipping_and_cosine_is_bitwise_the_uninterrupted_run(tiny, tmp_path_factory, tmp_path):
    """save_adapters, clipping that bites and the cosine schedule (one warm-up step, 4 steps in all), stopped
    after epoch 1 and resumed: parameters, moments, steps and every logged value of epoch 2 are those of the
    uninterrupted run. max_grad_norm comes back from train_state.json with the other hyper-parameters."""
    import json
    _, (_, _, logs_h) = _baseline(tiny, tmp_path_factory)
    extra = {"max_grad_norm": 0.5 * _steps(logs_h)[0][1]["train/grad_norm"], "lr_scheduler": "cosine",
             "lr_warmup_steps": 1}
    model_a, opt_a, logs_a = _run(tiny, tmp_path / "a", 2, extra, accum=1)
    out_b = tmp_path / "b"
    # the first epoch of a two-epoch plan (lr_total_steps = 4, what the two-epoch run derives)
    _run(tiny, out_b, 1, dict(extra, lr_total_steps=4), accum=1, save=True)
    with open(out_b / "adapter_epoch_1" / "train_state.json") as f:
        saved = json.load(f)["optimizer"]["param_groups"][0]
    assert saved["max_grad_norm"] == extra["max_grad_norm"]
    model_b, opt_b, logs_b = _run(tiny, out_b, 2, extra, accum=1, resume="auto")
    (pa, ma, sa), (pb, mb, sb) = _state(model_a, opt_a), _state(model_b, opt_b)
    _same(pa, pb)
    _same(ma, mb)
    assert sa == sb and set(sa.values()) == {4}
    assert len(logs_b) > 0 and logs_a[-len(logs_b):] == logs_b
    steps_b = _steps(logs_b)
    assert [s for s, _ in steps_b] == [3, 4]
    assert all(p["train/grad_norm"] > 0 and p["train/epoch"] == 1 for _, p in steps_b)
    from ltx_amd.training import LRSchedule
    assert [p["train/lr"] for _, p in steps_b] == [LRSchedule("cosine", 1e-3, 1, 4).at(s) for s in (2, 3)]
    assert float(opt_b.clip_coef) < 1.0 and steps_b[0][1]["train/lr"] != steps_b[1][1]["train/lr"]


def test_bucket_view_gradients_give_the_same_clipped_run(tiny, tmp_path_factory):
    """GradAllReduce at world size 1: the gradients are views into the reducer's flat buckets (other
    addresses and alignments than torch's own allocations); the clipped run is bitwise the one without
    the reducer, logged norms included."""
    from ltx_amd import io, training
    from ltx_amd.scheduler import RectifiedFlowScheduler
    _, (_, _, logs_h) = _baseline(tiny, tmp_path_factory)
    max_norm = 0.5 * _steps(logs_h)[0][1]["train/grad_norm"]

    def run(with_reducer):
        model = _build(tiny, {})
        params = [p for p in model.parameters() if p.requires_grad]
        opt = training.FusedAdamW(params, lr=1e-3, max_grad_norm=max_norm)
        red = None
        if with_reducer:
            red = training.GradAllReduce(params, bucket_mb=0.05, order=model.grad_ready_order()).install(model)
        loader = io.LatentLoader(tiny["ds"]["train"], 2, DEV, shuffle=True, seed=1)
        tc = _config({}, learning_rate=1e-3, num_epochs=2, gradient_accumulation_steps=2)
        logs, step = [], 0
        torch.manual_seed(SEED)
        for epoch in range(2):
            loader.set_epoch(epoch)  # as train_loop does
            step, _ = training.train_one_epoch(model, loader, opt, RectifiedFlowScheduler(), model.patchifier, DEV, tc,
                                               tiny["prompt"], tiny["mask"], epoch, step, red,
                                               lambda p, s: logs.append((s, p)))
        if with_reducer:
            assert len(red.buckets) >= 2  # at least one per dtype
            for b in red.buckets:
                lo, hi = b["flat"].data_ptr(), b["flat"].data_ptr() + b["flat"].numel() * b["flat"].element_size()
                assert all(lo <= p.grad.data_ptr() < hi for p in b["params"])
            red.uninstall()
        return model, opt, logs
    (ma, oa, la), (mb, ob, lb) = run(False), run(True)
    for x, y in zip(_state(ma, oa)[:2], _state(mb, ob)[:2]):
        _same(x, y)
    assert la == lb and len(la) == 2 and all("train/grad_norm" in p for _, p in la)
    assert float(oa.clip_coef) < 1.0 and float(oa.clip_coef) == float(ob.clip_coef)
