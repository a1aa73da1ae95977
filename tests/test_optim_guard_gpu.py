"""The non-finite guard of the LoRA optimizer step on the MI355X: FusedAdamW / FusedProdigy(skip_nonfinite=True)
skip, on the device, a step whose gradients are not all finite, and such a step is the step that was never
called. Every comparison is bitwise -- the guarded kernels run the unguarded kernels' row functions, so nothing
but equality is expected:

  * guarded steps on finite gradients are the unguarded steps;
  * a skipped step writes nothing but the guard's record, and settle() puts the host's counters back;
  * six steps with two poisoned ones leave what the four clean steps alone leave, the stochastic rounding's
    stream included;
  * through train_loop on the tiny model: without the guard a NaN batch poisons the weights, with it the weights
    stay finite and the log names the skipped steps; a run resumed from adapter_epoch_1 is the uninterrupted
    run with skips before and after the save; max_consecutive_skips ends a run that only skips.

The tensor set (optim_guard_utils) is small and reaches every branch of the row walks: numels 1, 7, 2047, 2048,
2049 and 5000 in f32 and bf16, gradients that are views one element into a buffer, a parameter without a
gradient."""
import json
import math
import shutil

import pytest
import torch

from optim_guard_utils import (MODES, NO_GRAD, POISONS, PoisonLoader, assert_same, clone_params, make_grads,
                               make_optimizer, make_params, poisoned, set_grads, snapshot)
from test_adapter_ckpt_gpu import _build, _config, _same, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _clipping(mode):
    return "max_grad_norm" in MODES[mode][1]


def _f64_norm(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads if g is not None))


# ---------------------------------------------------------------------------------------------
# the optimizers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_guarded_steps_on_finite_gradients_are_the_unguarded_steps(mode):
    pa = make_params(DEV)
    pb = clone_params(pa)
    off, on = make_optimizer(mode, pa), make_optimizer(mode, pb, skip_nonfinite=True)
    start = [p.detach().clone() for p in pa]
    for k in range(3):
        grads = make_grads(DEV, k)
        set_grads(pa, grads)
        set_grads(pb, grads)
        off.step()
        on.step()
        assert int(on.step_applied) == 1 and on.step_applied.dim() == 0 and on.step_applied.is_cuda
        assert off.step_applied is None
        (ta, ca), (tb, cb) = snapshot(off, pa), snapshot(on, pb)
        assert_same(ta, tb, (mode, k))
        assert ca == cb and ca["step.0"] == k + 1, (mode, k)
        # the pre-clip norm, also without max_grad_norm; the coefficient as today when clipping
        norm = _f64_norm(grads)
        assert on.grad_norm.dim() == 0 and abs(float(on.grad_norm) - norm) <= 1e-6 * norm
        if _clipping(mode):
            assert_same({"norm": off.grad_norm.reshape(1), "coef": off.clip_coef.reshape(1)},
                        {"norm": on.grad_norm.reshape(1), "coef": on.clip_coef.reshape(1)}, (mode, k))
            assert 0.0 < float(on.clip_coef) < 1.0  # the clip bites: the coefficient is in the arithmetic
        else:
            assert off.grad_norm is None and on.clip_coef is None
    assert on.skipped_steps == 0 and on.consecutive_skips == 0
    assert not on.state.get(pb[NO_GRAD]) and torch.equal(pb[NO_GRAD].detach(), start[NO_GRAD])
    moved = [not torch.equal(p.detach(), s) for p, s in zip(pb, start)]
    assert all(moved[:6]) and all(moved[8:12])  # every f32 tensor moved, and every bf16 one of many elements


@pytest.mark.parametrize("which", list(POISONS))
@pytest.mark.parametrize("mode", list(MODES))
def test_a_skipped_step_writes_nothing(mode, which):
    ps = make_params(DEV)
    opt = make_optimizer(mode, ps, skip_nonfinite=True)
    set_grads(ps, make_grads(DEV, 0))
    opt.step()  # a clean step first: moments, shadows and Prodigy's record are live
    before_t, before_c = snapshot(opt, ps)
    assert opt.skipped_steps == 0
    set_grads(ps, poisoned(make_grads(DEV, 1), which))
    opt.step()
    assert int(opt.step_applied) == 0
    after_t, _ = snapshot(opt, ps)
    if "record" in before_t:  # Prodigy: applied becomes 0, the other seven fields (k among them) stay
        assert float(before_t["record"][7]) == 1.0 and float(after_t["record"][7]) == 0.0
        assert float(after_t["record"][6]) == float(before_t["record"][6]) == 1.0
        before_t["record"], after_t["record"] = before_t["record"][:7], after_t["record"][:7]
    assert_same(before_t, after_t, (mode, which))
    assert not math.isfinite(float(opt.grad_norm))
    # the host counted the step; the outcome rolls it back
    assert opt.outcome_pending and opt.state[ps[0]]["step"] == 2
    opt.settle()
    assert not opt.outcome_pending and snapshot(opt, ps)[1] == before_c
    assert opt.skipped_steps == 1 and opt.consecutive_skips == 1
    # a second skipped step counts on from the device record; a clean one resets the run of skips
    opt.step()
    assert int(opt.step_applied) == 0 and opt.skipped_steps == 2 and opt.consecutive_skips == 2
    set_grads(ps, make_grads(DEV, 1))
    opt.step()
    assert int(opt.step_applied) == 1 and opt.skipped_steps == 2 and opt.consecutive_skips == 0
    assert opt.state[ps[0]]["step"] == 2 and all(bool(torch.isfinite(p.detach().float()).all()) for p in ps)


@pytest.mark.parametrize("mode", list(MODES))
def test_skipped_steps_are_steps_never_called(mode):
    pa = make_params(DEV)
    pb = clone_params(pa)
    guarded, clean = make_optimizer(mode, pa, skip_nonfinite=True), make_optimizer(mode, pb)
    bad = {2: "neginf_in_bf16", 5: "nan_first"}
    n = 0
    for k in range(1, 7):  # the bad gradients at steps 2 and 5
        if k in bad:
            set_grads(pa, poisoned(make_grads(DEV, 100 + k), bad[k]))
            guarded.step()
            continue
        grads = make_grads(DEV, n)
        n += 1
        set_grads(pa, grads)
        set_grads(pb, grads)
        guarded.step()
        clean.step()
    assert guarded.skipped_steps == 2 and n == 4  # settles
    (ta, ca), (tb, cb) = snapshot(guarded, pa), snapshot(clean, pb)
    assert_same(ta, tb, mode)
    assert ca == cb and ca["step.0"] == 4 and (ca["ema_steps"] == 4 or guarded.ema is None), (mode, ca)
    assert state_keys(guarded, pa) == state_keys(clean, pb)


def state_keys(opt, params):
    return [sorted(opt.state.get(p, {})) for p in params]


def test_state_dict_and_ema_swap_in_settle_first():
    ps = make_params(DEV)
    opt = make_optimizer("adamw_ema", ps, skip_nonfinite=True)
    set_grads(ps, make_grads(DEV, 0))
    opt.step()
    set_grads(ps, poisoned(make_grads(DEV, 1), "nan_first"))
    opt.step()
    assert opt.outcome_pending
    steps = {st["step"] for st in opt.state_dict()["state"].values()}
    assert steps == {1} and not opt.outcome_pending
    opt.step()
    assert opt.outcome_pending and opt.ema_steps == 2
    with opt.ema_weights():
        assert not opt.outcome_pending and opt.ema_steps == 1
    assert opt.skipped_steps == 2


@pytest.mark.parametrize("mode", ["adamw_sr_ema", "prodigy_clip_ema"])
def test_a_guarded_step_does_not_sync_with_the_host(mode):
    """The decision is taken on the device: guarded steps, a skipped one among them, run under torch's sync
    debug mode, where a blocking copy or a stream synchronize raises. What settle() waits for is an event
    behind the previous step's own launches."""
    ps = make_params(DEV)
    opt = make_optimizer(mode, ps, skip_nonfinite=True)
    grads = [make_grads(DEV, k) for k in range(2)] + [poisoned(make_grads(DEV, 2), "inf_tail"), make_grads(DEV, 3)]
    set_grads(ps, [None if g is None else g.clone() for g in grads[0]])
    set_grads([ps[12], ps[13]], grads[0][12:14])  # the views stay views
    opt.step()  # tables, partials, the record and the pinned slot warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gs in grads[1:]:
            for p, g in zip(ps, gs):
                if g is not None:
                    p.grad.copy_(g)  # the same buffers: the cached tables stay valid, as in a training loop
            opt.step()
        flag = opt.step_applied  # a device tensor: no sync yet
        with pytest.raises(RuntimeError):
            int(flag)  # reading it is the sync
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(opt.step_applied) == 1 and opt.skipped_steps == 1 and opt.state[ps[0]]["step"] == 3
    assert opt.ema_steps == 3


# ---------------------------------------------------------------------------------------------
# the tiny model through train_loop: 4 clips, batch 2, two optimizer steps per epoch
# ---------------------------------------------------------------------------------------------
POISON = {0: {1}, 1: {0}}  # steps 2 and 3 of a two-epoch run: one NaN batch per epoch, back to back
GUARD = {"skip_nonfinite": True, "max_grad_norm": 1.0, "ema_decay": 0.99}


def _run(tiny, out, epochs, extra, save=False, resume=None):
    """train_loop on fresh model / loader objects under torch.manual_seed(77) with the config attributes
    `extra` and the poisoned loader: (model, the optimizer train_loop built, logs)."""
    from ltx_amd import io, training
    made = []

    class Recording(training.FusedAdamW):  # train_loop keeps its optimizer to itself
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(training, "FusedAdamW", Recording)
        model = _build(tiny, {})
        loader = PoisonLoader(io.LatentLoader(tiny["ds"]["train"], 2, DEV, shuffle=True, seed=1), POISON)
        tc = _config(extra, learning_rate=1e-3, num_epochs=epochs, output_dir=str(out), save_every_n_epochs=1)
        if save:
            tc.save_adapters = True
        logs = []
        torch.manual_seed(77)
        try:
            training.train_loop(model, tc, loader, tiny["prompt"], tiny["mask"],
                                log_fn=lambda p, s: logs.append((s, p)), resume_from=resume)
        except FloatingPointError as e:
            return model, made[0], logs, e
    return model, made[0], logs, None


def _state(model, opt):
    names = {id(p): n for n, p in model.named_parameters()}
    tensors = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    steps = {}
    for p, st in opt.state.items():
        for k in ("exp_avg", "exp_avg_sq", "ema"):
            tensors[f"{k}.{names[id(p)]}"] = st[k]
        steps[names[id(p)]] = st["step"]
    return tensors, steps


_RUNS = {}


def _cached(tiny, tmp_path_factory, key):
    """The runs several tests read, each made once and left unchanged: "two" (two epochs, guarded), "first"
    (one epoch, guarded, with save_adapters), "off" (one epoch without the guard)."""
    if key not in _RUNS:
        out = tmp_path_factory.mktemp("guard_" + key) / "out"
        epochs, extra, save = {"two": (2, GUARD, False), "first": (1, GUARD, True),
                               "off": (1, {k: v for k, v in GUARD.items() if k != "skip_nonfinite"}, False)}[key]
        _RUNS[key] = (out,) + _run(tiny, out, epochs, extra, save=save)
    return _RUNS[key]


def _logged(logs, key):
    return [(s, p[key]) for s, p in logs if key in p]


def test_without_the_guard_a_nan_batch_poisons_the_weights_and_with_it_they_stay_finite(tiny, tmp_path_factory):
    _, model_off, opt_off, logs_off, _ = _cached(tiny, tmp_path_factory, "off")
    trained = [p for p in model_off.parameters() if p.requires_grad]
    assert trained and any(not bool(torch.isfinite(p.detach().float()).all()) for p in trained)  # today's run
    assert not _logged(logs_off, "train/step_applied") and not _logged(logs_off, "train/skipped_steps")
    _, model, opt, logs, err = _cached(tiny, tmp_path_factory, "two")
    assert err is None
    tensors, steps = _state(model, opt)
    assert all(bool(torch.isfinite(t.float()).all()) for t in tensors.values())
    # the log: 0 exactly at the poisoned steps, the running count, the norm of the skipped steps' gradients
    assert _logged(logs, "train/step_applied") == [(1, 1), (2, 0), (3, 0), (4, 1)]
    assert _logged(logs, "train/skipped_steps") == [(1, 0), (2, 1), (3, 2), (4, 2)]
    norms = [v for _, v in _logged(logs, "train/grad_norm")]
    assert [math.isfinite(v) for v in norms] == [True, False, False, True]
    losses = [v for _, v in _logged(logs, "train/loss")]
    assert [math.isfinite(v) for v in losses] == [True, False, False, True]
    # global_step counts attempts; the parameters and the EMA counted the two steps that happened
    assert set(steps.values()) == {2} and opt.ema_steps == 2 and opt.skipped_steps == 2
    assert _logged(logs, "train/ema_decay")[-1][1] == opt.ema.decay_at(2)


def test_resumed_run_is_bitwise_the_uninterrupted_run(tiny, tmp_path_factory, tmp_path):
    _, model_a, opt_a, logs_a, _ = _cached(tiny, tmp_path_factory, "two")
    out1, model_1, opt_1, logs_1, _ = _cached(tiny, tmp_path_factory, "first")
    out_b = tmp_path / "b"
    shutil.copytree(out1, out_b)
    with open(out_b / "adapter_epoch_1" / "train_state.json") as f:
        state = json.load(f)
    assert state["guard"] == {"skipped_steps": 1} and state["global_step"] == 2 and state["format_version"] == 1
    assert state["optimizer"]["param_groups"][0]["skip_nonfinite"] is True
    assert set(state["optimizer"]["step"].values()) == {1} and state["ema"]["ema_steps"] == 1  # rolled back
    model_b, opt_b, logs_b, err = _run(tiny, out_b, 2, GUARD, resume="auto")
    assert err is None
    (ta, sa), (tb, sb) = _state(model_a, opt_a), _state(model_b, opt_b)
    _same(ta, tb)
    assert sa == sb and opt_a.ema_steps == opt_b.ema_steps == 2 and opt_a.ema_decay == opt_b.ema_decay
    assert opt_b.skipped_steps == opt_a.skipped_steps == 2  # one before the save, one after
    epoch2 = lambda logs, key: [(s, v) for (s, v), (_, e) in zip(_logged(logs, key), _logged(logs, "train/epoch")) if e == 1]
    assert epoch2(logs_b, "train/step_applied") == epoch2(logs_a, "train/step_applied") == [(3, 0), (4, 1)]
    assert epoch2(logs_b, "train/skipped_steps") == epoch2(logs_a, "train/skipped_steps") == [(3, 2), (4, 2)]
    assert epoch2(logs_a, "train/loss")[1] == epoch2(logs_b, "train/loss")[1]  # the first is NaN on both sides
    assert not any(p.get("train/epoch") == 0 for _, p in logs_b)


def test_a_guard_mismatch_on_resume_raises_and_writes_nothing(tiny, tmp_path_factory):
    from ltx_amd import io
    from ltx_amd.training import EMASchedule, FusedAdamW
    path = _cached(tiny, tmp_path_factory, "first")[0] / "adapter_epoch_1"
    model = _build(tiny, {})
    params = [p for p in model.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in params]
    opt = FusedAdamW(params, lr=1e-3, max_grad_norm=1.0, ema=EMASchedule(0.99))
    with pytest.raises(ValueError, match="skip_nonfinite"):
        io.load_adapter_checkpoint(model, str(path), optimizer=opt)
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before)) and len(opt.state) == 0
    opt = FusedAdamW(params, lr=1e-3, max_grad_norm=1.0, ema=EMASchedule(0.99), skip_nonfinite=True)
    io.load_adapter_checkpoint(model, str(path), optimizer=opt)
    assert opt.skipped_steps == 1 and opt._guard_rec.is_cuda and opt._guard_rec[3:].view(torch.int64).tolist() == [1]


def test_max_consecutive_skips_ends_a_run_that_keeps_skipping(tiny, tmp_path):
    model, opt, logs, err = _run(tiny, tmp_path / "out", 2, dict(GUARD, max_consecutive_skips=1))
    assert isinstance(err, FloatingPointError) and "optimizer step 3" in str(err) and "max_consecutive_skips = 1" in str(err)
    assert _logged(logs, "train/step_applied") == [(1, 1), (2, 0), (3, 0)]
    assert all(bool(torch.isfinite(p.detach().float()).all()) for p in model.parameters() if p.requires_grad)
    # a limit the run stays under changes nothing
    _, _, logs2, err2 = _run(tiny, tmp_path / "out2", 2, dict(GUARD, max_consecutive_skips=2))
    assert err2 is None and _logged(logs2, "train/step_applied") == [(1, 1), (2, 0), (3, 0), (4, 1)]
