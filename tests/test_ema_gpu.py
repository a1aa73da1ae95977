"""The exponential moving average of the trained weights inside the LoRA optimizer step on the MI355X
(FusedAdamW(ema=EMASchedule): ltx_adamw_multi_ema, ltx_ema_load_multi, ltx_ema_restore_multi). Every
comparison is bitwise:

  * parameters, moments and steps against a twin optimizer without the EMA (the EMA only observes);
  * every shadow after every step against torch's unfused s.sub_((s - p.float()) * omd) on the device,
    omd = float32(1 - decay_at(n)) -- three separately rounded f32 operations, f32 shadows for bf16
    parameters, the first step (decay 0, omd = 1) included;
  * the swap kernels, and a forward under ema_weights() against a model loaded with weights="ema";
  * a resumed run against the uninterrupted one, shadows and val/loss_ema included;
  * with no EMA key set, the entry points called and the files written are today's.

Tensor sizes and dtypes are those of tests/test_optim_clip_gpu.py ([1, 2047, 2048, 2049, 5000], alternating
f32 and bf16: one element, one short of a chunk, a chunk, one over, several chunks with a ragged tail); the
model runs use the tiny config and helpers of tests/test_adapter_ckpt_gpu.py."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

import ltx_oracle as O
from test_adapter_ckpt_gpu import CASES, _build, _config, _fixed_inputs, _same, _state, tiny  # noqa: F401  (tiny: the fixture)
from test_optim_clip_gpu import DTYPES, SIZES, _params, _rand_grads, _step

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 77
NEW_ENTRY_POINTS = {"ltx_adamw_multi_ema", "ltx_ema_load_multi", "ltx_ema_restore_multi"}
FOUR = ["adapter_config.json", "adapter_model.safetensors", "optimizer.safetensors", "train_state.json"]
EMA = {"ema_decay": 0.999}


def _want_shadow(prev, p, decay):
    """torch's unfused update from the previous shadow and the new parameter, on the device"""
    omd = torch.tensor(1.0 - decay, dtype=torch.float32, device=DEV)  # float32(1 - decay)
    s = prev.clone()
    return s.sub_((s - p.detach().float()) * omd)


# ---------------------------------------------------------------------------------------------
# the fused step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_step_is_the_twin_optimizers_and_shadows_follow_the_unfused_arithmetic(max_norm):
    from ltx_amd.training import EMASchedule, FusedAdamW
    sched = EMASchedule(0.999)
    pe, pt = _params(3), _params(3)
    ema = FusedAdamW(pe, lr=1e-2, max_grad_norm=max_norm, ema=sched)
    twin = FusedAdamW(pt, lr=1e-2, max_grad_norm=max_norm)
    start = [p.detach().clone() for p in pe]
    for k in range(5):
        n = k + 1
        grads = _rand_grads(40 + k)
        prev = [ema.state[p]["ema"].clone() if k else p.detach().float().clone() for p in pe]
        _step(ema, pe, grads)
        _step(twin, pt, grads)
        assert ema.ema_steps == n and ema.ema_decay == sched.decay_at(n) and isinstance(ema.ema_decay, float)
        for i, (a, b) in enumerate(zip(pe, pt)):
            sa, sb = ema.state[a], twin.state[b]
            assert torch.equal(a, b) and not torch.equal(a, start[i]), (k, i)
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (k, i)
            assert sa["step"] == sb["step"] == n and "ema" not in sb
            shadow = sa["ema"]
            assert shadow.dtype == torch.float32 and shadow.shape == a.shape and shadow.is_cuda
            assert torch.equal(shadow, _want_shadow(prev[i], a, sched.decay_at(n))), (k, i, DTYPES[i])
        if max_norm:
            assert float(ema.clip_coef) < 1.0 and float(ema.clip_coef) == float(twin.clip_coef)
    assert [sched.decay_at(n) for n in (1, 2, 3)] == [0.0, 2 / 11, 0.25]
    # the shadows average: after five steps they are neither the weights nor the start
    for i, p in enumerate(pe):
        assert not torch.equal(ema.state[p]["ema"], p.detach().float())
        assert not torch.equal(ema.state[p]["ema"], start[i].float())


def test_launches_per_bucket_and_the_clip_launches_in_front(monkeypatch):
    """One ltx_adamw_multi_ema per (dtype, step) bucket -- a dtype group of one tensor included -- and with
    max_grad_norm the norm and coefficient launches in front, unchanged."""
    from ltx_amd import ops
    from ltx_amd.training import EMASchedule, FusedAdamW
    names = []
    real = ops.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(ops, "call", call)
    grads = [g if i != 3 else None for i, g in enumerate(_rand_grads(31))]  # bf16 is left with one tensor
    ps = _params(9)
    _step(FusedAdamW(ps, lr=1e-2, ema=EMASchedule(0.999)), ps, grads)
    assert names == ["ltx_adamw_multi_ema"] * 2
    del names[:]
    ps = _params(9)
    _step(FusedAdamW(ps, lr=1e-2, max_grad_norm=1.0, ema=EMASchedule(0.999)), ps, grads)
    assert names == ["ltx_grad_sumsq_multi"] * 2 + ["ltx_grad_clip_coef"] + ["ltx_adamw_multi_ema"] * 2


def test_rows_without_a_gradient_keep_shadow_and_moments_and_the_table_follows_the_shadow_pointer():
    from ltx_amd.training import EMASchedule, FusedAdamW
    sched = EMASchedule(0.999)
    ps = _params(4)
    opt = FusedAdamW(ps, lr=1e-2, ema=sched)
    _step(opt, ps, _rand_grads(50))
    _step(opt, ps, _rand_grads(51))
    mask = (True, False, False, True, True)
    keep = [{k: opt.state[p][k].clone() for k in ("ema", "exp_avg", "exp_avg_sq")} for p in ps]
    before = [p.detach().clone() for p in ps]
    _step(opt, ps, [g if m else None for g, m in zip(_rand_grads(52), mask)])
    assert opt.ema_steps == 3
    for i, (p, m) in enumerate(zip(ps, mask)):
        st = opt.state[p]
        assert st["step"] == (3 if m else 2)
        assert torch.equal(p, before[i]) != m
        for k in ("ema", "exp_avg", "exp_avg_sq"):
            assert torch.equal(st[k], keep[i][k]) != m, (i, k)
        if m:
            assert torch.equal(st["ema"], _want_shadow(keep[i]["ema"], p, sched.decay_at(3)))
    # a shadow that moved to another buffer (a restore that could not copy in place): the cached table
    # must not keep writing the old one
    old = opt.state[ps[4]]["ema"]
    held = old.clone()
    opt.state[ps[4]]["ema"] = new = old.clone()
    _step(opt, ps, _rand_grads(53))
    assert torch.equal(old, held)
    assert torch.equal(new, _want_shadow(held, ps[4], sched.decay_at(4)))


# ---------------------------------------------------------------------------------------------
# swap
# ---------------------------------------------------------------------------------------------
def test_swap_in_installs_the_shadows_and_swap_out_restores_bitwise():
    from ltx_amd import ops
    from ltx_amd.training import EMASchedule, FusedAdamW
    ps = _params(5)
    opt = FusedAdamW(ps, lr=1e-2, ema=EMASchedule(0.999))
    with pytest.raises(RuntimeError, match="not swapped in"):
        opt.ema_swap_out()
    for k in range(3):
        _step(opt, ps, _rand_grads(60 + k))
    live = [p.detach().clone() for p in ps]
    shadows = [opt.state[p]["ema"].clone() for p in ps]
    stashes = None
    for _ in range(2):
        gen = ops.weight_generation()
        opt.ema_swap_in()
        assert ops.weight_generation() > gen
        for p, s, dt, was in zip(ps, shadows, DTYPES, live):
            assert p.dtype == dt and torch.equal(p, s.to(dt)) and not torch.equal(p, was)
            if dt == torch.bfloat16 and p.numel() > 1:
                assert not torch.equal(p.float(), s)  # rounded, not truncated away: the shadow has more bits
        with pytest.raises(RuntimeError, match="swapped in"):
            opt.ema_swap_in()
        with pytest.raises(RuntimeError, match="swapped in"):
            opt.step()
        gen = ops.weight_generation()
        opt.ema_swap_out()
        assert ops.weight_generation() > gen
        for p, was, s in zip(ps, live, shadows):
            assert torch.equal(p, was) and torch.equal(opt.state[p]["ema"], s)
        ptrs = [opt._ema_stash[p].data_ptr() for p in ps]
        assert stashes in (None, ptrs)  # allocated on first use, then reused
        stashes = ptrs
    with pytest.raises(RuntimeError, match="not swapped in"):
        opt.ema_swap_out()
    with opt.ema_weights():
        assert torch.equal(ps[4], shadows[4])
    assert torch.equal(ps[4], live[4])
    _step(opt, ps, _rand_grads(70))  # and the step runs again
    assert opt.ema_steps == 4


# ---------------------------------------------------------------------------------------------
# the tiny model through train_loop
# ---------------------------------------------------------------------------------------------
def _run(tiny, case, out, epochs, extra=None, val=False, save=False, resume=None, record=None):
    """train_loop on fresh model / loader objects under torch.manual_seed(SEED) with the config attributes
    of CASES[case] and `extra`: (model, the optimizer train_loop built, logs)."""
    from ltx_amd import io, ops, training
    attrs, accum = CASES[case]
    made = []

    class Recording(training.FusedAdamW):  # train_loop keeps its optimizer to itself
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(training, "FusedAdamW", Recording)
        if record is not None:
            real = ops.call
            mp.setattr(ops, "call", lambda name, *a: (record.append(name), real(name, *a))[1])
        model = _build(tiny, attrs)
        loader = io.LatentLoader(tiny["ds"]["train"], 2, DEV, shuffle=True, seed=1)
        vloader = io.LatentLoader(tiny["ds"]["val"], 2, DEV, shuffle=False) if val else None
        tc = _config(dict(attrs, **(extra or {})), learning_rate=1e-3, num_epochs=epochs,
                     gradient_accumulation_steps=accum, output_dir=str(out), save_every_n_epochs=1)
        if save:
            tc.save_adapters = True
        logs = []
        torch.manual_seed(SEED)
        training.train_loop(model, tc, loader, tiny["prompt"], tiny["mask"], log_fn=lambda p, s: logs.append((s, p)),
                            val_dataloader=vloader, resume_from=resume)
    return model, made[0], logs


def _shadows(model, opt):
    names = {id(p): n for n, p in model.named_parameters()}
    return {names[id(p)]: st["ema"] for p, st in opt.state.items()}


_FIRST = {}


def _first_epoch(tiny, tmp_path_factory, case):
    """One epoch with the EMA and save_adapters (validation for attn2), run once per case and left
    unchanged: (output directory, model, optimizer, logs)."""
    if case not in _FIRST:
        out = tmp_path_factory.mktemp("ema_first") / "out"
        _FIRST[case] = (out,) + _run(tiny, case, out, 1, EMA, val=(case == "attn2"), save=True)
    return _FIRST[case]


@pytest.mark.parametrize("case", ["attn2", "all_dropout_accum2"])
def test_resumed_run_with_ema_is_bitwise_the_uninterrupted_run(tiny, tmp_path_factory, tmp_path, case):
    import shutil
    from ltx_amd.training import EMASchedule
    val = case == "attn2"
    per_epoch = 2 // CASES[case][1]
    model_a, opt_a, logs_a = _run(tiny, case, tmp_path / "a", 2, EMA, val=val)
    out_b = tmp_path / "b"
    first, _, _, logs_1 = _first_epoch(tiny, tmp_path_factory, case)
    shutil.copytree(first, out_b)
    assert sorted(os.listdir(out_b / "adapter_epoch_1")) == sorted(FOUR + ["ema_model.safetensors"])
    with open(out_b / "adapter_epoch_1" / "train_state.json") as f:
        block = json.load(f)["ema"]
    assert block == dict(EMASchedule(0.999).fields(), ema_steps=per_epoch)
    model_b, opt_b, logs_b = _run(tiny, case, out_b, 2, EMA, val=val, resume="auto")
    (pa, ma, sa), (pb, mb, sb) = _state(model_a, opt_a), _state(model_b, opt_b)
    _same(pa, pb)
    _same(ma, mb)
    assert sa == sb and set(sa.values()) == {2 * per_epoch}
    _same(_shadows(model_a, opt_a), _shadows(model_b, opt_b))
    assert sorted(_shadows(model_a, opt_a)) == sorted(pa)
    assert all(s.dtype == torch.float32 for s in _shadows(model_b, opt_b).values())
    assert opt_a.ema_steps == opt_b.ema_steps == 2 * per_epoch and opt_a.ema_decay == opt_b.ema_decay
    # every logged value of the second epoch, train/ema_decay and val/loss_ema among them
    assert len(logs_b) > 0 and logs_a[-len(logs_b):] == logs_b and logs_a[:len(logs_1)] == logs_1
    steps = [(s, p["train/ema_decay"]) for s, p in logs_a if "train/loss" in p]
    assert steps == [(n, EMASchedule(0.999).decay_at(n)) for n in range(1, 2 * per_epoch + 1)]
    assert [s for s, p in logs_b if "train/ema_decay" in p] == list(range(per_epoch + 1, 2 * per_epoch + 1))
    if val:
        kinds = ["val_ema" if "val/loss_ema" in p else "val" if "val/loss" in p else
                 "epoch" if "train/epoch_loss" in p else "step" for _, p in logs_a]
        assert kinds == ["step", "step", "val", "val_ema", "epoch"] * 2
        ve = [(s, p) for s, p in logs_a if "val/loss_ema" in p]
        assert [s for s, _ in ve] == [2, 4] and [p["val/epoch"] for _, p in ve] == [0, 1]
        assert all(set(p) == {"val/loss_ema", "val/epoch"} and isinstance(p["val/loss_ema"], float) for _, p in ve)
        # val/loss keeps its meaning: the first epoch's is that of a run without the EMA
        _, _, logs_off = _run(tiny, case, tmp_path / "off", 1, val=True)
        assert not any("val/loss_ema" in p or "train/ema_decay" in p for _, p in logs_off)
        off = [p["val/loss"] for _, p in logs_off if "val/loss" in p]
        on = [p["val/loss"] for _, p in logs_a if "val/loss" in p]
        assert len(off) == 1 and off[0] == on[0]
        # the averaged weights are other weights (and a second draw of t and noise)
        assert ve[0][1]["val/loss_ema"] != on[0]
    # the saved shadows are the ones the first epoch ended with
    saved = load_file(str(out_b / "adapter_epoch_1" / "ema_model.safetensors"))
    assert len(saved) == len(pa) and all(v.dtype == torch.float32 for v in saved.values())
    assert sorted(os.listdir(out_b)) == ["adapter_epoch_1", "best_model_epoch_1.safetensors",
                                         "best_model_epoch_2.safetensors"]
    if val:  # the per-epoch merged checkpoint stays the raw weights': it is the file of the run without the EMA
        _same(load_file(str(out_b / "best_model_epoch_1.safetensors")),
              load_file(str(tmp_path / "off" / "best_model_epoch_1.safetensors")))


def test_resume_refuses_another_schedule_and_a_directory_without_shadows(tiny, tmp_path_factory, tmp_path):
    import shutil
    first = _first_epoch(tiny, tmp_path_factory, "attn2")[0]
    out = tmp_path / "b"
    shutil.copytree(first, out)
    with pytest.raises(ValueError, match="decay"):
        _run(tiny, "attn2", out, 2, {"ema_decay": 0.9999}, resume="auto")
    os.remove(out / "adapter_epoch_1" / "ema_model.safetensors")
    with pytest.raises(ValueError, match="no EMA weights"):
        _run(tiny, "attn2", out, 2, EMA, resume="auto")
    # with the EMA off the file is not looked for
    _, opt, logs = _run(tiny, "attn2", out, 2, resume="auto")
    assert opt.ema is None and all("ema" not in st for st in opt.state.values())
    assert [s for s, p in logs if "train/loss" in p] == [3, 4]


def _sample(tiny, model, batch, t, noise):
    tok, coords = O.patchify(batch["latents"].bfloat16())
    x = O.add_noise(tok, noise, t).bfloat16()
    model.eval()
    with torch.no_grad():
        return model(hidden_states=x, indices_grid=coords.to(DEV),
                     ref_image_hidden_states=batch["ref_image_latents"].bfloat16(),
                     pose_hidden_states=batch["pose_latents"].bfloat16(),
                     encoder_hidden_states=tiny["prompt"].bfloat16().expand(2, -1, -1), timestep=t,
                     encoder_attention_mask=tiny["mask"].expand(2, -1)).sample.clone()


@pytest.mark.parametrize("case", ["attn2", "dora"])
def test_forward_under_ema_weights_is_the_model_loaded_with_weights_ema(tiny, tmp_path_factory, case):
    """The trained model's caches (splits, pieces, packs, DoRA's W_eff) are warm with the live weights;
    inside ema_weights() they must be rebuilt from the shadows, and again from the live weights after."""
    from ltx_amd import io
    out, model, opt, _ = _first_epoch(tiny, tmp_path_factory, case)
    ckpt = str(out / "adapter_epoch_1")
    batch, t, noise = _fixed_inputs(tiny)
    raw = _sample(tiny, model, batch, t, noise)
    live = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    with opt.ema_weights():
        inside = _sample(tiny, model, batch, t, noise)
        for n, s in _shadows(model, opt).items():
            assert torch.equal(dict(model.named_parameters())[n], s.to(live[n].dtype)), n
    after = _sample(tiny, model, batch, t, noise)
    _same({n: p.detach() for n, p in model.named_parameters() if p.requires_grad}, live)
    fresh = _build(tiny, CASES[case][0])
    io.load_adapter_checkpoint(fresh, ckpt, weights="ema")
    want = _sample(tiny, fresh, batch, t, noise)
    assert torch.equal(inside, want) and not torch.equal(inside, raw)
    assert torch.equal(after, raw)
    fresh_raw = _build(tiny, CASES[case][0])
    io.load_adapter_checkpoint(fresh_raw, ckpt)
    assert torch.equal(_sample(tiny, fresh_raw, batch, t, noise), raw)


def test_off_is_off(tiny, tmp_path):
    """No EMA key set: one train_loop epoch with save_adapters calls none of the new entry points, and
    the adapter directory holds exactly the four known files."""
    names = []
    _, opt, logs = _run(tiny, "attn2", tmp_path / "out", 1, save=True, record=names)
    assert "ltx_adamw_multi" in names and not NEW_ENTRY_POINTS & set(names)
    assert opt.ema is None and opt.ema_steps == 0 and all("ema" not in st for st in opt.state.values())
    assert sorted(os.listdir(tmp_path / "out" / "adapter_epoch_1")) == FOUR
    with open(tmp_path / "out" / "adapter_epoch_1" / "train_state.json") as f:
        assert "ema" not in json.load(f)
    assert not any("train/ema_decay" in p for _, p in logs)
    # ... and with the key the step is the fused one
    names_on = []
    _run(tiny, "attn2", tmp_path / "on", 1, EMA, record=names_on)
    assert names_on.count("ltx_adamw_multi_ema") == 4 and "ltx_adamw_multi" not in names_on  # 2 steps x 2 dtypes
