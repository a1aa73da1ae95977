"""The exponential moving average of the trained weights (FusedAdamW(ema=EMASchedule)), host side:
EMASchedule.decay_at against hand-computed values of diffusers' EMAModel.get_decay (diffusers is not
installed where the tests run; the formula is pinned to its published behaviour), the errors, the config
keys (setattr and YAML, read only when present), and the adapter directory's optional
ema_model.safetensors / "ema" block with the loads that read them and tools/merge_adapter.py --ema.
Models are the tiny config on the CPU (parameters only); shadows are set by hand, since the fused step
itself needs the GPU (tests/test_ema_gpu.py). No GPU, no kernel launches."""
import importlib.util
import json
import os
import types

import pytest
import torch
from safetensors.torch import load_file

from test_adapter_ckpt_cpu import CASES, PRE, _bare, _model, _same, _trainable

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMA_KEYS = ("ema_decay", "ema_warmup", "ema_inv_gamma", "ema_power", "ema_update_after_step", "ema_min_decay")
FOUR = ["adapter_config.json", "adapter_model.safetensors", "optimizer.safetensors", "train_state.json"]


# ---------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------
def test_decay_at_hand_computed_values():
    from ltx_amd.training import EMASchedule
    s = EMASchedule(0.999)
    assert s.decay_at(1) == 0.0  # k = 0: the shadow follows the weights
    assert s.decay_at(2) == 2 / 11
    assert s.decay_at(3) == 0.25
    # k = 8990: (1 + k) / (10 + k) = 8991 / 9000, which is 0.999 up to the rounding of the division
    assert s.decay_at(8991) == pytest.approx(0.999, rel=0, abs=2 ** -52) and s.decay_at(8991) <= 0.999
    assert s.decay_at(8992) == 0.999 and s.decay_at(10 ** 7) == 0.999  # capped exactly
    assert all(isinstance(s.decay_at(n), float) for n in (1, 2, 8992))
    assert s.decay_at(0) == 0.0


def test_decay_at_warmup_delay_and_floor():
    from ltx_amd.training import EMASchedule
    w = EMASchedule(0.999, use_warmup=True, inv_gamma=1.0, power=2 / 3)
    assert w.decay_at(1) == 0.0
    assert w.decay_at(2) == 1 - 2 ** (-2 / 3)
    assert w.decay_at(4) == 1 - (1 + 3 / 1.0) ** -(2 / 3)
    assert EMASchedule(0.999, use_warmup=True, inv_gamma=2.0, power=0.75).decay_at(5) == 1 - (1 + 4 / 2.0) ** -0.75
    assert w.decay_at(10 ** 9) == 0.999
    d = EMASchedule(0.999, update_after_step=5)
    assert [d.decay_at(n) for n in range(1, 7)] == [0.0] * 6
    assert d.decay_at(7) == 2 / 11 and d.decay_at(8) == 0.25
    f = EMASchedule(0.999, min_decay=0.5)
    assert f.decay_at(1) == 0.0  # the first step copies, as diffusers' (the floor applies after k > 0)
    assert f.decay_at(2) == 0.5 and f.decay_at(3) == 0.5 and f.decay_at(11) == 11 / 20 and f.decay_at(10 ** 6) == 0.999
    # a pure function of n: nothing is stored between calls
    assert [f.decay_at(n) for n in (11, 2, 11)] == [11 / 20, 0.5, 11 / 20]
    assert EMASchedule(1.0).decay_at(10 ** 6) == (10 ** 6) / (10 ** 6 + 9)


def test_schedule_errors():
    from ltx_amd.training import EMASchedule
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            EMASchedule(bad)
    with pytest.raises(ValueError, match="ema_update_after_step"):
        EMASchedule(0.999, update_after_step=-1)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="ema_inv_gamma"):
            EMASchedule(0.999, inv_gamma=bad)
    for bad in (-0.1, 0.9995):
        with pytest.raises(ValueError, match="ema_min_decay"):
            EMASchedule(0.999, min_decay=bad)
    EMASchedule(1.0, min_decay=1.0)
    s = EMASchedule(0.999)
    assert s.fields() == {"decay": 0.999, "use_warmup": False, "inv_gamma": 1.0, "power": 2 / 3,
                          "update_after_step": 0, "min_decay": 0.0}


# ---------------------------------------------------------------------------------------------
# config keys
# ---------------------------------------------------------------------------------------------
def _tc(mode="lora_audio", **kw):
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="-", learning_rate=1e-3, num_epochs=1)
    tc.train_mode = mode
    for k, v in kw.items():
        setattr(tc, k, v)
    return tc


def test_config_keys_are_read_only_when_present():
    from dataclasses import fields
    from ltx_amd.config import TrainConfig
    from ltx_amd.training import EMASchedule, ema_from_config
    bare = _tc()
    assert not any(hasattr(bare, k) for k in EMA_KEYS)
    assert not set(EMA_KEYS) & {f.name for f in fields(TrainConfig)}
    assert ema_from_config(bare) is None
    assert ema_from_config(_tc(ema_decay=0)) is None and ema_from_config(_tc(ema_decay=0.0)) is None
    assert ema_from_config(_tc("full")) is None  # off is off in every mode
    assert ema_from_config(_tc(ema_warmup=True, ema_power=0.5)) is None  # without ema_decay nothing is on
    s = ema_from_config(_tc(ema_decay=0.9999))
    assert isinstance(s, EMASchedule) and s.fields() == EMASchedule(0.9999).fields()
    s = ema_from_config(_tc(ema_decay=0.995, ema_warmup=True, ema_inv_gamma=2.0, ema_power=0.75,
                            ema_update_after_step=10, ema_min_decay=0.1))
    assert s.fields() == {"decay": 0.995, "use_warmup": True, "inv_gamma": 2.0, "power": 0.75,
                          "update_after_step": 10, "min_decay": 0.1}


def test_config_errors():
    from ltx_amd.training import ema_from_config
    with pytest.raises(NotImplementedError, match="lora_audio"):
        ema_from_config(_tc("full", ema_decay=0.999))
    for kw, match in (({"ema_decay": 1.5}, "ema_decay"), ({"ema_decay": -0.5}, "ema_decay"),
                      ({"ema_decay": 0.999, "ema_inv_gamma": 0.0}, "ema_inv_gamma"),
                      ({"ema_decay": 0.999, "ema_update_after_step": -3}, "ema_update_after_step"),
                      ({"ema_decay": 0.999, "ema_min_decay": 0.9999}, "ema_min_decay")):
        with pytest.raises(ValueError, match=match):
            ema_from_config(_tc(**kw))


def test_train_loop_raises_before_touching_the_model(monkeypatch):
    """train_loop reads the keys before it builds the optimizer: a bad one raises with an empty loader,
    a model it never looks into, and no FusedAdamW constructed."""
    from ltx_amd import training

    class Model(torch.nn.Module):
        patchifier = None
        device = "cpu"

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(3))

        def parameters(self, recurse=True):
            raise AssertionError("the model was looked into")

    def no_optimizer(*a, **k):
        raise AssertionError("an optimizer was built")
    monkeypatch.setattr(training, "FusedAdamW", no_optimizer)
    args = ([], torch.zeros(1, 4, 8), torch.ones(1, 4, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="lora_audio"):
        training.train_loop(Model(), _tc("full", ema_decay=0.999), *args, device="cpu")
    for kw, match in (({"ema_decay": 2.0}, "ema_decay"), ({"ema_decay": 0.99, "ema_min_decay": 0.995}, "ema_min_decay"),
                      ({"ema_decay": 0.99, "ema_inv_gamma": -1.0}, "ema_inv_gamma"),
                      ({"ema_decay": 0.99, "ema_update_after_step": -1}, "ema_update_after_step")):
        with pytest.raises(ValueError, match=match):
            training.train_loop(Model(), _tc(**kw), *args, device="cpu")


def test_train_loop_builds_the_optimizer_with_the_schedule_or_none(monkeypatch):
    """Absent keys (and ema_decay = 0) build FusedAdamW with ema=None; ema_decay builds it with the
    EMASchedule of the keys. The loader is empty, so no step runs."""
    from ltx_amd import training
    seen = []

    class Recording(training.FusedAdamW):
        def __init__(self, *a, **k):
            seen.append(k.get("ema"))
            super().__init__(*a, **k)
    monkeypatch.setattr(training, "FusedAdamW", Recording)
    m = _model(CASES["attn2"], seed=1)
    args = ([], torch.zeros(1, 4, 4096), torch.ones(1, 4, dtype=torch.long))
    for kw in ({}, {"ema_decay": 0}, {"ema_decay": 0.999, "ema_warmup": True, "ema_update_after_step": 2}):
        training.train_loop(m, _tc(**kw), *args, device="cpu")
    assert seen[0] is None and seen[1] is None
    assert seen[2].fields() == training.EMASchedule(0.999, use_warmup=True, update_after_step=2).fields()


def test_yaml_sets_the_keys_only_when_present(tmp_path):
    from dataclasses import asdict
    from ltx_amd.config import load_train_config_from_yaml
    from ltx_amd.training import ema_from_config
    base = "checkpoint_path: x.safetensors\ntrain:\n  lora_rank: 16\n"
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(base + "  ema_decay: 0.9999\n  ema_warmup: true\n  ema_inv_gamma: 2\n"
                                            "  ema_power: 0.75\n  ema_update_after_step: 100\n  ema_min_decay: 0.5\n")
    (tmp_path / "c.yaml").write_text(base + "  ema_decay: 0.999\n")
    a, b, c = (load_train_config_from_yaml(str(tmp_path / f"{n}.yaml")) for n in "abc")
    assert not any(hasattr(a, k) for k in EMA_KEYS)
    assert [getattr(b, k) for k in EMA_KEYS] == [0.9999, True, 2.0, 0.75, 100, 0.5]
    assert isinstance(b.ema_inv_gamma, float) and isinstance(b.ema_update_after_step, int) and b.ema_warmup is True
    assert c.ema_decay == 0.999 and not any(hasattr(c, k) for k in EMA_KEYS[1:])
    assert asdict(a) == asdict(b) == asdict(c)
    for cfg in (a, b, c):
        cfg.train_mode = "lora_audio"
    assert ema_from_config(a) is None
    assert ema_from_config(b).fields() == {"decay": 0.9999, "use_warmup": True, "inv_gamma": 2.0, "power": 0.75,
                                           "update_after_step": 100, "min_decay": 0.5}
    gold = load_train_config_from_yaml(os.path.join(REPO, "tests", "golden", "train-avatars.yaml"))
    assert not any(hasattr(gold, k) for k in EMA_KEYS)


# ---------------------------------------------------------------------------------------------
# the optimizer's host side
# ---------------------------------------------------------------------------------------------
def test_fused_adamw_ema_argument_and_cpu_refusals():
    from ltx_amd import _lib
    from ltx_amd.training import EMASchedule, FusedAdamW
    p = torch.nn.Parameter(torch.zeros(4))
    off = FusedAdamW([p], lr=1e-3)
    assert off.ema is None and off.ema_steps == 0 and off.ema_decay is None
    with pytest.raises(TypeError, match="EMASchedule"):
        FusedAdamW([p], lr=1e-3, ema=0.999)
    with pytest.raises(RuntimeError, match="ema=None"):
        off.ema_swap_in()
    opt = FusedAdamW([p], lr=1e-3, ema=EMASchedule(0.999))
    assert "ema" not in opt.param_groups[0]  # the schedule is not a hyper-parameter of the groups
    p.grad = torch.ones(4)
    with pytest.raises(_lib.LtxHipError):
        opt.step()  # every parameter goes through the table kernels, which need the device
    assert not opt.state[p] and opt.ema_steps == 0  # raised before any state was created
    with pytest.raises(RuntimeError, match="not swapped in"):
        opt.ema_swap_out()
    h = torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))
    h.grad = torch.ones(4, dtype=torch.float16)
    with pytest.raises((TypeError, _lib.LtxHipError)):
        FusedAdamW([h], lr=1e-3, ema=EMASchedule(0.999)).step()


# ---------------------------------------------------------------------------------------------
# adapter directories
# ---------------------------------------------------------------------------------------------
def _ema_optimizer(model, schedule, seed=None, steps=7):
    """FusedAdamW(ema=schedule) over the trainable set; with a seed, moments, steps and shadows as after
    `steps` steps (the shadows are random f32 values that no bf16 holds exactly)."""
    from ltx_amd.training import FusedAdamW
    opt = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, ema=schedule)
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        for p in opt.param_groups[0]["params"]:
            opt.state[p] = {"step": steps, "exp_avg": torch.randn(p.shape, generator=g).to(p.dtype),
                            "exp_avg_sq": torch.rand(p.shape, generator=g).to(p.dtype),
                            "ema": 0.05 * torch.randn(p.shape, generator=g) + (1.0 if p.dim() == 1 else 0.0)}
        opt.ema_steps = steps
        opt.ema_decay = schedule.decay_at(steps)
    return opt


def _shadows(model, opt):
    names = {id(p): n for n, p in model.named_parameters()}
    return {names[id(p)]: st["ema"].detach().clone() for p, st in opt.state.items() if "ema" in st}


def _save(model, opt, path):
    from ltx_amd import io
    return io.save_adapter_checkpoint(model, str(path), optimizer=opt,
                                      train_state={"epoch": 3, "global_step": 7, "best_loss": 0.5},
                                      loader=types.SimpleNamespace(seed=5))


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """Per case one directory written with an EMA and, for attn2, one without: written once, left unchanged."""
    from ltx_amd.training import EMASchedule
    out = {}
    for case, extra in CASES.items():
        m = _model(extra, seed=1)
        opt = _ema_optimizer(m, EMASchedule(0.999, update_after_step=2), seed=2)
        out[case] = (_save(m, opt, tmp_path_factory.mktemp(case) / "adapter_epoch_3"), m, opt)
    m = _model(CASES["attn2"], seed=1)
    out["off"] = (_save(m, _ema_optimizer(m, None, seed=None), tmp_path_factory.mktemp("off") / "adapter_epoch_3"), m, None)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_ema_file_key_names_dtype_and_block(saved, case):
    from ltx_amd.io import ADAPTER_FORMAT_VERSION, adapter_key
    path, m, opt = saved[case]
    assert sorted(os.listdir(path)) == sorted(FOUR + ["ema_model.safetensors"])
    ema, raw = load_file(os.path.join(path, "ema_model.safetensors")), load_file(os.path.join(path, "adapter_model.safetensors"))
    assert sorted(ema) == sorted(raw) and all(k.startswith(PRE) and ".default" not in k for k in ema)
    assert PRE + "transformer_blocks.0.attn2.to_q.lora_A.weight" in ema and PRE + "caption_projection.linear_1.weight" in ema
    assert all(v.dtype == torch.float32 for v in ema.values())
    assert raw[PRE + "caption_projection.linear_1.weight"].dtype == torch.bfloat16  # the f32 shadow of a bf16 tensor
    for name, s in _shadows(m, opt).items():
        assert torch.equal(ema[adapter_key(name)], s), name
    with open(os.path.join(path, "train_state.json")) as f:
        st = json.load(f)
    assert st["ema"] == {"decay": 0.999, "use_warmup": False, "inv_gamma": 1.0, "power": 2 / 3,
                         "update_after_step": 2, "min_decay": 0.0, "ema_steps": 7}
    assert st["format_version"] == ADAPTER_FORMAT_VERSION == 1
    assert "ema" not in st["optimizer"]["param_groups"][0]


def test_without_ema_the_directory_is_todays(saved):
    path = saved["off"][0]
    assert sorted(os.listdir(path)) == FOUR
    with open(os.path.join(path, "train_state.json")) as f:
        assert "ema" not in json.load(f)
    # ... and with an optimizer that has stepped, the same four files
    from ltx_amd import io
    from test_adapter_ckpt_cpu import _optimizer
    m = saved["off"][1]
    p2 = io.save_adapter_checkpoint(m, os.path.join(os.path.dirname(path), "adapter_epoch_4"), optimizer=_optimizer(m, seed=2))
    assert sorted(os.listdir(p2)) == FOUR
    with open(os.path.join(p2, "train_state.json")) as f:
        assert "ema" not in json.load(f)


def test_an_unstepped_parameter_is_saved_as_its_own_value(tmp_path):
    """A parameter the optimizer has not stepped has no shadow yet; its shadow will start from its value,
    and that is what the file holds, so the file always names every trainable tensor."""
    from ltx_amd.training import EMASchedule
    m = _model(CASES["attn2"], seed=1)
    opt = _ema_optimizer(m, EMASchedule(0.999))
    from ltx_amd.io import adapter_key
    ema = load_file(os.path.join(_save(m, opt, tmp_path / "a"), "ema_model.safetensors"))
    _same(ema, {adapter_key(n): p.float() for n, p in _trainable(m).items()})
    with open(tmp_path / "a" / "train_state.json") as f:
        assert json.load(f)["ema"]["ema_steps"] == 0


@pytest.mark.parametrize("case", list(CASES))
def test_weights_ema_gives_each_parameter_its_shadow_cast_to_its_dtype(saved, case):
    from ltx_amd import io, ops
    path, m, opt = saved[case]
    shadows = _shadows(m, opt)
    for target in (_model(CASES[case], seed=9), _bare()):
        gen = ops.weight_generation()
        st = io.load_adapter_checkpoint(target, path, weights="ema")
        assert st["epoch"] == 3 and ops.weight_generation() > gen
        got = _trainable(target)
        assert sorted(got) == sorted(shadows)
        for n, p in got.items():
            assert p.dtype == _trainable(m)[n].dtype and torch.equal(p, shadows[n].to(p.dtype)), n
        cp = got["caption_projection.linear_1.weight"]
        assert cp.dtype == torch.bfloat16 and not torch.equal(cp.float(), shadows["caption_projection.linear_1.weight"])
        assert not torch.equal(cp, _trainable(m)["caption_projection.linear_1.weight"])
    raw = _model(CASES[case], seed=9)
    io.load_adapter_checkpoint(raw, path)  # the default is the raw weights
    _same(_trainable(raw), _trainable(m))


def test_weights_ema_refusals(saved):
    from ltx_amd import io
    from test_adapter_ckpt_cpu import _refused
    _refused(_model(CASES["attn2"], seed=3), saved["off"][0], "no EMA weights", weights="ema")
    _refused(_model(CASES["attn2"], seed=3), saved["attn2"][0], "weights must be", weights="shadow")
    m = _model(CASES["attn2"], seed=3)
    _refused(m, saved["attn2"][0], "optimizer", weights="ema", optimizer=_ema_optimizer(m, None))
    _refused(_model(CASES["attn2"], seed=3), saved["dora"][0], "use_dora", weights="ema")


def test_resume_restores_shadows_and_ema_steps(saved):
    from ltx_amd import io
    from ltx_amd.training import EMASchedule
    path, m, opt = saved["all_dropout"]
    sched = EMASchedule(0.999, update_after_step=2)
    # into an optimizer that has not stepped (state is created) and into one that has (in place)
    for seed in (None, 4):
        m2 = _model(CASES["all_dropout"], seed=9)
        opt2 = _ema_optimizer(m2, sched, seed=seed, steps=3)
        ptrs = {id(p): st["ema"].data_ptr() for p, st in opt2.state.items()}
        io.load_adapter_checkpoint(m2, path, optimizer=opt2)
        _same(_shadows(m2, opt2), _shadows(m, opt))
        _same(_trainable(m2), _trainable(m))
        assert opt2.ema_steps == 7 and opt2.ema_decay == sched.decay_at(7) == 5 / 14
        assert all(st["ema"].dtype == torch.float32 for st in opt2.state.values())
        if seed is not None:
            assert {id(p): st["ema"].data_ptr() for p, st in opt2.state.items()} == ptrs


def test_directory_without_shadows_strict_and_not(saved):
    from ltx_amd import io
    from ltx_amd.training import EMASchedule
    from test_adapter_ckpt_cpu import _optimizer, _refused
    m = saved["off"][1]
    path = io.save_adapter_checkpoint(m, os.path.join(os.path.dirname(saved["off"][0]), "adapter_epoch_5"),
                                      optimizer=_optimizer(m, seed=2))
    m2 = _model(CASES["attn2"], seed=9)
    opt2 = _ema_optimizer(m2, EMASchedule(0.999), seed=4, steps=3)
    before = _shadows(m2, opt2)
    _refused(m2, path, "no EMA weights", optimizer=opt2)
    _same(_shadows(m2, opt2), before)
    assert opt2.ema_steps == 3
    io.load_adapter_checkpoint(m2, path, optimizer=opt2, strict=False)
    _same(_trainable(m2), _trainable(m))
    got = _shadows(m2, opt2)
    assert sorted(got) == sorted(before)
    for n, s in got.items():  # the shadows start from the loaded weights
        assert s.dtype == torch.float32 and torch.equal(s, _trainable(m)[n].float()), n
    assert opt2.ema_steps == 0 and opt2.ema_decay is None


def test_ema_off_ignores_the_file_and_a_changed_schedule_is_refused(saved):
    from ltx_amd import io
    from ltx_amd.training import EMASchedule
    from test_adapter_ckpt_cpu import _optimizer, _refused
    path, m, opt = saved["attn2"]
    m2 = _model(CASES["attn2"], seed=9)
    off = _optimizer(m2)
    io.load_adapter_checkpoint(m2, path, optimizer=off)
    _same(_trainable(m2), _trainable(m))
    assert all("ema" not in st for st in off.state.values()) and off.ema_steps == 0
    for sched, field in ((EMASchedule(0.9999, update_after_step=2), "decay"), (EMASchedule(0.999), "update_after_step"),
                         (EMASchedule(0.999, use_warmup=True, update_after_step=2), "use_warmup")):
        m3 = _model(CASES["attn2"], seed=9)
        opt3 = _ema_optimizer(m3, sched, seed=4, steps=3)
        before = _shadows(m3, opt3)
        _refused(m3, path, field, optimizer=opt3)  # before anything is written to the model
        _same(_shadows(m3, opt3), before)
        assert opt3.ema_steps == 3


# ---------------------------------------------------------------------------------------------
# tools/merge_adapter.py --ema
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["all_dropout", "dora"])
def test_merge_adapter_ema_is_the_export_of_a_model_given_the_shadows(saved, tmp_path, case):
    from ltx_amd import io
    spec = importlib.util.spec_from_file_location("merge_adapter", os.path.join(REPO, "tools", "merge_adapter.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path, m, opt = saved[case]
    io.save_module_safetensors(_bare(), str(tmp_path / "base.safetensors"))
    by_hand = _model(CASES[case], seed=1)
    shadows = _shadows(m, opt)
    with torch.no_grad():
        for n, p in by_hand.named_parameters():
            if p.requires_grad:
                p.copy_(shadows[n].to(p.dtype))
    io.export_merged_safetensors(by_hand, str(tmp_path / "want.safetensors"))
    io.export_merged_safetensors(m, str(tmp_path / "raw.safetensors"))
    tool.main(["--ema", str(tmp_path / "base.safetensors"), path, str(tmp_path / "ema.safetensors")])
    tool.main([str(tmp_path / "base.safetensors"), path, str(tmp_path / "plain.safetensors")])
    got, want = load_file(str(tmp_path / "ema.safetensors")), load_file(str(tmp_path / "want.safetensors"))
    _same(got, want)
    _same(load_file(str(tmp_path / "plain.safetensors")), load_file(str(tmp_path / "raw.safetensors")))
    name = "transformer_blocks.0.attn2.to_q.weight"
    assert not torch.equal(got[name], load_file(str(tmp_path / "raw.safetensors"))[name])
    with pytest.raises(ValueError, match="no EMA weights"):
        tool.main(["--ema", str(tmp_path / "base.safetensors"), saved["off"][0], str(tmp_path / "none.safetensors")])
