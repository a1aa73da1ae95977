"""The non-finite guard of the LoRA optimizer step (FusedAdamW / FusedProdigy(skip_nonfinite=True)), host
side: the config keys (training.guard_from_config, the YAML route), the constructor's keys and refusals,
the "guard" block and the param-group key through the train_state.json writer and reader, the mismatch
refusals (each before anything is written), and the library's new entry points. Models are the tiny config
on the CPU (parameters only). No GPU, no kernel launches."""
import json
import os
import re
import types

import pytest
import torch

from test_adapter_ckpt_cpu import CASES, _model, _moments, _same, _trainable

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ltx_grad_guard_record", "ltx_adamw_multi_guard", "ltx_adamw_multi_sr_guard",
                "ltx_prodigy_moments_multi_guard", "ltx_prodigy_d_update_guard")


def _config(**extra):
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="base.safetensors", lora_rank=8, lora_alpha=8)
    tc.train_mode = "lora_audio"
    for k, v in extra.items():
        setattr(tc, k, v)
    return tc


# ---------------------------------------------------------------------------------------------
# the config keys
# ---------------------------------------------------------------------------------------------
def test_guard_from_config_accepts_and_refuses():
    from ltx_amd.training import guard_from_config
    assert guard_from_config(_config()) == (False, None)  # the key absent: off
    assert guard_from_config(_config(skip_nonfinite=False)) == (False, None)
    assert guard_from_config(_config(skip_nonfinite=True)) == (True, None)
    assert guard_from_config(_config(skip_nonfinite=True, max_consecutive_skips=0)) == (True, None)  # 0: unlimited
    assert guard_from_config(_config(skip_nonfinite=True, max_consecutive_skips=3)) == (True, 3)
    for extra, match in (({"max_consecutive_skips": 3}, "without skip_nonfinite"),
                         ({"skip_nonfinite": False, "max_consecutive_skips": 3}, "without skip_nonfinite"),
                         ({"skip_nonfinite": True, "max_consecutive_skips": -1}, ">= 0"),
                         ({"skip_nonfinite": True, "max_consecutive_skips": 1.5}, ">= 0"),
                         ({"skip_nonfinite": True, "max_consecutive_skips": True}, ">= 0"),
                         ({"skip_nonfinite": "yes"}, "bool"),
                         ({"skip_nonfinite": 1}, "bool")):
        with pytest.raises(ValueError, match=match):
            guard_from_config(_config(**extra))
    for extra in ({"train_mode": "full"}, {"use_deepspeed": True}):
        with pytest.raises(NotImplementedError, match="lora_audio"):
            guard_from_config(_config(skip_nonfinite=True, **extra))
        assert guard_from_config(_config(**extra)) == (False, None)  # off: nothing to refuse


def test_yaml_and_setattr_routes_agree(tmp_path):
    from dataclasses import asdict, fields
    from ltx_amd.config import TrainConfig, load_train_config_from_yaml
    from ltx_amd.training import guard_from_config
    base = "checkpoint_path: x.safetensors\ntrain:\n  lora_rank: 8\n"
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(base + "  skip_nonfinite: true\n  max_consecutive_skips: 4\n")
    (tmp_path / "c.yaml").write_text(base + "  skip_nonfinite: false\n")
    (tmp_path / "d.yaml").write_text(base + "  skip_nonfinite: true\n  max_consecutive_skips: -2\n")
    a, b, c, d = (load_train_config_from_yaml(str(tmp_path / f"{n}.yaml")) for n in "abcd")
    assert not hasattr(a, "skip_nonfinite") and not hasattr(a, "max_consecutive_skips")
    assert b.skip_nonfinite is True and b.max_consecutive_skips == 4
    assert c.skip_nonfinite is False and not hasattr(c, "max_consecutive_skips")
    assert asdict(a) == asdict(b) == asdict(c)
    assert not {"skip_nonfinite", "max_consecutive_skips"} & {f.name for f in fields(TrainConfig)}
    for cfg in (a, b, c, d):
        cfg.train_mode = "lora_audio"
    assert guard_from_config(a) == guard_from_config(_config()) == (False, None)
    assert guard_from_config(b) == guard_from_config(_config(skip_nonfinite=True, max_consecutive_skips=4)) == (True, 4)
    assert guard_from_config(c) == (False, None)
    with pytest.raises(ValueError, match=">= 0"):
        guard_from_config(d)
    gold = load_train_config_from_yaml(os.path.join(REPO, "tests", "golden", "train-avatars.yaml"))
    assert not hasattr(gold, "skip_nonfinite")


def test_train_loop_validates_the_keys_before_anything_is_built(tmp_path):
    from ltx_amd.training import train_loop
    for extra, exc in (({"max_consecutive_skips": 2}, ValueError),
                       ({"skip_nonfinite": True, "max_consecutive_skips": -1}, ValueError),
                       ({"skip_nonfinite": True, "train_mode": "full"}, NotImplementedError)):
        tc = _config(num_epochs=1, learning_rate=1e-3, output_dir=str(tmp_path), **extra)
        with pytest.raises(exc):
            train_loop(None, tc, [], torch.zeros(1, 4, 4096), torch.ones(1, 4, dtype=torch.long), device="cpu")
    assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------------------------------------
# the optimizers' keys
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adamw", "prodigy"])
def test_the_key_enters_param_groups_only_when_on(kind):
    from ltx_amd.training import FusedAdamW, FusedProdigy, OptimizerSpec
    cls = FusedAdamW if kind == "adamw" else FusedProdigy
    p = [torch.nn.Parameter(torch.zeros(4))]
    off, off2, on = cls(p), cls(p, skip_nonfinite=False), cls(p, skip_nonfinite=True)
    assert "skip_nonfinite" not in off.param_groups[0] and "skip_nonfinite" not in off.defaults
    assert sorted(off.param_groups[0]) == sorted(off2.param_groups[0])
    assert on.param_groups[0]["skip_nonfinite"] is True
    assert sorted(set(on.param_groups[0]) - set(off.param_groups[0])) == ["skip_nonfinite"]
    assert (off._skip_nonfinite(), on._skip_nonfinite()) == (False, True)
    # nothing has stepped: nothing to settle, nothing skipped
    assert on.step_applied is None and on.skipped_steps == 0 and not on.outcome_pending
    on.settle()
    spec = OptimizerSpec(kind, 1e-3 if kind == "adamw" else 1.0, {})
    assert "skip_nonfinite" not in spec.build(p).param_groups[0]
    assert spec.build(p, skip_nonfinite=True).param_groups[0]["skip_nonfinite"] is True


def test_groups_that_disagree_and_cpu_parameters_are_refused():
    from ltx_amd import _lib
    from ltx_amd.training import FusedAdamW
    a, b = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdamW([{"params": [a]}, {"params": [b], "skip_nonfinite": False}], skip_nonfinite=True)
    a.grad, b.grad = torch.ones(4), torch.ones(4)
    with pytest.raises(ValueError, match="skip_nonfinite differs"):
        opt.step()
    # the guard always takes the table path: a CPU parameter is an error, as under the clip
    opt = FusedAdamW([a], skip_nonfinite=True)
    with pytest.raises(_lib.LtxHipError, match="skip_nonfinite"):
        opt.step()
    assert not opt.state.get(a) and torch.equal(a.detach(), torch.zeros(4))


# ---------------------------------------------------------------------------------------------
# train_state.json
# ---------------------------------------------------------------------------------------------
def _optimizer(model, seed=None, **kw):
    from ltx_amd.training import FusedAdamW
    opt = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=3e-4, **kw)
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        for p in opt.param_groups[0]["params"]:
            opt.state[p] = {"step": 7, "exp_avg": torch.randn(p.shape, generator=g).to(p.dtype),
                            "exp_avg_sq": torch.rand(p.shape, generator=g).to(p.dtype)}
    return opt


def _save(model, opt, path):
    from ltx_amd import io
    torch.manual_seed(1234)
    return io.save_adapter_checkpoint(model, str(path), optimizer=opt,
                                      train_state={"epoch": 3, "global_step": 6, "best_loss": 0.5},
                                      loader=types.SimpleNamespace(seed=5))


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """(guarded directory with 3 skipped steps, unguarded directory), written once from one model and moments."""
    m = _model(CASES["attn2"], seed=1)
    on = _optimizer(m, seed=2, skip_nonfinite=True)
    on.restore_skipped_steps(3, "cpu")
    off = _optimizer(m, seed=2)
    root = tmp_path_factory.mktemp("guard")
    return _save(m, on, root / "on" / "adapter_epoch_3"), _save(m, off, root / "off" / "adapter_epoch_3"), m, on


def test_guard_block_and_group_key_round_trip(saved):
    from ltx_amd import io
    on_dir, off_dir, m, opt = saved
    with open(os.path.join(on_dir, "train_state.json")) as f:
        st_on = json.load(f)
    with open(os.path.join(off_dir, "train_state.json")) as f:
        st_off = json.load(f)
    assert st_on["format_version"] == st_off["format_version"] == 1
    assert st_on["guard"] == {"skipped_steps": 3}
    assert st_on["optimizer"]["param_groups"][0]["skip_nonfinite"] is True
    # a directory written without the guard carries no trace of it: today's file
    assert "guard" not in st_off and "skip_nonfinite" not in st_off["optimizer"]["param_groups"][0]
    del st_on["guard"], st_on["optimizer"]["param_groups"][0]["skip_nonfinite"]
    assert st_on == st_off
    assert sorted(os.listdir(on_dir)) == sorted(os.listdir(off_dir))
    m2 = _model(CASES["attn2"], seed=3)
    opt2 = _optimizer(m2, skip_nonfinite=True)
    state = io.load_adapter_checkpoint(m2, on_dir, optimizer=opt2)
    assert state["guard"] == {"skipped_steps": 3} and state["global_step"] == 6
    assert opt2.skipped_steps == 3 and opt2.consecutive_skips == 0 and not opt2.outcome_pending
    # the device record the next step carries the count on from
    assert opt2._guard_rec.dtype == torch.float64 and opt2._guard_rec.numel() == 4
    assert opt2._guard_rec[3:].view(torch.int64).tolist() == [3] and opt2._guard_rec[:3].tolist() == [0.0, 0.0, 0.0]
    assert opt2.param_groups[0]["skip_nonfinite"] is True
    _same(_trainable(m2), _trainable(m))
    (ma, sa), (mb, sb) = _moments(m, opt), _moments(m2, opt2)
    _same(ma, mb)
    assert sa == sb and set(sa.values()) == {7}
    # saving again reproduces the file
    again = _save(m2, opt2, os.path.join(os.path.dirname(os.path.dirname(on_dir)), "again", "adapter_epoch_3"))
    with open(os.path.join(again, "train_state.json")) as fa, open(os.path.join(on_dir, "train_state.json")) as fb:
        assert fa.read() == fb.read()


def test_a_guard_mismatch_raises_before_anything_is_written(saved):
    from ltx_amd import io
    on_dir, off_dir, _, _ = saved
    for path, kw, match in ((on_dir, {}, "saved with skip_nonfinite"), (off_dir, {"skip_nonfinite": True}, "saved without")):
        m = _model(CASES["attn2"], seed=3)
        opt = _optimizer(m, seed=8, **kw)
        before, (mom, steps) = _trainable(m), _moments(m, opt)
        groups = [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups]
        rng = torch.get_rng_state()
        with pytest.raises(ValueError, match=match):
            io.load_adapter_checkpoint(m, path, optimizer=opt)
        _same(_trainable(m), before)
        _same(_moments(m, opt)[0], mom)
        assert _moments(m, opt)[1] == steps
        assert [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups] == groups
        assert torch.equal(torch.get_rng_state(), rng) and opt.skipped_steps == 0
    # without an optimizer the adapters of either directory load
    io.load_adapter_checkpoint(_model(CASES["attn2"], seed=3), on_dir)


def test_a_guarded_directory_without_its_count_is_refused(saved, tmp_path):
    import shutil
    from ltx_amd import io
    dst = tmp_path / "cut"
    shutil.copytree(saved[0], dst)
    with open(dst / "train_state.json") as f:
        st = json.load(f)
    del st["guard"]
    (dst / "train_state.json").write_text(json.dumps(st))
    m = _model(CASES["attn2"], seed=3)
    with pytest.raises(ValueError, match="skipped_steps"):
        io.load_adapter_checkpoint(m, str(dst), optimizer=_optimizer(m, skip_nonfinite=True))


# ---------------------------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------------------------
def test_library_exports_the_guard_entry_points():
    from ltx_amd import _lib
    src = open(os.path.join(REPO, "include", "ltx_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ltx_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.M))
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib._SIGNATURES and hasattr(lib, name), name
    assert lib.ltx_abi_version() == 1
    # the guarded forms take the unguarded ones' arguments and the guard record in front of the stream
    for guarded, plain in (("ltx_adamw_multi_sr_guard", "ltx_adamw_multi_sr"),
                           ("ltx_prodigy_moments_multi_guard", "ltx_prodigy_moments_multi"),
                           ("ltx_prodigy_d_update_guard", "ltx_prodigy_d_update")):
        sig = _lib._SIGNATURES[plain]
        assert _lib._SIGNATURES[guarded] == sig[:-1] + [_lib._p] + sig[-1:], guarded
