"""Adapter checkpoint directories (io.save_adapter_checkpoint / load_adapter_checkpoint), host side:
the round trip of every trainable tensor, moment and step, the peft-shaped key names and
adapter_config.json, loading into a bare model, the refusals (each leaves the model as it was), the
complete-or-absent rule behind resume_from="auto", the YAML keys and tools/merge_adapter.py.
Models are the tiny config on the CPU (parameters only). No GPU, no kernel launches."""
import importlib.util
import json
import os
import types

import pytest
import torch
from safetensors.torch import load_file, save_file

from lora_dora_utils import golden_meta

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE = "base_model.model."
CASES = {"attn2": {}, "all_dropout": {"lora_targets": "attn1+attn2", "lora_ff": True, "lora_dropout": 0.1},
         "dora": {"use_dora": True}}


def _config(extra, r=8, **kw):
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="base.safetensors", lora_rank=r, lora_alpha=2 * r, **kw)
    for k, v in extra.items():
        setattr(tc, k, v)
    return tc


def _bare(seed=0):
    from ltx_amd.transformer3d import Transformer3DModel
    torch.manual_seed(seed)
    return Transformer3DModel.from_config(golden_meta()["config"]).to(torch.bfloat16)


def _model(extra, seed, r=8, base=None):
    """The tiny model with the adapters of `extra`; every trainable tensor drawn from `seed` (B is not
    left at zero), on the base weights of `base` when given."""
    from ltx_amd.lora import apply_training_strategy
    m = _bare()
    if base is not None:
        m.load_state_dict(base.state_dict())
    apply_training_strategy(m, _config(extra, r), "lora_audio")
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.requires_grad:
                p.copy_(0.05 * torch.randn(p.shape, generator=g) + (1.0 if "magnitude" in n else 0.0))
    return m


def _optimizer(model, seed=None, lr=1e-3):
    """FusedAdamW over the trainable set; with a seed, moments and steps as after some steps."""
    from ltx_amd.training import FusedAdamW
    opt = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=lr)
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        for p in opt.param_groups[0]["params"]:
            opt.state[p] = {"step": 7, "exp_avg": torch.randn(p.shape, generator=g).to(p.dtype),
                            "exp_avg_sq": torch.rand(p.shape, generator=g).to(p.dtype)}
    return opt


def _trainable(model):
    return {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def _moments(model, opt):
    names = {id(p): n for n, p in model.named_parameters()}
    out, steps = {}, {}
    for p in opt.param_groups[0]["params"]:
        st = opt.state.get(p)
        if st:
            out["exp_avg." + names[id(p)]] = st["exp_avg"].detach().clone()
            out["exp_avg_sq." + names[id(p)]] = st["exp_avg_sq"].detach().clone()
            steps[names[id(p)]] = st["step"]
    return out, steps


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """One saved checkpoint per case, written once: (directory, model, optimizer, CPU RNG state at save)."""
    from ltx_amd import io
    out = {}
    for name, extra in CASES.items():
        m = _model(extra, seed=1)
        opt = _optimizer(m, seed=2, lr=3e-4)
        torch.manual_seed(1234)
        rng = torch.get_rng_state()
        path = io.save_adapter_checkpoint(m, str(tmp_path_factory.mktemp(name) / "adapter_epoch_3"), optimizer=opt,
                                          train_state={"epoch": 3, "global_step": 6, "best_loss": float("inf")},
                                          loader=types.SimpleNamespace(seed=5),
                                          metadata={"base_model_name_or_path": "base.safetensors"})
        out[name] = (path, m, opt, rng)
    return out


# ---------------------------------------------------------------------------------------------
# round trip
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_round_trip_is_bitwise_and_keeps_dtypes(saved, case):
    from ltx_amd import io, ops
    path, m, opt, rng = saved[case]
    m2 = _model(CASES[case], seed=9)
    opt2 = _optimizer(m2)  # has not stepped: its state must be created
    loader = types.SimpleNamespace(seed=0)
    assert not torch.equal(m2.transformer_blocks[0].attn2.to_q.lora_B["default"].weight,
                           m.transformer_blocks[0].attn2.to_q.lora_B["default"].weight)
    ptrs = {n: p.data_ptr() for n, p in m2.named_parameters()}
    gen = ops.weight_generation()
    torch.manual_seed(99)
    st = io.load_adapter_checkpoint(m2, path, optimizer=opt2, loader=loader)
    assert (st["epoch"], st["global_step"], st["best_loss"], st["world_size"]) == (3, 6, float("inf"), 1)
    _same(_trainable(m2), _trainable(m))
    dt = {p.dtype for n, p in m2.named_parameters() if p.requires_grad and "lora_" in n}
    assert dt == {torch.float32} and m2.caption_projection.linear_1.weight.dtype == torch.bfloat16
    assert {n: p.data_ptr() for n, p in m2.named_parameters()} == ptrs  # copied in place
    assert ops.weight_generation() > gen
    (mom2, steps2), (mom, steps) = _moments(m2, opt2), _moments(m, opt)
    _same(mom2, mom)
    assert steps2 == steps and set(steps.values()) == {7} and len(steps) == len(_trainable(m))
    assert all(type(s) is int for s in steps2.values())
    g2, g = opt2.param_groups[0], opt.param_groups[0]
    assert g2["lr"] == g["lr"] == 3e-4 and g2["betas"] == g["betas"] and isinstance(g2["betas"], tuple)
    assert g2["eps"] == g["eps"] and g2["weight_decay"] == g["weight_decay"]
    assert torch.equal(torch.get_rng_state(), rng) and loader.seed == 5


def test_moments_land_in_place_when_the_optimizer_has_state(saved):
    from ltx_amd import io
    path, m, opt, _ = saved["attn2"]
    m2 = _model(CASES["attn2"], seed=9)
    opt2 = _optimizer(m2, seed=4)
    before = {id(p): (st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()) for p, st in opt2.state.items()}
    io.load_adapter_checkpoint(m2, path, optimizer=opt2)
    assert {id(p): (st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()) for p, st in opt2.state.items()} == before
    _same(_moments(m2, opt2)[0], _moments(m, opt)[0])


# ---------------------------------------------------------------------------------------------
# names, config, files
# ---------------------------------------------------------------------------------------------
def test_literal_key_strings(saved):
    from ltx_amd.io import adapter_key
    keys = {c: set(load_file(os.path.join(saved[c][0], "adapter_model.safetensors"))) for c in CASES}
    b0 = PRE + "transformer_blocks.0."
    for c in CASES:
        assert b0 + "attn2.to_q.lora_A.weight" in keys[c] and b0 + "attn2.to_q.lora_B.weight" in keys[c]
        assert b0 + "attn2.to_out.0.lora_A.weight" in keys[c]
        assert PRE + "caption_projection.linear_1.weight" in keys[c]
        assert PRE + "caption_projection.linear_2.bias" in keys[c]
        assert not any(".default" in k or "base_layer" in k for k in keys[c])
        assert all(k.startswith(PRE) for k in keys[c])
    assert b0 + "attn1.to_k.lora_A.weight" in keys["all_dropout"]
    assert b0 + "ff.net.0.proj.lora_B.weight" in keys["all_dropout"]
    assert PRE + "transformer_blocks.1.ff.net.2.lora_A.weight" in keys["all_dropout"]
    assert b0 + "attn2.to_q.lora_magnitude_vector.weight" in keys["dora"]
    assert not any("magnitude" in k for k in keys["attn2"] | keys["all_dropout"])
    assert len(keys["attn2"]) == 16 + 4 and len(keys["dora"]) == 24 + 4 and len(keys["all_dropout"]) == 40 + 4
    # the one mapping, both directions
    for name in ("transformer_blocks.0.attn2.to_q.lora_A.default.weight",
                 "transformer_blocks.1.attn2.to_out.0.lora_magnitude_vector.default.weight",
                 "caption_projection.linear_1.weight"):
        assert adapter_key(adapter_key(name), to_model=True) == name
    assert adapter_key("transformer_blocks.0.attn2.to_q.lora_B.default.weight") == b0 + "attn2.to_q.lora_B.weight"
    with pytest.raises(ValueError):
        adapter_key("transformer_blocks.0.attn2.to_q.lora_A.weight", to_model=True)
    opt_keys = set(load_file(os.path.join(saved["dora"][0], "optimizer.safetensors")))
    assert "exp_avg.transformer_blocks.0.attn2.to_q.lora_magnitude_vector.default.weight" in opt_keys
    assert "exp_avg_sq.caption_projection.linear_1.weight" in opt_keys and "rng.cpu.rank0" in opt_keys


def test_adapter_config_fields(saved):
    from ltx_amd.lora import lora_ff_target_modules, lora_target_modules
    cfgs = {}
    for c in CASES:
        with open(os.path.join(saved[c][0], "adapter_config.json")) as f:
            cfgs[c] = json.load(f)
    for c, cfg in cfgs.items():
        assert cfg["peft_type"] == "LORA" and cfg["bias"] == "none" and cfg["r"] == 8 and cfg["lora_alpha"] == 16
        assert cfg["base_model_name_or_path"] == "base.safetensors"
        assert cfg["ltx_amd"]["format_version"] == 1
    assert cfgs["attn2"]["target_modules"] == lora_target_modules(2, "attn2") == cfgs["dora"]["target_modules"]
    assert sorted(cfgs["all_dropout"]["target_modules"]) == sorted(lora_target_modules(2, "attn1+attn2")
                                                                   + lora_ff_target_modules(2))
    assert [cfgs[c]["lora_dropout"] for c in CASES] == [0.0, 0.1, 0.0]
    assert [cfgs[c]["use_dora"] for c in CASES] == [False, False, True]
    want = {"r": 8, "lora_alpha": 16, "scaling": 2.0, "lora_dropout": 0.1, "use_dora": False}
    assert cfgs["all_dropout"]["ltx_amd"]["groups"] == {"attn1": want, "attn2": want, "ff": want}
    assert list(cfgs["dora"]["ltx_amd"]["groups"]) == ["attn2"]


def test_groups_may_differ_in_rank(tmp_path):
    from ltx_amd import io
    from ltx_amd.lora import inject_lora, lora_ff_target_modules, lora_target_modules
    m = _bare()
    inject_lora(m, lora_target_modules(2, "attn2"), 8, 8)
    inject_lora(m, lora_ff_target_modules(2), 16, 8, feed_forward=True)
    for n, p in m.named_parameters():
        p.requires_grad = "lora_" in n or "caption_projection" in n
    path = io.save_adapter_checkpoint(m, str(tmp_path / "a"))
    with open(os.path.join(path, "adapter_config.json")) as f:
        groups = json.load(f)["ltx_amd"]["groups"]
    assert (groups["attn2"]["r"], groups["ff"]["r"], groups["ff"]["scaling"]) == (8, 16, 0.5)
    m2 = _bare()
    m2.load_state_dict({k: v for k, v in m.state_dict().items() if "lora_" not in k and "base_layer" not in k},
                       strict=False)
    io.load_adapter_checkpoint(m2, path)
    assert m2.transformer_blocks[1].ff.net[2].r == 16 and m2.transformer_blocks[1].attn2.to_v.r == 8
    _same(_trainable(m2), _trainable(m))


def test_only_safetensors_and_json_files(saved):
    for c in CASES:
        path = saved[c][0]
        assert sorted(os.listdir(path)) == ["adapter_config.json", "adapter_model.safetensors",
                                            "optimizer.safetensors", "train_state.json"]
        assert not os.path.exists(path + ".tmp") and not os.path.exists(path + ".old")
        with open(os.path.join(path, "train_state.json")) as f:
            st = json.load(f)
        assert st["format_version"] == 1 and st["world_size"] == 1 and st["loader"] == {"seed": 5}
        assert st["optimizer"]["param_groups"][0]["lr"] == 3e-4 and st["best_loss"] is None


def test_overwriting_a_checkpoint_leaves_one_complete_directory(saved, tmp_path):
    from ltx_amd import io
    m = saved["attn2"][1]
    path = str(tmp_path / "adapter_epoch_1")
    io.save_adapter_checkpoint(m, path, optimizer=_optimizer(m, seed=2))
    io.save_adapter_checkpoint(m, path)  # no optimizer this time: no stale optimizer file survives
    assert sorted(os.listdir(path)) == ["adapter_config.json", "adapter_model.safetensors", "train_state.json"]
    assert sorted(os.listdir(tmp_path)) == ["adapter_epoch_1"]


# ---------------------------------------------------------------------------------------------
# bare model
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_loading_into_a_bare_model_injects_the_same_adapters(saved, case):
    from ltx_amd import io
    from ltx_amd.transformer3d import LoraLinear
    path, m, _, _ = saved[case]
    bare = _bare()
    io.load_adapter_checkpoint(bare, path)
    sig = lambda mm: [(n, type(x).__name__, getattr(x, "r", None), getattr(x, "scaling", None),
                       getattr(x, "lora_dropout_p", None), getattr(x, "use_dora", None)) for n, x in mm.named_modules()]
    assert sig(bare) == sig(m) and any(isinstance(x, LoraLinear) for x in bare.modules())
    assert [(n, p.requires_grad, p.dtype) for n, p in bare.named_parameters()] == \
        [(n, p.requires_grad, p.dtype) for n, p in m.named_parameters()]
    _same(io.merged_state_dict_cpu(bare), io.merged_state_dict_cpu(m))


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def _refused(model, path, match, exc=ValueError, **kw):
    from ltx_amd import io
    before = {k: v.clone() for k, v in model.state_dict().items()}
    flags = [(n, p.requires_grad) for n, p in model.named_parameters()]
    with pytest.raises(exc, match=match):
        io.load_adapter_checkpoint(model, path, **kw)
    _same(dict(model.state_dict()), before)
    assert [(n, p.requires_grad) for n, p in model.named_parameters()] == flags


def test_refuses_a_rank_mismatch(saved):
    _refused(_model(CASES["attn2"], seed=3, r=16), saved["attn2"][0], "attn2 r")


def test_refuses_a_dora_file_for_a_plain_model_and_the_reverse(saved):
    _refused(_model(CASES["attn2"], seed=3), saved["dora"][0], "use_dora")
    _refused(_model(CASES["dora"], seed=3), saved["attn2"][0], "use_dora")


def test_refuses_another_wrapped_set_and_dropout(saved):
    _refused(_model(CASES["attn2"], seed=3), saved["all_dropout"][0], "attn1.to_q")
    _refused(_model(CASES["all_dropout"], seed=3), saved["attn2"][0], "attn1.to_q")
    _refused(_model({"lora_targets": "attn1+attn2", "lora_ff": True}, seed=3), saved["all_dropout"][0], "lora_dropout")


def _copy_without(path, dst, fname, drop):
    import shutil
    shutil.copytree(path, dst)
    t = load_file(os.path.join(dst, fname))
    save_file({k: v for k, v in t.items() if k not in drop}, os.path.join(dst, fname))
    return str(dst)


def test_strict_refuses_missing_and_unexpected_keys(saved, tmp_path):
    from ltx_amd import io
    path, m, opt, _ = saved["attn2"]
    key = PRE + "transformer_blocks.1.attn2.to_v.lora_B.weight"
    cut = _copy_without(path, tmp_path / "missing", "adapter_model.safetensors", {key})
    _refused(_model(CASES["attn2"], seed=3), cut, "missing keys")
    _refused(_bare(), cut, "missing keys")  # a bare model gets its injected adapters taken out again
    m2 = _model(CASES["attn2"], seed=3)
    b_before = m2.transformer_blocks[1].attn2.to_v.lora_B["default"].weight.clone()
    io.load_adapter_checkpoint(m2, cut, strict=False)
    assert torch.equal(m2.transformer_blocks[1].attn2.to_v.lora_B["default"].weight, b_before)
    assert torch.equal(m2.transformer_blocks[0].attn2.to_q.lora_A["default"].weight,
                       m.transformer_blocks[0].attn2.to_q.lora_A["default"].weight)
    # a file with a key the model does not train
    frozen = _model(CASES["attn2"], seed=3)
    frozen.caption_projection.linear_1.weight.requires_grad = False
    _refused(frozen, path, "unexpected keys")
    # optimizer moments without their parameter
    m3 = _model(CASES["attn2"], seed=3)
    cut2 = _copy_without(path, tmp_path / "nomoment", "optimizer.safetensors",
                         {"exp_avg.transformer_blocks.0.attn2.to_q.lora_A.default.weight"})
    opt3 = _optimizer(m3, seed=8)
    mom3 = _moments(m3, opt3)[0]
    _refused(m3, cut2, "exp_avg", optimizer=opt3)
    _same(_moments(m3, opt3)[0], mom3)


def test_refuses_another_world_size_and_format(saved, tmp_path):
    import shutil
    for field, value, match in (("world_size", 2, "ranks"), ("format_version", 2, "format")):
        dst = tmp_path / field
        shutil.copytree(saved["attn2"][0], dst)
        with open(dst / "train_state.json") as f:
            st = json.load(f)
        st[field] = value
        (dst / "train_state.json").write_text(json.dumps(st))
        m = _model(CASES["attn2"], seed=3)
        _refused(m, str(dst), match, optimizer=_optimizer(m))


def test_full_mode_refuses_save_adapters_and_resume(tmp_path):
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.training import train_loop
    m = apply_training_strategy(_bare(), _config({}), "full")
    for extra in ({"save_adapters": True}, {"resume_from": "auto"}):
        tc = _config(dict(extra, train_mode="full"), num_epochs=1, learning_rate=1e-3, output_dir=str(tmp_path))
        with pytest.raises(NotImplementedError, match="lora_audio"):
            train_loop(m, tc, [], torch.zeros(1, 4, 4096), torch.ones(1, 4, dtype=torch.long), device="cpu")
    tc = _config({"train_mode": "full"}, num_epochs=1, learning_rate=1e-3, output_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="lora_audio"):
        train_loop(m, tc, [], torch.zeros(1, 4, 4096), torch.ones(1, 4, dtype=torch.long), device="cpu",
                   resume_from=str(tmp_path))
    assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------------------------------------
# complete or absent
# ---------------------------------------------------------------------------------------------
def test_auto_picks_the_highest_complete_epoch(saved, tmp_path):
    import shutil
    from ltx_amd import io
    out = tmp_path / "out"
    assert io.latest_adapter_checkpoint(str(out)) is None  # no directory at all
    out.mkdir()
    assert io.latest_adapter_checkpoint(str(out)) is None
    for e in (2, 10, 12):
        shutil.copytree(saved["attn2"][0], out / f"adapter_epoch_{e}")
    os.remove(out / "adapter_epoch_12" / "train_state.json")  # a write that did not finish
    shutil.copytree(saved["attn2"][0], out / "adapter_epoch_30.tmp")
    (out / "best_model_epoch_40.safetensors").write_bytes(b"")
    assert io.latest_adapter_checkpoint(str(out)) == str(out / "adapter_epoch_10")  # 10 > 2 as numbers
    with pytest.raises(FileNotFoundError, match="train_state.json"):
        io.load_adapter_checkpoint(_model(CASES["attn2"], seed=3), str(out / "adapter_epoch_12"))


# ---------------------------------------------------------------------------------------------
# YAML
# ---------------------------------------------------------------------------------------------
def test_yaml_sets_the_keys_only_when_present(tmp_path):
    from dataclasses import asdict, fields
    from ltx_amd.config import TrainConfig, load_train_config_from_yaml
    base = "checkpoint_path: x.safetensors\ntrain:\n  lora_rank: 8\n"
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(base + "  save_adapters: true\n  resume_from: auto\n")
    (tmp_path / "c.yaml").write_text(base + "  save_adapters: false\n  resume_from: out/adapter_epoch_130\n")
    a, b, c = (load_train_config_from_yaml(str(tmp_path / f"{n}.yaml")) for n in "abc")
    assert not hasattr(a, "save_adapters") and not hasattr(a, "resume_from")
    assert b.save_adapters is True and b.resume_from == "auto"
    assert c.save_adapters is False and c.resume_from == "out/adapter_epoch_130"
    assert asdict(a) == asdict(b) == asdict(c)
    assert not {"save_adapters", "resume_from"} & {f.name for f in fields(TrainConfig)}
    gold = load_train_config_from_yaml(os.path.join(REPO, "tests", "golden", "train-avatars.yaml"))
    assert not hasattr(gold, "save_adapters") and not hasattr(gold, "resume_from")


# ---------------------------------------------------------------------------------------------
# tools/merge_adapter.py
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["all_dropout", "dora"])
def test_merge_adapter_tool_writes_the_live_models_export(saved, tmp_path, case):
    from ltx_amd import io
    spec = importlib.util.spec_from_file_location("merge_adapter", os.path.join(REPO, "tools", "merge_adapter.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path, m, _, _ = saved[case]
    base = _bare()  # the base weights every _model() starts from
    io.save_module_safetensors(base, str(tmp_path / "base.safetensors"))
    io.export_merged_safetensors(m, str(tmp_path / "live.safetensors"))
    tool.main([str(tmp_path / "base.safetensors"), path, str(tmp_path / "merged.safetensors")])
    got, want = load_file(str(tmp_path / "merged.safetensors")), load_file(str(tmp_path / "live.safetensors"))
    _same(got, want)
    assert not any("lora_" in k for k in got)
    name = "transformer_blocks.0.attn2.to_q.weight"
    assert not torch.equal(got[name], base.state_dict()[name])
    assert not torch.equal(got["caption_projection.linear_1.weight"], base.state_dict()["caption_projection.linear_1.weight"])
