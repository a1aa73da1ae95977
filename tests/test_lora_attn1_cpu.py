"""LoRA adapters on the self-attention projections (lora_targets), host side: target selection,
what apply_training_strategy wraps and trains, the errors raised before anything is replaced, the
merge / unload of attn1 adapters, the YAML switch, and the oracle pinned on the new ground by a
golden of the reference's own step with peft adapters on attn1 + attn2
(tools/gen_golden_lora_attn1.py). No GPU, no kernel launches."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

import ltx_oracle as O
from lora_attn1_utils import PROJ, attn1_params, train_config
from params import canonical_name

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TARGET_SETS = [(("attn2",), ["attn2"]), (("attn1",), ["attn1"]), (("attn1", "attn2"), ["attn1", "attn2"])]


def _tiny_cfg():
    with open(os.path.join(GOLD, "tiny_train_step.json")) as f:
        return json.load(f)["config"]


def _bare(device="meta"):
    from ltx_amd.transformer3d import Transformer3DModel
    with torch.device(device):
        return Transformer3DModel.from_config(_tiny_cfg())


def _wrapped(m):
    from ltx_amd.transformer3d import LoraLinear
    return [n for n, mod in m.named_modules() if isinstance(mod, LoraLinear)]


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("attention,atts", TARGET_SETS)
def test_target_names_and_order(attention, atts):
    from ltx_amd.lora import lora_target_modules
    n = len(_bare().transformer_blocks)
    want = [f"transformer_blocks.{i}.{a}.{p}" for i in range(n) for a in atts for p in PROJ]
    assert lora_target_modules(n, attention) == want
    assert lora_target_modules(n, "+".join(atts)) == want
    assert lora_target_modules(n, list(reversed(atts))) == want  # block order, whatever the argument's
    assert lora_target_modules(n) == lora_target_modules(n, ("attn2",))  # the reference's default


@pytest.mark.parametrize("targets", ["attn2", "attn1", "attn1+attn2", ("attn1",), ["attn1", "attn2"]])
def test_apply_training_strategy_wraps_the_requested_modules(targets):
    from ltx_amd.lora import apply_training_strategy, lora_target_modules
    m = _bare()
    with torch.device("meta"):
        apply_training_strategy(m, train_config(8, targets), "lora_audio")
    assert _wrapped(m) == lora_target_modules(len(m.transformer_blocks), targets)
    for n, p in m.named_parameters():  # the reference rule (training.py:69-73)
        assert p.requires_grad == (("lora_" in n) or ("caption_projection" in n)), n
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert any(".attn1." in n for n in trainable) == ("attn1" in str(targets))
    assert m.grad_ready_order() and {id(p) for p in m.grad_ready_order()} == {
        id(p) for p in m.parameters() if p.requires_grad}


def test_default_targets_are_todays_module_tree():
    """No lora_targets on the config: the reference's attn2 adapters, module for module and
    parameter for parameter what an explicit ("attn2",) gives."""
    from ltx_amd.config import TrainConfig
    from ltx_amd.lora import apply_training_strategy
    a, b = _bare(), _bare()
    with torch.device("meta"):
        apply_training_strategy(a, TrainConfig(checkpoint_path="-", lora_rank=8, lora_alpha=8), "lora_audio")
        apply_training_strategy(b, train_config(8, ("attn2",)), "lora_audio")
    assert not hasattr(TrainConfig(checkpoint_path="-"), "lora_targets")
    assert [(n, type(x).__name__) for n, x in a.named_modules()] == [(n, type(x).__name__) for n, x in b.named_modules()]
    assert [(n, tuple(p.shape), p.dtype, p.requires_grad) for n, p in a.named_parameters()] == \
        [(n, tuple(p.shape), p.dtype, p.requires_grad) for n, p in b.named_parameters()]
    assert all(".attn2." in n for n in _wrapped(a)) and len(_wrapped(a)) == 4 * len(a.transformer_blocks)


@pytest.mark.parametrize("bad", ["attn3", "attn1+ff", ("attn2", "ff"), (), "attn1+attn1"])
def test_unknown_attention_raises_before_anything_is_replaced(bad):
    from ltx_amd.lora import apply_training_strategy, lora_target_modules
    m = _bare()
    with pytest.raises(ValueError, match=r"attn1.*attn2"):
        lora_target_modules(2, bad)
    with pytest.raises(ValueError, match=r"attn1.*attn2"):
        apply_training_strategy(m, train_config(8, bad), "lora_audio")
    assert _wrapped(m) == []


@pytest.mark.parametrize("name", ["transformer_blocks.0.ff.net.2", "transformer_blocks.0.attn1.q_norm",
                                  "transformer_blocks.7.attn1.to_q", "proj_out"])
def test_unknown_target_module_raises_before_anything_is_replaced(name):
    from ltx_amd.lora import inject_lora, lora_target_modules
    m = _bare()
    good = lora_target_modules(len(m.transformer_blocks), "attn1")
    with pytest.raises(ValueError, match=r"attn1\|attn2.*to_q\|to_k\|to_v\|to_out\.0"):
        inject_lora(m, good + [name], 8, 8)  # the bad name comes last: nothing before it was wrapped
    assert _wrapped(m) == []


@pytest.mark.parametrize("att", ["attn1", "attn2"])
def test_partial_wrap_raises_before_anything_is_replaced(att):
    from ltx_amd.lora import inject_lora, lora_target_modules
    from ltx_amd.transformer3d import _lora_params, _lora_params1
    m = _bare()
    part = [f"transformer_blocks.0.{att}.to_q", f"transformer_blocks.0.{att}.to_v"]
    with pytest.raises(NotImplementedError, match=f"all four.*{att}"):
        inject_lora(m, lora_target_modules(len(m.transformer_blocks), "attn2" if att == "attn1" else "attn1") + part, 8, 8)
    assert _wrapped(m) == []
    # completing an attention that is already partly wrapped is accepted; the block itself refuses a
    # partly wrapped attention (before its first launch) whoever built it
    with torch.device("meta"):
        from ltx_amd.transformer3d import LoraLinear
        a = getattr(m.transformer_blocks[0], att)
        a.to_q = LoraLinear(a.to_q, 8, 8)
        with pytest.raises(NotImplementedError, match=f"all four {att}"):
            (_lora_params1 if att == "attn1" else _lora_params)(m.transformer_blocks[0])
        with pytest.raises(NotImplementedError):
            inject_lora(m, [f"transformer_blocks.0.{att}.to_k"], 8, 8)
        inject_lora(m, [f"transformer_blocks.0.{att}.{p}" for p in PROJ[1:]], 8, 8)
    assert _wrapped(m) == [f"transformer_blocks.0.{att}.{p}" for p in PROJ]


def _cpu_model(targets, r=8, seed=5):
    from ltx_amd.lora import apply_training_strategy
    cfg = _tiny_cfg()
    m = _bare("cpu")
    apply_training_strategy(m, train_config(r, targets), "lora_audio")
    p = attn1_params(cfg, seed, r, targets=("attn1", "attn2"))
    m.load_state_dict({n: p[canonical_name(n)].clone() for n, _ in m.named_parameters()}, assign=True, strict=True)
    return m, p


@pytest.mark.parametrize("targets", ["attn1", "attn1+attn2"])
def test_merge_and_unload_fold_attn1_adapters(targets):
    from ltx_amd.lora import merged_state_dict, unload_lora
    from ltx_amd.transformer3d import LoraLinear
    r = 8
    m, p = _cpu_model(targets, r)
    names = _wrapped(m)
    assert any(".attn1." in n for n in names)
    sd = merged_state_dict(m)
    assert not any("lora_" in k or "base_layer" in k for k in sd)
    for n in names:
        w, a, b = p[n + ".weight"], p[n + ".lora_A.default.weight"], p[n + ".lora_B.default.weight"]
        want = (w.float() + (r / r) * (b @ a)).to(w.dtype)  # W + s B A, s = alpha / r = 1
        assert float((b @ a).abs().max()) > 0
        assert torch.equal(sd[n + ".weight"], want), n
        assert torch.equal(sd[n + ".bias"], p[n + ".bias"]), n
    untouched = "transformer_blocks.0.attn2.to_q.weight" if targets == "attn1" else "transformer_blocks.0.ff.net.2.weight"
    assert torch.equal(sd[untouched], p[untouched])
    for blk in m.transformer_blocks:  # a stale packed-weight cache would survive the unload
        blk._pack, blk._pack_key = {"qkv_w": None}, ("stale",)
    unload_lora(m)
    assert not any(isinstance(x, LoraLinear) for x in m.modules())
    got = m.state_dict()
    assert set(got) == set(sd)
    for n in names:  # peft's in-place promoted add rounded to the base dtype
        w, a, b = p[n + ".weight"], p[n + ".lora_A.default.weight"], p[n + ".lora_B.default.weight"]
        assert torch.equal(got[n + ".weight"], (w + (b @ a) * 1.0).to(w.dtype)), n
    assert all(blk._pack is None and blk._pack_key is None for blk in m.transformer_blocks)


def test_checkpoint_export_walks_attn1_adapters(tmp_path):
    from ltx_amd import io
    m, p = _cpu_model("attn1+attn2")
    path = io.save_training_checkpoint(m, str(tmp_path / "ckpt.safetensors"), "lora_audio")
    sd = load_file(path)
    n = "transformer_blocks.1.attn1.to_k"
    key = [k for k in sd if k.endswith(n + ".weight")]
    assert key and not any("lora_" in k for k in sd)
    w, a, b = p[n + ".weight"], p[n + ".lora_A.default.weight"], p[n + ".lora_B.default.weight"]
    assert torch.equal(sd[key[0]], (w + (b @ a) * 1.0).to(w.dtype))


def test_yaml_sets_lora_targets_only_when_present(tmp_path):
    from dataclasses import asdict
    from ltx_amd.config import load_train_config_from_yaml
    base = "checkpoint_path: x.safetensors\ntrain:\n  lora_rank: 16\n"
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(base + "  lora_targets: attn1+attn2\n")
    (tmp_path / "c.yaml").write_text(base + "  lora_targets: [attn1]\n")
    a = load_train_config_from_yaml(str(tmp_path / "a.yaml"))
    b = load_train_config_from_yaml(str(tmp_path / "b.yaml"))
    c = load_train_config_from_yaml(str(tmp_path / "c.yaml"))
    assert not hasattr(a, "lora_targets") and b.lora_targets == "attn1+attn2" and c.lora_targets == ("attn1",)
    assert asdict(a) == asdict(b) == asdict(c) and "lora_targets" not in asdict(b)


def test_oracle_matches_reference_with_attn1_adapters():
    """The oracle reproduces the reference's own step with peft adapters on the eight projections
    per block (config T, r = 8, two layers), within the thresholds tests/test_oracle_golden.py uses
    for tiny_train_step: sample 2e-3, loss 1 %, every trainable gradient 5e-3 (rel-Frobenius)."""
    from params import weights_sha256
    d = load_file(os.path.join(GOLD, "tiny_lora_attn1_step.safetensors"))
    with open(os.path.join(GOLD, "tiny_lora_attn1_step.json")) as f:
        meta = json.load(f)
    assert os.path.getsize(os.path.join(GOLD, "tiny_lora_attn1_step.safetensors")) < \
        os.path.getsize(os.path.join(GOLD, "tiny_train_step.safetensors"))
    cfg, r = meta["config"], meta["lora_rank"]
    assert r == 8 and cfg["num_layers"] == 2 and meta["lora_alpha"] == r
    p = attn1_params(cfg, meta["param_seed"], r)

    class _Named(torch.nn.Module):  # the hash walks named_parameters
        def __init__(self, tensors):
            super().__init__()
            self._t = tensors

        def named_parameters(self, *a, **k):
            return iter(self._t.items())
    assert weights_sha256(_Named(p)) == meta["weights_sha256"]
    for k, v in p.items():
        if ("lora_" in k) or ("caption_projection" in k):
            v.requires_grad_(True)
    torch.manual_seed(meta["train_seed"])
    res = O.train_step(p, cfg, d["in.latents"], d["in.ref_image_latents"], d["in.pose_latents"],
                       d["in.prompt_embeds"], d["in.prompt_attention_mask"])
    assert torch.equal(res["t"], d["out.t"]) and torch.equal(res["noise"], d["out.noise"])
    assert torch.equal(res["x_t"], d["out.hidden_states"]) and torch.equal(res["v_target"], d["out.v_target"])
    assert _rel(res["sample"], d["out.sample"]) < 2e-3
    assert abs(float(res["loss"]) - float(d["out.loss"])) <= 0.01 * abs(float(d["out.loss"]))
    res["loss"].backward()
    grads = [k[5:] for k in d if k.startswith("grad.")]
    assert sorted(grads) == sorted(k for k in p if p[k].requires_grad)
    assert sum(".attn1." in k and "lora_" in k for k in grads) == 16
    for name in grads:
        assert float(d["grad." + name].float().abs().max()) > 0, name
        assert _rel(p[name].grad, d["grad." + name]) < 5e-3, name
