"""LoRA adapters on the feed-forward linears (config.lora_ff), host side: target names, what
apply_training_strategy wraps and trains, the errors raised before anything is replaced, merge /
unload / checkpoint export of the new adapters, the YAML switch, and the chain-rule reference of the
GPU tests validated against the reference's own fp32 step (tools/gen_golden_lora_ff.py).
No GPU, no kernel launches."""
import importlib.util
import json
import os

import pytest
import torch
from safetensors.torch import load_file

from lora_attn1_utils import PROJ
from lora_ff_utils import FF, chain_oracle_step, ff_names, ff_params, train_config
from params import canonical_name

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _tiny_cfg():
    with open(os.path.join(GOLD, "tiny_lora_ff_step.json")) as f:
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


def _expected(n, atts):
    """module-tree order: a block's attentions, then its feed-forward"""
    return [f"transformer_blocks.{i}.{a}.{p}" for i in range(n) for a, ps in
            ([(a, PROJ) for a in atts] + [("ff", FF)]) for p in ps]


def test_ff_target_names_and_order():
    from ltx_amd.lora import lora_ff_target_modules
    assert lora_ff_target_modules(2) == [
        "transformer_blocks.0.ff.net.0.proj", "transformer_blocks.0.ff.net.2",
        "transformer_blocks.1.ff.net.0.proj", "transformer_blocks.1.ff.net.2"]
    assert lora_ff_target_modules(3) == ff_names(3) and lora_ff_target_modules(0) == []


@pytest.mark.parametrize("targets,atts", [(None, ["attn2"]), ("attn1", ["attn1"]), ("attn1+attn2", ["attn1", "attn2"])])
def test_lora_ff_wraps_the_expected_modules(targets, atts):
    from ltx_amd.lora import apply_training_strategy
    m = _bare()
    with torch.device("meta"):
        apply_training_strategy(m, train_config(8, targets, True, alpha=16), "lora_audio")
    n = len(m.transformer_blocks)
    assert _wrapped(m) == _expected(n, atts)
    for blk in m.transformer_blocks:  # config.lora_rank / lora_alpha
        for lin in (blk.ff.net[0].proj, blk.ff.net[2]):
            assert lin.r == 8 and lin.scaling == 2.0
    for name, p in m.named_parameters():  # the reference rule (training.py:69-73)
        assert p.requires_grad == (("lora_" in name) or ("caption_projection" in name)), name
    trainable = [name for name, p in m.named_parameters() if p.requires_grad]
    assert sum(".ff." in name for name in trainable) == 4 * n
    order = m.grad_ready_order()
    assert len(order) == len(trainable) and {id(p) for p in order} == {id(p) for p in m.parameters() if p.requires_grad}


@pytest.mark.parametrize("ff", [None, False])
def test_without_lora_ff_the_module_tree_is_todays(ff):
    from ltx_amd.config import TrainConfig
    from ltx_amd.lora import apply_training_strategy
    a, b = _bare(), _bare()
    with torch.device("meta"):
        apply_training_strategy(a, TrainConfig(checkpoint_path="-", lora_rank=8, lora_alpha=8), "lora_audio")
        apply_training_strategy(b, train_config(8, None, ff), "lora_audio")
    assert not hasattr(TrainConfig(checkpoint_path="-"), "lora_ff")
    assert [(n, type(x).__name__) for n, x in a.named_modules()] == [(n, type(x).__name__) for n, x in b.named_modules()]
    assert [(n, tuple(p.shape), p.dtype, p.requires_grad) for n, p in a.named_parameters()] == \
        [(n, tuple(p.shape), p.dtype, p.requires_grad) for n, p in b.named_parameters()]
    assert not any(".ff." in n for n in _wrapped(a))


@pytest.mark.parametrize("name", ["transformer_blocks.0.ff.net.0.proj", "transformer_blocks.1.ff.net.2"])
def test_inject_lora_without_the_keyword_refuses_ff_names(name):
    from ltx_amd.lora import inject_lora, lora_target_modules
    m = _bare()
    good = lora_target_modules(len(m.transformer_blocks), "attn2")
    with pytest.raises(ValueError, match=r"attn1\|attn2.*to_q\|to_k\|to_v\|to_out\.0"):
        inject_lora(m, good + [name], 8, 8)
    assert _wrapped(m) == []
    with pytest.raises(ValueError):  # the keyword admits the two ff linears, nothing else of the ff
        inject_lora(m, ["transformer_blocks.0.ff.net.1"], 8, 8, feed_forward=True)
    with pytest.raises(ValueError):
        inject_lora(m, ["transformer_blocks.9.ff.net.2"], 8, 8, feed_forward=True)
    assert _wrapped(m) == []


def test_ff_only_is_legal_at_the_inject_level():
    from ltx_amd.lora import inject_lora, lora_ff_target_modules
    m = _bare()
    with torch.device("meta"):
        inject_lora(m, lora_ff_target_modules(2), 16, 16, feed_forward=True)
    assert _wrapped(m) == ff_names(2)


@pytest.mark.parametrize("half", FF)
def test_half_wrapped_ff_raises_before_anything_is_replaced(half):
    from ltx_amd.lora import inject_lora, lora_target_modules
    from ltx_amd.transformer3d import LoraLinear, _block_ab as _lora_abf, _lora_params_ff
    m = _bare()
    with pytest.raises(NotImplementedError, match="both linears.*ff"):
        inject_lora(m, lora_target_modules(2, "attn2") + ff_names(1) + [f"transformer_blocks.1.ff.{half}"], 8, 8,
                    feed_forward=True)
    assert _wrapped(m) == []
    # the block refuses a half-wrapped feed-forward (before its first launch) whoever built it; completing it
    # is accepted
    with torch.device("meta"):
        net = m.transformer_blocks[0].ff.net
        if half == "net.2":
            net[2] = LoraLinear(net[2], 8, 8)
        else:
            net[0].proj = LoraLinear(net[0].proj, 8, 8)
        for fn in (_lora_params_ff, _lora_abf):
            with pytest.raises(NotImplementedError, match="both feed-forward linears"):
                fn(m.transformer_blocks[0])
        assert _lora_params_ff(m.transformer_blocks[1]) is None and _lora_abf(m.transformer_blocks[1]) == []
        other = [p for p in FF if p != half][0]
        inject_lora(m, [f"transformer_blocks.0.ff.{other}"], 8, 8, feed_forward=True)
        assert len(_lora_abf(m.transformer_blocks[0])) == 4
        # the two adapters of a block share rank and scaling
        net[2].scaling = 0.5
        with pytest.raises(NotImplementedError, match="share rank and scaling"):
            _lora_params_ff(m.transformer_blocks[0])
    assert _wrapped(m) == ff_names(1)


def _shim_peft():
    path = os.path.join(os.path.dirname(GOLD), os.pardir, "oracle", "shim", "peft", "__init__.py")
    spec = importlib.util.spec_from_file_location("_shim_peft_for_ff_tests", os.path.normpath(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cpu_model(r=8, seed=5):
    from ltx_amd.lora import apply_training_strategy
    cfg = _tiny_cfg()
    m = _bare("cpu")
    apply_training_strategy(m, train_config(r, "attn2", True), "lora_audio")
    p = ff_params(cfg, seed, r)
    m.load_state_dict({n: p[canonical_name(n)].clone() for n, _ in m.named_parameters()}, assign=True, strict=True)
    return m, p


def test_merge_and_unload_fold_ff_adapters_as_peft_does():
    """merged_state_dict and unload_lora against the shim's merge_and_unload (peft 0.17.1) on the same
    module tree, weights and adapters: bitwise."""
    from ltx_amd.lora import merged_state_dict, unload_lora
    from ltx_amd.transformer3d import LoraLinear
    r = 8
    m, p = _cpu_model(r)
    names = _wrapped(m)
    assert [n for n in names if ".ff." in n] == ff_names(2)
    peft = _shim_peft()
    ref = _bare("cpu")
    ref.load_state_dict({n: p[n].clone() for n, _ in ref.named_parameters()}, assign=True, strict=True)
    pm = peft.get_peft_model(ref, peft.LoraConfig(r=r, lora_alpha=r, target_modules=names))
    with torch.no_grad():
        for n, mod in ref.named_modules():
            if isinstance(mod, peft.LoraLinear):
                mod.lora_A["default"].weight.copy_(p[n + ".lora_A.default.weight"])
                mod.lora_B["default"].weight.copy_(p[n + ".lora_B.default.weight"])
    want = pm.merge_and_unload().state_dict()
    sd = merged_state_dict(m)
    assert set(sd) == set(want) and not any("lora_" in k or "base_layer" in k for k in sd)
    for n in ff_names(2):
        assert not torch.equal(want[n + ".weight"], p[n + ".weight"]), n  # the fold changed the weight
    for k in want:
        assert torch.equal(sd[k], want[k]), k
    for blk in m.transformer_blocks:  # a stale packed-weight cache (ff1_wT / ff2_wT) would survive the unload
        blk._pack, blk._pack_key = {"ff1_wT": None, "ff2_wT": None}, ("stale",)
    unload_lora(m)
    assert not any(isinstance(x, LoraLinear) for x in m.modules())
    got = m.state_dict()
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert all(blk._pack is None and blk._pack_key is None for blk in m.transformer_blocks)


def test_checkpoint_export_carries_the_ff_keys(tmp_path):
    from ltx_amd import io
    m, p = _cpu_model()
    path = io.save_training_checkpoint(m, str(tmp_path / "ckpt.safetensors"), "lora_audio")
    sd = load_file(path)
    assert not any("lora_" in k or "base_layer" in k for k in sd)
    for n in ff_names(2):
        key = [k for k in sd if k.endswith(n + ".weight")]
        assert len(key) == 1 and [k for k in sd if k.endswith(n + ".bias")], n
        w, a, b = p[n + ".weight"], p[n + ".lora_A.default.weight"], p[n + ".lora_B.default.weight"]
        assert torch.equal(sd[key[0]], (w + (b @ a) * 1.0).to(w.dtype)), n


def test_yaml_sets_lora_ff_only_when_present(tmp_path):
    from dataclasses import asdict
    from ltx_amd.config import load_train_config_from_yaml
    base = "checkpoint_path: x.safetensors\ntrain:\n  lora_rank: 16\n"
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(base + "  lora_ff: true\n")
    (tmp_path / "c.yaml").write_text(base + "  lora_ff: false\n  lora_targets: attn1\n")
    a = load_train_config_from_yaml(str(tmp_path / "a.yaml"))
    b = load_train_config_from_yaml(str(tmp_path / "b.yaml"))
    c = load_train_config_from_yaml(str(tmp_path / "c.yaml"))
    assert not hasattr(a, "lora_ff") and b.lora_ff is True and c.lora_ff is False and c.lora_targets == "attn1"
    assert not hasattr(b, "lora_targets")
    assert asdict(a) == asdict(b) == asdict(c) and "lora_ff" not in asdict(b)


def test_chain_rule_reference_matches_the_reference_fp32_step():
    """The reference method of the GPU tests, validated on the CPU: the unchanged oracle in fp32 on
    config T with W' = W + s B A as trainable feed-forward weights, its dW' mapped to dB = s dW' A^T and
    dA = s B^T dW', against the reference's own fp32 step with peft adapters on attn2 + ff (the
    golden's out32. / grad32. tensors). The two compute the same function and differ by fp32 summation
    order only. Measured here (rel-Frobenius): sample 2.54e-7, worst gradient 6.93e-7 (block 1's
    ff.net.0.proj lora_A, also the worst of all trainable gradients); asserted at ten times those,
    2.54e-6 and 6.93e-6. The loss came out equal to the last bit (distance 0), so ten times the
    measurement is no usable bound: it is held to ten roundings of its format instead, 10 x 2^-24
    relative (the fp32 mean of 32768 squared errors)."""
    from lora_ff_utils import ff_params as _ffp
    from params import weights_sha256
    d = load_file(os.path.join(GOLD, "tiny_lora_ff_step.safetensors"))
    with open(os.path.join(GOLD, "tiny_lora_ff_step.json")) as f:
        meta = json.load(f)
    assert os.path.getsize(os.path.join(GOLD, "tiny_lora_ff_step.safetensors")) < 1 << 20
    cfg, r = meta["config"], meta["lora_rank"]
    assert r == 8 and cfg["num_layers"] == 2 and meta["lora_alpha"] == r and meta["lora_ff"] is True
    p = _ffp(cfg, meta["param_seed"], r)

    class _Named(torch.nn.Module):  # the hash walks named_parameters
        def __init__(self, tensors):
            super().__init__()
            self._t = tensors

        def named_parameters(self, *a, **k):
            return iter(self._t.items())
    assert weights_sha256(_Named(p)) == meta["weights_sha256"]
    dd = {k: v for k, v in d.items() if k.startswith("in.") or k in ("out.t", "out.noise")}
    sample, grads, loss = chain_oracle_step(p, cfg, dd, torch.float32, device="cpu")
    names = sorted(k[7:] for k in d if k.startswith("grad32."))
    assert sorted(grads) == names == sorted(k[5:] for k in d if k.startswith("grad."))
    assert sum(".ff." in k for k in names) == 8
    e_s = _rel(sample, d["out32.sample"])
    e_l = abs(loss - float(d["out32.loss"])) / abs(float(d["out32.loss"]))
    e_g = {k: _rel(grads[k], d["grad32." + k]) for k in names}
    worst = max(e_g, key=e_g.get)
    worst_ff = max((k for k in names if ".ff." in k), key=e_g.get)
    print(f"chain rule vs reference fp32: sample {e_s:.3e} loss {e_l:.3e} worst grad {worst} {e_g[worst]:.3e} "
          f"worst ff grad {worst_ff} {e_g[worst_ff]:.3e}")
    assert e_s < 2.54e-6 and e_l <= 10 * 2.0 ** -24
    for k in names:
        assert float(d["grad32." + k].abs().max()) > 0, k
        assert e_g[k] < 6.93e-6, (k, e_g[k])
