"""LoRA ranks 8 / 16 / 32 / 64 / 128 on the host side (no GPU, no kernel launches): the rank
validation where adapters are created, and the merged checkpoint export at r = 64."""
import json
import os

import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _tiny_cfg():
    with open(os.path.join(GOLD, "tiny_train_step.json")) as f:
        return json.load(f)["config"]


def _model(r, alpha, device="meta"):
    from ltx_amd.config import TrainConfig
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.transformer3d import Transformer3DModel
    with torch.device(device):
        m = Transformer3DModel.from_config(_tiny_cfg())
        apply_training_strategy(m, TrainConfig(checkpoint_path="-", lora_rank=r, lora_alpha=alpha), "lora_audio")
    return m


def test_supported_rank_set():
    from ltx_amd import ops
    assert ops.LORA_RANKS == (8, 16, 32, 64, 128)
    for r in ops.LORA_RANKS:
        assert ops.check_lora_rank(r) == r
        assert ops.lora_k2(r) % 64 == 0 and ops.lora_k2(r) >= 3 * r
    assert ops.lora_k2(64) == 192 and ops.lora_k2(128) == 384


@pytest.mark.parametrize("r", [8, 16, 32, 64, 128])
def test_supported_ranks_create_adapters(r):
    m = _model(r, r)
    a = m.transformer_blocks[0].attn2.to_q
    assert a.r == r and a.lora_A["default"].weight.shape[0] == r and a.lora_B["default"].weight.shape[1] == r


@pytest.mark.parametrize("r", [24, 0, 4, 48, 256, 16.0])
def test_unsupported_rank_raises_when_adapters_are_created(r):
    """ValueError naming the supported set, from apply_training_strategy / inject_lora / LoraLinear,
    before any module of the model is replaced."""
    from ltx_amd.config import TrainConfig
    from ltx_amd.lora import apply_training_strategy, inject_lora, lora_target_modules
    from ltx_amd.transformer3d import LoraLinear, Transformer3DModel
    with torch.device("meta"):
        m = Transformer3DModel.from_config(_tiny_cfg())
        with pytest.raises(ValueError, match=r"8, 16, 32, 64, 128"):
            apply_training_strategy(m, TrainConfig(checkpoint_path="-", lora_rank=r, lora_alpha=8), "lora_audio")
        with pytest.raises(ValueError, match=r"8, 16, 32, 64, 128"):
            inject_lora(m, lora_target_modules(len(m.transformer_blocks)), r, 8)
        assert not any(isinstance(x, LoraLinear) for x in m.modules())
        with pytest.raises(ValueError, match=r"8, 16, 32, 64, 128"):
            LoraLinear(torch.nn.Linear(64, 64), r, 8)


def test_processor_refuses_unsupported_rank_before_any_launch():
    """HipAttnProcessor adopts peft-style adapters it did not create: the rank check runs when it
    takes the projections apart, on CPU modules here (a kernel launch would fail on them first)."""
    from ltx_amd.processor import _Proj

    class _PeftLinear(torch.nn.Module):
        def __init__(self, r):
            super().__init__()
            self.base_layer = torch.nn.Linear(64, 64)
            self.lora_A = torch.nn.ModuleDict({"default": torch.nn.Linear(64, r, bias=False)})
            self.lora_B = torch.nn.ModuleDict({"default": torch.nn.Linear(r, 64, bias=False)})
            self.scaling = {"default": 1.0}

    with pytest.raises(ValueError, match=r"8, 16, 32, 64, 128"):
        _Proj(_PeftLinear(24))
    assert _Proj(_PeftLinear(64)).A.shape[0] == 64


def test_merged_export_rank_64(tmp_path):
    """save_training_checkpoint('lora_audio') at r = 64, alpha = 32: every wrapped projection leaves
    as W + (alpha / r) . B . A, the delta in fp32 and the promoted sum rounded once to the base
    dtype (ltx_amd.io.merged_state_dict_cpu); adapter keys are gone, everything else is unchanged."""
    from safetensors.torch import load_file
    from ltx_amd.io import save_training_checkpoint
    r, alpha = 64, 32
    torch.manual_seed(3)
    m = _model(r, alpha, device="cpu").to(torch.bfloat16)
    want = {}
    for name, mod in m.named_modules():
        if hasattr(mod, "lora_B"):
            mod.lora_A["default"].weight.data = torch.randn(r, mod.in_features)
            mod.lora_B["default"].weight.data = torch.randn(mod.out_features, r) * 0.05
            w = (torch.randn(mod.out_features, mod.in_features) * 0.1).to(torch.bfloat16)
            mod.base_layer.weight.data = w
            a, b = mod.lora_A["default"].weight, mod.lora_B["default"].weight
            assert a.dtype == torch.float32 and b.dtype == torch.float32
            want[name + ".weight"] = (w.float() + (b.float() @ a.float()) * (alpha / r)).to(torch.bfloat16)
    assert len(want) == 4 * len(m.transformer_blocks)
    path = save_training_checkpoint(m, str(tmp_path / "ckpt.safetensors"), "lora_audio")
    got = load_file(path)
    assert not any("lora_" in k or "base_layer" in k for k in got)
    for k, v in want.items():
        assert got[k].dtype == torch.bfloat16 and torch.equal(got[k], v), k
        # the adapters moved the weight (the case would prove nothing with a zero delta)
        assert not torch.equal(got[k], dict(m.named_parameters())[k.replace(".weight", ".base_layer.weight")])
    for k, v in m.state_dict().items():
        if "lora_" not in k and "base_layer" not in k:
            assert torch.equal(got[k], v), k
