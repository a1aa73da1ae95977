"""Helpers of the attn1-adapter tests (tests/test_lora_attn1_cpu.py, tests/test_lora_attn1_gpu.py):
parameter dicts with adapters on the self-attention projections and models built from them."""
import torch

from params import canonical_name, init_value

PROJ = ("to_q", "to_k", "to_v", "to_out.0")


def attn1_params(cfg, seed, r, targets=("attn1", "attn2"), dtype=torch.bfloat16):
    """O.make_params (attn2 adapters when targeted) plus the attn1 adapter keys drawn with
    params.init_value: the flat canonical-name dict the oracle and build_targets_model take."""
    import ltx_oracle as O
    p = O.make_params(cfg, seed, dtype=dtype, lora_rank=r if "attn2" in targets else 0, requires_grad=False)
    D = cfg["num_attention_heads"] * cfg["attention_head_dim"]
    if "attn1" in targets:
        for i in range(cfg["num_layers"]):
            for lin in PROJ:
                pre = f"transformer_blocks.{i}.attn1.{lin}"
                p[pre + ".lora_A.default.weight"] = init_value(pre + ".lora_A.default.weight", (r, D), seed)
                p[pre + ".lora_B.default.weight"] = init_value(pre + ".lora_B.default.weight", (D, r), seed)
    return p


def train_config(r, targets=None, alpha=None):
    """TrainConfig with lora_targets set the way the reference sets train_mode (setattr)."""
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="-", lora_rank=r, lora_alpha=r if alpha is None else alpha)
    if targets is not None:
        setattr(tc, "lora_targets", targets)
    return tc


def build_targets_model(cfg, params, r, targets, device="cuda"):
    """tests/model_utils.build_model with config.lora_targets = targets."""
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.patchifier import SymmetricPatchifier
    from ltx_amd.transformer3d import Transformer3DModel
    with torch.device("meta"):
        m = Transformer3DModel.from_config(cfg)
        apply_training_strategy(m, train_config(r, targets), "lora_audio")
    sd = {name: params[canonical_name(name)].detach().to(device).clone() for name, _ in m.named_parameters()}
    m.load_state_dict(sd, assign=True, strict=True)
    for n, p in m.named_parameters():
        p.requires_grad_(("lora_" in n) or ("caption_projection" in n))
    m.patchifier = SymmetricPatchifier(1)
    return m
