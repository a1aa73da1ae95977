"""Helpers of the DoRA tests (tests/test_lora_dora_cpu.py, tests/test_lora_dora_gpu.py): the golden
step's parameters, DoRA models built from a flat canonical-name dict, and the float64 statement of
one DoRA linear (peft 0.17.1 DoraLinearLayer with lora_dropout = 0)."""
import json
import os

import torch

from params import canonical_name

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "tiny_lora_dora_step"
MAG = ".lora_magnitude_vector.default.weight"
PROJ = ("to_q", "to_k", "to_v", "to_out.0")


def golden_meta():
    with open(os.path.join(GOLD, NAME + ".json")) as f:
        return json.load(f)


def dora_names(num_layers):
    return [f"transformer_blocks.{i}.attn2.{p}" for i in range(num_layers) for p in PROJ]


def golden_params(meta, raw):
    """The golden step's parameters by canonical name: oracle/params.py's draw with attn2 adapters
    (non-zero B) plus the fixture's stored magnitudes w.<name>."""
    from lora_attn1_utils import attn1_params
    p = attn1_params(meta["config"], meta["param_seed"], meta["lora_rank"], targets=("attn2",))
    for k, v in raw.items():
        if k.startswith("w."):
            p[k[2:]] = v.clone()
    return p


def dora_config(r, dora=True, alpha=None):
    """TrainConfig with use_dora set the way the reference sets train_mode (setattr); dora=None leaves
    the attribute absent."""
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="-", lora_rank=r, lora_alpha=r if alpha is None else alpha)
    if dora is not None:
        setattr(tc, "use_dora", dora)
    return tc


def build_dora_model(cfg, params, r, dora=True, device="cuda"):
    """tests/model_utils.build_model with config.use_dora = dora. A magnitude missing from `params` is
    the torch statement of the row norm (a fresh adapter: c = 1 up to the norm's own rounding)."""
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.patchifier import SymmetricPatchifier
    from ltx_amd.transformer3d import Transformer3DModel, dora_weight_norm
    with torch.device("meta"):
        m = Transformer3DModel.from_config(cfg)
        apply_training_strategy(m, dora_config(r, dora), "lora_audio")
    sd = {}
    for name, _ in m.named_parameters():
        k = canonical_name(name)
        if k not in params and k.endswith(MAG):
            pre = k[:-len(MAG)]
            sd[name] = dora_weight_norm(params[pre + ".weight"], params[pre + ".lora_A.default.weight"],
                                        params[pre + ".lora_B.default.weight"], 1.0).to(device)
        else:
            sd[name] = params[k].detach().to(device).clone()
    m.load_state_dict(sd, assign=True, strict=True)
    for n, p in m.named_parameters():
        p.requires_grad_(("lora_" in n) or ("caption_projection" in n))
    m.patchifier = SymmetricPatchifier(1)
    return m


def dora_statement(x, W, b, A, B, m, s):
    """peft's DoRA linear in the dtype of its arguments (float64 in the tests), the norm detached:
    y = (m / ||W + s B A||_row) * (x W^T + s (x A^T) B^T) + b."""
    norm = torch.linalg.norm(W + s * (B @ A), dim=1).detach()
    c = m / norm
    return c * (x @ W.t() + s * ((x @ A.t()) @ B.t())) + b
