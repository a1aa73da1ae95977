"""Helpers of the feed-forward-adapter tests (tests/test_lora_ff_cpu.py, tests/test_lora_ff_gpu.py):
parameter dicts with adapters on ff.net.0.proj / ff.net.2, models built from them, and the chain-rule
reference that lets the unchanged oracle (which has no adapter on the feed-forward) stand in for one.

The chain rule: an adapted linear computes x . (W + s B A)^T + b, so with W' = W + s B A made a
trainable weight of a model WITHOUT the adapter, dL/dW' is the gradient of the merged weight and
    dB = s . dW' . A^T          dA = s . B^T . dW'
exactly (W' enters the loss only through that product)."""
import torch

from lora_attn1_utils import attn1_params
from params import canonical_name, init_value

FF = ("net.0.proj", "net.2")


def ff_names(num_layers):
    return [f"transformer_blocks.{i}.ff.{p}" for i in range(num_layers) for p in FF]


def ff_params(cfg, seed, r, targets=("attn2",), dtype=torch.bfloat16):
    """attn1_params for the targeted attentions plus the adapter keys of both feed-forward linears of
    every block, drawn with params.init_value (non-zero lora_B)."""
    p = attn1_params(cfg, seed, r, targets=tuple(targets), dtype=dtype)
    for pre in ff_names(cfg["num_layers"]):
        out_f, in_f = p[pre + ".weight"].shape
        p[pre + ".lora_A.default.weight"] = init_value(pre + ".lora_A.default.weight", (r, in_f), seed)
        p[pre + ".lora_B.default.weight"] = init_value(pre + ".lora_B.default.weight", (out_f, r), seed)
    return p


def train_config(r, targets=None, ff=None, alpha=None):
    """TrainConfig with lora_targets / lora_ff set the way the reference sets train_mode (setattr)."""
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="-", lora_rank=r, lora_alpha=r if alpha is None else alpha)
    if targets is not None:
        setattr(tc, "lora_targets", targets)
    if ff is not None:
        setattr(tc, "lora_ff", ff)
    return tc


def build_ff_model(cfg, params, r, targets="attn2", ff=True, device="cuda", alpha=None):
    """tests/model_utils.build_model with config.lora_targets = targets and config.lora_ff = ff;
    targets = () builds feed-forward adapters only, through inject_lora(..., feed_forward=True)."""
    from ltx_amd.lora import apply_training_strategy, inject_lora, lora_ff_target_modules
    from ltx_amd.patchifier import SymmetricPatchifier
    from ltx_amd.transformer3d import Transformer3DModel
    with torch.device("meta"):
        m = Transformer3DModel.from_config(cfg)
        if targets == ():
            inject_lora(m, lora_ff_target_modules(len(m.transformer_blocks)), r, r if alpha is None else alpha,
                        feed_forward=True)
        else:
            apply_training_strategy(m, train_config(r, targets, ff, alpha), "lora_audio")
    sd = {name: params[canonical_name(name)].detach().to(device).clone() for name, _ in m.named_parameters()}
    m.load_state_dict(sd, assign=True, strict=True)
    for n, p in m.named_parameters():
        p.requires_grad_(("lora_" in n) or ("caption_projection" in n))
    m.patchifier = SymmetricPatchifier(1)
    return m


def merged_ff_params(params, s=1.0, dtype=torch.float32):
    """The oracle's parameter dict for the chain-rule reference: the feed-forward adapter keys removed
    and each ff weight replaced by W' = W + s B A (summed in fp32, then `dtype`)."""
    q = {k: v for k, v in params.items() if not (".ff." in k and "lora_" in k)}
    for k in list(q):
        if ".ff." in k and k.endswith(".weight"):
            pre = k[:-len(".weight")]
            a, b = params[pre + ".lora_A.default.weight"], params[pre + ".lora_B.default.weight"]
            q[k] = (params[k].float() + s * (b.float() @ a.float())).to(dtype)
    return q


def is_ff_chain_trainable(name):
    """What the chain-rule reference differentiates: the reference's trainable set plus the merged
    feed-forward weights."""
    return ("lora_" in name) or ("caption_projection" in name) or (".ff." in name and name.endswith(".weight"))


def chain_rule_grads(grads, params, s=1.0):
    """Gradients by canonical name of the adapted model from those of the merged one: the ff weight
    gradients become dB = s dW' A^T and dA = s B^T dW' (fp32), everything else passes through."""
    out = {}
    for k, gw in grads.items():
        if ".ff." in k and k.endswith(".weight"):
            pre = k[:-len(".weight")]
            a = params[pre + ".lora_A.default.weight"].to(gw.device).float()
            b = params[pre + ".lora_B.default.weight"].to(gw.device).float()
            out[pre + ".lora_B.default.weight"] = s * (gw.float() @ a.t())
            out[pre + ".lora_A.default.weight"] = s * (b.t() @ gw.float())
        else:
            out[k] = gw
    return out


def chain_oracle_step(params, cfg, d, dtype, device="cuda", s=1.0):
    """model_utils.oracle_step on the merged parameters, mapped back through the chain rule:
    (sample, {name: grad} for the adapted model's trainable names, f32 mse)."""
    from model_utils import oracle_step
    q = merged_ff_params(params, s, dtype=torch.float32 if dtype == torch.float32 else dtype)
    sample, grads, loss = oracle_step(q, cfg, d, dtype, is_ff_chain_trainable, device=device)
    return sample, chain_rule_grads(grads, params, s), loss
