"""Generate tests/golden/tiny_lora_attn1_step.{safetensors,json}: the reference's train step with
peft adapters on the self-attention as well as the cross-attention projections.

TEST INFRASTRUCTURE, in the style of oracle/gen_golden.py (whose helpers it imports): it runs only
where the reference checkout exists, puts the test-only shim (oracle/shim) ahead of it and imports
the reference modules UNMODIFIED. The reference hard-codes the attn2 targets (training.py:50-68), so
the adapters are placed the way its apply_training_strategy places them, with peft's own
get_peft_model / LoraConfig, on the eight names per block; the requires_grad rule is the
reference's. Only data is written: inputs, the captured scheduler draws, the reference's sample,
loss and the gradient of every trainable parameter. The weights are not stored: they are re-drawn
from oracle/params.py (seed recorded) and pinned by a SHA-256, as ltx2b_block does.

    python tools/gen_golden_lora_attn1.py

Config T (2 layers, 4 x 32 heads, caption 64), r = alpha = 8, latents [2, 128, 2, 8, 8], 4 prompt
tokens (3 valid). lora_B is drawn non-zero (oracle/params.py) after the peft init, so no dA is
identically zero.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import gen_golden as G  # noqa: E402  (sets up the shim + reference import paths)
import torch  # noqa: E402
from peft import LoraConfig, get_peft_model  # noqa: E402  (oracle/shim)

NAME = "tiny_lora_attn1_step"
PROJ = ("to_q", "to_k", "to_v", "to_out.0")


def build(seed, dtype, rank):
    pf = G.SymmetricPatchifier(patch_size=1)
    model = G.Transformer3DModel.from_config(G.TINY_CONFIG)
    model.patchifier = pf
    G.P.init_module_(model, seed, dtype=dtype)
    targets = [f"transformer_blocks.{i}.{a}.{p}" for i in range(len(model.transformer_blocks))
               for a in ("attn1", "attn2") for p in PROJ]
    model = get_peft_model(model, LoraConfig(r=rank, lora_alpha=rank, target_modules=targets,
                                             lora_dropout=0.0, bias="none"))
    for n, p in model.named_parameters():  # training.py:69-73
        p.requires_grad = ("lora_" in n) or ("caption_projection" in n)
    G.P.init_module_(model, seed, dtype=dtype)  # the adapters now exist: A / B per params.py
    return model, pf


def main():
    seed, train_seed, rank, B = 4242, 1717, 8, 2
    g = torch.Generator().manual_seed(61)
    batch = {"latents": torch.randn(B, 128, 2, 8, 8, generator=g),
             "ref_image_latents": torch.randn(B, 128, 1, 8, 8, generator=g),
             "pose_latents": torch.randn(B, 128, 2, 8, 8, generator=g)}
    prompt = torch.randn(1, 4, 64, generator=g)
    mask = torch.tensor([[1, 1, 1, 0]], dtype=torch.long)
    model, pf = build(seed, torch.bfloat16, rank)
    cap = G._capture_train_step(model, pf, batch, prompt, mask, seed=train_seed, rank=rank)
    grads = G._grads(model)
    attn1 = [k for k in grads if ".attn1." in k and "lora_" in k]
    assert len(attn1) == 2 * 2 * 4 and all(float(grads[k].abs().max()) > 0 for k in attn1)
    tensors = {f"in.{k}": v for k, v in batch.items()}
    tensors["in.prompt_embeds"] = prompt
    tensors["in.prompt_attention_mask"] = mask
    for k in ("noise", "t", "hidden_states", "sample", "loss", "v_target"):
        tensors[f"out.{k}"] = cap[k]
    for k, v in grads.items():
        tensors[f"grad.{k}"] = v
    meta = {"config": G.TINY_CONFIG, "param_seed": seed, "train_seed": train_seed, "lora_rank": rank,
            "lora_alpha": rank, "lora_targets": ["attn1", "attn2"],
            "weights_sha256": G.P.weights_sha256(model),
            "source": "reference ltx_video/training.py:94-166 train_step via oracle/shim, peft "
                      "get_peft_model on attn1 + attn2 to_q / to_k / to_v / to_out.0"}
    G._save(NAME, tensors, meta)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
