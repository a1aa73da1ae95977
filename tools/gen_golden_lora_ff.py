"""Generate tests/golden/tiny_lora_ff_step.{safetensors,json}: the reference's train step with peft
adapters on the cross-attention projections and on both feed-forward linears, run twice on the same
draws: once in bf16 (the reference as it trains) and once with the model in fp32.

TEST INFRASTRUCTURE, in the style of tools/gen_golden_lora_attn1.py: it runs only where the reference
checkout exists, puts the test-only shim (oracle/shim) ahead of it and imports the reference modules
UNMODIFIED. The adapters are placed with peft's own get_peft_model / LoraConfig on attn2's four
projections plus ff.net.0.proj and ff.net.2 of every block; the requires_grad rule is the
reference's (training.py:69-73). oracle/ltx_oracle.py has no adapter on the feed-forward, so the fp32
side of the tests' noise criterion is the reference itself: the same module tree with its bf16
weights widened to fp32 (adapters are fp32 in both runs), the same t (the seed is shared and t is
drawn in fp32 whatever the model's dtype) and the bf16 run's noise handed back through
torch.randn_like for the one call train_step makes. Only data is written: inputs, the captured
draws, and sample, loss and every trainable gradient of both runs ("out." / "grad." for bf16,
"out32." / "grad32." for fp32). The weights are not stored: they are re-drawn from oracle/params.py
(seed recorded) and pinned by a SHA-256.

    python tools/gen_golden_lora_ff.py

Config T (2 layers, 4 x 32 heads, caption 64), r = alpha = 8, latents [2, 128, 2, 8, 8], 4 prompt
tokens (3 valid): the batch of tiny_lora_attn1_step. lora_B is drawn non-zero (oracle/params.py).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import gen_golden as G  # noqa: E402  (sets up the shim + reference import paths)
import torch  # noqa: E402
from peft import LoraConfig, get_peft_model  # noqa: E402  (oracle/shim)

NAME = "tiny_lora_ff_step"
PROJ = ("to_q", "to_k", "to_v", "to_out.0")
FF = ("net.0.proj", "net.2")


def build(seed, rank, fp32):
    pf = G.SymmetricPatchifier(patch_size=1)
    model = G.Transformer3DModel.from_config(G.TINY_CONFIG)
    model.patchifier = pf
    G.P.init_module_(model, seed, dtype=torch.bfloat16)
    n = len(model.transformer_blocks)
    targets = [f"transformer_blocks.{i}.attn2.{p}" for i in range(n) for p in PROJ]
    targets += [f"transformer_blocks.{i}.ff.{p}" for i in range(n) for p in FF]
    model = get_peft_model(model, LoraConfig(r=rank, lora_alpha=rank, target_modules=targets,
                                             lora_dropout=0.0, bias="none"))
    for name, p in model.named_parameters():  # training.py:69-73
        p.requires_grad = ("lora_" in name) or ("caption_projection" in name)
    G.P.init_module_(model, seed, dtype=torch.bfloat16)  # the adapters now exist: A / B per params.py
    if fp32:  # the same bf16 weight values, computed with in fp32
        model = model.to(torch.float32)
    return model, pf


def main():
    seed, train_seed, rank, B = 4242, 1717, 8, 2
    g = torch.Generator().manual_seed(61)
    # the draws of tiny_lora_attn1_step, stored as the bf16 values the bf16 model computes with: both
    # runs see the same inputs (the fp32 run widens them), and the fixture stays under 1 MiB
    batch = {"latents": torch.randn(B, 128, 2, 8, 8, generator=g).bfloat16(),
             "ref_image_latents": torch.randn(B, 128, 1, 8, 8, generator=g).bfloat16(),
             "pose_latents": torch.randn(B, 128, 2, 8, 8, generator=g).bfloat16()}
    prompt = torch.randn(1, 4, 64, generator=g).bfloat16()
    mask = torch.tensor([[1, 1, 1, 0]], dtype=torch.long)
    model, pf = build(seed, rank, fp32=False)
    cap = G._capture_train_step(model, pf, batch, prompt, mask, seed=train_seed, rank=rank)
    grads = G._grads(model)
    sha = G.P.weights_sha256(model)

    model32, pf32 = build(seed, rank, fp32=True)
    assert G.P.weights_sha256(model32) == sha
    randn_like = torch.randn_like
    calls = []

    def noise_of_the_bf16_run(x, *a, **k):
        calls.append(tuple(x.shape))
        assert x.shape == cap["noise"].shape
        return cap["noise"].to(x.dtype)

    torch.randn_like = noise_of_the_bf16_run
    try:
        cap32 = G._capture_train_step(model32, pf32, batch, prompt, mask, seed=train_seed, rank=rank)
    finally:
        torch.randn_like = randn_like
    assert len(calls) == 1 and torch.equal(cap32["t"], cap["t"])
    assert torch.equal(cap32["noise"], cap["noise"].float())
    grads32 = G._grads(model32)
    assert sorted(grads) == sorted(grads32)
    ff = [k for k in grads if ".ff." in k and "lora_" in k]
    assert len(ff) == 2 * 2 * 2 and all(float(grads[k].abs().max()) > 0 for k in ff)

    tensors = {f"in.{k}": v for k, v in batch.items()}
    tensors["in.prompt_embeds"] = prompt
    tensors["in.prompt_attention_mask"] = mask
    for k in ("noise", "t", "sample", "loss", "v_target"):
        tensors[f"out.{k}"] = cap[k]
    for k in ("sample", "loss"):
        tensors[f"out32.{k}"] = cap32[k]
    for k, v in grads.items():
        tensors[f"grad.{k}"] = v
    for k, v in grads32.items():
        tensors[f"grad32.{k}"] = v
    meta = {"config": G.TINY_CONFIG, "param_seed": seed, "train_seed": train_seed, "lora_rank": rank,
            "lora_alpha": rank, "lora_targets": ["attn2"], "lora_ff": True, "weights_sha256": sha,
            "source": "reference ltx_video/training.py:94-166 train_step via oracle/shim, peft "
                      "get_peft_model on attn2 to_q / to_k / to_v / to_out.0 and ff.net.0.proj / ff.net.2; "
                      "out. / grad. from the bf16 model, out32. / grad32. from the same weights in fp32 on "
                      "the same t and noise"}
    G._save(NAME, tensors, meta)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
