"""Generate tests/golden/tiny_lora_dropout_step.{safetensors,json}: the reference's train step with
peft adapters on attn1, attn2 and both feed-forward linears under LoRA dropout (p = 0.25, a fixed
64-bit key), run twice on the same draws: once in bf16 and once with the model in fp32.

TEST INFRASTRUCTURE, in the style of tools/gen_golden_lora_ff.py: it runs only where the reference
checkout exists, puts the test-only shim (oracle/shim) ahead of it and imports the reference modules
UNMODIFIED. peft computes base(x) + s B(A(dropout(x))) with a torch.nn.Dropout per wrapped linear; this
project's mask is its own counter-based stream (DESIGN.md "LoRA dropout"), so the tool states peft's
lora_A(dropout(x)) with that mask: each wrapped module's lora_A["default"] is replaced by an nn.Linear
subclass defined here (same parameter, same name) that multiplies its input by c * keep, with keep =
ltx_amd.lora.lora_dropout_mask_reference(key, sid, rows, K, p) over the flattened rows the adapter
sees (b N + n on the token side, b L + l on the text side) and sid = lora_dropout_stream(name).
Everything else is gen_golden_lora_ff's: the same batch, the fp32 run on the bf16 run's t and noise.
Only data is written (sample, loss, v_target and every trainable gradient of both runs; the inputs, t
and noise are bitwise those of tests/golden/tiny_lora_ff_step and are read from there); the weights are re-drawn from oracle/params.py (seed recorded) and pinned by a SHA-256.

    python tools/gen_golden_lora_dropout.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import gen_golden as G  # noqa: E402  (sets up the shim + reference import paths)
import torch  # noqa: E402
from peft import LoraConfig, get_peft_model  # noqa: E402  (oracle/shim)

sys.path.insert(0, os.path.join(REPO, "video-generation-for-human-avatars_amd"))
from ltx_amd.lora import LORA_DROPOUT_SLOTS, lora_dropout_mask_reference, lora_dropout_stream  # noqa: E402
from ltx_amd.ops import lora_dropout_threshold  # noqa: E402

NAME = "tiny_lora_dropout_step"
INPUTS_FROM = "tiny_lora_ff_step"  # in.*, out.noise and out.t are read from that fixture
P_DROP = 0.25
KEY = 0x5EEDC0DE0DDBA11


class MaskedLoraA(torch.nn.Linear):
    """lora_A(dropout(x)) under this project's mask: x * (c * keep) before the product."""

    def bind(self, key, sid, p):
        self.key, self.sid, self.p = key, sid, p
        self.c = lora_dropout_threshold(p)[1]
        self.seen = []
        return self

    def forward(self, x):
        K = x.shape[-1]
        rows = x.numel() // K
        keep = torch.from_numpy(lora_dropout_mask_reference(self.key, self.sid, rows, K, self.p))
        self.seen.append((rows, K))
        scale = keep.to(x.dtype) * torch.tensor(self.c, dtype=torch.float32).to(x.dtype)
        return super().forward(x * scale.view(x.shape))


def build(seed, rank, fp32):
    pf = G.SymmetricPatchifier(patch_size=1)
    model = G.Transformer3DModel.from_config(G.TINY_CONFIG)
    model.patchifier = pf
    G.P.init_module_(model, seed, dtype=torch.bfloat16)
    n = len(model.transformer_blocks)
    targets = [f"transformer_blocks.{i}.{s}" for i in range(n) for s in LORA_DROPOUT_SLOTS]
    model = get_peft_model(model, LoraConfig(r=rank, lora_alpha=rank, target_modules=targets,
                                             lora_dropout=0.0, bias="none"))
    for name, p in model.named_parameters():  # training.py:69-73
        p.requires_grad = ("lora_" in name) or ("caption_projection" in name)
    G.P.init_module_(model, seed, dtype=torch.bfloat16)  # the adapters now exist: A / B per params.py
    masked = []
    for name, mod in list(model.named_modules()):
        if hasattr(mod, "lora_A") and hasattr(mod, "base_layer"):
            old = mod.lora_A["default"]
            new = MaskedLoraA(old.in_features, old.out_features, bias=False).bind(KEY, lora_dropout_stream(name), P_DROP)
            new.weight = old.weight  # the same parameter under the same name
            mod.lora_A["default"] = new
            masked.append(new)
    assert len(masked) == len(targets)
    if fp32:  # the same bf16 weight values, computed with in fp32
        model = model.to(torch.float32)
    return model, pf, masked


def main():
    seed, train_seed, rank, B = 4242, 1717, 8, 2
    g = torch.Generator().manual_seed(61)
    # the draws of tiny_lora_ff_step, stored as the bf16 values the bf16 model computes with
    batch = {"latents": torch.randn(B, 128, 2, 8, 8, generator=g).bfloat16(),
             "ref_image_latents": torch.randn(B, 128, 1, 8, 8, generator=g).bfloat16(),
             "pose_latents": torch.randn(B, 128, 2, 8, 8, generator=g).bfloat16()}
    prompt = torch.randn(1, 4, 64, generator=g).bfloat16()
    mask = torch.tensor([[1, 1, 1, 0]], dtype=torch.long)
    model, pf, masked = build(seed, rank, fp32=False)
    cap = G._capture_train_step(model, pf, batch, prompt, mask, seed=train_seed, rank=rank)
    grads = G._grads(model)
    sha = G.P.weights_sha256(model)
    assert all(len(m.seen) == 1 for m in masked), [m.seen for m in masked]  # one forward, no recompute
    rows = sorted({m.seen[0] for m in masked})

    model32, pf32, _ = build(seed, rank, fp32=True)
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
    lora = [k for k in grads if "lora_" in k]
    assert len(lora) == 2 * 10 * 2 and all(float(grads[k].abs().max()) > 0 for k in lora)

    # the inputs and the draws are those of tiny_lora_ff_step (the same batch generator and train seed):
    # checked here and not stored again, which keeps this fixture under 1 MiB
    from safetensors.torch import load_file
    shared = load_file(os.path.join(G.OUT, INPUTS_FROM + ".safetensors"))
    same = {f"in.{k}": v for k, v in batch.items()}
    same.update({"in.prompt_embeds": prompt, "in.prompt_attention_mask": mask, "out.noise": cap["noise"],
                 "out.t": cap["t"]})
    for k, v in same.items():
        assert shared[k].dtype == v.dtype and torch.equal(shared[k], v), k
    tensors = {}
    for k in ("sample", "loss", "v_target"):
        tensors[f"out.{k}"] = cap[k]
    for k in ("sample", "loss"):
        tensors[f"out32.{k}"] = cap32[k]
    for k, v in grads.items():
        tensors[f"grad.{k}"] = v
    for k, v in grads32.items():
        tensors[f"grad32.{k}"] = v
    meta = {"config": G.TINY_CONFIG, "param_seed": seed, "train_seed": train_seed, "lora_rank": rank,
            "lora_alpha": rank, "lora_targets": ["attn1", "attn2"], "lora_ff": True, "lora_dropout": P_DROP,
            "lora_dropout_key": KEY, "inputs_from": INPUTS_FROM, "adapter_input_shapes": [list(r) for r in rows], "weights_sha256": sha,
            "source": "reference ltx_video/training.py:94-166 train_step via oracle/shim, peft get_peft_model on "
                      "the four projections of attn1 and attn2 and ff.net.0.proj / ff.net.2, each lora_A fed "
                      "c * keep * x with keep = ltx_amd.lora.lora_dropout_mask_reference(key, sid, rows, K, p); "
                      "out. / grad. from the bf16 model, out32. / grad32. from the same weights in fp32 on the "
                      "same t, noise and masks"}
    G._save(NAME, tensors, meta)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
