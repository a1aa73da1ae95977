"""Generate tests/golden/tiny_lora_dora_step.{safetensors,json}: the reference's train step with peft
DoRA adapters (use_dora, lora_dropout = 0) on the four attn2 projections of every block, run twice on
the same draws: once in bf16 and once with the model in fp32.

TEST INFRASTRUCTURE, in the style of tools/gen_golden_lora_dropout.py: it runs only where the reference
checkout exists, puts the test-only shim (oracle/shim) ahead of it and imports the reference modules
UNMODIFIED. The shim's peft has no DoRA, so the tool states peft 0.17.1's DoRA forward
(lora.Linear.forward with use_dora + DoraLinearLayer.forward / get_weight_norm) in a subclass of the
shim's LoraLinear defined here; each wrapped module becomes that subclass and gains the parameter
`lora_magnitude_vector.default.weight`:

    result = base_layer(x)                                   # bf16 in the bf16 run, bias included
    x      = x.to(lora_A.weight.dtype)                       # fp32 adapters
    V      = W.to(x.dtype) + scaling * lora_B(lora_A(eye)).T # lora_weight detached
    norm   = linalg.norm(V, dim=1).detach()
    c      = (m / norm).view(1, -1)
    result = result + (c - 1) * (result - bias) + c * lora_B(lora_A(x)) * scaling
    return result.to(result_dtype)

A and B come from oracle/params.py (non-zero B); the magnitudes are m = norm * (1 + 0.2 * seeded randn),
norm the torch statement above, and are STORED in the fixture (with m = norm, c = 1 and a test could
not see a wrong c). Everything else is gen_golden_lora_dropout's: the batch, t and noise are bitwise
those of tests/golden/tiny_lora_ff_step and are read from there by the tests; the fp32 run reuses the
bf16 run's t and noise. Only data is written: sample, loss, v_target, every trainable gradient of both
runs and the magnitudes; the other weights are re-drawn from oracle/params.py (seed recorded) and
pinned, magnitudes included, by a SHA-256.

    python tools/gen_golden_lora_dora.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import gen_golden as G  # noqa: E402  (sets up the shim + reference import paths)
import peft  # noqa: E402  (oracle/shim)
import torch  # noqa: E402
from peft import LoraConfig, get_peft_model  # noqa: E402

NAME = "tiny_lora_dora_step"
INPUTS_FROM = "tiny_lora_ff_step"  # in.*, out.noise and out.t are read from that fixture
MAG_SEED = 2718
PROJECTIONS = ("to_q", "to_k", "to_v", "to_out.0")


class Magnitude(torch.nn.Module):
    def __init__(self, weight):
        super().__init__()
        self.weight = torch.nn.Parameter(weight, requires_grad=True)


class DoraLinear(peft.LoraLinear):
    """peft 0.17.1 lora.Linear.forward with use_dora=True and an Identity dropout (module docstring)."""

    def weight_norm(self, dtype):
        lora_A, lora_B = self.lora_A["default"], self.lora_B["default"]
        x_eye = torch.eye(lora_A.weight.shape[1], dtype=dtype)
        lora_weight = lora_B(lora_A(x_eye)).T.detach()
        weight = self.base_layer.weight.to(dtype) + self.scaling * lora_weight
        return torch.linalg.norm(weight, dim=1).to(weight.dtype).detach()

    def forward(self, x, *args, **kwargs):
        result = self.base_layer(x, *args, **kwargs)
        result_dtype = result.dtype
        lora_A, lora_B = self.lora_A["default"], self.lora_B["default"]
        x = x.to(lora_A.weight.dtype)
        magnitude = self.lora_magnitude_vector["default"].weight
        mag_norm_scale = (magnitude / self.weight_norm(x.dtype)).view(1, -1)
        base_result = result - self.base_layer.bias
        result = result + ((mag_norm_scale - 1) * base_result + mag_norm_scale * lora_B(lora_A(x)) * self.scaling)
        return result.to(result_dtype)


def magnitudes(model):
    """{canonical name: m} = norm * (1 + 0.2 randn), one seeded generator per name (order-free)."""
    out = {}
    for name, mod in model.named_modules():
        if isinstance(mod, peft.LoraLinear):
            canon = G.P.canonical_name(name + ".lora_magnitude_vector.default.weight")
            g = G.P._gen(MAG_SEED, canon)
            with torch.no_grad():
                norm = DoraLinear.weight_norm(mod, torch.float32)
            out[canon] = (norm * (1.0 + 0.2 * torch.randn(norm.shape, generator=g))).float()
    return out


def build(seed, rank, fp32, mags=None):
    pf = G.SymmetricPatchifier(patch_size=1)
    model = G.Transformer3DModel.from_config(G.TINY_CONFIG)
    model.patchifier = pf
    G.P.init_module_(model, seed, dtype=torch.bfloat16)
    n = len(model.transformer_blocks)
    targets = [f"transformer_blocks.{i}.attn2.{p}" for i in range(n) for p in PROJECTIONS]  # training.py:52-60
    model = get_peft_model(model, LoraConfig(r=rank, lora_alpha=rank, target_modules=targets,
                                             lora_dropout=0.0, bias="none"))
    G.P.init_module_(model, seed, dtype=torch.bfloat16)  # the adapters now exist: A / B per params.py
    mags = magnitudes(model) if mags is None else mags
    wrapped = 0
    for name, mod in list(model.named_modules()):
        if isinstance(mod, peft.LoraLinear):
            mod.__class__ = DoraLinear
            canon = G.P.canonical_name(name + ".lora_magnitude_vector.default.weight")
            mod.lora_magnitude_vector = torch.nn.ModuleDict({"default": Magnitude(mags[canon].clone())})
            wrapped += 1
    assert wrapped == len(targets) == len(mags)
    for name, p in model.named_parameters():  # training.py:69-73
        p.requires_grad = ("lora_" in name) or ("caption_projection" in name)
    if fp32:  # the same bf16 weight values, computed with in fp32
        model = model.to(torch.float32)
    return model, pf, mags


def main():
    seed, train_seed, rank, B = 4242, 1717, 8, 2
    g = torch.Generator().manual_seed(61)
    # the draws of tiny_lora_ff_step, stored as the bf16 values the bf16 model computes with
    batch = {"latents": torch.randn(B, 128, 2, 8, 8, generator=g).bfloat16(),
             "ref_image_latents": torch.randn(B, 128, 1, 8, 8, generator=g).bfloat16(),
             "pose_latents": torch.randn(B, 128, 2, 8, 8, generator=g).bfloat16()}
    prompt = torch.randn(1, 4, 64, generator=g).bfloat16()
    mask = torch.tensor([[1, 1, 1, 0]], dtype=torch.long)
    model, pf, mags = build(seed, rank, fp32=False)
    cap = G._capture_train_step(model, pf, batch, prompt, mask, seed=train_seed, rank=rank)
    grads = G._grads(model)
    sha = G.P.weights_sha256(model)

    model32, pf32, _ = build(seed, rank, fp32=True, mags=mags)
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
    n_mag = len([k for k in lora if "lora_magnitude_vector" in k])
    assert len(lora) == 2 * 4 * 3 and n_mag == 8 and all(float(grads[k].abs().max()) > 0 for k in lora)

    # the inputs and the draws are those of tiny_lora_ff_step (the same batch generator and train seed):
    # checked here and not stored again
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
    for k, v in mags.items():
        tensors[f"w.{k}"] = v
    meta = {"config": G.TINY_CONFIG, "param_seed": seed, "train_seed": train_seed, "lora_rank": rank,
            "lora_alpha": rank, "lora_targets": ["attn2"], "use_dora": True, "magnitude_seed": MAG_SEED,
            "inputs_from": INPUTS_FROM, "weights_sha256": sha,
            "source": "reference ltx_video/training.py:94-166 train_step via oracle/shim, peft get_peft_model on "
                      "the four attn2 projections, each wrapped module given peft 0.17.1's DoRA forward "
                      "(tools/gen_golden_lora_dora.py DoraLinear) and the magnitude w.<name> = norm * (1 + 0.2 "
                      "randn); out. / grad. from the bf16 model, out32. / grad32. from the same weights in fp32 "
                      "on the same t and noise"}
    G._save(NAME, tensors, meta)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
