"""Adapter checkpoints, resume and the validation epoch on the MI355X. Every comparison is bitwise:
the kernels, their inputs and the reduction orders are the same on both sides, so nothing but equality
is expected (the same ground as test_train_steps_are_bitwise_reproducible).

  * a run resumed from adapter_epoch_1 is the uninterrupted run: parameters, AdamW moments and steps,
    and the logged losses of epoch 2 -- for plain attn2 adapters, for attn1 + attn2 + ff under dropout
    with accumulation (the CPU generator's key stream must survive), for DoRA, and with a validation
    pass between the epochs (the device generator's state is taken after it);
  * load_adapter_checkpoint into a model whose weight-derived caches are warm with other values;
  * the loaded adapters merge to the merged checkpoint train_loop wrote at that epoch;
  * validate_epoch: the forward-only train step over the loader, nothing else touched.

The shape is the tiny config of test_train_loop_writes_reference_checkpoints: 2 layers, D = 128,
4 clips of [1, 128, 2, 8, 8], batch 2, a 4-token prompt."""
import json
import os
import shutil

import pytest
import torch
from safetensors.torch import load_file

import ltx_oracle as O
from lora_ff_utils import ff_params
from params import canonical_name

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
R = 8
SEED = 77
MAG = ".lora_magnitude_vector.default.weight"
# name -> (config attributes, gradient_accumulation_steps)
CASES = {"attn2": ({}, 1),
         "all_dropout_accum2": ({"lora_targets": "attn1+attn2", "lora_ff": True, "lora_dropout": 0.1}, 2),
         "dora": ({"use_dora": True}, 1)}


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """The tiny config, its parameters (adapters for every target, non-zero B), the prompt, and the
    training (4 clips) and validation (2 clips) latents on disk."""
    from ltx_amd import io
    with open(os.path.join(GOLD, "tiny_train_step.json")) as f:
        meta = json.load(f)
    d = load_file(os.path.join(GOLD, "tiny_train_step.safetensors"))
    root = tmp_path_factory.mktemp("latents")
    g = torch.Generator().manual_seed(0)
    dirs = {}
    for split, n in (("train", 4), ("val", 2)):
        enc, cond = root / split / "enc", root / split / "cond"
        enc.mkdir(parents=True)
        cond.mkdir()
        for i in range(n):
            io.save_latents_pt(torch.randn(1, 128, 2, 8, 8, generator=g), enc / f"clip{i}.pt")
            io.save_latents_pt(torch.randn(1, 128, 2, 8, 8, generator=g), cond / f"clip{i}.pt")
            io.save_latents_pt(torch.randn(1, 128, 1, 8, 8, generator=g), cond / f"clip{i}_ref.pt")
        dirs[split] = io.LatentPairDataset(str(cond), str(enc))
    return {"cfg": meta["config"], "params": ff_params(meta["config"], meta["param_seed"], R, ("attn1", "attn2")),
            "prompt": d["in.prompt_embeds"].to(DEV), "mask": d["in.prompt_attention_mask"].to(DEV), "ds": dirs}


def _config(extra, **kw):
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="-", lora_rank=R, lora_alpha=R, **kw)
    tc.train_mode = "lora_audio"  # set by the CLI in the reference (training.py:497-505)
    for k, v in extra.items():
        setattr(tc, k, v)
    return tc


def _build(tiny, extra, adapters=True):
    """tests/model_utils.build_model under the config attributes of `extra` (adapters=False: the bare
    model); a DoRA magnitude is the row norm scaled away from c = 1."""
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.patchifier import SymmetricPatchifier
    from ltx_amd.transformer3d import Transformer3DModel, dora_weight_norm
    params = tiny["params"]
    with torch.device("meta"):
        m = Transformer3DModel.from_config(tiny["cfg"])
        if adapters:
            apply_training_strategy(m, _config(extra), "lora_audio")
    sd = {}
    for name, _ in m.named_parameters():
        k = canonical_name(name)
        if k.endswith(MAG):
            pre = k[:-len(MAG)]
            sd[name] = (1.25 * dora_weight_norm(params[pre + ".weight"], params[pre + ".lora_A.default.weight"],
                                                params[pre + ".lora_B.default.weight"], 1.0)).to(DEV)
        else:
            sd[name] = params[k].detach().to(DEV).clone()
    m.load_state_dict(sd, assign=True, strict=True)
    for n, p in m.named_parameters():
        p.requires_grad_(adapters and (("lora_" in n) or ("caption_projection" in n)))
    m.patchifier = SymmetricPatchifier(1)
    return m


def _run(tiny, case, out, epochs, val=False, save=False, resume=None):
    """train_loop on fresh model / loader objects under torch.manual_seed(SEED): (model, the
    optimizer train_loop built, logs)."""
    from ltx_amd import io, training
    extra, accum = CASES[case]
    made = []

    class Recording(training.FusedAdamW):  # train_loop keeps its optimizer to itself
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(training, "FusedAdamW", Recording)
        model = _build(tiny, extra)
        loader = io.LatentLoader(tiny["ds"]["train"], 2, DEV, shuffle=True, seed=1)
        vloader = io.LatentLoader(tiny["ds"]["val"], 2, DEV, shuffle=False) if val else None
        tc = _config(extra, learning_rate=1e-3, num_epochs=epochs, gradient_accumulation_steps=accum,
                     output_dir=str(out), save_every_n_epochs=1)
        if save:
            tc.save_adapters = True
        logs = []
        torch.manual_seed(SEED)
        training.train_loop(model, tc, loader, tiny["prompt"], tiny["mask"], log_fn=lambda p, s: logs.append((s, p)),
                            val_dataloader=vloader, resume_from=resume)
    return model, made[0], logs


_FIRST = {}


def _first_epoch(tiny, tmp_path_factory, case, val=False):
    """One epoch with save_adapters, run once per (case, val) and left unchanged: its output directory."""
    key = (case, val)
    if key not in _FIRST:
        out = tmp_path_factory.mktemp("first") / "out"
        _run(tiny, case, out, 1, val=val, save=True)
        _FIRST[key] = out
    return _FIRST[key]


def _state(model, opt):
    names = {id(p): n for n, p in model.named_parameters()}
    params = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    moments, steps = {}, {}
    for p, st in opt.state.items():
        n = names[id(p)]
        moments["exp_avg." + n], moments["exp_avg_sq." + n], steps[n] = st["exp_avg"], st["exp_avg_sq"], st["step"]
    return params, moments, steps


def _same(a, b):
    assert sorted(a) == sorted(b) and len(a) > 0
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------
# resume
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,val", [("attn2", False), ("all_dropout_accum2", False), ("dora", False),
                                      ("attn2", True)])
def test_resumed_run_is_bitwise_the_uninterrupted_run(tiny, tmp_path_factory, tmp_path, case, val):
    # run A: two epochs in one go
    model_a, opt_a, logs_a = _run(tiny, case, tmp_path / "a", 2, val=val)
    # run B: one epoch with save_adapters, then fresh objects resumed from its directory
    out_b = tmp_path / "b"
    shutil.copytree(_first_epoch(tiny, tmp_path_factory, case, val), out_b)
    assert sorted(os.listdir(out_b)) == ["adapter_epoch_1", "best_model_epoch_1.safetensors"]
    assert sorted(os.listdir(out_b / "adapter_epoch_1")) == ["adapter_config.json", "adapter_model.safetensors",
                                                             "optimizer.safetensors", "train_state.json"]
    model_b, opt_b, logs_b = _run(tiny, case, out_b, 2, val=val, resume="auto")
    (pa, ma, sa), (pb, mb, sb) = _state(model_a, opt_a), _state(model_b, opt_b)
    _same(pa, pb)
    _same(ma, mb)
    per_epoch = 2 // CASES[case][1]
    assert sa == sb and set(sa.values()) == {2 * per_epoch} and len(sa) == len(pa)
    epoch2 = lambda logs, key: [(s, p[key]) for s, p in logs if key in p and p.get("train/epoch", 1) == 1]
    for key in ("train/loss", "train/rel_mse", "train/nrmse", "train/epoch_loss"):
        assert epoch2(logs_a, key)[-len(epoch2(logs_b, key)):] == epoch2(logs_b, key), key
    assert [s for s, _ in epoch2(logs_b, "train/loss")] == list(range(per_epoch + 1, 2 * per_epoch + 1))
    assert len(epoch2(logs_a, "train/loss")) == len(epoch2(logs_b, "train/loss")) == per_epoch
    assert not any(p.get("train/epoch") == 0 for _, p in logs_b)  # the resumed run starts at the second epoch
    if val:
        va = [(s, p["val/loss"], p["val/epoch"]) for s, p in logs_a if "val/loss" in p]
        vb = [(s, p["val/loss"], p["val/epoch"]) for s, p in logs_b if "val/loss" in p]
        assert len(va) == 2 and va[1:] == vb and vb[0][2] == 1
    # the resumed run wrote epoch 2's merged checkpoint, and the run moved
    assert (out_b / "best_model_epoch_2.safetensors").exists()
    first = load_file(str(out_b / "adapter_epoch_1" / "adapter_model.safetensors"))
    key = "base_model.model.transformer_blocks.0.attn2.to_q.lora_A.weight"
    assert not torch.equal(first[key].to(DEV), pb["transformer_blocks.0.attn2.to_q.lora_A.default.weight"])


def test_resume_auto_without_a_checkpoint_starts_from_scratch(tiny, tmp_path):
    _, opt, logs = _run(tiny, "attn2", tmp_path / "out", 1, resume="auto")
    assert [s for s, p in logs if "train/loss" in p] == [1, 2]
    assert sorted(os.listdir(tmp_path / "out")) == ["best_model_epoch_1.safetensors"]  # save_adapters is off


# ---------------------------------------------------------------------------------------------
# load into live models
# ---------------------------------------------------------------------------------------------
def _fixed_inputs(tiny):
    g = torch.Generator(device=DEV).manual_seed(5)
    item = [tiny["ds"]["train"][i] for i in (0, 1)]
    batch = {k: torch.stack([b[k] for b in item]).to(DEV) for k in ("latents", "pose_latents", "ref_image_latents")}
    t = torch.rand(2, generator=g, device=DEV) * 0.9 + 0.05
    noise = torch.randn(2, 2 * 8 * 8, 128, generator=g, device=DEV).bfloat16()
    return batch, t, noise


def _forward_and_grads(tiny, model, batch, t, noise):
    """(eval / no_grad sample, f32 mse and gradients of one training step) on fixed t and noise"""
    from ltx_amd.scheduler import RectifiedFlowScheduler
    from ltx_amd.training import train_step
    tok, coords = O.patchify(batch["latents"].bfloat16())
    x = O.add_noise(tok, noise, t).bfloat16()
    model.eval()
    with torch.no_grad():
        sample = model(hidden_states=x, indices_grid=coords.to(DEV),
                       ref_image_hidden_states=batch["ref_image_latents"].bfloat16(),
                       pose_hidden_states=batch["pose_latents"].bfloat16(),
                       encoder_hidden_states=tiny["prompt"].bfloat16().expand(2, -1, -1), timestep=t,
                       encoder_attention_mask=tiny["mask"].expand(2, -1)).sample
    model.train()
    model.lora_dropout_key = 5
    for p in model.parameters():
        p.grad = None
    _, _, _, ld = train_step(model, batch, RectifiedFlowScheduler(), model.patchifier, _config({}), tiny["prompt"],
                             tiny["mask"], t=t, noise=noise)
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad}
    return sample, ld["_mse_f32"].clone(), grads


@pytest.mark.parametrize("case", list(CASES))
def test_load_into_a_trained_model_leaves_no_stale_pack(tiny, tmp_path_factory, case):
    """A model that has run a step (its splits, pieces, QKV / text packs and DoRA W_eff are built) and
    then moved to other adapter values is loaded in place: its next forward and backward are a fresh
    model's loaded from the same directory."""
    from ltx_amd import io
    from ltx_amd.training import FusedAdamW
    ckpt = _first_epoch(tiny, tmp_path_factory, case) / "adapter_epoch_1"
    batch, t, noise = _fixed_inputs(tiny)
    live = _build(tiny, CASES[case][0])
    opt = FusedAdamW([p for p in live.parameters() if p.requires_grad], lr=1e-2)
    before = _forward_and_grads(tiny, live, batch, t, noise)
    opt.step()  # other values, and caches warm with them after the next forward
    stale = _forward_and_grads(tiny, live, batch, t, noise)
    assert not torch.equal(stale[0], before[0])
    io.load_adapter_checkpoint(live, str(ckpt))
    got = _forward_and_grads(tiny, live, batch, t, noise)
    fresh = _build(tiny, CASES[case][0])
    io.load_adapter_checkpoint(fresh, str(ckpt))
    want = _forward_and_grads(tiny, fresh, batch, t, noise)
    assert torch.equal(got[0], want[0]) and not torch.equal(got[0], stale[0])
    assert torch.equal(got[1], want[1])
    _same(got[2], want[2])
    # ... and a bare model that gets its adapters from adapter_config.json computes the same
    bare = _build(tiny, {}, adapters=False)
    io.load_adapter_checkpoint(bare, str(ckpt))
    out = _forward_and_grads(tiny, bare, batch, t, noise)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    _same(out[2], want[2])


@pytest.mark.parametrize("case", list(CASES))
def test_loaded_adapters_merge_to_the_checkpoint_train_loop_wrote(tiny, tmp_path_factory, case):
    """unload_lora after load_adapter_checkpoint into a bare model holds bitwise the tensors of
    best_model_epoch_1.safetensors. The bare model is on the CPU, where train_loop's export merges
    (io.merged_state_dict_cpu): the same arithmetic on the same values."""
    from ltx_amd import io
    from ltx_amd.lora import unload_lora
    from ltx_amd.transformer3d import LoraLinear
    out = _first_epoch(tiny, tmp_path_factory, case)
    bare = _build(tiny, {}, adapters=False).to("cpu")
    io.load_adapter_checkpoint(bare, str(out / "adapter_epoch_1"))
    assert any(isinstance(m, LoraLinear) for m in bare.modules())
    unload_lora(bare)
    assert not any(isinstance(m, LoraLinear) for m in bare.modules())
    _same({k: v.detach() for k, v in bare.state_dict().items()}, load_file(str(out / "best_model_epoch_1.safetensors")))


# ---------------------------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------------------------
def _validate(tiny, model, tc, seed=SEED):
    from ltx_amd import io
    from ltx_amd.scheduler import RectifiedFlowScheduler
    from ltx_amd.validation import validate_epoch
    loader = io.LatentLoader(tiny["ds"]["train"], 2, DEV, shuffle=False)
    torch.manual_seed(seed)
    return validate_epoch(model, loader, RectifiedFlowScheduler(), model.patchifier, tc, tiny["prompt"],
                          tiny["mask"], DEV)


def test_validate_epoch_is_the_forward_only_train_step(tiny):
    from ltx_amd import io
    from ltx_amd.scheduler import RectifiedFlowScheduler
    from ltx_amd.training import train_step
    model = _build(tiny, {})
    model.train()
    tc = _config({})
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    got = _validate(tiny, model, tc)
    assert isinstance(got, float) and got > 0
    assert model.training is False and all(not m.training for m in model.modules())
    assert all(p.grad is None for p in model.parameters())
    _same({n: p.detach() for n, p in model.named_parameters()}, before)
    loader = io.LatentLoader(tiny["ds"]["train"], 2, DEV, shuffle=False)
    assert len(loader) == 2
    torch.manual_seed(SEED)
    losses = []
    with torch.no_grad():
        for batch in loader:
            loss, _, _, _ = train_step(model, batch, RectifiedFlowScheduler(), model.patchifier, tc, tiny["prompt"],
                                       tiny["mask"], DEV, backward=False)
            losses.append(float(loss))
    assert got == sum(losses) / len(losses) and losses[0] != losses[1]
    assert _validate(tiny, model, tc, seed=SEED + 1) != got  # it draws t and noise from the device generator
    # transformer_loss_weight is not applied (validation.py:91)
    tc2 = _config({}, transformer_loss_weight=2.0)
    assert _validate(tiny, model, tc2) == got


def test_validate_epoch_under_dropout_is_the_p0_model(tiny):
    extra = dict(CASES["all_dropout_accum2"][0])
    dropped = _build(tiny, extra)
    plain = _build(tiny, dict(extra, lora_dropout=0.0))
    dropped.train()
    plain.train()
    torch.manual_seed(SEED)
    cpu_rng = torch.get_rng_state()
    a = _validate(tiny, dropped, _config(extra))
    # no mask key was drawn: the CPU generator is where _validate's torch.manual_seed(SEED) left it
    assert torch.equal(torch.get_rng_state(), cpu_rng)
    assert a == _validate(tiny, plain, _config(extra))


def test_train_loop_logs_one_val_loss_per_epoch(tiny, tmp_path):
    model, _, logs = _run(tiny, "attn2", tmp_path / "out", 2, val=True)
    val = [(s, p) for s, p in logs if "val/loss" in p]
    assert [s for s, _ in val] == [2, 4] and [p["val/epoch"] for _, p in val] == [0, 1]
    assert all(set(p) == {"val/loss", "val/epoch"} and isinstance(p["val/loss"], float) and p["val/loss"] > 0
               for _, p in val)
    # the reference's order within an epoch: the steps, the validation pass, the epoch loss
    kinds = ["val" if "val/loss" in p else "epoch" if "train/epoch_loss" in p else "step" for _, p in logs]
    assert kinds == ["step", "step", "val", "epoch"] * 2
    assert model.training is False  # left in eval mode by the last validation pass, as the reference
