"""On-disk formats around the training step.

* Precomputed latents: ``{stem}.pt`` = {"latents": Tensor[1,128,F,H,W]} in the encoder dir, the
  pose-frame latents ``{stem}.pt`` and the reference-image latent ``{stem}_ref.pt`` in the
  condition dir (ltx_video/dataset.py:5-97, written by save_vae_latents.py /
  save_condition_encoder_latents.py). LatentPairDataset / collate_latent_pairs keep the
  reference's names, pairing rule and output dict. Files load with torch.load(weights_only=True):
  nothing in a latent file is executed.
* LatentLoader: the DataLoader the MI355X step wants -- rank-strided shard of the dataset per DP
  rank (one process per GPU), pinned host batches and the H2D copy on a side stream one batch
  ahead, so the copy overlaps the previous step's kernels (the timed region of bench.py is
  HBM-resident; this is the data-path for real training).
* Checkpoints: single-file safetensors with metadata["config"] = JSON {"transformer": {...}}
  (+ "scheduler"), as ltx_video/utils/torch_utils.py:39-133 writes them and
  Transformer3DModel.from_pretrained / RectifiedFlowScheduler.from_pretrained read them.
  lora_audio checkpoints export the peft merge (W + (B @ A) * scaling, rounded to the base dtype,
  adapters dropped); full checkpoints save the state dict.
* Adapter checkpoints (save_adapter_checkpoint / load_adapter_checkpoint): a directory of
  safetensors and JSON files only -- the trainable tensors under peft's saved names, peft's
  adapter_config.json, the FusedAdamW moments and the RNG states, and train_state.json, written
  last. What train_loop resumes from; nothing in it is executed on load. With FusedAdamW(ema) also
  ema_model.safetensors, the f32 moving averages of the same tensors, which
  load_adapter_checkpoint(weights="ema") installs as the weights.
"""
import json
import math
import os
import re
import shutil
from pathlib import Path
from typing import Dict, List, Optional

import torch
from torch.utils.data import Dataset


# ---------------------------------------------------------------------------------------------
# latents
# ---------------------------------------------------------------------------------------------
def load_latents_pt(path):
    """{"latents": Tensor} from a precomputed-latent .pt file (no code execution on load)."""
    data = torch.load(path, map_location="cpu", weights_only=True)
    return data["latents"]


def save_latents_pt(latents, path):
    torch.save({"latents": latents.detach().cpu()}, path)


def collate_latent_pairs(batch: List[Dict]):
    """dataset.py:5-44; with the items' "face_bbox" (LatentPairDataset(face_bbox_dir)) also its stack,
    f32 [B, 4]."""
    out = {
        "latents": torch.stack([b["latents"] for b in batch], dim=0),
        "pose_latents": torch.stack([b["pose_latents"] for b in batch], dim=0),
        "ref_image_latents": torch.stack([b["ref_image_latents"] for b in batch], dim=0),
        "stem": [b["stem"] for b in batch],
    }
    if batch and "face_bbox" in batch[0]:
        out["face_bbox"] = torch.stack([b["face_bbox"] for b in batch], dim=0)
    return out


_BBOX_KEYS = ("x_min", "y_min", "x_max", "y_max")


def load_face_bbox(path):
    """f32 [4] (x_min, y_min, x_max, y_max, normalised to the frame) from the `face_bbox` entry of a
    clip's conditioning JSON, as the reference's preprocessing writes it beside every clip
    (preprocessing/save_condition_latents.py:168-191: a dict of the four names). All NaN -- which the
    loss weighting treats as "no box" -- when the file or the key is missing or does not hold the four
    numbers."""
    try:
        with open(path, "r") as f:
            box = json.load(f)["face_bbox"]
        return torch.tensor([float(box[k]) for k in _BBOX_KEYS], dtype=torch.float32)
    except (OSError, ValueError, KeyError, TypeError):
        return torch.full((4,), float("nan"), dtype=torch.float32)


class LatentPairDataset(Dataset):
    """dataset.py:47-97: encoder latents {stem}.pt (not *_ref) paired with the condition dir's
    {stem}.pt (pose) and {stem}_ref.pt (reference image); stems sorted, unpaired ones skipped.

    `face_bbox_dir` (None: the reference's item dict, unchanged): every item also carries "face_bbox",
    load_face_bbox of {face_bbox_dir}/{stem}.json."""

    def __init__(self, condition_latents_dir: str, encoder_latents_dir: str, face_bbox_dir: Optional[str] = None):
        self.condition_dir = Path(condition_latents_dir)
        self.encoder_dir = Path(encoder_latents_dir)
        self.face_bbox_dir = Path(face_bbox_dir) if face_bbox_dir else None
        files = [f for f in sorted(self.encoder_dir.glob("*.pt")) if not f.stem.endswith("_ref")]
        self.items = [f.stem for f in files
                      if (self.condition_dir / f"{f.stem}.pt").exists()
                      and (self.condition_dir / f"{f.stem}_ref.pt").exists()]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, idx):
        stem = self.items[idx]
        latents = load_latents_pt(self.encoder_dir / f"{stem}.pt").squeeze()
        pose = load_latents_pt(self.condition_dir / f"{stem}.pt").squeeze()
        ref = load_latents_pt(self.condition_dir / f"{stem}_ref.pt").squeeze()
        if ref.ndim == 3:
            ref = ref.unsqueeze(1)
        item = {"latents": latents, "pose_latents": pose, "ref_image_latents": ref, "stem": stem}
        if self.face_bbox_dir is not None:
            item["face_bbox"] = load_face_bbox(self.face_bbox_dir / f"{stem}.json")
        return item


class LatentLoader:
    """Rank-strided batches of a LatentPairDataset on `device`, prefetched one batch ahead:
    pinned host collate, then a non-blocking H2D copy on a side stream; the consumer's stream
    waits on it. drop_last like the reference's DataLoader (training.py:586-592 uses shuffle)."""

    def __init__(self, dataset, batch_size, device, rank=0, world_size=1, shuffle=True, seed=0,
                 drop_last=True, dtype=torch.bfloat16):
        self.ds, self.bs, self.device = dataset, batch_size, torch.device(device)
        self.rank, self.world, self.shuffle, self.seed = rank, world_size, shuffle, seed
        self.drop_last, self.dtype, self.epoch = drop_last, dtype, 0
        self.stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _indices(self):
        n = len(self.ds)
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            order = torch.randperm(n, generator=g).tolist()
        else:
            order = list(range(n))
        mine = order[self.rank::self.world]
        nb = len(mine) // self.bs if self.drop_last else -(-len(mine) // self.bs)
        return [mine[i * self.bs:(i + 1) * self.bs] for i in range(nb)]

    def __len__(self):
        return len(self._indices())

    def _host_batch(self, idx):
        b = collate_latent_pairs([self.ds[i] for i in idx])
        for k in ("latents", "pose_latents", "ref_image_latents"):
            t = b[k].to(self.dtype)
            b[k] = t.pin_memory() if self.stream is not None else t
        if "face_bbox" in b and self.stream is not None:
            b["face_bbox"] = b["face_bbox"].pin_memory()  # the box stays f32: it is coordinates, not latents
        return b

    def _to_device(self, hb):
        if self.stream is None:
            return {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in hb.items()}
        with torch.cuda.stream(self.stream):
            db = {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v)
                  for k, v in hb.items()}
        return db

    def __iter__(self):
        batches = self._indices()
        nxt = self._to_device(self._host_batch(batches[0])) if batches else None
        for i in range(len(batches)):
            cur = nxt
            if self.stream is not None:
                torch.cuda.current_stream(self.device).wait_stream(self.stream)
                for v in cur.values():
                    if torch.is_tensor(v):
                        v.record_stream(torch.cuda.current_stream(self.device))
            if i + 1 < len(batches):
                nxt = self._to_device(self._host_batch(batches[i + 1]))
            yield cur


# ---------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------
def _config_dict(module):
    cfg = getattr(module, "config", None)
    if cfg is None:
        return None
    return {k: v for k, v in dict(cfg).items() if not str(k).startswith("_")}


def _string_meta(meta):
    return {str(k): (v if isinstance(v, str) else str(v)) for k, v in meta.items()}


def save_module_safetensors(module, target_path, metadata: Optional[dict] = None):
    """torch_utils.py:39-63: the state dict (CPU) + metadata with an embedded config."""
    from safetensors.torch import save_file
    state = {k: v.detach().cpu().contiguous() for k, v in module.state_dict().items()}
    meta = dict(metadata or {})
    if "config" not in meta:
        cfg = _config_dict(module)
        if cfg is not None:
            meta["config"] = json.dumps({"transformer": cfg})
    save_file(state, target_path, metadata=_string_meta(meta))


def export_merged_safetensors(model, target_path, metadata: Optional[dict] = None):
    """torch_utils.py:66-102: peft merge_and_unload of a copy -> safetensors; the model being
    trained is not modified. The merge runs on CPU f32 tensors (delta = (B @ A) * scaling, then
    the promoted add rounded to the base dtype)."""
    from safetensors.torch import save_file
    state = merged_state_dict_cpu(model)
    meta = dict(metadata or {})
    cfg = _config_dict(model)
    if cfg is not None:
        root = {"transformer": cfg}
        sch = meta.pop("scheduler", None)
        if sch is not None:
            root["scheduler"] = sch
        meta["config"] = json.dumps(root)
    save_file(state, target_path, metadata=_string_meta(meta))


@torch.no_grad()
def merged_state_dict_cpu(model):
    from .transformer3d import LoraLinear
    out, wrapped = {}, []
    for name, mod in model.named_modules():
        if isinstance(mod, LoraLinear):
            wrapped.append(name + ".")
            w = mod.base_layer.weight.detach().cpu()
            a = mod.lora_A["default"].weight.detach().cpu()
            b = mod.lora_B["default"].weight.detach().cpu()
            delta = (b @ a) * mod.scaling
            if mod.use_dora:  # LoraLinear.merged_weight's statement on the CPU copies
                v = w.float() + mod.scaling * (b @ a)
                m = mod.lora_magnitude_vector["default"].weight.detach().cpu()
                merged = ((m / torch.linalg.norm(v, dim=1)).view(-1, 1) * v).to(w.dtype)
            else:
                merged = w.clone()
                merged += delta
            out[name + ".weight"] = merged
            if mod.base_layer.bias is not None:
                out[name + ".bias"] = mod.base_layer.bias.detach().cpu().clone()
    for k, v in model.state_dict().items():
        if not any(k.startswith(p) for p in wrapped):
            out[k] = v.detach().cpu().contiguous()
    return out


def save_training_checkpoint(model, target_path, train_mode, metadata: Optional[dict] = None,
                             is_best=False):
    """torch_utils.py:105-133 (best_ prefix, merged export for lora_audio)."""
    if is_best:
        d, f = os.path.dirname(target_path), os.path.basename(target_path)
        if not f.startswith("best_"):
            f = f"best_{f}"
        target_path = os.path.join(d, f)
    if train_mode == "lora_audio":
        export_merged_safetensors(model, target_path, metadata)
    else:
        save_module_safetensors(model, target_path, metadata)
    return target_path


# ---------------------------------------------------------------------------------------------
# adapter checkpoints
# ---------------------------------------------------------------------------------------------
ADAPTER_FORMAT_VERSION = 1
ADAPTER_WEIGHTS = "adapter_model.safetensors"
ADAPTER_CONFIG = "adapter_config.json"
ADAPTER_OPTIMIZER = "optimizer.safetensors"
ADAPTER_TRAIN_STATE = "train_state.json"
ADAPTER_EMA = "ema_model.safetensors"  # optional: written when the optimizer keeps an EMA
_PEFT_PREFIX = "base_model.model."
_ADAPTER_HOLDERS = ("lora_A", "lora_B", "lora_magnitude_vector")  # ModuleDicts keyed by the adapter name
_ADAPTER_GROUPS = ("attn1", "attn2", "ff")
_GROUP_FIELDS = ("r", "lora_alpha", "scaling", "lora_dropout", "use_dora")
_ADAPTER_DIR = re.compile(r"adapter_epoch_(\d+)$")


def adapter_key(name, to_model=False):
    """The one mapping between this model's parameter names and the keys of adapter_model.safetensors.

    Model -> file: the prefix 'base_model.model.' is put in front, and the adapter name 'default' is
    removed where it is the key of a lora_A / lora_B / lora_magnitude_vector ModuleDict:
      transformer_blocks.0.attn2.to_q.lora_A.default.weight
        -> base_model.model.transformer_blocks.0.attn2.to_q.lora_A.weight
      ....lora_magnitude_vector.default.weight -> base_model.model.....lora_magnitude_vector.weight
      caption_projection.linear_1.weight -> base_model.model.caption_projection.linear_1.weight
    to_model=True is the inverse (ValueError for a key without the prefix).

    This is what peft 0.17.1's get_peft_model_state_dict writes for a LoraConfig model (the keys of
    PeftModel.state_dict() that contain 'lora_', with '.default' removed). It is pinned to peft's
    published behaviour only: peft is not a dependency of this project and the oracle's peft shim has
    no save path, so no test compares against a file peft wrote. The caption_projection keys are an
    extension: peft would not save a trainable base parameter."""
    if to_model:
        if not name.startswith(_PEFT_PREFIX):
            raise ValueError(f"adapter key {name!r}: expected the prefix {_PEFT_PREFIX!r}")
        parts = name[len(_PEFT_PREFIX):].split(".")
        if len(parts) >= 2 and parts[-2] in _ADAPTER_HOLDERS:
            parts.insert(len(parts) - 1, "default")
        return ".".join(parts)
    parts = name.split(".")
    if len(parts) >= 3 and parts[-2] == "default" and parts[-3] in _ADAPTER_HOLDERS:
        del parts[-2]
    return _PEFT_PREFIX + ".".join(parts)


def _adapter_layout(model):
    """(wrapped module names in module order, {group: {r, lora_alpha, scaling, lora_dropout, use_dora}})
    of the model's LoraLinears; the groups are attn1, attn2 and ff. ValueError when the adapters of one
    group differ among themselves (adapter_config.json states one description per group)."""
    from .transformer3d import LoraLinear
    targets, groups = [], {}
    for name, mod in model.named_modules():
        if not isinstance(mod, LoraLinear):
            continue
        parts = name.split(".")
        group = parts[2] if len(parts) > 3 and parts[0] == "transformer_blocks" else None
        if group not in _ADAPTER_GROUPS:
            raise ValueError(f"adapter on {name!r}: expected transformer_blocks.<i>.<{'|'.join(_ADAPTER_GROUPS)}>.*")
        desc = {"r": int(mod.r), "lora_alpha": mod.lora_alpha, "scaling": float(mod.scaling),
                "lora_dropout": float(mod.lora_dropout_p), "use_dora": bool(mod.use_dora)}
        if groups.setdefault(group, desc) != desc:
            raise ValueError(f"adapter on {name!r} is {desc}, the other {group} adapters are {groups[group]}: "
                             f"an adapter checkpoint holds one description per group")
        targets.append(name)
    return targets, groups


def _layout_difference(have, want):
    """The first difference between two _adapter_layout results as a sentence, or None."""
    (have_t, have_g), (want_t, want_g) = have, want
    have_set, want_set = set(have_t), set(want_t)
    for name in want_t:
        if name not in have_set:
            return f"the checkpoint has an adapter on {name}, the model has none"
    for name in have_t:
        if name not in want_set:
            return f"the model has an adapter on {name}, the checkpoint has none"
    for group in _ADAPTER_GROUPS:
        for field in _GROUP_FIELDS:
            a, b = have_g.get(group, {}).get(field), want_g.get(group, {}).get(field)
            if a != b:
                return f"{group} {field}: the model has {a!r}, the checkpoint {b!r}"
    return None


def _dist_rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _model_device(model):
    return next(model.parameters()).device


def _gathered_rng_states(device):
    """{'rng.cpu.rank{r}', 'rng.device.rank{r}': uint8 state} of every rank (a collective when
    torch.distributed is initialised): torch's CPU generator, the source of the LoRA-dropout keys,
    and `device`'s generator (t and noise); no device entry for a CPU model."""
    import torch.distributed as dist
    rank, world = _dist_rank_world()
    mine = {"cpu": torch.get_rng_state()}
    if device.type == "cuda":
        mine["device"] = torch.cuda.get_rng_state(device)
    out = {}
    for kind, t in mine.items():
        if world == 1:
            out[f"rng.{kind}.rank0"] = t.clone()
            continue
        on = device if dist.get_backend() == "nccl" else torch.device("cpu")
        parts = [torch.empty(t.shape, dtype=t.dtype, device=on) for _ in range(world)]
        dist.all_gather(parts, t.to(on))
        for r, p in enumerate(parts):
            out[f"rng.{kind}.rank{r}"] = p.cpu()
    return out


def _plain(v):
    """A hyper-parameter as JSON holds it, or None when it is not a plain value."""
    if isinstance(v, (bool, int, float, str)) or v is None:
        return v
    if isinstance(v, (tuple, list)) and all(isinstance(x, (bool, int, float, str)) for x in v):
        return list(v)
    return None


def _write_json(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")


_PRODIGY_STATE = ("s", "p0")


def _is_guarded(optimizer):
    """an optimizer whose parameter groups carry skip_nonfinite (training.FusedAdamW(skip_nonfinite=True))"""
    return optimizer is not None and any(g.get("skip_nonfinite", False) for g in optimizer.param_groups)


def _is_prodigy(optimizer):
    """training.FusedProdigy (or a subclass), without importing training here"""
    return optimizer is not None and hasattr(optimizer, "RECORD") and hasattr(optimizer, "ensure_record")


def save_adapter_checkpoint(model, path, *, optimizer=None, train_state=None, loader=None,
                            metadata: Optional[dict] = None):
    """Write the adapter checkpoint directory `path` (safetensors and JSON only) and return it:

    * adapter_model.safetensors: every parameter with requires_grad, in its own dtype, under
      adapter_key's names; `metadata` becomes its string metadata;
    * adapter_config.json: peft's LoraConfig fields that apply (r / lora_alpha / lora_dropout /
      use_dora of the attn2 group, or of the first group present; base_model_name_or_path =
      metadata['base_model_name_or_path'] when given) and an 'ltx_amd' block with the format version
      and each group's own rank, alpha, scaling, dropout and DoRA flag;
    * optimizer.safetensors (with `optimizer`): exp_avg.<parameter name> / exp_avg_sq.<parameter name>
      in their stored dtype (f32 for a bf16 parameter under bf16_update="stochastic", whose mode and
      seed train_state.json holds among the hyper-parameters) and every rank's RNG states
      (_gathered_rng_states);
    * ema_model.safetensors (with an `optimizer` that keeps an EMA, FusedAdamW(ema)): the f32 shadow
      of every parameter the optimizer holds under adapter_key's names (the parameter's own value in
      f32 where it has not stepped yet, which is what its shadow starts from); every rank's shadows
      are identical by construction, so nothing is gathered. A directory written without an EMA has
      neither this file nor the "ema" block below;
    * train_state.json, written last: the format version, `train_state`'s epoch / global_step /
      best_loss, the world size, the optimizer's hyper-parameters and per-parameter step,
      `loader`'s seed, and with an EMA the block "ema": the EMASchedule's fields and ema_steps.

    With a training.FusedProdigy optimizer.safetensors also holds s.<parameter name> / p0.<parameter name>
    and train_state.json the block "prodigy": {"hyper": the hyper-parameters (FusedProdigy.hyper()),
    "record": the device record's float64 values as float.hex() strings}. A directory written with another
    optimizer has neither.

    An optimizer that guards (FusedAdamW(skip_nonfinite=True)) is settled first (the last step's outcome is
    waited for, so a skipped step's counters are rolled back before they are read); `skip_nonfinite` is among
    its hyper-parameters and train_state.json gains the block "guard": {"skipped_steps": the count}. A
    directory written without the guard has neither.

    Everything is written under `path`.tmp and moved into place with os.replace, so a checkpoint is
    complete or absent. Under torch.distributed every rank calls this (the RNG states are gathered);
    rank 0 writes."""
    from safetensors.torch import save_file
    path = os.fspath(path)
    rank, world = _dist_rank_world()
    targets, groups = _adapter_layout(model)
    if not targets:
        raise ValueError("save_adapter_checkpoint: the model has no LoRA adapters")
    if getattr(optimizer, "_ema_swapped", None) is not None:
        raise RuntimeError("save_adapter_checkpoint: the optimizer's EMA weights are swapped in; the model "
                           "holds the averages, not the trained weights")
    if hasattr(optimizer, "settle"):
        optimizer.settle()  # every rank: a skipped last step leaves no trace in the host's counters
    # the one collective, before rank 0 goes its own way
    rng = _gathered_rng_states(_model_device(model)) if optimizer is not None else None
    if rank != 0:
        return path
    named = list(model.named_parameters())
    tensors = {adapter_key(n): p.detach().cpu().contiguous() for n, p in named if p.requires_grad}
    state = {"format_version": ADAPTER_FORMAT_VERSION, "epoch": 0, "global_step": 0, "best_loss": None}
    state.update(train_state or {})
    best = state["best_loss"]
    state["best_loss"] = float(best) if best is not None and math.isfinite(best) else None
    state["world_size"] = world
    opt_tensors = None
    if optimizer is not None:
        names = {id(p): n for n, p in named}
        opt_tensors, steps = {}, {}
        for group in optimizer.param_groups:
            for p in group["params"]:
                if id(p) not in names:
                    raise ValueError("save_adapter_checkpoint: the optimizer holds a parameter that is not the model's")
                st = optimizer.state.get(p)
                if st:
                    name = names[id(p)]
                    steps[name] = int(st["step"])
                    opt_tensors["exp_avg." + name] = st["exp_avg"].detach().cpu().contiguous()
                    opt_tensors["exp_avg_sq." + name] = st["exp_avg_sq"].detach().cpu().contiguous()
                    for k in _PRODIGY_STATE:  # FusedProdigy's two further tensors per parameter
                        if k in st:
                            opt_tensors[f"{k}.{name}"] = st[k].detach().cpu().contiguous()
        opt_tensors.update(rng)
        hyper = [{k: _plain(v) for k, v in g.items() if k != "params" and _plain(v) is not None}
                 for g in optimizer.param_groups]
        state["optimizer"] = {"class": type(optimizer).__name__, "param_groups": hyper, "step": steps}
        if _is_prodigy(optimizer):
            record = optimizer.ensure_record(_model_device(model)).tolist()
            state["prodigy"] = {"hyper": optimizer.hyper(),
                                "record": {k: float(v).hex() for k, v in zip(optimizer.RECORD, record)}}
        if _is_guarded(optimizer):
            state["guard"] = {"skipped_steps": int(optimizer.skipped_steps)}
    ema_tensors = None
    schedule = getattr(optimizer, "ema", None)
    if schedule is not None:
        ema_tensors = {}
        for group in optimizer.param_groups:
            for p in group["params"]:
                shadow = (optimizer.state.get(p) or {}).get("ema")
                src = p if shadow is None else shadow
                ema_tensors[adapter_key(names[id(p)])] = src.detach().float().cpu().contiguous()
        state["ema"] = dict(schedule.fields(), ema_steps=int(optimizer.ema_steps))
    if loader is not None and hasattr(loader, "seed"):
        state["loader"] = {"seed": int(loader.seed)}
    meta = dict(metadata or {})
    main = groups.get("attn2") or next(groups[g] for g in _ADAPTER_GROUPS if g in groups)
    config = {"peft_type": "LORA", "base_model_name_or_path": meta.get("base_model_name_or_path"),
              "r": main["r"], "lora_alpha": main["lora_alpha"], "target_modules": targets,
              "lora_dropout": main["lora_dropout"], "use_dora": main["use_dora"], "bias": "none",
              "ltx_amd": {"format_version": ADAPTER_FORMAT_VERSION, "groups": groups}}
    tmp = path.rstrip("/\\") + ".tmp"
    if os.path.isdir(tmp):
        shutil.rmtree(tmp)
    os.makedirs(tmp)
    meta = _string_meta({k: v for k, v in meta.items() if v is not None})
    meta.setdefault("format", "pt")
    save_file(tensors, os.path.join(tmp, ADAPTER_WEIGHTS), metadata=meta)
    _write_json(os.path.join(tmp, ADAPTER_CONFIG), config)
    if opt_tensors is not None:
        save_file(opt_tensors, os.path.join(tmp, ADAPTER_OPTIMIZER))
    if ema_tensors is not None:
        save_file(ema_tensors, os.path.join(tmp, ADAPTER_EMA))
    _write_json(os.path.join(tmp, ADAPTER_TRAIN_STATE), state)
    old = None
    if os.path.isdir(path):  # os.replace does not move onto a directory that has files
        old = path.rstrip("/\\") + ".old"
        if os.path.isdir(old):
            shutil.rmtree(old)
        os.replace(path, old)
    os.replace(tmp, path)
    if old is not None:
        shutil.rmtree(old)
    return path


def _inject_from_config(model, targets, groups):
    """inject_lora per group of an adapter_config.json into a model without adapters, then the
    lora_audio trainable set (lora.apply_training_strategy's rule)."""
    from .lora import inject_lora
    for group in _ADAPTER_GROUPS:
        if group not in groups:
            continue
        d = groups[group]
        names = [t for t in targets if t.split(".")[2] == group]
        inject_lora(model, names, d["r"], d["lora_alpha"], feed_forward=(group == "ff"),
                    dropout=d["lora_dropout"], dora=d["use_dora"])
    for n, p in model.named_parameters():
        p.requires_grad = ("lora_" in n) or ("caption_projection" in n)


def _remove_adapters(model, requires_grad):
    """Undo _inject_from_config after a refusal: every LoraLinear back to its base linear (no merge),
    requires_grad as recorded."""
    from .transformer3d import LoraLinear
    for name, mod in list(model.named_modules()):
        if isinstance(mod, LoraLinear):
            parent_name, _, child = name.rpartition(".")
            parent = model.get_submodule(parent_name)
            if child.isdigit():
                parent[int(child)] = mod.base_layer
            else:
                setattr(parent, child, mod.base_layer)
    for p in model.parameters():
        p.requires_grad = requires_grad[id(p)]


def _read_json(path):
    with open(path) as f:
        return json.load(f)


def load_adapter_checkpoint(model, path, *, optimizer=None, loader=None, strict=True, weights="raw"):
    """Restore the directory save_adapter_checkpoint wrote and return its train_state dict
    (best_loss = inf when none was recorded).

    A model without adapters first gets them from adapter_config.json through lora.inject_lora (rank,
    alpha, targets, feed_forward, dropout and dora per group, so every refusal of inject_lora
    applies) and the lora_audio trainable set. A model with adapters must match the file: wrapped
    set, ranks, alphas, scalings, dropout and DoRA flags. Every check runs before the first tensor is
    written, and a refusal leaves the model as it was: ValueError naming the first difference, a
    missing or unexpected key (strict=True), a shape or dtype that does not fit, or another world size.

    Values are copied in place (copy_), so pointers held elsewhere (GradAllReduce buckets, the
    FusedAdamW chunk table) stay valid; then ops.bump_weight_generation() and every block's packed
    weights are dropped, as unload_lora does. With `optimizer` the moments, per-parameter steps
    (state is created where the optimizer has not stepped yet), hyper-parameters and this rank's two
    RNG states are restored; with `loader` its seed.

    `weights="ema"` (for inference and export; not together with `optimizer`): the shadows of
    ema_model.safetensors are loaded as the model's weights in place of the raw adapters, each cast to
    its parameter's dtype; ValueError when the directory has none.

    An `optimizer` that keeps an EMA (FusedAdamW(ema)) gets its shadows and ema_steps back from
    ema_model.safetensors and the "ema" block: ValueError, before anything is written, when the saved
    schedule's fields differ from the optimizer's, and under `strict` when the directory has no
    shadows (strict=False: the shadows start from the loaded weights with ema_steps = 0). An
    optimizer without an EMA ignores the file.

    A training.FusedProdigy gets s, p0 and its record back in place from the "prodigy" block; ValueError,
    before anything is written, when the directory was written by the other kind of optimizer (a Prodigy
    checkpoint into FusedAdamW or the reverse) or with other Prodigy hyper-parameters.

    The moments come back in their stored dtype -- f32 for a bf16 parameter of an optimizer with
    bf16_update="stochastic". ValueError, before anything is written, when the directory was written in the
    other bf16_update mode or with another sr_seed than the live optimizer's.

    An optimizer that guards (FusedAdamW(skip_nonfinite=True)) gets the skipped count of the "guard" block
    back, on the host and in its device record. ValueError, before anything is written, when the directory
    was written with the guard and the live optimizer has none, or the reverse."""
    from safetensors.torch import load_file

    from . import ops
    path = os.fspath(path)
    if not os.path.isfile(os.path.join(path, ADAPTER_TRAIN_STATE)):
        raise FileNotFoundError(f"{path}: no {ADAPTER_TRAIN_STATE} (not a complete adapter checkpoint)")
    state = _read_json(os.path.join(path, ADAPTER_TRAIN_STATE))
    config = _read_json(os.path.join(path, ADAPTER_CONFIG))
    block = config.get("ltx_amd") or {}
    for v in (state.get("format_version"), block.get("format_version")):
        if v != ADAPTER_FORMAT_VERSION:
            raise ValueError(f"{path}: adapter checkpoint format {v!r}, this build reads {ADAPTER_FORMAT_VERSION}")
    rank, world = _dist_rank_world()
    if state.get("world_size") != world:
        raise ValueError(f"{path}: written by {state.get('world_size')} ranks, loaded by {world}: the RNG "
                         f"states are per rank")
    if weights not in ("raw", "ema"):
        raise ValueError(f"weights must be 'raw' or 'ema', got {weights!r}")
    has_ema = "ema" in state and os.path.isfile(os.path.join(path, ADAPTER_EMA))
    if weights == "ema":
        if optimizer is not None:
            raise ValueError("load_adapter_checkpoint(weights='ema') with an optimizer: the moments belong to "
                             "the raw weights")
        if not has_ema:
            raise ValueError(f"{path}: holds no EMA weights ({ADAPTER_EMA})")
    if getattr(optimizer, "_ema_swapped", None) is not None:
        raise RuntimeError("load_adapter_checkpoint: the optimizer's EMA weights are swapped in")
    if hasattr(optimizer, "settle"):
        optimizer.settle()  # a pending rollback belongs to the counters of before the restore
    fname = ADAPTER_EMA if weights == "ema" else ADAPTER_WEIGHTS
    tensors = load_file(os.path.join(path, fname))
    # the optimizer's EMA: (saved shadows or None, ema_steps) once the checks below have passed
    ema_plan = None
    schedule = getattr(optimizer, "ema", None)
    if schedule is not None:
        if has_ema:
            saved = {k: v for k, v in state["ema"].items() if k != "ema_steps"}
            if saved != schedule.fields():
                diff = sorted(k for k in set(saved) | set(schedule.fields()) if saved.get(k) != schedule.fields().get(k))
                raise ValueError(f"{path}: the saved EMA schedule differs from the optimizer's in {', '.join(diff)} "
                                 f"(saved {saved}, the optimizer's {schedule.fields()})")
            ema_plan = (load_file(os.path.join(path, ADAPTER_EMA)), int(state["ema"]["ema_steps"]))
        elif strict:
            raise ValueError(f"{path}: holds no EMA weights ({ADAPTER_EMA}) and the optimizer keeps an EMA")
        else:
            ema_plan = (None, 0)
    opt_tensors = None
    if optimizer is not None:
        if "optimizer" not in state or not os.path.isfile(os.path.join(path, ADAPTER_OPTIMIZER)):
            raise ValueError(f"{path}: holds no optimizer state")
        _check_prodigy(path, optimizer, state)
        _check_bf16_update(path, optimizer, state)
        _check_guard(path, optimizer, state)
        opt_tensors = load_file(os.path.join(path, ADAPTER_OPTIMIZER))
    want = (list(config["target_modules"]), block["groups"])
    have = _adapter_layout(model)
    injected, requires_grad = False, {id(p): p.requires_grad for p in model.parameters()}
    try:
        if not have[0]:
            injected = True
            _inject_from_config(model, *want)
            have = _adapter_layout(model)
        diff = _layout_difference(have, want)
        if diff is not None:
            raise ValueError(f"{path}: {diff}")
        named = list(model.named_parameters())
        trainable = {adapter_key(n): p for n, p in named if p.requires_grad}
        missing = [k for k in trainable if k not in tensors]
        unexpected = [k for k in tensors if k not in trainable]
        if strict and (missing or unexpected):
            raise ValueError(f"{path}: {fname} missing keys {missing[:3]}, unexpected keys "
                             f"{unexpected[:3]} ({len(missing)} / {len(unexpected)} in all)")
        for k, p in trainable.items():
            t = tensors.get(k)
            want_dtype = torch.float32 if weights == "ema" else p.dtype  # the shadows are f32, cast on the copy
            if t is not None and (t.shape != p.shape or (strict and t.dtype != want_dtype)):
                raise ValueError(f"{path}: {k} is {t.dtype} {tuple(t.shape)}, the model's parameter "
                                 f"{p.dtype} {tuple(p.shape)}")
        plan = None
        if optimizer is not None:
            plan = _optimizer_plan(path, optimizer, named, state["optimizer"], opt_tensors, rank, strict)
            if ema_plan is not None and ema_plan[0] is not None:
                for p, name, step in plan:
                    t = ema_plan[0].get(adapter_key(name))
                    if step is not None and (t is None or t.shape != p.shape or t.dtype != torch.float32):
                        raise ValueError(f"{path}: {ADAPTER_EMA} has no f32 {tuple(p.shape)} shadow of {name}")
    except Exception:
        if injected:
            _remove_adapters(model, requires_grad)
        raise
    with torch.no_grad():
        for k, p in trainable.items():
            if k in tensors:
                p.copy_(tensors[k])
    ops.bump_weight_generation()  # weight-derived caches (splits, pieces, DoRA operands, text stack)
    for blk in getattr(model, "transformer_blocks", ()):
        blk._pack = blk._pack_key = None
        blk._dora_pack = None
    if optimizer is not None:
        _restore_optimizer(optimizer, state["optimizer"], opt_tensors, plan, rank, _model_device(model),
                           state.get("prodigy"))
        if ema_plan is not None:
            _restore_ema(optimizer, plan, *ema_plan)
        if _is_guarded(optimizer):
            optimizer.restore_skipped_steps(state["guard"]["skipped_steps"], _model_device(model))
    if loader is not None and "loader" in state and hasattr(loader, "seed"):
        loader.seed = state["loader"]["seed"]
    if state.get("best_loss") is None:
        state["best_loss"] = float("inf")
    return state


def _check_prodigy(path, optimizer, state):
    """ValueError when the checkpoint's optimizer kind (a "prodigy" block or none) or Prodigy's
    hyper-parameters differ from the live optimizer's: its moments mean something else then."""
    saved = state.get("prodigy")
    if (saved is not None) != _is_prodigy(optimizer):
        kinds = ("Prodigy", type(optimizer).__name__) if saved is not None else ("AdamW", "Prodigy")
        raise ValueError(f"{path}: holds {kinds[0]} optimizer state, the live optimizer is {kinds[1]}")
    if saved is None:
        return
    live = optimizer.hyper()
    if saved.get("hyper") != live:
        diff = sorted(k for k in set(saved.get("hyper") or {}) | set(live) if (saved.get("hyper") or {}).get(k) != live.get(k))
        raise ValueError(f"{path}: the saved Prodigy hyper-parameters differ from the optimizer's in {', '.join(diff)}")
    missing = [k for k in optimizer.RECORD if k not in (saved.get("record") or {})]
    if missing:
        raise ValueError(f"{path}: the prodigy record lacks {', '.join(missing)}")


def _check_bf16_update(path, optimizer, state):
    """ValueError when the checkpoint was written in the other bf16_update mode of the optimizer
    (training.FusedAdamW(bf16_update)) or with another sr_seed: the moments' dtype and the rounding's
    stream would not continue the run that wrote them. A directory without the keys is nearest mode's."""
    saved = state["optimizer"].get("param_groups") or []
    for i, (group, hyper) in enumerate(zip(optimizer.param_groups, saved)):
        have = (group.get("bf16_update", "nearest"), group.get("sr_seed"))
        want = (hyper.get("bf16_update", "nearest"), hyper.get("sr_seed"))
        if have[0] != want[0]:
            raise ValueError(f"{path}: parameter group {i} was saved with bf16_update {want[0]!r}, the live "
                             f"optimizer's is {have[0]!r}")
        if have[1] != want[1]:
            raise ValueError(f"{path}: parameter group {i} was saved with sr_seed {want[1]}, the live "
                             f"optimizer's is {have[1]}")


def _check_guard(path, optimizer, state):
    """ValueError when the checkpoint was written with the non-finite guard (skip_nonfinite among the
    hyper-parameters, a "guard" block) and the live optimizer has none, or the reverse: the run that wrote it
    would not be the run that continues."""
    saved = state["optimizer"].get("param_groups") or []
    want = any(h.get("skip_nonfinite", False) for h in saved) or "guard" in state
    have = _is_guarded(optimizer)
    if want != have:
        raise ValueError(f"{path}: was saved {'with' if want else 'without'} skip_nonfinite, the live optimizer "
                         f"runs {'with' if have else 'without'} it")
    if want and not isinstance((state.get("guard") or {}).get("skipped_steps"), int):
        raise ValueError(f"{path}: saved with skip_nonfinite but holds no guard.skipped_steps count")


def _optimizer_plan(path, optimizer, named, saved, opt_tensors, rank, strict):
    """The checks of the optimizer restore, before anything is written: [(parameter, its name, saved
    step or None)] in the optimizer's order."""
    names = {id(p): n for n, p in named}
    if len(saved["param_groups"]) != len(optimizer.param_groups):
        raise ValueError(f"{path}: {len(saved['param_groups'])} optimizer parameter groups, the optimizer "
                         f"has {len(optimizer.param_groups)}")
    plan, seen = [], set()
    for group in optimizer.param_groups:
        for p in group["params"]:
            name = names.get(id(p))
            if name is None:
                raise ValueError(f"{path}: the optimizer holds a parameter that is not the model's")
            step = saved["step"].get(name)
            for k in ("exp_avg.", "exp_avg_sq.") + (tuple(k + "." for k in _PRODIGY_STATE) if _is_prodigy(optimizer) else ()):
                t = opt_tensors.get(k + name)
                if (t is None) != (step is None):
                    raise ValueError(f"{path}: {k + name} and the step of {name} do not go together")
                if t is not None and t.shape != p.shape:
                    raise ValueError(f"{path}: {k + name} is {tuple(t.shape)}, the parameter {tuple(p.shape)}")
            seen.add(name)
            plan.append((p, name, step))
    extra = [k for k in opt_tensors if not k.startswith("rng.") and k.split(".", 1)[1] not in seen]
    extra += [n for n in saved["step"] if n not in seen]
    if strict and extra:
        raise ValueError(f"{path}: optimizer state for {extra[:3]}, which the optimizer does not hold "
                         f"({len(extra)} in all)")
    if f"rng.cpu.rank{rank}" not in opt_tensors:
        raise ValueError(f"{path}: no RNG state of rank {rank}")
    return plan


@torch.no_grad()
def _restore_optimizer(optimizer, saved, opt_tensors, plan, rank, device, saved_prodigy=None):
    for group, hyper in zip(optimizer.param_groups, saved["param_groups"]):
        for k, v in hyper.items():
            group[k] = tuple(v) if isinstance(group.get(k), tuple) and isinstance(v, list) else v
    for p, name, step in plan:
        if step is None:
            optimizer.state.pop(p, None)
            continue
        st = optimizer.state[p]
        for k in ("exp_avg", "exp_avg_sq") + (_PRODIGY_STATE if _is_prodigy(optimizer) else ()):
            src = opt_tensors[f"{k}.{name}"]
            cur = st.get(k)
            if torch.is_tensor(cur) and cur.shape == src.shape and cur.dtype == src.dtype:
                cur.copy_(src)  # in place: the chunk table's pointers stay valid
            else:
                st[k] = src.to(p.device, copy=True)
        cur = st.get("step")
        st["step"] = cur.fill_(step) if torch.is_tensor(cur) else int(step)
    if _is_prodigy(optimizer):
        values = [float.fromhex(saved_prodigy["record"][k]) for k in optimizer.RECORD]
        optimizer.ensure_record(device).copy_(torch.tensor(values, dtype=torch.float64))  # in place: step() holds it
    torch.set_rng_state(opt_tensors[f"rng.cpu.rank{rank}"])
    dev_state = opt_tensors.get(f"rng.device.rank{rank}")
    if dev_state is not None and device.type == "cuda":
        torch.cuda.set_rng_state(dev_state, device)


@torch.no_grad()
def _restore_ema(optimizer, plan, shadows, ema_steps):
    """The shadows of every parameter that has optimizer state, in place where they exist; `shadows`
    None: each starts again from its parameter's (loaded) value."""
    for p, name, step in plan:
        if step is None:
            continue  # no state: the shadow is created with the moments at the first step
        st = optimizer.state[p]
        src = p.detach().float() if shadows is None else shadows[adapter_key(name)]
        cur = st.get("ema")
        if torch.is_tensor(cur) and cur.shape == src.shape and cur.dtype == torch.float32:
            cur.copy_(src)  # in place: the chunk table's pointers stay valid
        else:
            st["ema"] = src.to(device=p.device, dtype=torch.float32, copy=True)
    optimizer.ema_steps = int(ema_steps)
    optimizer.ema_decay = optimizer.ema.decay_at(ema_steps) if ema_steps > 0 else None


def latest_adapter_checkpoint(output_dir):
    """The complete `adapter_epoch_{E}` directory with the highest E in `output_dir` (complete: it
    holds train_state.json, the file written last), or None."""
    best = None
    if output_dir and os.path.isdir(output_dir):
        for entry in os.listdir(output_dir):
            m = _ADAPTER_DIR.match(entry)
            full = os.path.join(output_dir, entry)
            if m and os.path.isfile(os.path.join(full, ADAPTER_TRAIN_STATE)):
                if best is None or int(m.group(1)) > best[0]:
                    best = (int(m.group(1)), full)
    return None if best is None else best[1]
