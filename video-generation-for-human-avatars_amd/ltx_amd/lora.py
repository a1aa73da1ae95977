"""apply_training_strategy (ltx_video/training.py:42-91) without the peft dependency.

'lora_audio': wraps transformer_blocks.{i}.attn2.{to_q,to_k,to_v,to_out.0} in LoraLinear (peft
0.17.1 parameter names and init: kaiming-uniform(a=sqrt(5)) A, zero B, f32 adapters on the bf16
base, scaling = alpha / r) and makes only `lora_*` and `caption_projection` trainable.
`config.lora_targets` ("attn2" by default; "attn1", "attn1+attn2" or a tuple of those names) also
or instead wraps the same four projections of the self-attention attn1. `config.lora_ff` (a bool,
absent = False) also wraps both feed-forward linears of every block, ff.net.0.proj and ff.net.2.
'full': the reference's substring rule (training.py:75-91); the fused block backward raises for
it until the wgrad path (next row) lands.
"""
import torch

from . import ops
from .transformer3d import LoraLinear


LORA_ATTENTIONS = ("attn1", "attn2")  # the attentions whose four projections can carry adapters
_PROJECTIONS = ("to_q", "to_k", "to_v", "to_out.0")  # the reference's order (training.py:52-60)
_FF_LINEARS = ("net.0.proj", "net.2")  # the feed-forward's two linears, in forward order


def _attentions(attention):
    """`attention` (a tuple / list of names, or "attn2" / "attn1" / "attn1+attn2") as a tuple in
    block order (attn1 before attn2); ValueError for anything outside LORA_ATTENTIONS."""
    names = tuple(a.strip() for a in attention.split("+")) if isinstance(attention, str) else tuple(attention)
    bad = [a for a in names if a not in LORA_ATTENTIONS]
    if bad or not names or len(set(names)) != len(names):
        raise ValueError(f"LoRA targets {attention!r}: expected a non-empty subset of {LORA_ATTENTIONS} "
                         f"(or 'attn2', 'attn1', 'attn1+attn2')")
    return tuple(a for a in LORA_ATTENTIONS if a in names)


def lora_target_modules(num_blocks, attention=("attn2",)):
    out = []
    for i in range(num_blocks):
        for a in _attentions(attention):
            out += [f"transformer_blocks.{i}.{a}.{p}" for p in _PROJECTIONS]
    return out


def lora_ff_target_modules(num_blocks):
    """Both feed-forward linears of every block, in block order (config.lora_ff; inject_lora accepts
    these names with feed_forward=True)."""
    return [f"transformer_blocks.{i}.ff.{p}" for i in range(num_blocks) for p in _FF_LINEARS]


def _check_targets(model, targets, feed_forward=False):
    """Before any module is replaced: every name is `transformer_blocks.<i>.<attn1|attn2>.<to_q|to_k|
    to_v|to_out.0>` of this model (ValueError naming the accepted set), and together with the
    adapters already present each attention ends up with none or all four of its projections
    wrapped (NotImplementedError: the fused block has no path for a partly adapted attention). With
    feed_forward=True the names `transformer_blocks.<i>.ff.<net.0.proj|net.2>` are accepted as well,
    under the same rule: both linears of a block's feed-forward or none."""
    n = len(model.transformer_blocks)
    want = set()
    for name in targets:
        parts = name.split(".", 3)
        if (feed_forward and len(parts) == 4 and parts[0] == "transformer_blocks" and parts[1].isdigit()
                and int(parts[1]) < n and parts[2] == "ff" and parts[3] in _FF_LINEARS):
            want.add((int(parts[1]), "ff", parts[3]))
            continue
        ok = (len(parts) == 4 and parts[0] == "transformer_blocks" and parts[1].isdigit() and int(parts[1]) < n
              and parts[2] in LORA_ATTENTIONS and parts[3] in _PROJECTIONS)
        if not ok:
            raise ValueError(f"LoRA target {name!r}: accepted are transformer_blocks.<0..{n - 1}>."
                             f"<{'|'.join(LORA_ATTENTIONS)}>.<{'|'.join(_PROJECTIONS)}>")
        want.add((int(parts[1]), parts[2], parts[3]))
    for i, blk in enumerate(model.transformer_blocks):
        for a in LORA_ATTENTIONS:
            att = getattr(blk, a)
            have = [isinstance(att.to_out[0] if p == "to_out.0" else getattr(att, p), LoraLinear) or (i, a, p) in want
                    for p in _PROJECTIONS]
            if any(have) and not all(have):
                raise NotImplementedError(f"LoRA must wrap all four projections of transformer_blocks.{i}.{a} "
                                          f"({', '.join(_PROJECTIONS)}) or none (training.py:52-60)")
        net = blk.ff.net
        have = [isinstance(net[0].proj, LoraLinear) or (i, "ff", _FF_LINEARS[0]) in want,
                isinstance(net[2], LoraLinear) or (i, "ff", _FF_LINEARS[1]) in want]
        if any(have) and not all(have):
            raise NotImplementedError(f"LoRA must wrap both linears of transformer_blocks.{i}.ff "
                                      f"({', '.join(_FF_LINEARS)}) or none")


def inject_lora(model, targets, r, alpha, *, feed_forward=False):
    """Wrap the named linears in LoraLinear. feed_forward=True also accepts the names of
    lora_ff_target_modules; without it they are refused like any name outside the attentions."""
    ops.check_lora_rank(r)  # before the first module is replaced
    targets = list(targets)
    _check_targets(model, targets, feed_forward)
    for name in targets:
        parent_name, _, child = name.rpartition(".")
        parent = model.get_submodule(parent_name)
        base = getattr(parent, child) if not child.isdigit() else parent[int(child)]
        if isinstance(base, LoraLinear):
            continue
        wrapped = LoraLinear(base, r, alpha)
        if child.isdigit():
            parent[int(child)] = wrapped
        else:
            setattr(parent, child, wrapped)
    return model


def apply_training_strategy(model, config, train_mode: str):
    if train_mode == "lora_audio":
        # the attentions that carry adapters: config.lora_targets, set with setattr as the reference
        # sets train_mode (not a TrainConfig field); default = the reference's attn2 (training.py:50-60)
        attention = getattr(config, "lora_targets", ("attn2",))
        targets = lora_target_modules(len(model.transformer_blocks), attention)
        # config.lora_ff (setattr or train.lora_ff in the YAML; absent = False): both feed-forward
        # linears of every block as well
        ff = bool(getattr(config, "lora_ff", False))
        if ff:
            targets = targets + lora_ff_target_modules(len(model.transformer_blocks))
        if ff:
            inject_lora(model, targets, config.lora_rank, config.lora_alpha, feed_forward=True)
        else:
            inject_lora(model, targets, config.lora_rank, config.lora_alpha)
        for n, p in model.named_parameters():
            p.requires_grad = ("lora_" in n) or ("caption_projection" in n)
        return model
    for n, p in model.named_parameters():
        p.requires_grad = any(k in n for k in ("proj_out", "scale_shift_table", "adaln_single",
                                              "caption_projection", "attn", "attn2"))
    return model


def trainable_parameters(model):
    return [(n, p) for n, p in model.named_parameters() if p.requires_grad]


@torch.no_grad()
def merged_state_dict(model):
    """peft merge_and_unload(): W + s*B@A folded into each wrapped base weight, adapter keys
    dropped (what save_training_checkpoint exports, torch_utils.py:66-102)."""
    out = {}
    skip = set()
    for name, mod in model.named_modules():
        if isinstance(mod, LoraLinear):
            out[name + ".weight"] = mod.merged_weight()
            if mod.base_layer.bias is not None:
                out[name + ".bias"] = mod.base_layer.bias.detach().clone()
            skip.add(name + ".")
    for k, v in model.state_dict().items():
        if any(k.startswith(s) for s in skip):
            continue
        out[k] = v
    return out


@torch.no_grad()
def unload_lora(model):
    """peft merge_and_unload in place: base_layer.weight += (B @ A) * scaling (promoted add
    rounded to the base dtype), each LoraLinear replaced by its base nn.Linear. The sum is taken in
    f32 and rounded once (LoraLinear.merged_weight), so the unloaded model holds bitwise the weights
    of merged_state_dict on every device (torch's in-place bf16 += f32 on the GPU came out one bf16
    step away from that on some elements)."""
    for name, mod in list(model.named_modules()):
        if isinstance(mod, LoraLinear):
            mod.base_layer.weight.data.copy_(mod.merged_weight())
            parent_name, _, child = name.rpartition(".")
            parent = model.get_submodule(parent_name)
            if child.isdigit():
                parent[int(child)] = mod.base_layer
            else:
                setattr(parent, child, mod.base_layer)
    # the merge wrote through .data (no version bump): drop every block's packed-weight cache (fused
    # QKV, W^T copies) so the next forward packs the merged weights
    for blk in getattr(model, "transformer_blocks", ()):
        blk._pack = blk._pack_key = None
    return model
