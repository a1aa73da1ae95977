"""apply_training_strategy (ltx_video/training.py:42-91) without the peft dependency.

'lora_audio': wraps transformer_blocks.{i}.attn2.{to_q,to_k,to_v,to_out.0} in LoraLinear (peft
0.17.1 parameter names and init: kaiming-uniform(a=sqrt(5)) A, zero B, f32 adapters on the bf16
base, scaling = alpha / r) and makes only `lora_*` and `caption_projection` trainable.
`config.lora_targets` ("attn2" by default; "attn1", "attn1+attn2" or a tuple of those names) also
or instead wraps the same four projections of the self-attention attn1. `config.lora_ff` (a bool,
absent = False) also wraps both feed-forward linears of every block, ff.net.0.proj and ff.net.2.
`config.lora_dropout` (a float in [0, 1), absent = 0.0) is peft's lora_dropout on every adapter; the
keep mask is this build's own counter-based stream (lora_dropout_mask_reference states it in numpy).
`config.use_dora` (a bool, absent = False) is peft's use_dora, weight-decomposed LoRA: every wrapped
linear also holds the f32 magnitude `lora_magnitude_vector.default.weight` (DESIGN.md "DoRA (use_dora)").
It is built for the reference's own targets, the four attn2 projections, without dropout.
'full': the reference's substring rule (training.py:75-91); the fused block backward raises for
it until the wgrad path (next row) lands.
"""
import torch

from . import ops
from .transformer3d import LoraLinear, check_lora_dropout


LORA_ATTENTIONS = ("attn1", "attn2")  # the attentions whose four projections can carry adapters
_PROJECTIONS = ("to_q", "to_k", "to_v", "to_out.0")  # the reference's order (training.py:52-60)
_FF_LINEARS = ("net.0.proj", "net.2")  # the feed-forward's two linears, in forward order


# the mask streams of one block's adapters (sid = 16 * block index + slot), in this order: every wrapped
# linear owns its own dropout module in peft, so q / k / v get independent masks on their shared input
LORA_DROPOUT_SLOTS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0",
                      "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
                      "ff.net.0.proj", "ff.net.2")


def lora_dropout_stream(module_name):
    """The mask stream sid of the adapter on `transformer_blocks.<i>.<slot>` (a leading prefix such as
    'base_model.model.' is accepted): 16 * i + the slot's index in LORA_DROPOUT_SLOTS."""
    _, sep, rest = module_name.rpartition("transformer_blocks.")
    idx, _, slot = rest.partition(".")
    if not sep or not idx.isdigit() or slot not in LORA_DROPOUT_SLOTS:
        raise ValueError(f"{module_name!r}: expected transformer_blocks.<i>.<{'|'.join(LORA_DROPOUT_SLOTS)}>")
    return 16 * int(idx) + LORA_DROPOUT_SLOTS.index(slot)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Random123) in numpy: counter = four uint32 arrays (or ints) of one shape, key =
    two; returns the four output words as uint32 arrays."""
    import numpy as np
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def lora_dropout_mask_reference(key, sid, M, K, p):
    """The keep mask (numpy bool [M, K]) of adapter stream sid under the 64-bit key at rate p, as the
    kernels regenerate it (DESIGN.md "LoRA dropout"): Philox4x32-10 on the counter (m, k // 8, sid, 0)
    with the key (key & 0xffffffff, key >> 32); element k takes the 16-bit lane j = k % 8 (low half of
    o[j // 2] for even j, high half for odd j) and is kept iff lane >= T = round(p * 65536) clamped to
    [1, 65535]. CPU only: the tests' and the golden tool's statement of the mask."""
    import numpy as np
    if K % 8:
        raise ValueError("lora_dropout_mask_reference: K must be a multiple of 8")
    T, _ = ops.lora_dropout_threshold(p)
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    m = np.arange(M, dtype=np.uint64)[:, None]
    kg = np.arange(K // 8, dtype=np.uint64)[None, :]
    o = philox4x32_10((m, kg, int(sid), 0), (key & 0xFFFFFFFF, key >> 32))
    lanes = np.empty((M, K // 8, 8), dtype=np.uint32)
    for j in range(8):
        lanes[:, :, j] = (o[j // 2] >> np.uint32(16 * (j % 2))) & np.uint32(0xFFFF)
    return (lanes >= T).reshape(M, K)


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


def _check_dropout(model, targets, dropout):
    """Before any module is replaced: the rate is in [0, 1) (ValueError), and no block ends up with
    adapters of different rates (NotImplementedError: one key, threshold and scale per block)."""
    p = check_lora_dropout(dropout)
    for i in sorted({int(name.split(".")[1]) for name in targets}):
        blk = model.transformer_blocks[i]
        have = {getattr(m, "lora_dropout_p", 0.0) for m in blk.modules() if isinstance(m, LoraLinear)}
        new = any(not isinstance(model.get_submodule(name), LoraLinear) for name in targets
                  if name.startswith(f"transformer_blocks.{i}."))
        if new and have - {p}:
            raise NotImplementedError(f"transformer_blocks.{i} already has adapters with lora_dropout "
                                      f"{sorted(have)}: the adapters of one block must share one rate, got {p}")
    return p


def _check_dora(model, targets, dora, dropout):
    """Before any module is replaced (NotImplementedError): DoRA adapters go on attn2 only and take no
    dropout, and no block ends up with DoRA and plain adapters side by side."""
    if dora and dropout > 0.0:
        raise NotImplementedError("use_dora with lora_dropout > 0 is not supported")
    if dora and any(name.split(".", 3)[2] != "attn2" for name in targets):
        raise NotImplementedError("use_dora is supported on the attn2 projections only (lora_targets 'attn2', "
                                  "no lora_ff)")
    for i in sorted({int(name.split(".")[1]) for name in targets}):
        blk = model.transformer_blocks[i]
        have = {m.use_dora for m in blk.modules() if isinstance(m, LoraLinear)}
        new = any(not isinstance(model.get_submodule(name), LoraLinear) for name in targets
                  if name.startswith(f"transformer_blocks.{i}."))
        if new and have - {bool(dora)}:
            raise NotImplementedError(f"transformer_blocks.{i} already has {'plain' if dora else 'DoRA'} adapters: "
                                      f"DoRA and plain LoRA adapters cannot be mixed within one block")


def inject_lora(model, targets, r, alpha, *, feed_forward=False, dropout=0.0, dora=False):
    """Wrap the named linears in LoraLinear. feed_forward=True also accepts the names of
    lora_ff_target_modules; without it they are refused like any name outside the attentions.
    dropout = peft's lora_dropout, one rate for every adapter created here. dora=True = peft's
    use_dora: the adapters created here are DoRA adapters (attn2 only, no dropout)."""
    ops.check_lora_rank(r)  # before the first module is replaced
    targets = list(targets)
    _check_targets(model, targets, feed_forward)
    dropout = _check_dropout(model, targets, dropout)
    _check_dora(model, targets, dora, dropout)
    for name in targets:
        parent_name, _, child = name.rpartition(".")
        parent = model.get_submodule(parent_name)
        base = getattr(parent, child) if not child.isdigit() else parent[int(child)]
        if isinstance(base, LoraLinear):
            continue
        wrapped = LoraLinear(base, r, alpha, dropout, use_dora=bool(dora))
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
        # config.lora_dropout (setattr or train.lora_dropout in the YAML; absent = 0.0): peft's
        # lora_dropout, one rate for every adapter of the model (the reference fixes 0.0, training.py:65)
        extra = {}
        if ff:
            extra["feed_forward"] = True
        p = float(getattr(config, "lora_dropout", 0.0))
        if p != 0.0:
            extra["dropout"] = p
        # config.use_dora (setattr or train.use_dora in the YAML; absent = False): peft's use_dora
        if bool(getattr(config, "use_dora", False)):
            extra["dora"] = True
        inject_lora(model, targets, config.lora_rank, config.lora_alpha, **extra)
        for n, p in model.named_parameters():
            p.requires_grad = ("lora_" in n) or ("caption_projection" in n)
        return model
    for n, p in model.named_parameters():
        p.requires_grad = any(k in n for k in ("proj_out", "scale_shift_table", "adaln_single",
                                              "caption_projection", "attn", "attn2"))
    return model


def trainable_parameters(model):
    return [(n, p) for n, p in model.named_parameters() if p.requires_grad]


def adapter_pairs(model):
    """[(module name, lora_A weight [r, K], lora_B weight [N, r], scaling)] of every LoraLinear, DoRA ones
    included, in module order: the pairs whose update s B A the max-norm pass of the optimizer step bounds
    (FusedAdamW(scale_weight_norms=..., norm_pairs=...)). The magnitudes of DoRA and the caption projection
    are not adapters and do not appear."""
    return [(name, mod.lora_A["default"].weight, mod.lora_B["default"].weight, float(mod.scaling))
            for name, mod in model.named_modules() if isinstance(mod, LoraLinear)]


@torch.no_grad()
def merged_state_dict(model):
    """peft merge_and_unload(): W + s*B@A (under DoRA (m / norm)[:, None] times it) folded into each
    wrapped base weight, adapter and magnitude keys dropped (what save_training_checkpoint exports,
    torch_utils.py:66-102)."""
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
        blk._dora_pack = None
    return model
