"""DoRA (peft use_dora), host side: the module surface (state dict, trainable set, refusals, YAML,
gradient order), the design's identity on one linear in float64 (the column scale folded into the
operands, the magnitude gradient from y), the merge statement, and the golden fixture.
No GPU, no kernel launches."""
import os

import pytest
import torch
from safetensors.torch import load_file

from lora_dora_utils import GOLD, MAG, NAME, dora_config, dora_names, dora_statement, golden_meta, golden_params


def _tiny_cfg():
    return golden_meta()["config"]


def _bare(device="meta"):
    from ltx_amd.transformer3d import Transformer3DModel
    with torch.device(device):
        return Transformer3DModel.from_config(_tiny_cfg())


def _wrapped(m):
    from ltx_amd.transformer3d import LoraLinear
    return [n for n, mod in m.named_modules() if isinstance(mod, LoraLinear)]


def _cpu_dora_model(params=None):
    """The tiny model with DoRA adapters on the CPU (parameters only: no forward without a GPU)."""
    from ltx_amd.lora import apply_training_strategy
    m = _bare("cpu").to(torch.bfloat16)
    apply_training_strategy(m, dora_config(8), "lora_audio")
    if params is not None:
        from params import canonical_name
        m.load_state_dict({n: params[canonical_name(n)].clone() for n, _ in m.named_parameters()}, strict=True)
    return m


# ---------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------
def test_state_dict_names_dtypes_and_trainable_set():
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.transformer3d import LoraLinear, dora_weight_norm
    plain, m = _bare("cpu").to(torch.bfloat16), _bare("cpu").to(torch.bfloat16)
    apply_training_strategy(plain, dora_config(8, None), "lora_audio")
    apply_training_strategy(m, dora_config(8), "lora_audio")
    names = dora_names(2)
    assert _wrapped(m) == _wrapped(plain) == names
    mags = [n + MAG for n in names]
    sd, sp = m.state_dict(), plain.state_dict()
    assert sorted(set(sd) - set(sp)) == sorted(mags) and set(sp) <= set(sd)
    for n in names:
        lin = m.get_submodule(n)
        assert isinstance(lin, LoraLinear) and lin.use_dora and list(lin.lora_magnitude_vector) == ["default"]
        mv = sd[n + MAG]
        assert mv.dtype == torch.float32 and tuple(mv.shape) == (lin.out_features,)
        assert sd[n + ".lora_A.default.weight"].dtype == sd[n + ".lora_B.default.weight"].dtype == torch.float32
        assert sd[n + ".base_layer.weight"].dtype == torch.bfloat16
        # a fresh adapter (B = 0): m is the torch statement of the row norm, here the row norms of W
        want = torch.linalg.norm(lin.base_layer.weight.float(), dim=1)
        assert torch.equal(mv, want) and torch.equal(mv, dora_weight_norm(
            lin.base_layer.weight, lin.lora_A["default"].weight, lin.lora_B["default"].weight, lin.scaling))
    train = {n for n, p in m.named_parameters() if p.requires_grad}
    assert train == {n for n in sd if "lora_" in n or "caption_projection" in n} and set(mags) <= train
    assert not any(hasattr(x, "lora_magnitude_vector") for x in plain.modules())


def test_use_dora_false_and_absent_build_the_same_tree():
    from ltx_amd.config import TrainConfig
    from ltx_amd.lora import apply_training_strategy
    assert not hasattr(TrainConfig(checkpoint_path="-"), "use_dora")
    a, b = _bare(), _bare()
    with torch.device("meta"):
        apply_training_strategy(a, dora_config(8, None), "lora_audio")
        apply_training_strategy(b, dora_config(8, False), "lora_audio")
    sig = lambda mm: [(n, tuple(p.shape), p.dtype, p.requires_grad) for n, p in mm.named_parameters()]
    assert sig(a) == sig(b) and [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]


def _refused(setup, match):
    from ltx_amd.lora import apply_training_strategy
    m = _bare()
    tc = dora_config(8)
    setup(tc)
    with torch.device("meta"), pytest.raises(NotImplementedError, match=match):
        apply_training_strategy(m, tc, "lora_audio")
    assert _wrapped(m) == [] and not any(hasattr(x, "lora_magnitude_vector") for x in m.modules())


def test_refused_with_dropout():
    _refused(lambda tc: setattr(tc, "lora_dropout", 0.1), "lora_dropout")


@pytest.mark.parametrize("targets", ["attn1", "attn1+attn2", ("attn1",)])
def test_refused_on_other_targets(targets):
    _refused(lambda tc: setattr(tc, "lora_targets", targets), "attn2")


def test_refused_with_lora_ff():
    _refused(lambda tc: setattr(tc, "lora_ff", True), "attn2")


def test_refused_mixed_with_plain_adapters_in_one_block():
    from ltx_amd.lora import inject_lora, lora_target_modules
    from ltx_amd.transformer3d import LoraLinear, _block_dora
    m = _bare()
    with torch.device("meta"):
        inject_lora(m, lora_target_modules(2, "attn1"), 8, 8)
        before = _wrapped(m)
        with pytest.raises(NotImplementedError, match="mixed"):
            inject_lora(m, lora_target_modules(2, "attn2"), 8, 8, dora=True)
        assert _wrapped(m) == before
    n = _bare()
    with torch.device("meta"):
        inject_lora(n, lora_target_modules(2, "attn2"), 8, 8, dora=True)
        before = _wrapped(n)
        with pytest.raises(NotImplementedError, match="mixed"):
            inject_lora(n, lora_target_modules(2, "attn1"), 8, 8)
        with pytest.raises(NotImplementedError, match="attn2"):
            inject_lora(n, lora_target_modules(2, "attn1"), 8, 8, dora=True)
        with pytest.raises(NotImplementedError, match="lora_dropout"):
            LoraLinear(n.transformer_blocks[0].attn1.to_q, 8, 8, 0.1, use_dora=True)
        assert _wrapped(n) == before
        # the block refuses a mix whoever built it
        assert _block_dora(n.transformer_blocks[0]) is True and _block_dora(_bare().transformer_blocks[0]) is False
        blk = n.transformer_blocks[1]
        blk.attn2.to_k = LoraLinear(blk.attn2.to_k.base_layer, 8, 8)
        with pytest.raises(NotImplementedError, match="mixed"):
            _block_dora(blk)


def test_processor_refuses_a_dora_linear():
    from ltx_amd.processor import _linear_parts
    from ltx_amd.transformer3d import LoraLinear
    with pytest.raises(NotImplementedError, match="DoRA"):
        _linear_parts(LoraLinear(torch.nn.Linear(16, 16), 8, 8, use_dora=True))
    plain = LoraLinear(torch.nn.Linear(16, 16), 8, 8)
    assert _linear_parts(plain)[2] is plain.lora_A["default"].weight


def test_yaml_sets_use_dora_only_when_present(tmp_path):
    from dataclasses import asdict
    from ltx_amd.config import load_train_config_from_yaml
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.transformer3d import LoraLinear
    base = "checkpoint_path: x.safetensors\ntrain:\n  lora_rank: 8\n"
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(base + "  use_dora: true\n")
    (tmp_path / "c.yaml").write_text(base + "  use_dora: false\n")
    a, b, c = (load_train_config_from_yaml(str(tmp_path / f"{n}.yaml")) for n in "abc")
    assert not hasattr(a, "use_dora") and b.use_dora is True and c.use_dora is False
    assert asdict(a) == asdict(b) and "use_dora" not in asdict(b)
    # ... and reaches apply_training_strategy
    for tc, want in ((a, False), (b, True), (c, False)):
        m = _bare()
        with torch.device("meta"):
            apply_training_strategy(m, tc, "lora_audio")
        lins = [x for x in m.modules() if isinstance(x, LoraLinear)]
        assert len(lins) == 8 and all(x.use_dora is want for x in lins)


def test_grad_ready_order_names_every_trainable_parameter_once():
    m = _cpu_dora_model()
    order = m.grad_ready_order()
    train = [p for p in m.parameters() if p.requires_grad]
    assert len(order) == len(train) == len({id(p) for p in order}) and {id(p) for p in order} == {id(p) for p in train}
    mags = {id(p) for n, p in m.named_parameters() if n.endswith(MAG)}
    assert len(mags) == 8 and mags <= {id(p) for p in order}
    assert m._text_structure() is None  # a DoRA model takes the per-block text path
    # the last block's parameters come first, its magnitudes among them
    first = {id(p) for p in m.transformer_blocks[1].parameters() if p.requires_grad}
    assert {id(p) for p in order[:len(first)]} == first


# ---------------------------------------------------------------------------------------------
# the design's identity: one linear in float64
# ---------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_folded_form_and_magnitude_gradient_from_y_in_float64():
    """y, dx, dA, dB and dm of the folded form (W_eff = c W, B_eff = c s B; dm = sum dY (y - b) / m)
    against autograd of the peft statement, relative error <= 1e-10; a column with m_j = 0 gives
    dm_j = 0 in the folded form."""
    g = torch.Generator().manual_seed(11)
    M, K, N, r, s = 48, 40, 24, 8, 0.75
    f = dict(dtype=torch.float64, generator=g)
    x, W, b = torch.randn(M, K, **f), torch.randn(N, K, **f) / K ** 0.5, 0.1 * torch.randn(N, **f)
    A, B = torch.randn(r, K, **f) / K ** 0.5, 0.05 * torch.randn(N, r, **f)
    norm = torch.linalg.norm(W + s * (B @ A), dim=1)
    m = norm * (1 + 0.2 * torch.randn(N, **f)).abs()
    dY = torch.randn(M, N, **f)
    for zero in (False, True):
        mm = m.clone()
        if zero:
            mm[5] = 0.0
        leaves = [t.clone().requires_grad_(True) for t in (x, A, B, mm)]
        y_ref = dora_statement(leaves[0], W, b, leaves[1], leaves[2], leaves[3], s)
        dx_ref, dA_ref, dB_ref, dm_ref = torch.autograd.grad(y_ref, leaves, dY)
        # the folded form, with the launches' operands
        c = mm / norm
        W_eff, B_eff = c[:, None] * W, c[:, None] * (s * B)
        u = x @ A.t()
        y = x @ W_eff.t() + u @ B_eff.t() + b
        w = dY @ B_eff                      # already the w of dA and dx
        dx = dY @ W_eff + w @ A
        dA = w.t() @ x
        dB = (s * c)[:, None] * (dY.t() @ u)   # the plain dB kernels' dY^T u, row-scaled by s c_j
        safe = torch.where(mm != 0, mm, torch.ones_like(mm))
        dm = torch.where(mm != 0, (dY * (y - b)).sum(0) / safe, torch.zeros_like(mm))
        errs = {"y": _rel(y, y_ref.detach()), "dx": _rel(dx, dx_ref), "dA": _rel(dA, dA_ref), "dB": _rel(dB, dB_ref)}
        if zero:
            keep = torch.arange(N) != 5
            errs["dm"] = _rel(dm[keep], dm_ref[keep])
            assert float(dm[5]) == 0.0 and float(dm_ref[5]) != 0.0  # the one divergence from peft
            assert float(y[:, 5].sub(b[5]).abs().max()) == 0.0
        else:
            errs["dm"] = _rel(dm, dm_ref)
        print(f"m_j = 0 column: {zero}; folded form vs peft statement (float64): {errs}")
        assert all(e <= 1e-10 for e in errs.values()), errs


# ---------------------------------------------------------------------------------------------
# merge / export
# ---------------------------------------------------------------------------------------------
def _fixture():
    meta = golden_meta()
    raw = load_file(os.path.join(GOLD, NAME + ".safetensors"))
    return meta, raw, golden_params(meta, raw)


def test_merged_weight_is_the_statement_bitwise():
    from ltx_amd.transformer3d import LoraLinear
    meta, raw, params = _fixture()
    m = _cpu_dora_model(params)
    n_checked = 0
    for name, lin in m.named_modules():
        if not isinstance(lin, LoraLinear):
            continue
        W, A, B = lin.base_layer.weight, lin.lora_A["default"].weight, lin.lora_B["default"].weight
        mv = lin.lora_magnitude_vector["default"].weight
        V = W.float() + lin.scaling * (B @ A)
        c = mv / torch.linalg.norm(V, dim=1)
        want = (c[:, None] * V).to(torch.bfloat16)
        got = lin.merged_weight()
        assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16)), name
        plain = LoraLinear(lin.base_layer, lin.r, lin.lora_alpha)
        plain.load_state_dict({k: v for k, v in lin.state_dict().items() if "magnitude" not in k})
        assert not torch.equal(got, plain.merged_weight())  # the fixture's c is not 1
        # with m = norm (c = 1 exactly) the merge is bitwise the plain-LoRA merge
        with torch.no_grad():
            mv.copy_(torch.linalg.norm(V, dim=1))
        assert torch.equal(lin.merged_weight().view(torch.int16), plain.merged_weight().view(torch.int16)), name
        n_checked += 1
    assert n_checked == 8


def test_merged_state_dict_and_unload_drop_adapter_and_magnitude_keys():
    from ltx_amd.io import merged_state_dict_cpu
    from ltx_amd.lora import merged_state_dict, unload_lora
    from ltx_amd.transformer3d import LoraLinear
    meta, raw, params = _fixture()
    m = _cpu_dora_model(params)
    bare_keys = sorted(_bare().state_dict())
    sd = merged_state_dict(m)
    assert sorted(sd) == bare_keys and not any("lora_" in k or "base_layer" in k for k in sd)
    cpu = merged_state_dict_cpu(m)
    assert sorted(cpu) == bare_keys
    want = {n: m.get_submodule(n).merged_weight() for n in dora_names(2)}
    for n, w in want.items():
        assert torch.equal(sd[n + ".weight"], w) and torch.equal(cpu[n + ".weight"], w)
        assert not torch.equal(w, m.get_submodule(n).base_layer.weight)
    unload_lora(m)
    assert _wrapped(m) == [] and sorted(m.state_dict()) == bare_keys
    assert not any(isinstance(x, LoraLinear) or hasattr(x, "lora_magnitude_vector") for x in m.modules())
    for n, w in want.items():
        assert torch.equal(m.get_submodule(n).weight, w)


# ---------------------------------------------------------------------------------------------
# fixture
# ---------------------------------------------------------------------------------------------
def test_golden_fixture_shapes_and_weight_hash():
    from params import weights_sha256
    meta, raw, params = _fixture()
    assert os.path.getsize(os.path.join(GOLD, NAME + ".safetensors")) < 1 << 20
    cfg, r = meta["config"], meta["lora_rank"]
    assert r == 8 and meta["lora_alpha"] == r and meta["use_dora"] is True and meta["lora_targets"] == ["attn2"]
    assert cfg["num_layers"] == 2 and meta["inputs_from"] == "tiny_lora_ff_step"
    D = cfg["num_attention_heads"] * cfg["attention_head_dim"]
    names = dora_names(2)
    mags = sorted(n + MAG for n in names)
    assert sorted(k[2:] for k in raw if k.startswith("w.")) == mags
    g16 = sorted(k[5:] for k in raw if k.startswith("grad."))
    assert g16 == sorted(k[7:] for k in raw if k.startswith("grad32.")) and set(mags) <= set(g16)
    assert len([k for k in g16 if "lora_" in k]) == 8 * 3 and any("caption_projection" in k for k in g16)
    for n in names:
        for pre in ("w.", "grad.", "grad32."):
            t = raw[pre + n + MAG]
            assert t.dtype == torch.float32 and tuple(t.shape) == (D,)
        # m = norm * (1 + 0.2 randn): positive here, and not the norm itself (c != 1)
        W, A, B = (params[n + s] for s in (".weight", ".lora_A.default.weight", ".lora_B.default.weight"))
        norm = torch.linalg.norm(W.float() + (B @ A), dim=1)
        c = raw["w." + n + MAG] / norm
        assert float(B.abs().max()) > 0 and float((c - 1).abs().max()) > 0.1 and float(c.min()) > 0
        assert float(raw["grad." + n + MAG].abs().max()) > 0
    shared = load_file(os.path.join(GOLD, meta["inputs_from"] + ".safetensors"))
    assert raw["out.sample"].shape == raw["out32.sample"].shape == shared["out.noise"].shape
    assert raw["out.sample"].dtype == torch.bfloat16 and raw["out32.sample"].dtype == torch.float32

    class _Named(torch.nn.Module):  # the hash walks named_parameters
        def __init__(self, tensors):
            super().__init__()
            self._t = tensors

        def named_parameters(self, *a, **k):
            return iter(self._t.items())
    assert weights_sha256(_Named(params)) == meta["weights_sha256"]
