"""The max-norm pass of the LoRA optimizer step (FusedAdamW / FusedProdigy(scale_weight_norms=c)), host side:
the statement (max_norm_utils) against a literal transcription of kohya's loop, the Gram form the device
computes against the direct form, lora.adapter_pairs, the config key (training.max_norm_from_config and the
YAML route), the constructor's keys and refusals, the two host tables and the library's entry points. Models are
the tiny config on the meta device or the CPU (parameters only). No GPU, no kernel launches."""
import os
import re

import numpy as np
import pytest
import torch

from max_norm_utils import (adversarial_pair, exact_pair, kohya_loop, norm_direct, norm_gram, pair_with_norm,
                            random_pair, statement, sumsq_direct, ulps_f32)
from lora_dora_utils import golden_meta

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ltx_max_norm_plan", "ltx_max_norm_sumsq", "ltx_max_norm_finish", "ltx_max_norm_scale_multi")
PROJ = ("to_q", "to_k", "to_v", "to_out.0")


def _config(**extra):
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="base.safetensors", lora_rank=8, lora_alpha=8)
    tc.train_mode = "lora_audio"
    for k, v in extra.items():
        setattr(tc, k, v)
    return tc


# ---------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------
def test_statement_is_kohyas_loop_clamp_included():
    """Random pairs with norms of 0, under c / 2, in (c / 2, c] and above c: the decisions are kohya's, the
    factors within one f32 ulp (sqrt against ** 0.5), the scaled weights one f32 multiply by kohya's factor,
    the record kohya's return value. The clamp changes nothing: every ratio under c is exactly 1."""
    c = 1.0
    targets = [0.0, 0.3, 0.45, 0.6, 0.9, 1.1, 1.7, 5.0, 0.0, 2.5]
    shapes = [(40, 136, 8), (64, 48, 16), (24, 72, 8), (96, 32, 32), (16, 128, 8)]
    pairs = []
    for i, target in enumerate(targets):
        N, K, r = shapes[i % len(shapes)]
        alpha = (4.0, 8.0, 16.0)[i % 3]
        A, B = pair_with_norm(N, K, r, alpha / r, target * c, seed=100 + i)
        pairs.append((A, B, alpha / r, alpha))
    st = statement([(A, B, s) for A, B, s, _ in pairs], c)
    norms = np.asarray(st["norm"])
    assert (norms == 0).sum() == 2 and ((norms > 0) & (norms < c / 2)).sum() == 2
    assert ((norms > c / 2) & (norms <= c)).sum() == 2 and (norms > c).sum() == 4
    torch_pairs = [(torch.from_numpy(A.copy()), torch.from_numpy(B.copy()), alpha) for A, B, _, alpha in pairs]
    keys, avg, mx, decisions = kohya_loop(torch_pairs, c)
    assert keys == st["keys_scaled"] == 4
    for i, (scaled, f_k) in enumerate(decisions):
        assert scaled == (st["ratio"][i] != 1.0), i
        assert ulps_f32(f_k, st["f"][i]) <= 1, (i, f_k, st["f"][i])
        if not scaled:
            assert f_k == np.float32(1.0) and st["ratio"][i] == 1.0
        # torch's `*=` with the 0-dim factor is one f32 multiply per element by float32(factor)
        down, up, _ = torch_pairs[i]
        assert np.array_equal(down.numpy(), pairs[i][0] * f_k if scaled else pairs[i][0]), i
        assert np.array_equal(up.numpy(), pairs[i][1] * f_k if scaled else pairs[i][1]), i
        if f_k == st["f"][i]:
            assert np.array_equal(down.numpy(), st["A"][i]) and np.array_equal(up.numpy(), st["B"][i])
    assert abs(avg - st["avg_key_norm"]) <= 1e-12 * avg and abs(mx - st["max_key_norm"]) <= 1e-12 * mx
    # on the cap afterwards: a second application scales nothing beyond f32 rounding of the weights
    again = statement([(A, B, s) for (A, B), (_, _, s, _) in zip(zip(st["A"], st["B"]), pairs)], c)
    assert all(abs(n - c) <= 1e-6 * c for n, r in zip(again["norm"], st["ratio"]) if r != 1.0)


@pytest.mark.parametrize("shape", [(2048, 2048, 16), (40, 136, 8)])
def test_f64_gram_form_is_the_direct_form_and_f32_is_not(shape):
    """What the device computes, sum_ij (B^T B)_ij (A A^T)_ij in f64, against ||B A||_F^2 with the product
    formed: 1e-13 on a random pair, 1e-9 on the adversarial one, where the same form in f32 is off by more than
    1e-4 -- the reason the Gram products are f64."""
    N, K, r = shape
    A, B = random_pair(N, K, r, seed=1)
    assert abs(norm_gram(A, B, 0.5) - norm_direct(A, B, 0.5)) <= 1e-13 * norm_direct(A, B, 0.5)
    A, B = adversarial_pair(N, K, r, seed=2)
    want = norm_direct(A, B, 1.0)
    assert abs(norm_gram(A, B, 1.0) - want) <= 1e-9 * want
    assert abs(norm_gram(A, B, 1.0, np.float32) - want) > 1e-4 * want


def test_exact_fixture_is_order_independent():
    """exact_pair's claim: the Gram form and the direct form give the same f64, bit for bit."""
    for (N, K, r), seed in (((16, 128, 8), 1), ((40, 136, 8), 2), ((2048, 64, 16), 3), ((64, 8192, 128), 4)):
        A, B = exact_pair(N, K, r, seed)
        ga, gb = A.astype(np.float64) @ A.astype(np.float64).T, B.astype(np.float64).T @ B.astype(np.float64)
        assert np.sum(ga * gb) == sumsq_direct(A, B) == np.sum((ga * gb)[::-1, ::-1])


# ---------------------------------------------------------------------------------------------
# adapter_pairs
# ---------------------------------------------------------------------------------------------
def _meta_model(**extra):
    from ltx_amd.lora import apply_training_strategy
    from ltx_amd.transformer3d import Transformer3DModel
    with torch.device("meta"):
        m = Transformer3DModel.from_config(golden_meta()["config"])
        apply_training_strategy(m, _config(lora_alpha=4, **extra), "lora_audio")
    return m


@pytest.mark.parametrize("extra,per_block", [
    ({}, ["attn2." + p for p in PROJ]),
    ({"lora_targets": "attn1+attn2", "lora_ff": True},
     ["attn1." + p for p in PROJ] + ["attn2." + p for p in PROJ] + ["ff.net.0.proj", "ff.net.2"]),
    ({"use_dora": True}, ["attn2." + p for p in PROJ]),
])
def test_adapter_pairs_order_and_contents(extra, per_block):
    from ltx_amd.lora import adapter_pairs
    from ltx_amd.transformer3d import LoraLinear
    m = _meta_model(**extra)
    pairs = adapter_pairs(m)
    want = [f"transformer_blocks.{i}.{n}" for i in range(2) for n in per_block]
    assert [p[0] for p in pairs] == want == [n for n, mod in m.named_modules() if isinstance(mod, LoraLinear)]
    named = dict(m.named_parameters())
    for name, A, B, s in pairs:
        assert A is named[name + ".lora_A.default.weight"] and B is named[name + ".lora_B.default.weight"]
        assert A.shape[0] == B.shape[1] == 8 and A.dtype == B.dtype == torch.float32
        assert s == 4 / 8 and isinstance(s, float)
    # neither the caption projection nor a DoRA magnitude is a pair's tensor
    held = {id(t) for _, A, B, _ in pairs for t in (A, B)}
    assert not any(id(p) in held for n, p in m.named_parameters() if "lora_A" not in n and "lora_B" not in n)
    assert len(held) == 2 * len(pairs)


# ---------------------------------------------------------------------------------------------
# the config key
# ---------------------------------------------------------------------------------------------
def test_max_norm_from_config_accepts_and_refuses():
    from ltx_amd.training import max_norm_from_config
    assert max_norm_from_config(_config()) is None  # the key absent: off
    assert max_norm_from_config(_config(scale_weight_norms=None)) is None
    assert max_norm_from_config(_config(scale_weight_norms=0)) is None
    assert max_norm_from_config(_config(scale_weight_norms=0.0)) is None
    assert max_norm_from_config(_config(scale_weight_norms=1)) == 1.0
    got = max_norm_from_config(_config(scale_weight_norms=0.75))
    assert got == 0.75 and isinstance(got, float)
    for bad in (True, False, "1.0", -1, -0.5, float("inf"), float("nan"), [1.0]):
        with pytest.raises(ValueError, match="scale_weight_norms"):
            max_norm_from_config(_config(scale_weight_norms=bad))
    for extra in ({"train_mode": "full"}, {"use_deepspeed": True}):
        with pytest.raises(NotImplementedError, match="lora_audio"):
            max_norm_from_config(_config(scale_weight_norms=1.0, **extra))
        assert max_norm_from_config(_config(**extra)) is None  # off: nothing to refuse
        assert max_norm_from_config(_config(scale_weight_norms=0, **extra)) is None


def test_yaml_sets_the_key_only_when_present(tmp_path):
    from dataclasses import asdict, fields
    from ltx_amd.config import TrainConfig, load_train_config_from_yaml
    from ltx_amd.training import max_norm_from_config
    base = "checkpoint_path: x.safetensors\ntrain:\n  lora_rank: 8\n"
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(base + "  scale_weight_norms: 1.5\n")
    (tmp_path / "c.yaml").write_text(base + "  scale_weight_norms: 0\n")
    (tmp_path / "d.yaml").write_text(base + "  scale_weight_norms: \"1.5\"\n")
    (tmp_path / "e.yaml").write_text(base + "  scale_weight_norms: null\n")
    a, b, c, d, e = (load_train_config_from_yaml(str(tmp_path / f"{n}.yaml")) for n in "abcde")
    assert not hasattr(a, "scale_weight_norms") and b.scale_weight_norms == 1.5 and c.scale_weight_norms == 0
    assert e.scale_weight_norms is None
    assert asdict(a) == asdict(b) == asdict(c)
    assert "scale_weight_norms" not in {f.name for f in fields(TrainConfig)}
    for cfg in (a, b, c, d, e):
        cfg.train_mode = "lora_audio"
    assert max_norm_from_config(a) is None and max_norm_from_config(c) is None and max_norm_from_config(e) is None
    assert max_norm_from_config(b) == 1.5
    with pytest.raises(ValueError, match="scale_weight_norms"):  # passed on as written: a string is refused
        max_norm_from_config(d)
    gold = load_train_config_from_yaml(os.path.join(REPO, "tests", "golden", "train-avatars.yaml"))
    assert not hasattr(gold, "scale_weight_norms")


def test_train_loop_validates_the_key_before_anything_is_built(tmp_path):
    from ltx_amd.training import train_loop
    for extra, exc in (({"scale_weight_norms": -1.0}, ValueError), ({"scale_weight_norms": "2"}, ValueError),
                       ({"scale_weight_norms": 1.0, "train_mode": "full"}, NotImplementedError)):
        tc = _config(num_epochs=1, learning_rate=1e-3, output_dir=str(tmp_path), **extra)
        with pytest.raises(exc):
            train_loop(None, tc, [], torch.zeros(1, 4, 4096), torch.ones(1, 4, dtype=torch.long), device="cpu")
    assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------------------------------------
# the optimizers' keys and refusals
# ---------------------------------------------------------------------------------------------
def _pair_params(r=8, N=12, K=16):
    A, B = torch.nn.Parameter(torch.randn(r, K)), torch.nn.Parameter(torch.randn(N, r))
    return A, B


@pytest.mark.parametrize("kind", ["adamw", "prodigy"])
def test_the_key_enters_param_groups_only_when_on(kind):
    from ltx_amd.training import FusedAdamW, FusedProdigy, OptimizerSpec
    cls = FusedAdamW if kind == "adamw" else FusedProdigy
    A, B = _pair_params()
    extra = torch.nn.Parameter(torch.zeros(4))
    pairs = [("m", A, B, 0.5)]
    p = [A, B, extra]
    off, off2, off3 = cls(p), cls(p, scale_weight_norms=None), cls(p, scale_weight_norms=0, norm_pairs=pairs)
    on = cls(p, scale_weight_norms=2, norm_pairs=pairs)
    for o in (off, off2, off3):
        assert "scale_weight_norms" not in o.param_groups[0] and "scale_weight_norms" not in o.defaults
        assert o.norm_pairs is None and o._scale_weight_norms() == 0.0
    assert sorted(off.param_groups[0]) == sorted(off2.param_groups[0]) == sorted(off3.param_groups[0])
    assert on.param_groups[0]["scale_weight_norms"] == 2.0 and isinstance(on.param_groups[0]["scale_weight_norms"], float)
    assert sorted(set(on.param_groups[0]) - set(off.param_groups[0])) == ["scale_weight_norms"]
    assert on._scale_weight_norms() == 2.0 and on.norm_pairs == [("m", A, B, 0.5)]
    assert on.keys_scaled is None and on.avg_key_norm is None and on.max_key_norm is None  # nothing has stepped
    spec = OptimizerSpec(kind, 1e-3 if kind == "adamw" else 1.0, {})
    assert "scale_weight_norms" not in spec.build(p).param_groups[0]
    assert "scale_weight_norms" not in spec.build(p, scale_weight_norms=None, norm_pairs=None).param_groups[0]
    built = spec.build(p, scale_weight_norms=1.5, norm_pairs=pairs)
    assert built.param_groups[0]["scale_weight_norms"] == 1.5 and type(built) is cls


def test_constructor_refusals():
    from ltx_amd import _lib
    from ltx_amd.training import FusedAdamW
    A, B = _pair_params()
    A2, B2 = _pair_params()
    stranger = torch.nn.Parameter(torch.randn(8, 16))
    params = [A, B, A2, B2]
    ok = [("a", A, B, 1.0), ("b", A2, B2, 1.0)]
    FusedAdamW(params, scale_weight_norms=1.0, norm_pairs=ok)
    for cap in (1.0, 0.5):
        for none in (None, []):
            with pytest.raises(ValueError, match="without norm_pairs"):
                FusedAdamW(params, scale_weight_norms=cap, norm_pairs=none)
    for bad in (-1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="scale_weight_norms"):
            FusedAdamW(params, scale_weight_norms=bad, norm_pairs=ok)
    half = torch.nn.Parameter(torch.randn(8, 16).bfloat16())
    strided = torch.nn.Parameter(torch.randn(16, 8).t())
    plain = torch.randn(8, 16)
    cases = [
        ([("a", stranger, B, 1.0)], "not a parameter of this optimizer"),          # an unknown tensor
        ([("a", plain, B, 1.0)], "not a parameter of this optimizer"),             # not a parameter at all
        ([("a", A, B, 1.0), ("b", A, B2, 1.0)], "appears in two pairs"),           # a duplicate
        ([("a", A, B, 1.0), ("b", A2, B, 1.0)], "appears in two pairs"),
        ([("a", half, B, 1.0)], "contiguous f32"),                                 # a wrong dtype
        ([("a", strided, B, 1.0)], "contiguous f32"),
        ([("a", A, B2.detach().new_zeros(12, 16).requires_grad_(), 1.0)], "not a parameter"),
        ([("a", B, A, 1.0)], r"A \[r, K\] and B \[N, r\]"),                          # shapes that disagree
        ([("a", A, B, float("nan"))], "scaling must be finite"),
        ([(A, B, 1.0)], "tuples expected"),
    ]
    for pairs, match in cases:
        with pytest.raises(ValueError, match=match):
            FusedAdamW(params + [half, strided], scale_weight_norms=1.0, norm_pairs=pairs)
    # a rank outside ops.LORA_RANKS
    A3, B3 = torch.nn.Parameter(torch.randn(4, 16)), torch.nn.Parameter(torch.randn(12, 4))
    with pytest.raises(ValueError, match="r one of 8, 16, 32, 64, 128"):
        FusedAdamW([A3, B3], scale_weight_norms=1.0, norm_pairs=[("a", A3, B3, 1.0)])
    # the pass always takes the table path: a CPU parameter is an error, as under the clip and the guard
    opt = FusedAdamW(params, scale_weight_norms=1.0, norm_pairs=ok)
    for p in params:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in params]
    with pytest.raises(_lib.LtxHipError, match="scale_weight_norms"):
        opt.step()
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
    # groups that disagree
    opt = FusedAdamW([{"params": [A, B]}, {"params": [A2, B2], "scale_weight_norms": 2.0}], scale_weight_norms=1.0,
                     norm_pairs=ok)
    with pytest.raises(ValueError, match="scale_weight_norms differs"):
        opt.step()


# ---------------------------------------------------------------------------------------------
# the host tables and the library
# ---------------------------------------------------------------------------------------------
def test_layouts_stay_the_five_and_the_new_tables_are_their_own():
    from ltx_amd import ops, training
    assert sorted(training.LAYOUTS) == ["adamw", "ema", "prodigy", "sr", "swap"]
    assert len(training.MAX_NORM_PAIR) == ops.MAX_NORM_PAIR_FIELDS == 12
    assert training.MAX_NORM_ROW == ("param", "shadow or 0", "start", "count", "pair")
    assert len(training.MAX_NORM_ROW) == ops.MAX_NORM_ROW_FIELDS
    rows = training.max_norm_scale_rows([(5000, 0x1000, 0, 0), (16, 0x9000, 0xA000, 0), (2048, 0xB000, 0, 1)], 2048)
    assert rows == [(0x1000, 0, 0, 2048, 0), (0x1000, 0, 2048, 2048, 0), (0x1000, 0, 4096, 904, 0),
                    (0x9000, 0xA000, 0, 16, 0), (0xB000, 0, 0, 2048, 1)]


def test_pair_rows_follow_the_librarys_plan():
    """The plan: T = min(r, 64), the tiles on and above the diagonal, slabs of 1024 up to r = 16 and 2048 above;
    a pair's workgroups and partials lie behind the previous pair's, and the scaling travels as the f64's bits."""
    import struct
    from ltx_amd import ops, training
    shapes = [(16, 128, 8), (40, 136, 8), (2048, 64, 16), (1100, 2048, 16), (72, 200, 32), (100, 264, 64),
              (64, 8192, 128), (8192, 2048, 128)]
    pairs = [(0x10000 * (2 * i + 1), 0x10000 * (2 * i + 2), N, K, r, 0.25 * (i + 1)) for i, (N, K, r) in enumerate(shapes)]
    rows, nwg, ws = training.max_norm_pair_rows(pairs)
    at_wg = at_ws = 0
    for (a, b, N, K, r, s), row in zip(pairs, rows):
        T = min(r, 64)
        nt = r // T
        ntile, slab = nt * (nt + 1) // 2, 1024 if r <= 16 else 2048
        sa, sb = -(-K // slab), -(-N // slab)
        assert ops.max_norm_plan(N, K, r) == (slab, sa, sb, (sa + sb) * ntile, sa * ntile * T * T, sb * ntile * T * T)
        assert row == (a, b, N, K, r, struct.unpack("<q", struct.pack("<d", s))[0], at_ws, at_ws + sa * ntile * T * T,
                       at_wg, slab, sa, sb)
        at_wg += (sa + sb) * ntile
        at_ws += (sa + sb) * ntile * T * T
    assert (nwg, ws) == (at_wg, at_ws)
    assert ops.max_norm_plan(8192, 2048, 128)[4:] == (3 * 4096, 4 * 3 * 4096)  # 480 KiB of partials at the largest pair
    for r in (0, 4, 12, 24, 256):
        with pytest.raises(ValueError):
            ops.max_norm_plan(64, 64, r)


def test_library_exports_the_max_norm_entry_points():
    from ltx_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ltx_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib._SIGNATURES
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
    # host-side argument checks answer without a device
    assert lib.ltx_max_norm_sumsq(None, 1, 1, None, None, None) != 0
    assert lib.ltx_max_norm_finish(None, None, 1, 1.0, None, None, None, None) != 0
    assert lib.ltx_max_norm_scale_multi(None, 1, None, 0.0, None, None) != 0
