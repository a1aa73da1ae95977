"""LoRA dropout (peft lora_dropout), host side: the Philox4x32-10 generator against the published
Random123 known answers, the numpy statement of the keep mask the kernels regenerate
(lora.lora_dropout_mask_reference), the mask streams, and the surface: LoraLinear / inject_lora /
config.lora_dropout / the YAML key, with the errors raised before anything is replaced.
No GPU, no kernel launches."""
import json
import math
import os

import numpy as np
import pytest
import torch

from lora_ff_utils import train_config

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _tiny_cfg():
    with open(os.path.join(GOLD, "tiny_lora_ff_step.json")) as f:
        return json.load(f)["config"]


def _bare(device="meta"):
    from ltx_amd.transformer3d import Transformer3DModel
    with torch.device(device):
        return Transformer3DModel.from_config(_tiny_cfg())


def _wrapped(m):
    from ltx_amd.transformer3d import LoraLinear
    return [n for n, mod in m.named_modules() if isinstance(mod, LoraLinear)]


# the Random123 known-answer vectors of philox4x32-10 (kat_vectors): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    from ltx_amd.lora import philox4x32_10
    got = philox4x32_10(counter, key)
    assert tuple(int(v) for v in got) == want
    # vectorised: the same answers at every position of an array counter
    arr = philox4x32_10(tuple(np.full((3, 2), c, dtype=np.uint64) for c in counter), key)
    assert all(a.shape == (3, 2) and (a == w).all() for a, w in zip(arr, want))


def _scalar_philox(c, k):
    """Philox4x32-10 on python ints (a second statement, element by element)."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_mask_reference_is_the_per_element_statement():
    """One Philox call serves the 8 columns of a group: element (m, k) takes lane k % 8 of the call
    with counter (m, k // 8, sid, 0), low half of o[j // 2] for even j, high half for odd j."""
    from ltx_amd.lora import lora_dropout_mask_reference
    from ltx_amd.ops import lora_dropout_threshold
    key, sid, M, K, p = 0x0123456789ABCDEF, 37, 5, 24, 0.3
    T, c = lora_dropout_threshold(p)
    assert T == round(p * 65536) and c == float(np.float32(1.0) / (np.float32(1.0) - np.float32(T / 65536.0)))
    got = lora_dropout_mask_reference(key, sid, M, K, p)
    assert got.dtype == np.bool_ and got.shape == (M, K)
    for m in range(M):
        for k in range(K):
            o = _scalar_philox((m, k // 8, sid, 0), (key & 0xFFFFFFFF, key >> 32))
            j = k % 8
            lane = (o[j // 2] >> (16 * (j % 2))) & 0xFFFF
            assert bool(got[m, k]) == (lane >= T), (m, k)


def test_mask_reference_streams_keys_and_rate():
    from ltx_amd.lora import lora_dropout_mask_reference
    from ltx_amd.ops import lora_dropout_threshold
    a = lora_dropout_mask_reference(7, 3, 64, 128, 0.1)
    assert np.array_equal(a, lora_dropout_mask_reference(7, 3, 64, 128, 0.1))  # deterministic
    assert not np.array_equal(a, lora_dropout_mask_reference(7, 4, 64, 128, 0.1))  # another stream
    assert not np.array_equal(a, lora_dropout_mask_reference(8, 3, 64, 128, 0.1))  # another key
    assert not np.array_equal(a, lora_dropout_mask_reference(7 + (1 << 32), 3, 64, 128, 0.1))  # the key's high word
    # a larger M or K extends the mask, it does not reshuffle it
    assert np.array_equal(lora_dropout_mask_reference(7, 3, 80, 256, 0.1)[:64, :128], a)
    # the kept fraction over 2^20 elements: within 5 sigma (binomial) of the realised rate 1 - T / 65536
    T, _ = lora_dropout_threshold(0.1)
    q = 1.0 - T / 65536.0
    n = 1 << 20
    big = lora_dropout_mask_reference(0xDEADBEEFCAFEF00D, 21, 1024, 1024, 0.1)
    assert big.size == n
    assert abs(big.mean() - q) <= 5.0 * math.sqrt(q * (1.0 - q) / n)
    # the threshold is clamped into [1, 65535] for 0 < p < 1
    assert lora_dropout_threshold(1e-9)[0] == 1 and lora_dropout_threshold(1.0 - 1e-9)[0] == 65535
    with pytest.raises(ValueError):
        lora_dropout_mask_reference(7, 3, 8, 12, 0.1)  # K % 8


def test_dropout_streams_of_the_ten_slots():
    from ltx_amd.lora import LORA_DROPOUT_SLOTS, lora_dropout_stream
    slots = ["attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v",
             "attn2.to_out.0", "ff.net.0.proj", "ff.net.2"]
    assert list(LORA_DROPOUT_SLOTS) == slots
    for i in (0, 1, 27):
        for j, s in enumerate(slots):
            assert lora_dropout_stream(f"transformer_blocks.{i}.{s}") == 16 * i + j
    assert lora_dropout_stream("base_model.model.transformer_blocks.3.ff.net.2") == 57
    for bad in ("transformer_blocks.0.attn1.q_norm", "transformer_blocks.x.attn1.to_q", "proj_out"):
        with pytest.raises(ValueError):
            lora_dropout_stream(bad)


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5, True, "0.1"])
def test_dropout_outside_the_unit_interval_raises(p):
    from ltx_amd.lora import inject_lora, lora_target_modules
    from ltx_amd.transformer3d import LoraLinear
    m = _bare()
    with torch.device("meta"):
        with pytest.raises(ValueError, match="lora_dropout"):
            LoraLinear(m.transformer_blocks[0].attn2.to_q, 8, 8, p)
        with pytest.raises(ValueError, match="lora_dropout"):
            inject_lora(m, lora_target_modules(2), 8, 8, dropout=p)
    assert _wrapped(m) == []


def test_lora_linear_dropout_module_and_state_dict():
    from ltx_amd.transformer3d import LoraLinear
    m = _bare()
    with torch.device("meta"):
        base = m.transformer_blocks[0].attn2.to_q
        a, b, c = LoraLinear(base, 8, 8), LoraLinear(base, 8, 8, 0.0), LoraLinear(base, 8, 8, 0.25)
    for lin in (a, b):
        assert type(lin.lora_dropout["default"]) is torch.nn.Identity and lin.lora_dropout_p == 0.0
    assert type(c.lora_dropout["default"]) is torch.nn.Dropout and c.lora_dropout["default"].p == 0.25
    assert isinstance(c.lora_dropout, torch.nn.ModuleDict) and list(c.lora_dropout) == ["default"]
    # no parameters, no buffers: the state dict is that of p = 0
    assert list(c.state_dict()) == list(a.state_dict()) == [
        "base_layer.weight", "base_layer.bias", "lora_A.default.weight", "lora_B.default.weight"]


def test_inject_lora_and_config_carry_the_rate():
    from ltx_amd.lora import apply_training_strategy, inject_lora, lora_ff_target_modules, lora_target_modules
    from ltx_amd.transformer3d import LoraLinear, _block_dropout
    m = _bare()
    with torch.device("meta"):
        inject_lora(m, lora_target_modules(2, "attn1+attn2") + lora_ff_target_modules(2), 8, 8, feed_forward=True,
                    dropout=0.1)
    lins = [x for x in m.modules() if isinstance(x, LoraLinear)]
    assert len(lins) == 20 and all(x.lora_dropout_p == 0.1 and x.lora_dropout["default"].p == 0.1 for x in lins)
    assert [_block_dropout(b) for b in m.transformer_blocks] == [0.1, 0.1]
    # config.lora_dropout (setattr, like lora_targets / lora_ff); absent = 0.0, and not a TrainConfig field
    from ltx_amd.config import TrainConfig
    assert not hasattr(TrainConfig(checkpoint_path="-"), "lora_dropout")
    a, b, c = _bare(), _bare(), _bare()
    tc = train_config(8, "attn1+attn2", True)
    setattr(tc, "lora_dropout", 0.25)
    tz = train_config(8, "attn1+attn2", True)
    setattr(tz, "lora_dropout", 0.0)
    with torch.device("meta"):
        apply_training_strategy(a, tc, "lora_audio")
        apply_training_strategy(b, train_config(8, "attn1+attn2", True), "lora_audio")
        apply_training_strategy(c, tz, "lora_audio")
    assert all(x.lora_dropout_p == 0.25 for x in a.modules() if isinstance(x, LoraLinear))
    assert all(x.lora_dropout_p == 0.0 for mm in (b, c) for x in mm.modules() if isinstance(x, LoraLinear))
    assert [_block_dropout(blk) for blk in b.transformer_blocks] == [0.0, 0.0]
    # the same parameters, names and trainability with and without the rate
    sig = lambda mm: [(n, tuple(p.shape), p.dtype, p.requires_grad) for n, p in mm.named_parameters()]
    assert sig(a) == sig(b) == sig(c) and list(a.state_dict()) == list(b.state_dict())
    bad = train_config(8)
    setattr(bad, "lora_dropout", 1.0)
    d = _bare()
    with torch.device("meta"), pytest.raises(ValueError, match="lora_dropout"):
        apply_training_strategy(d, bad, "lora_audio")
    assert _wrapped(d) == []
    # train_mode='full' does not read it
    e = _bare()
    apply_training_strategy(e, bad, "full")
    assert _wrapped(e) == []


def test_mixed_rates_in_a_block_raise_before_anything_is_replaced():
    from ltx_amd.lora import inject_lora, lora_ff_target_modules, lora_target_modules
    from ltx_amd.transformer3d import _block_dropout
    m = _bare()
    with torch.device("meta"):
        inject_lora(m, lora_target_modules(2, "attn2"), 8, 8, dropout=0.1)
        before = _wrapped(m)
        with pytest.raises(NotImplementedError, match="share one rate"):
            inject_lora(m, lora_target_modules(2, "attn1"), 8, 8, dropout=0.2)
        with pytest.raises(NotImplementedError, match="share one rate"):
            inject_lora(m, lora_ff_target_modules(2), 8, 8, feed_forward=True)  # 0.0 beside 0.1
        assert _wrapped(m) == before
        inject_lora(m, lora_target_modules(2, "attn1"), 8, 8, dropout=0.1)  # the same rate is accepted
        assert len(_wrapped(m)) == 16
        # the block refuses mixed rates whoever built it
        m.transformer_blocks[1].attn1.to_q.lora_dropout_p = 0.3
        with pytest.raises(NotImplementedError, match="share one lora_dropout"):
            _block_dropout(m.transformer_blocks[1])
        assert _block_dropout(m.transformer_blocks[0]) == 0.1


def test_yaml_sets_lora_dropout_only_when_present(tmp_path):
    from dataclasses import asdict
    from ltx_amd.config import load_train_config_from_yaml
    base = "checkpoint_path: x.safetensors\ntrain:\n  lora_rank: 16\n"
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(base + "  lora_dropout: 0.1\n")
    a = load_train_config_from_yaml(str(tmp_path / "a.yaml"))
    b = load_train_config_from_yaml(str(tmp_path / "b.yaml"))
    assert not hasattr(a, "lora_dropout") and b.lora_dropout == 0.1 and isinstance(b.lora_dropout, float)
    assert asdict(a) == asdict(b) and "lora_dropout" not in asdict(b)


def test_processor_keeps_refusing_peft_dropout():
    """The plug-in path (HipAttnProcessor on a peft-wrapped module) is out of scope: p > 0 in training
    mode raises, eval() passes the check."""
    from ltx_amd.processor import _linear_parts
    from ltx_amd.transformer3d import LoraLinear
    lin = LoraLinear(torch.nn.Linear(16, 16), 8, 8, 0.1)
    lin.train()
    with pytest.raises(NotImplementedError, match="dropout"):
        _linear_parts(lin)
    lin.eval()
    assert _linear_parts(lin)[2] is lin.lora_A["default"].weight
