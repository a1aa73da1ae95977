"""Stochastically rounded bf16 weights (FusedAdamW / FusedProdigy bf16_update="stochastic"), host side:
training.stochastic_round_bf16, the CPU statement of the rounding and of its random numbers, and the
constructor and config surface with its errors. No GPU, no kernel launches."""
import numpy as np
import pytest
import torch

from bf16_sr_utils import philox_scalar, sr_bits_scalar


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# finite values over the exponent range (a subnormal and the largest finite bf16 among them) whose low 16
# bits are not zero, so each lies strictly between two bf16 neighbours
INEXACT = np.array([1.0 + 2.0 ** -9, 3.14159274, 1e-3, 65504.3, 2.0 ** -130 * 1.3, 1.0000001, 0.03 + 1e-6,
                    float(np.uint32(0x7F7F0001).view(np.float32))], dtype=np.float32)
EXACT = np.array([0.0, 1.0, -1.0, 0.03125, 1.0078125, 3.3895314e38, 2.0 ** -133, -0.0], dtype=np.float32)


def test_r_zero_truncates_toward_zero_and_the_result_is_a_neighbour():
    from ltx_amd.training import stochastic_round_bf16
    for x in (INEXACT, -INEXACT):
        lo = (_bits(x) >> 16).astype(np.uint16)  # the neighbour toward zero; the other one is one pattern up
        assert ((_bits(x) & 0xFFFF) != 0).all()
        assert np.array_equal(stochastic_round_bf16(x, 0, 0, 1, r=0), lo)
        assert np.array_equal(stochastic_round_bf16(x, 0, 0, 1, r=0xFFFF), lo + 1)
        for seed in range(20):
            got = stochastic_round_bf16(x, seed, 3, 5)
            assert got.dtype == np.uint16 and ((got == lo) | (got == lo + 1)).all()
    # the threshold: up exactly when r reaches 2^16 - the discarded bits
    x = np.array([1.0 + 2.0 ** -9], dtype=np.float32)  # discards 0x4000
    assert stochastic_round_bf16(x, 0, 0, 1, r=0xBFFF)[0] == 0x3F80
    assert stochastic_round_bf16(x, 0, 0, 1, r=0xC000)[0] == 0x3F81


def test_representable_values_stay_for_every_r():
    from ltx_amd.training import stochastic_round_bf16
    assert ((_bits(EXACT) & 0xFFFF) == 0).all()
    for r in (0, 1, 0x7FFF, 0xFFFF):
        assert np.array_equal(stochastic_round_bf16(EXACT, 0, 0, 1, r=r), (_bits(EXACT) >> 16).astype(np.uint16))
    for seed in (0, 1, 2 ** 64 - 1):
        assert np.array_equal(stochastic_round_bf16(EXACT, seed, 7, 9), (_bits(EXACT) >> 16).astype(np.uint16))


def test_rounding_is_symmetric_in_sign():
    from ltx_amd.training import stochastic_round_bf16
    g = np.random.default_rng(0)
    x = (g.standard_normal(4096) * np.exp(g.uniform(-20, 20, 4096))).astype(np.float32)
    pos, neg = stochastic_round_bf16(x, 11, 2, 3), stochastic_round_bf16(-x, 11, 2, 3)
    assert np.array_equal(pos ^ np.uint16(0x8000), neg)
    # and as tensors: the same bits, as bf16 values
    t = stochastic_round_bf16(torch.from_numpy(x).view(64, 64), 11, 2, 3)
    assert t.dtype == torch.bfloat16 and t.shape == (64, 64)
    assert np.array_equal(t.view(torch.int16).numpy().view(np.uint16).reshape(-1), pos)
    assert torch.equal(stochastic_round_bf16(torch.from_numpy(-x).view(64, 64), 11, 2, 3), -t)


def test_nan_and_infinities_pass_through():
    from ltx_amd.training import stochastic_round_bf16
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), 1.0 + 2.0 ** -9])
    for r in (None, 0, 0xFFFF):
        got = stochastic_round_bf16(x, 5, 0, 1, r=r)
        assert torch.isnan(got[0]) and got[1] == float("inf") and got[2] == float("-inf")
        assert float(got[3]) in (1.0, 1.0078125)
    with pytest.raises(TypeError):
        stochastic_round_bf16(x.double(), 5, 0, 1)


def test_known_answer_of_the_scalar_philox():
    """the scalar statement is Philox4x32-10: a Random123 known-answer vector"""
    assert philox_scalar((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


@pytest.mark.parametrize("seed,ordinal,step", [(0, 0, 1), (1, 0, 1), (0x0123456789ABCDEF, 37, 5),
                                                (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 + 3)])
def test_random_bits_are_the_scalar_statements(seed, ordinal, step):
    """Element i's r under (seed, ordinal, step), for i below and above 2^35 (where i >> 3 needs the
    counter's second word) and lanes 0 and 7 of a call among them; the step enters mod 2^32."""
    from ltx_amd.training import stochastic_round_bits, stochastic_round_bf16
    idx = [0, 7, 8, 13, 2047, 2048, 2 ** 35 - 8, 2 ** 35 - 1, 2 ** 35, 2 ** 35 + 7, 2 ** 40 + 3, 2 ** 62 + 16 + 7]
    want = [sr_bits_scalar(seed, ordinal, step, i) for i in idx]
    got = stochastic_round_bits(seed, ordinal, step, idx)
    assert got.shape == (len(idx),) and [int(v) for v in got] == want
    assert all(0 <= v < 2 ** 16 for v in want) and len(set(want)) > len(want) // 2
    assert np.array_equal(got, stochastic_round_bits(seed, ordinal, step % 2 ** 32, idx))
    # the rounding of a tensor uses element i's number
    x = np.full(32, 1.0 + 2.0 ** -9, dtype=np.float32)
    r = [sr_bits_scalar(seed, ordinal, step, i) for i in range(32)]
    assert np.array_equal(stochastic_round_bf16(x, seed, ordinal, step),
                          np.array([0x3F81 if v >= 0xC000 else 0x3F80 for v in r], dtype=np.uint16))
    # another ordinal, step or seed is another stream
    base = stochastic_round_bits(seed, ordinal, step, np.arange(64))
    assert not np.array_equal(base, stochastic_round_bits(seed, ordinal ^ 1, step, np.arange(64)))
    assert not np.array_equal(base, stochastic_round_bits(seed, ordinal, step + 1, np.arange(64)))
    assert not np.array_equal(base, stochastic_round_bits(seed ^ (1 << 40), ordinal, step, np.arange(64)))


@pytest.mark.parametrize("seed", [1, 12345])
def test_rounding_is_unbiased(seed):
    """65 536 copies of 1 + 2^-9 (a quarter of the way to the next bf16): the share rounded up is a
    binomial mean with sigma = sqrt(0.25 0.75 / N) = 0.0017; within 5 sigma of 0.25."""
    from ltx_amd.training import stochastic_round_bf16
    n = 65536
    got = stochastic_round_bf16(np.full(n, 1.0 + 2.0 ** -9, dtype=np.float32), seed, 0, 1)
    assert set(np.unique(got)) == {0x3F80, 0x3F81}
    share = float((got == 0x3F81).mean())
    sigma = (0.25 * 0.75 / n) ** 0.5
    print(f"seed {seed}: share rounded up {share:.6f}, {(share - 0.25) / sigma:+.2f} sigma")
    assert abs(share - 0.25) <= 5 * sigma


# ---------------------------------------------------------------------------------------------
# constructors and config
# ---------------------------------------------------------------------------------------------
def _config(**extra):
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="-")
    tc.train_mode = "lora_audio"
    for k, v in extra.items():
        setattr(tc, k, v)
    return tc


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedProdigy"])
def test_constructor_errors_and_param_groups(cls):
    from ltx_amd import training
    from ltx_amd._lib import LtxHipError
    make = getattr(training, cls)
    p = lambda dt=torch.bfloat16: [torch.nn.Parameter(torch.ones(16, dtype=dt))]
    with pytest.raises(ValueError, match="bf16_update"):
        make(p(), bf16_update="truncate")
    for seed in (-1, 2 ** 64, 1.5, "7", True):
        with pytest.raises(ValueError, match="sr_seed"):
            make(p(), bf16_update="stochastic", sr_seed=seed)
    # the two values enter param_groups in stochastic mode only
    today = set(make(p()).param_groups[0])
    assert set(make(p(), bf16_update="nearest").param_groups[0]) == today
    assert not {"bf16_update", "sr_seed"} & today
    opt = make(p(), bf16_update="stochastic", sr_seed=2 ** 64 - 1)
    group = opt.param_groups[0]
    assert set(group) == today | {"bf16_update", "sr_seed"}
    assert group["bf16_update"] == "stochastic" and group["sr_seed"] == 2 ** 64 - 1
    # a CPU parameter: the mode has table kernels only
    params = p()
    opt = make(params, bf16_update="stochastic")
    params[0].grad = torch.ones_like(params[0])
    with pytest.raises(LtxHipError):
        opt.step()


def test_config_keys_reach_the_constructor_only_in_stochastic_mode():
    from ltx_amd.training import OptimizerSpec, optimizer_from_config
    spec = optimizer_from_config(_config())
    assert isinstance(spec, OptimizerSpec) and spec.kind == "adamw" and spec.kwargs == {}
    assert optimizer_from_config(_config(bf16_update="nearest")).kwargs == {}
    assert optimizer_from_config(_config(optimizer="prodigy")).kwargs == {}
    spec = optimizer_from_config(_config(bf16_update="stochastic"))
    assert spec.kwargs == {"bf16_update": "stochastic", "sr_seed": 0}
    spec = optimizer_from_config(_config(bf16_update="stochastic", bf16_sr_seed=2 ** 63 + 5, optimizer="prodigy",
                                         prodigy_d0=1e-5, weight_decay=0.0))
    assert spec.kind == "prodigy"
    assert spec.kwargs == {"bf16_update": "stochastic", "sr_seed": 2 ** 63 + 5, "d0": 1e-5, "weight_decay": 0.0}
    opt = spec.build([torch.nn.Parameter(torch.ones(8, dtype=torch.bfloat16))])
    assert opt.bf16_update == "stochastic" and opt.sr_seed == 2 ** 63 + 5


def test_config_errors():
    from ltx_amd.training import optimizer_from_config
    with pytest.raises(ValueError, match="bf16_update"):
        optimizer_from_config(_config(bf16_update="sr"))
    for seed in (-1, 2 ** 64, 0.5):
        with pytest.raises(ValueError, match="sr_seed"):
            optimizer_from_config(_config(bf16_update="stochastic", bf16_sr_seed=seed))
    for extra in ({}, {"bf16_update": "nearest"}):
        with pytest.raises(ValueError, match="without bf16_update"):
            optimizer_from_config(_config(bf16_sr_seed=3, **extra))
    tc = _config(bf16_update="stochastic")
    tc.train_mode = "full"
    with pytest.raises(NotImplementedError):
        optimizer_from_config(tc)
    with pytest.raises(NotImplementedError):
        optimizer_from_config(_config(bf16_update="stochastic", use_deepspeed=True))


def test_yaml_keys_are_read_like_the_other_optional_keys(tmp_path):
    """train.bf16_update / train.bf16_sr_seed in the YAML reach the config object, where
    optimizer_from_config reads them; absent keys set nothing"""
    from ltx_amd.config import load_train_config_from_yaml
    from ltx_amd.training import optimizer_from_config
    path = tmp_path / "c.yaml"
    path.write_text("checkpoint_path: x\ntrain:\n  bf16_update: stochastic\n  bf16_sr_seed: 18446744073709551615\n")
    tc = load_train_config_from_yaml(str(path))
    tc.train_mode = "lora_audio"  # set by the CLI
    assert optimizer_from_config(tc).kwargs == {"bf16_update": "stochastic", "sr_seed": 2 ** 64 - 1}
    path.write_text("checkpoint_path: x\ntrain:\n  bf16_update: stochastic\n  bf16_sr_seed: 0.5\n")
    with pytest.raises(ValueError, match="sr_seed"):
        optimizer_from_config(load_train_config_from_yaml(str(path)))
    path.write_text("checkpoint_path: x\ntrain:\n  batch_size: 1\n")
    tc = load_train_config_from_yaml(str(path))
    assert not hasattr(tc, "bf16_update") and not hasattr(tc, "bf16_sr_seed")
