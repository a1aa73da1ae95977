"""Prodigy for the LoRA optimizer step, host side: the config keys (setattr and YAML, read only when
present), optimizer_from_config's validation ahead of anything being built, the statement itself
(tests/prodigy_utils.ProdigyStatement) against the formulae recomputed in plain Python floats, and the
adapter directory's "prodigy" block with the loads that read and refuse it. Models are the tiny config on
the CPU (parameters only); the fused step itself needs the GPU (tests/test_prodigy_gpu.py). No GPU, no
kernel launches."""
import json
import math
import os
import types

import pytest
import torch
from safetensors.torch import load_file

from prodigy_utils import ProdigyStatement
from test_adapter_ckpt_cpu import CASES, _model, _optimizer, _refused, _same, _trainable

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KEYS = ("optimizer", "weight_decay", "adam_beta1", "adam_beta2", "adam_eps", "prodigy_d0", "prodigy_d_coef",
            "prodigy_growth_rate", "prodigy_beta3", "prodigy_use_bias_correction", "prodigy_safeguard_warmup",
            "prodigy_decouple")
FOUR = ["adapter_config.json", "adapter_model.safetensors", "optimizer.safetensors", "train_state.json"]


def _tc(mode="lora_audio", lr=1e-3, **kw):
    from ltx_amd.config import TrainConfig
    tc = TrainConfig(checkpoint_path="-", learning_rate=lr, num_epochs=1)
    tc.train_mode = mode
    for k, v in kw.items():
        setattr(tc, k, v)
    return tc


# ---------------------------------------------------------------------------------------------
# config keys
# ---------------------------------------------------------------------------------------------
def test_absent_keys_build_fused_adamw_with_todays_defaults():
    from dataclasses import fields
    from ltx_amd.config import TrainConfig
    from ltx_amd.training import FusedAdamW, FusedProdigy, optimizer_from_config
    bare = _tc()
    assert not any(hasattr(bare, k) for k in NEW_KEYS)
    assert not set(NEW_KEYS) & {f.name for f in fields(TrainConfig)}
    p = torch.nn.Parameter(torch.zeros(3))
    for cfg in (bare, _tc(optimizer="adamw")):
        spec = optimizer_from_config(cfg)
        assert spec.kind == "adamw" and spec.kwargs == {} and spec.lr == 1e-3
        opt = spec.build([p], max_grad_norm=None, ema=None)
        assert type(opt) is FusedAdamW
        g = opt.param_groups[0]
        assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 1e-2)
    opt = optimizer_from_config(_tc(weight_decay=0.0, adam_beta2=0.95, adam_eps=1e-6)).build([p])
    g = opt.param_groups[0]
    assert type(opt) is FusedAdamW and (g["betas"], g["eps"], g["weight_decay"]) == ((0.9, 0.95), 1e-6, 0.0)
    # Prodigy: the published defaults; learning_rate null means 1.0
    opt = optimizer_from_config(_tc(lr=None, optimizer="prodigy")).build([p], max_grad_norm=1.0)
    g = opt.param_groups[0]
    assert type(opt) is FusedProdigy and g["max_grad_norm"] == 1.0
    assert (g["lr"], g["betas"], g["beta3"], g["eps"], g["weight_decay"], g["decouple"], g["use_bias_correction"],
            g["safeguard_warmup"], g["d0"], g["d_coef"], g["growth_rate"]) == \
        (1.0, (0.9, 0.999), None, 1e-8, 0.0, True, False, False, 1e-6, 1.0, float("inf"))
    opt = optimizer_from_config(_tc(lr=0.5, optimizer="prodigy", weight_decay=0.01, adam_beta1=0.8, prodigy_d0=1e-5,
                                    prodigy_d_coef=2.0, prodigy_growth_rate=1.02, prodigy_beta3=0.9,
                                    prodigy_use_bias_correction=True, prodigy_safeguard_warmup=True,
                                    prodigy_decouple=False)).build([p])
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["beta3"], g["weight_decay"], g["decouple"], g["use_bias_correction"],
            g["safeguard_warmup"], g["d0"], g["d_coef"], g["growth_rate"]) == \
        (0.5, (0.8, 0.999), 0.9, 0.01, False, True, True, 1e-5, 2.0, 1.02)
    with pytest.raises(ValueError, match="one parameter group"):
        FusedProdigy([{"params": [p]}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])


def test_yaml_sets_the_keys_only_when_present(tmp_path):
    from dataclasses import asdict
    from ltx_amd.config import load_train_config_from_yaml
    base = "checkpoint_path: x.safetensors\ntrain:\n  lora_rank: 16\n"
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(
        base + "  learning_rate: null\n  optimizer: prodigy\n  weight_decay: 0.01\n  adam_beta1: 0.8\n  adam_beta2: 0.99\n"
               "  adam_eps: 1.0e-6\n  prodigy_d0: 1.0e-5\n  prodigy_d_coef: 2\n  prodigy_growth_rate: 1.02\n"
               "  prodigy_beta3: 0.9\n  prodigy_use_bias_correction: true\n  prodigy_safeguard_warmup: true\n"
               "  prodigy_decouple: false\n")
    (tmp_path / "c.yaml").write_text(base + "  optimizer: adamw\n")
    a, b, c = (load_train_config_from_yaml(str(tmp_path / f"{n}.yaml")) for n in "abc")
    assert not any(hasattr(a, k) for k in NEW_KEYS)
    assert [getattr(b, k) for k in NEW_KEYS] == ["prodigy", 0.01, 0.8, 0.99, 1e-6, 1e-5, 2.0, 1.02, 0.9, True, True, False]
    assert isinstance(b.prodigy_d_coef, float) and b.prodigy_decouple is False and b.learning_rate is None
    assert c.optimizer == "adamw" and not any(hasattr(c, k) for k in NEW_KEYS[1:])
    assert asdict(a) == asdict(b) == asdict(c)
    gold = load_train_config_from_yaml(os.path.join(REPO, "tests", "golden", "train-avatars.yaml"))
    assert not any(hasattr(gold, k) for k in NEW_KEYS)


BAD = (({"optimizer": "lion"}, ValueError, "optimizer"),
       ({"optimizer": "Prodigy"}, ValueError, "optimizer"),
       ({"adam_beta1": 1.0}, ValueError, "adam_beta1"),
       ({"adam_beta2": -0.1}, ValueError, "adam_beta"),
       ({"adam_eps": 0.0}, ValueError, "adam_eps"),
       ({"weight_decay": -1.0}, ValueError, "weight_decay"),
       ({"prodigy_d0": 1e-5}, ValueError, "without optimizer: prodigy"),
       ({"optimizer": "prodigy", "prodigy_d0": 0.0}, ValueError, "prodigy_d0"),
       ({"optimizer": "prodigy", "prodigy_d_coef": -1.0}, ValueError, "prodigy_d_coef"),
       ({"optimizer": "prodigy", "prodigy_growth_rate": 0.0}, ValueError, "prodigy_growth_rate"),
       ({"optimizer": "prodigy", "prodigy_beta3": 1.0}, ValueError, "prodigy_beta3"),
       ({"optimizer": "prodigy", "use_deepspeed": True}, NotImplementedError, "use_deepspeed"))


def test_config_errors():
    from ltx_amd.training import optimizer_from_config
    for kw, exc, match in BAD:
        with pytest.raises(exc, match=match):
            optimizer_from_config(_tc(**kw))
    with pytest.raises(NotImplementedError, match="lora_audio"):
        optimizer_from_config(_tc("full", optimizer="prodigy"))
    assert optimizer_from_config(_tc("full")).kind == "adamw"  # AdamW stays available in every mode


def test_train_loop_raises_before_touching_the_model(monkeypatch):
    """train_loop reads the keys before it builds anything: a bad one raises with an empty loader, a
    model it never looks into, and no optimizer constructed."""
    from ltx_amd import training

    class Model(torch.nn.Module):
        patchifier = None
        device = "cpu"

        def parameters(self, recurse=True):
            raise AssertionError("the model was looked into")

    def no_optimizer(*a, **k):
        raise AssertionError("an optimizer was built")
    monkeypatch.setattr(training, "FusedAdamW", no_optimizer)
    monkeypatch.setattr(training, "FusedProdigy", no_optimizer)
    args = ([], torch.zeros(1, 4, 8), torch.ones(1, 4, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="lora_audio"):
        training.train_loop(Model(), _tc("full", optimizer="prodigy"), *args, device="cpu")
    for kw, exc, match in BAD:
        with pytest.raises(exc, match=match):
            training.train_loop(Model(), _tc(**kw), *args, device="cpu")


def test_train_loop_builds_what_the_keys_name(monkeypatch):
    """Absent keys: FusedAdamW(params, lr=, max_grad_norm=, ema=) and nothing else, today's call; with
    `optimizer: prodigy` FusedProdigy, and a schedule whose base rate is Prodigy's 1.0 for
    learning_rate null. The loader is empty, so no step runs."""
    from ltx_amd import training
    seen = []

    def recording(cls):
        class Recording(cls):
            def __init__(self, *a, **k):
                seen.append((cls.__name__, sorted(k), k.get("lr")))
                super().__init__(*a, **k)
        return Recording
    monkeypatch.setattr(training, "FusedAdamW", recording(training.FusedAdamW))
    monkeypatch.setattr(training, "FusedProdigy", recording(training.FusedProdigy))
    m = _model(CASES["attn2"], seed=1)
    args = ([], torch.zeros(1, 4, 4096), torch.ones(1, 4, dtype=torch.long))
    training.train_loop(m, _tc(), *args, device="cpu")
    training.train_loop(m, _tc(optimizer="adamw"), *args, device="cpu")
    training.train_loop(m, _tc(adam_eps=1e-6), *args, device="cpu")
    training.train_loop(m, _tc(lr=None, optimizer="prodigy", lr_scheduler="cosine", lr_total_steps=10, prodigy_d0=1e-5),
                        *args, device="cpu")
    today = ("FusedAdamW", ["ema", "lr", "max_grad_norm"], 1e-3)
    assert seen[0] == today and seen[1] == today
    assert seen[2] == ("FusedAdamW", ["ema", "eps", "lr", "max_grad_norm"], 1e-3)
    assert seen[3] == ("FusedProdigy", ["d0", "ema", "lr", "max_grad_norm"], 1.0)


# ---------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------
def _by_hand(ps, p0s, grads_per_step, lr, beta1, beta2, eps, d0, wd=0.0, decouple=True):
    """The statement's formulae in plain Python floats, element by element: (parameters, d, d_numerator)
    after every step."""
    beta3 = math.sqrt(beta2)
    n = len(ps)
    m, v, s = [0.0] * n, [0.0] * n, [0.0] * n
    d = d_max = d0
    d_num, k = 0.0, 0
    out = []
    for grads in grads_per_step:
        dlr = d * lr * 1.0
        if lr != 0:
            num = den = 0.0
            for i, g in enumerate(grads):
                if wd != 0 and not decouple:
                    g = g + wd * ps[i]
                num += (p0s[i] - ps[i]) * g
                m[i] = m[i] * beta1 + d * (1 - beta1) * g
                v[i] = v[i] * beta2 + d * d * (1 - beta2) * g * g
                s[i] = s[i] * beta3 + (d / d0) * dlr * g
                den += abs(s[i])
            if den != 0:
                d_num = beta3 * d_num + (d / d0) * dlr * num
                d_hat = 1.0 * d_num / den
                if d == d0:
                    d = max(d, d_hat)
                d_max = max(d_max, d_hat)
                d = min(d_max, d * float("inf"))
                k += 1
                for i in range(n):
                    den_i = math.sqrt(v[i]) + d * eps
                    if wd != 0 and decouple:
                        ps[i] = ps[i] + (-wd * dlr) * ps[i]
                    ps[i] = ps[i] + (-dlr) * (m[i] / den_i)
        out.append((list(ps), d, d_num, k))
    return out


# Tolerance of the float64 comparisons below: the statement runs torch's float64 CPU ops, which may fuse
# a multiply-add (alpha * g + x in one rounding) where plain Python rounds twice; every value is the result
# of at most a few dozen float64 operations without cancellation, each within 2^-53 relative of either
# evaluation, so the two agree to far better than 1e-12 relative, while a wrong formula (a missing factor,
# beta in place of 1 - beta, the old d in place of the new one) is off by parts in ten at least.
REL = 1e-12


@pytest.mark.parametrize("wd, decouple", [(0.0, True), (0.1, True), (0.1, False)])
def test_statement_on_a_hand_sized_problem(wd, decouple):
    a = torch.nn.Parameter(torch.tensor([0.5, -1.25], dtype=torch.float64))
    b = torch.nn.Parameter(torch.tensor([2.0, 0.75, -0.5], dtype=torch.float64))
    steps = [[0.3, -0.7, 1.1, 0.2, -0.9], [0.25, -0.6, 0.9, 0.35, -1.0], [0.2, -0.4, 1.0, 0.1, -0.8]]
    lr, beta1, beta2, eps, d0 = 1.0, 0.9, 0.999, 1e-8, 1e-6
    st = ProdigyStatement([a, b], lr=lr, betas=(beta1, beta2), eps=eps, d0=d0, weight_decay=wd, decouple=decouple)
    p0 = a.tolist() + b.tolist()
    want = _by_hand(list(p0), list(p0), steps, lr, beta1, beta2, eps, d0, wd, decouple)
    ds = []
    for g, (ps, d, d_num, k) in zip(steps, want):
        st.step([torch.tensor(g[:2], dtype=torch.float64), torch.tensor(g[2:], dtype=torch.float64)])
        assert a.tolist() + b.tolist() == pytest.approx(ps, rel=REL, abs=0)
        assert st.d == pytest.approx(d, rel=REL, abs=0) and st.d_numerator == pytest.approx(d_num, rel=REL, abs=0)
        assert st.k == k and st.applied
        ds.append(st.d)
    # the first step has p0 == p: the numerator is 0 and d stays at d0; later d grows above it
    assert ds[0] == d0 and ds[2] > ds[1] > d0
    assert a.tolist() + b.tolist() != p0
    for p in (a, b):
        assert torch.equal(st.state[p]["p0"], torch.tensor(p0[:2] if p is a else p0[2:], dtype=torch.float64))
        assert st.state[p]["exp_avg"].dtype == torch.float64


def test_statement_zero_gradient_and_zero_lr_steps_change_nothing():
    a = torch.nn.Parameter(torch.tensor([0.5, -1.25], dtype=torch.float64))
    b = torch.nn.Parameter(torch.tensor([2.0, 0.75, -0.5], dtype=torch.float64))
    start = [a.detach().clone(), b.detach().clone()]
    st = ProdigyStatement([a, b])
    st.step([torch.zeros(2, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)])
    assert not st.applied and st.d_denom == 0.0
    assert (st.d, st.d_max, st.d_numerator, st.k) == (1e-6, 1e-6, 0.0, 0)
    assert torch.equal(a, start[0]) and torch.equal(b, start[1])
    for p in (a, b):
        assert all(not st.state[p][key].any() for key in ("exp_avg", "exp_avg_sq", "s"))
    st.lr = 0.0
    st.step([torch.ones(2, dtype=torch.float64), torch.ones(3, dtype=torch.float64)])
    assert (st.d, st.d_max, st.d_numerator, st.k) == (1e-6, 1e-6, 0.0, 0)
    assert torch.equal(a, start[0]) and torch.equal(b, start[1])
    for p in (a, b):
        assert all(not st.state[p][key].any() for key in ("exp_avg", "exp_avg_sq", "s"))
    # a parameter without a gradient keeps everything while the other one steps
    st.lr = 1.0
    st.step([None, torch.ones(3, dtype=torch.float64)])
    assert st.applied and st.k == 1 and torch.equal(a, start[0]) and not torch.equal(b, start[1])
    assert a not in st.state or not st.state[a]["s"].any()


def test_fused_prodigy_host_side():
    from ltx_amd import _lib
    from ltx_amd.training import FusedProdigy
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedProdigy([p])
    assert opt.RECORD == ("d", "d_max", "d_numerator", "d_denom", "d_hat", "dlr", "k", "applied")
    rec = opt.ensure_record()
    assert rec.dtype == torch.float64 and rec.tolist() == [1e-6, 1e-6, 0, 0, 0, 0, 0, 0]
    assert opt.d.dim() == 0 and float(opt.d) == 1e-6 and opt.d.data_ptr() == rec.data_ptr()
    p.grad = torch.ones(4)
    with pytest.raises(_lib.LtxHipError):
        opt.step()  # the table kernels need the device
    assert not opt.state[p]  # raised before any state was created
    opt.param_groups[0]["lr"] = 0.0
    opt.step()  # lr == 0: nothing is launched, so nothing needs the device
    assert not opt.state[p] and rec.tolist() == [1e-6, 1e-6, 0, 0, 0, 0, 0, 0]
    for kw, match in (({"betas": (1.0, 0.999)}, "betas"), ({"beta3": 1.0}, "beta3"), ({"eps": 0.0}, "eps"),
                      ({"weight_decay": -1.0}, "weight_decay"), ({"d0": 0.0}, "d0"), ({"d_coef": 0.0}, "d_coef"),
                      ({"growth_rate": 0.0}, "growth_rate"), ({"max_grad_norm": -1.0}, "max_grad_norm")):
        with pytest.raises(ValueError, match=match):
            FusedProdigy([p], **kw)
    with pytest.raises(TypeError, match="EMASchedule"):
        FusedProdigy([p], ema=0.999)


# ---------------------------------------------------------------------------------------------
# adapter directories
# ---------------------------------------------------------------------------------------------
RECORD = [2.0 ** -12 * 1.2345678901234567, 3.3e-4, -1.2345678901234567e-7, 9876.54321, 3.1e-4, 2.9e-4, 7.0, 1.0]


def _prodigy(model, seed=None, **kw):
    """FusedProdigy over the trainable set; with a seed, the four states per parameter, steps and the
    record as after some steps (the record holds values no short decimal string reproduces)."""
    from ltx_amd.training import FusedProdigy
    opt = FusedProdigy([p for p in model.parameters() if p.requires_grad], **kw)
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        for p in opt.param_groups[0]["params"]:
            opt.state[p] = {"step": 7, "exp_avg": torch.randn(p.shape, generator=g).to(p.dtype),
                            "exp_avg_sq": torch.rand(p.shape, generator=g).to(p.dtype),
                            "s": torch.randn(p.shape, generator=g).to(p.dtype),
                            "p0": torch.randn(p.shape, generator=g).to(p.dtype)}
        opt.ensure_record().copy_(torch.tensor(RECORD, dtype=torch.float64))
    return opt


def _states(model, opt):
    names = {id(p): n for n, p in model.named_parameters()}
    return {f"{k}.{names[id(p)]}": st[k].detach().clone() for p, st in opt.state.items()
            for k in ("exp_avg", "exp_avg_sq", "s", "p0")}


def _save(model, opt, path):
    from ltx_amd import io
    return io.save_adapter_checkpoint(model, str(path), optimizer=opt,
                                      train_state={"epoch": 3, "global_step": 7, "best_loss": 0.5},
                                      loader=types.SimpleNamespace(seed=5))


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """One directory written by FusedProdigy and one by FusedAdamW: written once, left unchanged."""
    m = _model(CASES["attn2"], seed=1)
    opt = _prodigy(m, seed=2, weight_decay=0.01, growth_rate=1.02)
    pro = (_save(m, opt, tmp_path_factory.mktemp("prodigy") / "adapter_epoch_3"), m, opt)
    m2 = _model(CASES["attn2"], seed=1)
    opt2 = _optimizer(m2, seed=2)
    return {"prodigy": pro, "adamw": (_save(m2, opt2, tmp_path_factory.mktemp("adamw") / "adapter_epoch_3"), m2, opt2)}


def test_prodigy_block_round_trips_the_record_bit_for_bit(saved):
    from ltx_amd import io
    path, m, opt = saved["prodigy"]
    assert sorted(os.listdir(path)) == FOUR
    with open(os.path.join(path, "train_state.json")) as f:
        block = json.load(f)["prodigy"]
    assert sorted(block) == ["hyper", "record"] and block["hyper"] == opt.hyper()
    assert block["record"] == {k: v.hex() for k, v in zip(opt.RECORD, RECORD)}
    assert block["hyper"]["growth_rate"] == (1.02).hex() and block["hyper"]["beta3"] is None
    tensors = load_file(os.path.join(path, "optimizer.safetensors"))
    want = _states(m, opt)
    _same({k: v for k, v in tensors.items() if not k.startswith("rng.")}, want)
    assert any(k.startswith("s.") for k in tensors) and any(k.startswith("p0.") for k in tensors)
    # into an optimizer that has not stepped (state and record are created) and into one that has (in place)
    for seed in (None, 4):
        m2 = _model(CASES["attn2"], seed=9)
        opt2 = _prodigy(m2, seed=seed, weight_decay=0.01, growth_rate=1.02)
        if seed is not None:
            opt2.record.mul_(3.0)
        ptrs = {id(p): st["s"].data_ptr() for p, st in opt2.state.items()}
        rec_ptr = None if opt2.record is None else opt2.record.data_ptr()
        io.load_adapter_checkpoint(m2, path, optimizer=opt2)
        _same(_trainable(m2), _trainable(m))
        _same(_states(m2, opt2), want)
        assert [v.hex() for v in opt2.record.tolist()] == [v.hex() for v in RECORD]
        assert opt2.record.dtype == torch.float64 and all(st["step"] == 7 for st in opt2.state.values())
        if seed is not None:
            assert {id(p): st["s"].data_ptr() for p, st in opt2.state.items()} == ptrs
            assert opt2.record.data_ptr() == rec_ptr


def test_a_checkpoint_without_prodigy_is_todays(saved):
    path = saved["adamw"][0]
    assert sorted(os.listdir(path)) == FOUR
    with open(os.path.join(path, "train_state.json")) as f:
        st = json.load(f)
    assert "prodigy" not in st and sorted(st["optimizer"]["param_groups"][0]) == ["betas", "eps", "lr", "weight_decay"]
    keys = [k for k in load_file(os.path.join(path, "optimizer.safetensors")) if not k.startswith("rng.")]
    assert keys and all(k.startswith(("exp_avg.", "exp_avg_sq.")) for k in keys)


def test_mismatched_kind_or_hyper_parameters_are_refused_with_nothing_written(saved):
    pro, ada = saved["prodigy"][0], saved["adamw"][0]

    def untouched(opt, before, record):
        _same(_states_or_moments(opt), before)
        assert (None if opt_record(opt) is None else opt_record(opt).tolist()) == record

    def opt_record(opt):
        return getattr(opt, "record", None)

    def _states_or_moments(opt):
        return {f"{k}.{i}": v.detach().clone() for i, st in enumerate(opt.state.values())
                for k, v in st.items() if torch.is_tensor(v)}
    # a Prodigy checkpoint into FusedAdamW
    m = _model(CASES["attn2"], seed=3)
    opt = _optimizer(m, seed=4)
    before = _states_or_moments(opt)
    _refused(m, pro, "Prodigy", optimizer=opt)
    untouched(opt, before, None)
    # an AdamW checkpoint into FusedProdigy
    m = _model(CASES["attn2"], seed=3)
    opt = _prodigy(m, seed=4)
    before = _states_or_moments(opt)
    _refused(m, ada, "AdamW", optimizer=opt)
    untouched(opt, before, RECORD)
    # other hyper-parameters: each names the field that differs
    for kw, field in (({"weight_decay": 0.01}, "growth_rate"), ({"growth_rate": 1.02}, "weight_decay"),
                      ({"weight_decay": 0.01, "growth_rate": 1.02, "d0": 1e-5}, "d0"),
                      ({"weight_decay": 0.01, "growth_rate": 1.02, "decouple": False}, "decouple"),
                      ({"weight_decay": 0.01, "growth_rate": 1.02, "betas": (0.9, 0.99)}, "betas"),
                      ({"weight_decay": 0.01, "growth_rate": 1.02, "beta3": 0.9}, "beta3")):
        m = _model(CASES["attn2"], seed=3)
        opt = _prodigy(m, seed=4, **kw)
        before = _states_or_moments(opt)
        _refused(m, pro, field, optimizer=opt)
        untouched(opt, before, RECORD)
    # without an optimizer the adapters load from either
    from ltx_amd import io
    m = _model(CASES["attn2"], seed=3)
    io.load_adapter_checkpoint(m, pro)
    _same(_trainable(m), _trainable(saved["prodigy"][1]))
