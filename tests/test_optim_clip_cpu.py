"""Gradient-norm clipping and learning-rate schedules of the LoRA optimizer step, host side:
LRSchedule against torch's LambdaLR, the config keys (setattr and YAML, read only when present), the
errors, the default total-step count, and FusedAdamW keeping max_grad_norm in its parameter groups.
No GPU, no kernel launches."""
import math

import pytest
import torch

NAMES = ("constant", "constant_with_warmup", "linear", "cosine")
BASE, T = 2e-4, 10


def _lambda(name, W, T):
    """The factor of transformers.get_scheduler, written out independently of LRSchedule."""
    def f(s):
        if s < W:
            return float(s) / float(max(1, W))
        if name == "linear":
            return max(0.0, float(T - s) / float(max(1, T - W)))
        if name == "cosine":
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * (float(s - W) / float(max(1, T - W))))))
        return 1.0
    return f


@pytest.mark.parametrize("W", [0, 3])
@pytest.mark.parametrize("name", NAMES)
def test_lr_schedule_is_lambda_lr(name, W):
    """The lr of every step, and two past the end, equals as Python floats what LambdaLR sets on a
    torch.optim.AdamW with the same lambda."""
    from ltx_amd.training import LRSchedule
    sched = LRSchedule(name, BASE, W, T)
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(2))], lr=BASE)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, _lambda(name, W, T))
    want, got = [], []
    for s in range(T + 2):
        want.append(opt.param_groups[0]["lr"])
        got.append(sched.at(s))
        opt.step()
        lam.step()
    assert got == want
    assert all(isinstance(v, float) for v in got)
    if W:
        assert got[0] == 0.0 and got[W] == BASE  # the first step runs at lr 0, as transformers'
    if name in ("linear", "cosine"):
        assert got[T] == 0.0 and got[W] == BASE and got[T - 1] < got[W + 1]
        assert name == "cosine" or got[T + 1] == 0.0  # (the cosine comes back up past T, as transformers')
    else:
        assert got[W:] == [BASE] * (T + 2 - W)


def test_cosine_warmup_values():
    from ltx_amd.training import LRSchedule
    got = [LRSchedule("cosine", 2e-4, 3, 10).at(s) for s in range(5)]
    assert got[:4] == [0.0, 2e-4 * (1 / 3), 2e-4 * (2 / 3), 2e-4]
    assert got[4] == 2e-4 * (0.5 * (1.0 + math.cos(math.pi * (1 / 7))))


def test_schedule_errors():
    from ltx_amd.training import LRSchedule
    with pytest.raises(ValueError, match="lr_scheduler"):
        LRSchedule("polynomial", 1e-3, 0, 10)
    with pytest.raises(ValueError, match="lr_warmup_steps"):
        LRSchedule("constant", 1e-3, -1, 10)
    with pytest.raises(ValueError, match="lr_total_steps"):
        LRSchedule("cosine", 1e-3, 0, None)
    LRSchedule("constant", 1e-3, 2, None)  # a constant rate needs no total


def _tc(**kw):
    from ltx_amd.config import TrainConfig
    attrs = {k: kw.pop(k) for k in list(kw) if k in ("max_grad_norm", "lr_scheduler", "lr_warmup_steps",
                                                      "lr_total_steps")}
    tc = TrainConfig(checkpoint_path="-", learning_rate=1e-3, num_epochs=3, **kw)
    for k, v in attrs.items():
        setattr(tc, k, v)
    return tc


class _Sized:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(())


def test_config_keys_are_read_only_when_present():
    from ltx_amd.config import TrainConfig
    from ltx_amd.training import schedule_from_config
    bare = TrainConfig(checkpoint_path="-", learning_rate=1e-3, num_epochs=3)
    for k in ("max_grad_norm", "lr_scheduler", "lr_warmup_steps", "lr_total_steps"):
        assert not hasattr(bare, k)
    # nothing set: no clipping, no schedule (the loop then never touches the lr), unsized loader accepted
    assert schedule_from_config(bare, iter(())) == (None, None)
    assert schedule_from_config(_tc(max_grad_norm=0), None) == (None, None)
    assert schedule_from_config(_tc(lr_scheduler="constant"), None) == (None, None)
    norm, sched = schedule_from_config(_tc(max_grad_norm=1.5, lr_scheduler="cosine", lr_warmup_steps=2,
                                           lr_total_steps=40), None)
    assert norm == 1.5 and isinstance(norm, float)
    assert (sched.name, sched.base_lr, sched.warmup_steps, sched.total_steps) == ("cosine", 1e-3, 2, 40)
    # a warm-up alone is a schedule
    _, sched = schedule_from_config(_tc(lr_warmup_steps=4), None)
    assert (sched.name, sched.warmup_steps, sched.total_steps) == ("constant", 4, None)
    assert sched.at(1) == 1e-3 * 0.25 and sched.at(9) == 1e-3


def test_default_total_steps_counts_optimizer_steps():
    """num_epochs * (len(dataloader) // gradient_accumulation_steps): 3 epochs of 7 batches with
    accumulation 2 are 3 * 3 optimizer steps (the odd batch out takes no step)."""
    from ltx_amd.training import schedule_from_config
    _, sched = schedule_from_config(_tc(lr_scheduler="linear", gradient_accumulation_steps=2), _Sized(7))
    assert sched.total_steps == 9
    _, sched = schedule_from_config(_tc(lr_scheduler="linear", gradient_accumulation_steps=2, lr_total_steps=5),
                                    _Sized(7))
    assert sched.total_steps == 5  # the key wins


def test_config_errors_are_raised_before_the_first_step():
    from ltx_amd.training import schedule_from_config
    with pytest.raises(ValueError, match="lr_total_steps"):
        schedule_from_config(_tc(lr_scheduler="cosine"), iter(()))  # decaying, no key, unsized loader
    with pytest.raises(ValueError, match="lr_total_steps"):
        schedule_from_config(_tc(lr_scheduler="linear"), None)
    with pytest.raises(ValueError, match="lr_scheduler"):
        schedule_from_config(_tc(lr_scheduler="cosine_with_restarts"), _Sized(4))
    with pytest.raises(ValueError, match="lr_warmup_steps"):
        schedule_from_config(_tc(lr_warmup_steps=-1), _Sized(4))
    with pytest.raises(ValueError, match="max_grad_norm"):
        schedule_from_config(_tc(max_grad_norm=-1.0), _Sized(4))
    with pytest.raises(ValueError, match="max_grad_norm"):
        schedule_from_config(_tc(max_grad_norm=float("nan")), _Sized(4))


def test_train_loop_raises_before_touching_the_model():
    """train_loop reads the keys before it builds the optimizer: a bad one raises with an empty loader
    and a model it never looks into."""
    from ltx_amd.training import train_loop

    class Model(torch.nn.Module):
        patchifier = None
        device = "cpu"

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(3))
    tc = _tc(lr_scheduler="nope")
    tc.train_mode = "lora_audio"
    with pytest.raises(ValueError, match="lr_scheduler"):
        train_loop(Model(), tc, [], torch.zeros(1, 4, 8), torch.ones(1, 4, dtype=torch.long), device="cpu")
    tc = _tc(lr_scheduler="cosine")
    tc.train_mode = "lora_audio"
    with pytest.raises(ValueError, match="lr_total_steps"):
        train_loop(Model(), tc, iter(()), torch.zeros(1, 4, 8), torch.ones(1, 4, dtype=torch.long), device="cpu")


def test_yaml_sets_the_keys_only_when_present(tmp_path):
    from dataclasses import asdict
    from ltx_amd.config import load_train_config_from_yaml
    base = "checkpoint_path: x.safetensors\ntrain:\n  lora_rank: 16\n"
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(base + "  max_grad_norm: 1\n  lr_scheduler: cosine\n  lr_warmup_steps: 100\n"
                                            "  lr_total_steps: 5000\n")
    a = load_train_config_from_yaml(str(tmp_path / "a.yaml"))
    b = load_train_config_from_yaml(str(tmp_path / "b.yaml"))
    keys = ("max_grad_norm", "lr_scheduler", "lr_warmup_steps", "lr_total_steps")
    assert not any(hasattr(a, k) for k in keys)
    assert [getattr(b, k) for k in keys] == [1.0, "cosine", 100, 5000]
    assert isinstance(b.max_grad_norm, float) and isinstance(b.lr_warmup_steps, int)
    assert asdict(a) == asdict(b) and not any(k in asdict(b) for k in keys)


def test_fused_adamw_keeps_max_grad_norm_in_its_param_groups():
    """... so the adapter checkpoint's train_state.json carries it with the other hyper-parameters
    (io._plain keeps plain values of every param-group key) and the restore puts it back."""
    from ltx_amd import io
    from ltx_amd.training import FusedAdamW
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdamW([p], lr=1e-3, max_grad_norm=0.5)
    assert opt.param_groups[0]["max_grad_norm"] == 0.5 and opt.defaults["max_grad_norm"] == 0.5
    assert opt.grad_norm is None and opt.clip_coef is None
    hyper = {k: io._plain(v) for k, v in opt.param_groups[0].items() if k != "params" and io._plain(v) is not None}
    assert hyper["max_grad_norm"] == 0.5 and hyper["lr"] == 1e-3
    off = FusedAdamW([p], lr=1e-3)
    assert off.param_groups[0]["max_grad_norm"] is None
    sd = opt.state_dict()
    off.load_state_dict(sd)
    assert off.param_groups[0]["max_grad_norm"] == 0.5
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdamW([p], lr=1e-3, max_grad_norm=-1.0)
    # one global norm takes one value
    two = FusedAdamW([{"params": [p], "max_grad_norm": 1.0},
                      {"params": [torch.nn.Parameter(torch.zeros(2))], "max_grad_norm": 2.0}], lr=1e-3)
    with pytest.raises(ValueError, match="max_grad_norm"):
        two.step()


def test_clipping_refuses_cpu_parameters():
    from ltx_amd import _lib
    from ltx_amd.training import FusedAdamW
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    opt = FusedAdamW([p], lr=1e-3, max_grad_norm=1.0)
    with pytest.raises(_lib.LtxHipError):
        opt.step()
    assert not opt.state[p]  # raised before any state was created
