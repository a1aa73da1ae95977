"""The robust velocity loss on the CPU: the float64 statement (training.robust_loss_ref) against values
worked out by hand and against its limits, the threshold schedules (training.huber_threshold) against
their closed forms, and the config keys (training.robust_loss_from_config, the YAML route) with every
refusal, which come before anything is launched."""
import pytest
import torch

from loss_weight_utils import config, namespace
from robust_loss_utils import KINDS, closed_form_threshold

F64 = torch.float64


def _ref(*a, **k):
    from ltx_amd.training import robust_loss_ref
    return robust_loss_ref(*a, **k)


# ---------------------------------------------------------------------------------------------
# the statement against hand-computed values. c = 0.5, residuals 0, c and -100 c on v = 1:
#   r(0.5) = sqrt(0.5) = 0.70710678118654752, r(-50) = sqrt(2500.25) = 50.002499937503125
#   huber (k = 1):     l = r - c:     0, 0.20710678118654752, 49.502499937503125;  g = e / r
#   smooth_l1 (k = 2): l = 2 (r - c): 0, 0.41421356237309505, 99.004999875006250;  g = 2 e / r
# ---------------------------------------------------------------------------------------------
HAND = {
    "huber": ([0.0, 0.20710678118654752, 49.502499937503125], [0.0, 0.70710678118654752, -0.99995000374968753]),
    "smooth_l1": ([0.0, 0.41421356237309505, 99.004999875006250], [0.0, 1.4142135623730950, -1.9999000074993751]),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_statement_against_hand_computed_values(kind):
    v = torch.ones(1, 3, 1, dtype=F64)
    out = v + torch.tensor([0.0, 0.5, -50.0], dtype=F64).reshape(1, 3, 1)
    c = torch.tensor([0.5], dtype=F64)
    want_l, want_g = (torch.tensor(x, dtype=F64) for x in HAND[kind])
    sums, dout = _ref(out, v, c, KINDS[kind])
    assert sums.dtype == F64 and sums.shape == (5,) and dout.dtype == F64 and dout.shape == out.shape
    assert float(sums[0]) == pytest.approx(float(want_l.sum()), rel=1e-14)
    assert float(sums[4]) == pytest.approx(float(want_l.sum()), rel=1e-14)
    # sum v, sum v^2, and the shipped squared error: bf16(0.25) + bf16(2500) = 0.25 + 2496 (2500 lies between
    # the bf16 neighbours 2496 and 2512)
    assert sums[1:4].tolist() == [3.0, 3.0, 2496.25]
    assert torch.allclose(dout.reshape(3), want_g / 3, rtol=1e-14, atol=0)
    assert float(dout[0, 0, 0]) == 0.0  # e == 0: exactly 0, not a small number
    # with a weight per token and a gradient scale: s0 and dout carry them, s4 and the shipped sums do not
    wt = torch.tensor([[2.0, 3.0, 0.5]], dtype=F64)
    sums_w, dout_w = _ref(out, v, c, KINDS[kind], wt=wt, grad_scale=0.25)
    assert float(sums_w[0]) == pytest.approx(float((wt.reshape(3) * want_l).sum()), rel=1e-14)
    assert torch.equal(sums_w[1:], sums[1:])
    assert torch.allclose(dout_w.reshape(3), wt.reshape(3) * want_g * 0.25 / 3, rtol=1e-14, atol=0)


def test_statement_takes_each_samples_own_threshold():
    # two samples, the same residual 0.5: c = 0.5 gives the values above, c = 50 (e = c / 100) is deep in
    # the quadratic part: huber l = 2 c (r - c) with r = sqrt(2500.25) again: 100 * 0.002499937503125
    out = torch.full((2, 1, 2), 1.5, dtype=F64)
    v = torch.ones(2, 1, 2, dtype=F64)
    sums, dout = _ref(out, v, torch.tensor([0.5, 50.0], dtype=F64), 1)
    assert float(sums[4]) == pytest.approx(2 * 0.20710678118654752 + 2 * 100 * 0.002499937503124805, rel=1e-12)
    assert torch.allclose(dout[0], torch.full((1, 2), 0.70710678118654752 / 4, dtype=F64), rtol=1e-14, atol=0)
    assert torch.allclose(dout[1], torch.full((1, 2), 100 * 0.5 / 50.002499937503125 / 4, dtype=F64), rtol=1e-14,
                          atol=0)
    with pytest.raises(ValueError):
        _ref(out, v, torch.tensor([0.5, 50.0]), 3)


def _residuals():
    g = torch.Generator().manual_seed(5)
    e = torch.randn(2, 37, 3, generator=g, dtype=F64) * 3.0
    return torch.where(e.abs() < 2.0 ** -8, torch.full_like(e, 0.25), e)


def test_huber_tends_to_the_squared_error():
    e = _residuals()
    v = torch.randn(e.shape, generator=torch.Generator().manual_seed(6), dtype=F64)
    sums, dout = _ref(v + e, v, torch.full((2,), 2.0 ** 20, dtype=F64), 1)
    assert float(sums[4]) == pytest.approx(float((e * e).sum()), rel=1e-9)
    assert torch.allclose(dout, 2.0 * e / e.numel(), rtol=1e-9, atol=0)


def test_smooth_l1_tends_to_twice_the_absolute_error():
    e = _residuals()
    assert float(e.abs().min()) >= 2.0 ** -8
    v = torch.zeros_like(e)  # out - v is then e exactly
    sums, dout = _ref(e, v, torch.full((2,), 2.0 ** -40, dtype=F64), 2)
    assert float(sums[4]) == pytest.approx(float(2.0 * e.abs().sum()), rel=1e-9)
    assert torch.allclose(dout, 2.0 * torch.sign(e) / e.numel(), rtol=1e-9, atol=0)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_gradient_is_the_central_difference_of_the_loss(kind):
    """dout against (L(o + h) - L(o - h)) / 2h of L = sum wt l / n per element, in float64 with h = 1e-5. The
    truncation error is h^2 |l'''| / 6 with |l'''| <= 0.86 k / c^2, at most 688 (smooth_l1, c = 0.05): 1.2e-8
    where the gradient is of order 1. The rounding error is a few ulps of the sum (about 50, so 1e-14) over
    2h: 1e-9. Hence 1e-6 relative with an absolute floor of 1e-8 on wt g."""
    g = torch.Generator().manual_seed(9)
    v = torch.randn(3, 5, 4, generator=g, dtype=F64)
    out = v + torch.randn(3, 5, 4, generator=g, dtype=F64)
    out[0, 0, 0] = v[0, 0, 0]  # the minimum: gradient 0
    c = torch.tensor([0.05, 0.3, 1.0], dtype=F64)
    wt = torch.rand(3, 5, generator=g, dtype=F64) + 0.1
    n = out.numel()
    _, dout = _ref(out, v, c, KINDS[kind], wt=wt)
    h = 1e-5
    fd = torch.empty_like(out)
    flat = out.reshape(-1)
    for i in range(n):
        lo, hi = flat.clone(), flat.clone()
        lo[i] -= h
        hi[i] += h
        s_lo, _ = _ref(lo.reshape(out.shape), v, c, KINDS[kind], wt=wt)
        s_hi, _ = _ref(hi.reshape(out.shape), v, c, KINDS[kind], wt=wt)
        fd.reshape(-1)[i] = (s_hi[0] - s_lo[0]) / (2 * h) / n
    assert torch.allclose(dout, fd, rtol=1e-6, atol=1e-8 / n)
    assert float(dout[0, 0, 0]) == 0.0


# ---------------------------------------------------------------------------------------------
# the threshold schedules
# ---------------------------------------------------------------------------------------------
T_POINTS = [0.0, 0.25, 0.5, 1.0]


@pytest.mark.parametrize("huber_c", [0.1, 0.01, 0.5])
def test_thresholds_match_their_closed_forms(huber_c):
    from ltx_amd.training import HUBER_SCHEDULES, huber_threshold
    t = torch.tensor(T_POINTS, dtype=torch.float32)
    assert HUBER_SCHEDULES == ("constant", "exponential", "snr")
    for schedule in HUBER_SCHEDULES:
        got = huber_threshold(t, schedule, huber_c)
        assert got.dtype == torch.float32 and got.shape == t.shape and got.is_contiguous()
        # a handful of f32 roundings on values in (0, 1]: 1e-6 relative
        assert torch.allclose(got.double(), closed_form_threshold(t, schedule, huber_c), rtol=1e-6, atol=0), schedule
        assert bool((got > 0).all())
    # written out by hand at c = 0.1: 0.1^0.25, 0.1^0.5; 0.9 * 0.5625 + 0.1, 0.9 * 0.25 + 0.1
    if huber_c == 0.1:
        assert huber_threshold(t, "constant", 0.1).tolist() == [pytest.approx(0.1, rel=1e-6)] * 4
        assert huber_threshold(t, "exponential", 0.1).tolist() == pytest.approx(
            [1.0, 0.5623413251903491, 0.31622776601683794, 0.1], rel=1e-6)
        assert huber_threshold(t, "snr", 0.1).tolist() == pytest.approx([1.0, 0.60625, 0.325, 0.1], rel=1e-6)
    with pytest.raises(ValueError, match="huber_schedule"):
        huber_threshold(t, "linear", huber_c)


@pytest.mark.parametrize("schedule", ["exponential", "snr"])
def test_scheduled_thresholds_run_from_one_to_huber_c(schedule):
    from ltx_amd.training import huber_threshold
    for huber_c in (0.1, 0.003, 0.75):
        got = huber_threshold(torch.tensor([0.0, 1.0], dtype=torch.float32), schedule, huber_c)
        assert float(got[0]) == pytest.approx(1.0, rel=2e-7)
        assert float(got[1]) == pytest.approx(huber_c, rel=2e-7)
        # and monotonically in between: loose at low noise, tight at high noise
        mid = huber_threshold(torch.linspace(0, 1, 33), schedule, huber_c)
        assert bool((mid[1:] < mid[:-1]).all())


def test_threshold_constants_are_built_once():
    from ltx_amd import training
    t = torch.tensor([0.2, 0.4, 0.9], dtype=torch.float32)
    for schedule in ("constant", "exponential"):
        a = training.huber_threshold(t, schedule, 0.125)
        before = dict(training._HUBER_CONSTS)
        b = training.huber_threshold(t.clone(), schedule, 0.125)
        assert torch.equal(a, b)
        assert training._HUBER_CONSTS.keys() == before.keys()
        assert all(training._HUBER_CONSTS[k] is v for k, v in before.items())


# ---------------------------------------------------------------------------------------------
# the config keys
# ---------------------------------------------------------------------------------------------
def test_nothing_configured_is_none():
    from ltx_amd.training import robust_loss_from_config
    assert robust_loss_from_config(config()) is None
    assert robust_loss_from_config(config(loss_type="l2")) is None
    assert robust_loss_from_config(config(loss_type=None, huber_c=None, huber_schedule=None)) is None
    assert robust_loss_from_config(namespace()) is None


def test_every_key_is_read():
    from ltx_amd.training import RobustLoss, robust_loss_from_config
    assert robust_loss_from_config(config(loss_type="huber")) == RobustLoss("huber", 0.1, "snr")
    assert robust_loss_from_config(config(loss_type="smooth_l1")) == RobustLoss("smooth_l1", 0.1, "snr")
    got = robust_loss_from_config(config(loss_type="huber", huber_c=0.25, huber_schedule="exponential"))
    assert got == RobustLoss("huber", 0.25, "exponential") and isinstance(got.huber_c, float)
    assert robust_loss_from_config(config(loss_type="smooth_l1", huber_c=2, huber_schedule="constant")) == \
        RobustLoss("smooth_l1", 2.0, "constant")


@pytest.mark.parametrize("keys,match", [
    (dict(loss_type="l1"), "loss_type"),
    (dict(loss_type="Huber"), "loss_type"),
    (dict(loss_type=1), "loss_type"),
    (dict(loss_type=True), "loss_type"),
    (dict(loss_type="huber", huber_c=0.0), "huber_c"),
    (dict(loss_type="huber", huber_c=-0.1), "huber_c"),
    (dict(loss_type="huber", huber_c=float("nan")), "huber_c"),
    (dict(loss_type="huber", huber_c=float("inf")), "huber_c"),
    (dict(loss_type="huber", huber_c="0.1"), "huber_c"),
    (dict(loss_type="huber", huber_c=True), "huber_c"),
    (dict(loss_type="huber", huber_schedule="linear"), "huber_schedule"),
    (dict(loss_type="huber", huber_schedule=2), "huber_schedule"),
    # the Prodigy keys' rule: a key nothing would read is refused, not ignored
    (dict(huber_c=0.1), "huber_c"),
    (dict(huber_schedule="snr"), "huber_schedule"),
    (dict(loss_type="l2", huber_c=0.1), "huber_c"),
    (dict(loss_type="l2", huber_schedule="constant"), "huber_schedule"),
])
def test_refusals(keys, match):
    from ltx_amd.training import robust_loss_from_config
    with pytest.raises(ValueError, match=match):
        robust_loss_from_config(config(**keys))


def test_train_step_refuses_before_anything_is_launched():
    """A bad key raises out of train_step with CPU tensors and no model: nothing was touched."""
    from ltx_amd.training import train_step
    batch = {k: torch.zeros(1, 4, 1, 2, 2) for k in ("latents", "ref_image_latents", "pose_latents")}
    with pytest.raises(ValueError, match="huber_c"):
        train_step(None, batch, None, None, config(loss_type="huber", huber_c=-1.0), None, None, device="cpu")
    with pytest.raises(ValueError, match="huber_schedule"):
        train_step(None, batch, None, None, config(huber_schedule="snr"), None, None, device="cpu")


def test_yaml_keys_reach_the_config(tmp_path):
    from ltx_amd.config import TrainConfig, load_train_config_from_yaml
    from ltx_amd.training import RobustLoss, robust_loss_from_config
    plain = tmp_path / "plain.yaml"
    plain.write_text("checkpoint_path: x\ntrain:\n  batch_size: 2\n")
    tc = load_train_config_from_yaml(str(plain))
    for key in ("loss_type", "huber_c", "huber_schedule"):
        assert not hasattr(tc, key), key  # absent keys set nothing, and they are not TrainConfig fields
        assert key not in TrainConfig.__dataclass_fields__
    assert robust_loss_from_config(tc) is None
    full = tmp_path / "full.yaml"
    full.write_text("checkpoint_path: x\ntrain:\n  loss_type: smooth_l1\n  huber_c: 0.05\n"
                    "  huber_schedule: exponential\n")
    tc = load_train_config_from_yaml(str(full))
    assert (tc.loss_type, tc.huber_c, tc.huber_schedule) == ("smooth_l1", 0.05, "exponential")
    assert robust_loss_from_config(tc) == RobustLoss("smooth_l1", 0.05, "exponential")
    # values are passed on as written: a quoted number is refused where it is read, not converted
    bad = tmp_path / "bad.yaml"
    bad.write_text("checkpoint_path: x\ntrain:\n  loss_type: huber\n  huber_c: '0.1'\n")
    with pytest.raises(ValueError, match="huber_c"):
        robust_loss_from_config(load_train_config_from_yaml(str(bad)))
    stray = tmp_path / "stray.yaml"
    stray.write_text("checkpoint_path: x\ntrain:\n  huber_schedule: snr\n")
    with pytest.raises(ValueError, match="huber_schedule"):
        robust_loss_from_config(load_train_config_from_yaml(str(stray)))


def test_binding_and_header_declare_the_entry():
    import os
    from ltx_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "ltx_hip.h")).read()
    assert "int ltx_robust_loss_fwd_bwd(" in header
    assert len(_lib._SIGNATURES["ltx_robust_loss_fwd_bwd"]) == 12
    assert hasattr(_lib.load(), "ltx_robust_loss_fwd_bwd")
    assert ops.ROBUST_KINDS == KINDS


def test_wrapper_refuses_cpu_tensors_and_wrong_dtypes():
    from ltx_amd import _lib, ops
    o = torch.zeros(2, 4, 8, dtype=torch.bfloat16)
    with pytest.raises(_lib.LtxHipError):
        ops.robust_loss_fwd_bwd(o, o, torch.ones(2), 1)
    with pytest.raises(TypeError):
        ops.robust_loss_fwd_bwd(o.float(), o, torch.ones(2), 1)


def test_entry_refuses_bad_arguments_before_any_launch():
    """The C entry's own refusals, with addresses that are never dereferenced (host only: every check comes
    before the launch): a null out, v, c or stats, a kind other than 1 or 2, a non-positive shape."""
    import ctypes
    from ltx_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x10000)

    def rc(out=p, v=p, c=p, stats=p, kind=1, B=2, rows=4, C=8):
        return lib.ltx_robust_loss_fwd_bwd(out, v, None, c, kind, None, stats, B, rows, C, 1.0, None)
    for kw in (dict(out=None), dict(v=None), dict(c=None), dict(stats=None), dict(kind=0), dict(kind=3),
               dict(kind=-1), dict(B=0), dict(rows=0), dict(C=0), dict(B=-2), dict(rows=-1), dict(C=-8)):
        assert rc(**kw) != 0, kw
        assert b"robust_loss" in lib.ltx_last_error(), kw
