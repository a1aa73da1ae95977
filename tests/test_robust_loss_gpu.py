"""The robust velocity loss on the MI355X: ltx_robust_loss_fwd_bwd against its float64 statement
(training.robust_loss_ref) and, for the sums it shares with it, against the shipped ltx_mse_fwd_bwd bit for
bit; and the robust train step of one LTX-2B-width block against the pinned oracle run live with the same
robust loss.

Tolerances. s0 and s4, relative 5e-5: sums of non-negative terms; the longest chain of f32 additions at
these shapes (a thread's elements, the wave tree, four waves, 256 partials in a strided loop and a tree) is
under 600, times 2^-24 = 3.6e-5, plus about ten f32 roundings per element. dout, relative 4.0e-3 per
element: one bf16 rounding, at most 2^-8 = 3.906e-3 at the bottom of a binade, plus f32 slop under 1e-5;
exactly 0 where the statement is 0. Measured on these seeded inputs, the worst over both kinds and with and
without weights: s0 and s4 8.6e-08 (at (1, 1, 1); 7.9e-08 at (2, 64, 128)); dout 1.951e-03 at (1, 1, 1), 3.861e-03 at
(2, 64, 128), 3.887e-03 at (3, 1001, 7) and 3.890e-03 at (3, 1792, 128): the one bf16 rounding, found near
the bottom of a binade once there are enough elements, inside the bound as set. The step: model_utils.noise_crit / loss_crit at their
defaults, relative to the oracle's own bf16 noise on the same robust loss."""
import pytest
import torch

import ltx_oracle as O
from loss_weight_utils import StepCapture, config, step_boxes, within_relative
from model_utils import build_model, is_lora_trainable, loss_crit, noise_crit, synth_inputs
from robust_loss_utils import KINDS, closed_form_threshold, oracle_robust_step, robust_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEW_KERNELS = ("ltx::robust_loss_kernel<true>", "ltx::robust_loss_kernel<false>")
# (1, 1, 1): one element, the scalar tail alone; (2, 64, 128): the vector path; (3, 1001, 7): the per-element
# path, rows * C = 7007 is no multiple of 8, so sample and token boundaries fall inside vectors, and there
# is a scalar tail; (3, 1792, 128): 688 128 elements = 86 016 vectors on 65 536 threads, so some threads
# take a second vector
SHAPES = [(1, 1, 1), (2, 64, 128), (3, 1001, 7), (3, 1792, 128)]
GS = 1 / 16


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from ltx_amd import _lib as L
    L.ensure_device()
    return L


_INPUTS = {}


def _inputs(shape, weights):
    """Operands on the device and the float64 statement of both kinds, computed once and left unchanged."""
    key = (shape, weights)
    if key not in _INPUTS:
        from ltx_amd.training import robust_loss_ref
        o, v, c, wt = robust_inputs(shape, seed=sum(shape) + 17 * weights, weights=weights, device=DEV)
        refs = {kind: robust_loss_ref(o, v, c, k, wt=wt, grad_scale=GS) for kind, k in KINDS.items()}
        _INPUTS[key] = (o, v, c, wt, refs)
    return _INPUTS[key]


# ---------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_and_gradient_against_the_f64_statement(shape, kind, weights):
    from ltx_amd import ops
    o, v, c, wt, refs = _inputs(shape, weights)
    ref_sums, ref_d = refs[kind]
    if o.numel() >= 100:
        e = o.float() - v.float()
        assert int((e == 0).sum()) > 0  # the minimum occurs
        cb = c.reshape(-1, 1, 1)
        assert bool((e.abs() > 4 * cb).any()) and bool(((e.abs() < cb / 4) & (e != 0)).any())  # both regimes
    stats, dout = ops.robust_loss_fwd_bwd(o, v, c, KINDS[kind], wt=wt, grad_scale=GS)
    assert stats.shape == (5,) and stats.dtype == torch.float32
    assert dout.shape == o.shape and dout.dtype == torch.bfloat16
    ok0, worst0 = within_relative(stats[0], ref_sums[0], 5e-5)
    ok4, worst4 = within_relative(stats[4], ref_sums[4], 5e-5)
    okd, worstd = within_relative(dout, ref_d, 4.0e-3)
    print(f"{shape} {kind} weights={weights}: worst relative error s0 {worst0:.3e}, s4 {worst4:.3e}, "
          f"dout {worstd:.3e}")
    assert ok0 and ok4, (worst0, worst4)
    assert okd, worstd
    assert bool((dout[(ref_d == 0).to(DEV)] == 0).all())
    if weights and shape[0] > 1:
        assert int((ref_d == 0).sum()) > ref_d[0].numel() // 100  # the zero weights made zeros of their own
    # sum v and sum v^2 against float64 too (they are the shipped kernel's, compared bitwise below)
    assert within_relative(stats[2], ref_sums[2], 5e-5)[0]
    assert abs(float(stats[1]) - float(ref_sums[1])) <= 5e-5 * float(v.double().abs().sum())


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_shared_sums_are_the_shipped_losss(shape, weights):
    from ltx_amd import ops
    o, v, c, wt, _ = _inputs(shape, weights)
    s_mse, _ = ops.mse_fwd_bwd(o, v, grad_scale=GS)
    for kind in KINDS.values():
        stats, _ = ops.robust_loss_fwd_bwd(o, v, c, kind, wt=wt, grad_scale=GS)
        assert torch.equal(stats[1], s_mse[1]) and torch.equal(stats[2], s_mse[2]), shape
        assert torch.equal(stats[3], s_mse[0]), shape


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("shape", SHAPES)
def test_deterministic_and_forward_only(shape, kind):
    from ltx_amd import ops
    o, v, c, wt, _ = _inputs(shape, True)
    s1, d1 = ops.robust_loss_fwd_bwd(o, v, c, KINDS[kind], wt=wt, grad_scale=GS)
    s2, d2 = ops.robust_loss_fwd_bwd(o, v, c, KINDS[kind], wt=wt, grad_scale=GS)
    assert torch.equal(s1, s2) and torch.equal(d1, d2)
    s3, d3 = ops.robust_loss_fwd_bwd(o, v, c, KINDS[kind], wt=wt, grad_scale=GS, want_grad=False)
    assert d3 is None and torch.equal(s3, s1)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("shape", SHAPES)
def test_weights(shape, kind):
    from ltx_amd import ops
    o, v, c, wt, _ = _inputs(shape, True)
    B, rows, C = shape
    # ones are the null pointer
    s_null, d_null = ops.robust_loss_fwd_bwd(o, v, c, KINDS[kind], grad_scale=GS)
    s_ones, d_ones = ops.robust_loss_fwd_bwd(o, v, c, KINDS[kind], wt=torch.ones(B, rows, device=DEV), grad_scale=GS)
    assert torch.equal(s_null[0], s_null[4]) and torch.equal(s_ones[0], s_ones[4])
    assert torch.equal(s_ones, s_null) and torch.equal(d_ones, d_null)
    if B == 1:
        return
    # the last sample's weights are all zero: it adds exactly 0 to s0 and gets exactly 0 gradients, so s0 is
    # bitwise unchanged when that sample's `out` is replaced by anything finite
    assert bool((wt[-1] == 0).all()) and bool((wt[:-1] > 0).any())
    s_w, d_w = ops.robust_loss_fwd_bwd(o, v, c, KINDS[kind], wt=wt, grad_scale=GS)
    assert bool((d_w[-1] == 0).all()) and bool((d_w[:-1] != 0).any())
    o2 = o.clone()
    o2[-1] = (o[-1].float() * 3.0 + 1.0).bfloat16()
    s_w2, d_w2 = ops.robust_loss_fwd_bwd(o2, v, c, KINDS[kind], wt=wt, grad_scale=GS)
    assert torch.equal(s_w2[0], s_w[0]) and not torch.equal(s_w2[4], s_w[4])
    assert torch.equal(d_w2, d_w)


def test_exact_zero_at_the_minimum_and_non_finite_inputs_show():
    from ltx_amd import ops
    o = torch.randn(2, 8, 16, generator=torch.Generator().manual_seed(3)).bfloat16().to(DEV)
    c = torch.tensor([0.05, 1.0], device=DEV)
    for kind in KINDS.values():
        stats, dout = ops.robust_loss_fwd_bwd(o, o.clone(), c, kind)
        assert float(stats[0]) == 0.0 and float(stats[4]) == 0.0 and float(stats[3]) == 0.0
        assert bool((dout == 0).all())
        # thresholds whose square underflows, one of them subnormal: still exactly 0, not 0 / 0
        tiny = torch.tensor([1e-30, 1e-39], device=DEV)
        stats, dout = ops.robust_loss_fwd_bwd(o, o.clone(), tiny, kind)
        assert float(stats[0]) == 0.0 and float(stats[4]) == 0.0 and bool((dout == 0).all())
        for bad in (float("nan"), float("inf")):
            o2 = o.clone()
            o2[1, 3, 5] = bad
            stats, dout = ops.robust_loss_fwd_bwd(o2, o, c, kind)
            assert not bool(torch.isfinite(stats[0])) and not bool(torch.isfinite(stats[4]))
            assert not bool(torch.isfinite(dout[1, 3, 5].float()))
            assert bool(torch.isfinite(dout[0].float()).all())


def test_refusals_come_before_any_launch():
    from ltx_amd import _lib, ops
    o, v, c, wt, _ = _inputs((2, 64, 128), True)
    timer = ops.LaunchTimer()
    ops.set_launch_timer(timer)
    try:
        with pytest.raises(ValueError):
            ops.robust_loss_fwd_bwd(o, v, c, 1, wt=torch.ones(127, device=DEV))  # one weight short
        with pytest.raises(ValueError):
            ops.robust_loss_fwd_bwd(o, v, torch.ones(3, device=DEV), 1)  # c of another batch
        with pytest.raises(ValueError):
            ops.robust_loss_fwd_bwd(o, v, torch.ones(4, device=DEV)[::2], 1)  # non-contiguous c
        with pytest.raises(ValueError):
            ops.robust_loss_fwd_bwd(o, v, c, 1, wt=torch.ones(2, 128, device=DEV)[:, ::2])  # non-contiguous wt
        with pytest.raises(ValueError):
            ops.robust_loss_fwd_bwd(o, v[:, :32], c, 1)
        for kind in (0, 3, "huber"):
            with pytest.raises(ValueError):
                ops.robust_loss_fwd_bwd(o, v, c, kind)
        with pytest.raises(TypeError):
            ops.robust_loss_fwd_bwd(o, v, c.double(), 1)
        with pytest.raises(TypeError):
            ops.robust_loss_fwd_bwd(o.float(), v, c, 1)
        with pytest.raises(_lib.LtxHipError):
            ops.robust_loss_fwd_bwd(o, v, c.cpu(), 1)
        with pytest.raises(_lib.LtxHipError):
            ops.robust_loss_fwd_bwd(o, v, c, 1, wt=wt.cpu())
        with pytest.raises(_lib.LtxHipError):
            ops.robust_loss_fwd_bwd(o.cpu(), v, c, 1)
        # the library's own refusal of a kind the wrapper would not pass on
        with pytest.raises(_lib.LtxHipError, match="kind"):
            ops.call("ltx_robust_loss_fwd_bwd", ops._p(o), ops._p(v), None, ops._p(c), 3, None,
                     ops._p(torch.empty(8 + 5 * 256, device=DEV)), 2, 64, 128, 1.0, ops._s())
    finally:
        ops.set_launch_timer(None)
    assert timer.records == []


# ---------------------------------------------------------------------------------------------
# the step: one LTX-2B-width block, B = 8 samples of 2 x 16 x 16 tokens (tests/test_loss_weight_gpu.py's)
# ---------------------------------------------------------------------------------------------
RANK = 32
SHAPE = (8, 2, 16, 16)
ROBUST_KEYS = dict(loss_type="huber", huber_schedule="snr", huber_c=0.1)
_CASE = {}


def _case():
    """The model, its inputs and the unconfigured step, built once and left unchanged."""
    if not _CASE:
        from ltx_amd.transformer3d import OURS_TRANSFORMER_CONFIG
        cfg = dict(OURS_TRANSFORMER_CONFIG, num_layers=1)
        params = O.make_params(cfg, 100 + RANK, lora_rank=RANK, requires_grad=False)
        B, F, H, W = SHAPE
        d = synth_inputs(B, F, H, W, 256, 16, seed=7 + RANK, device=DEV)
        model = build_model(cfg, params, RANK, device=DEV)
        _CASE.update(cfg=cfg, params=params, d=d, model=model, boxes=step_boxes(B, DEV),
                     plain=StepCapture(model, d, config()))
    return _CASE


@pytest.mark.parametrize("face", [False, True])
def test_robust_step_matches_the_oracle_with_the_robust_loss(face):
    from ltx_amd.training import token_loss_weights_ref
    c = _case()
    B, F, H, W = SHAPE
    d, model, plain = c["d"], c["model"], c["plain"]
    # the oracle's thresholds from the closed form, its weights from the float64 statement
    thr = closed_form_threshold(d["out.t"], "snr", 0.1).float()
    assert float(thr.max() / thr.min()) > 2  # the schedule is not a formality
    wt_ref, keys, extra = None, dict(ROBUST_KEYS), {}
    if face:
        wt_ref, _ = token_loss_weights_ref(B, F, H, W, bbox=c["boxes"], face_weight=4.0)
        keys["loss_face_weight"] = 4.0
        extra = {"face_bbox": c["boxes"]}
    refs = {dt: oracle_robust_step(c["params"], c["cfg"], d, dt, is_lora_trainable, thr, 1, wt=wt_ref, device=DEV)
            for dt in (torch.float32, torch.bfloat16)}
    got = StepCapture(model, d, config(**keys), extra)
    (s32, g32, l32), (s16, g16, l16) = refs[torch.float32], refs[torch.bfloat16]
    e_b, e_r = loss_crit("robust loss", got.ld["_robust_f32"], l16, l32)
    print(f"_robust_f32 {float(got.ld['_robust_f32']):.6f} vs fp32 oracle {l32:.6f} (bf16 oracle {l16:.6f}): "
          f"{e_b:.3e} vs {e_r:.3e}")
    e_b, e_r = noise_crit("sample", got.sample, s16, s32)
    print(f"sample: build {e_b:.3e} vs reference bf16 noise {e_r:.3e}")
    assert len(g32) > 0 and set(g32) == set(got.grads)
    for k in g32:
        assert got.grads[k] is not None and float(got.grads[k].abs().max()) > 0, k
        e_b, e_r = noise_crit(k, got.grads[k], g16[k], g32[k])
        print(f"{k}: build {e_b:.3e} vs reference bf16 noise {e_r:.3e}")
    # the loss changes the backward seed and nothing in front of it
    assert torch.equal(got.sample, plain.sample)
    assert set(got.ld) == {"transformer_mse", "_mse_f32", "transformer_robust", "_robust_f32"}
    assert torch.equal(got.ld["_mse_f32"], plain.ld["_mse_f32"])
    assert torch.equal(got.ld["transformer_mse"], plain.ld["transformer_mse"])
    assert torch.equal(got.ld["transformer_robust"], got.ld["_robust_f32"].bfloat16())
    assert torch.equal(got.loss, 1.0 * got.ld["transformer_robust"])
    assert not torch.equal(got.ld["_robust_f32"], got.ld["_mse_f32"])
    assert any(not torch.equal(got.grads[k], plain.grads[k]) for k in g32)
    # rel_mse and nrmse: today's formulas on that loss, the std behind them the plain step's
    std2 = plain.loss / plain.rel_mse
    assert torch.allclose((got.loss / got.rel_mse).float(), std2.float(), rtol=2e-2)
    # the robust kernel in the loss's place (behind the weights kernel with a face weight), the rest the
    # same kernels in the same order
    new = NEW_KERNELS + ("ltx::loss_token_weights_kernel",)
    assert [n for n in got.launches if n not in new] == plain.launches
    assert got.launches.count(NEW_KERNELS[0]) == 1 and got.launches.count(NEW_KERNELS[1]) == 0
    assert got.launches.count("ltx::loss_token_weights_kernel") == (1 if face else 0)
    assert not any("wmse" in n for n in got.launches)


def _same_step(got, plain):
    assert torch.equal(got.loss, plain.loss) and torch.equal(got.rel_mse, plain.rel_mse)
    assert torch.equal(got.nrmse, plain.nrmse)
    assert torch.equal(got.sample, plain.sample)
    assert set(got.ld) == set(plain.ld) == {"transformer_mse", "_mse_f32"}
    for k in plain.ld:
        assert torch.equal(got.ld[k], plain.ld[k]), k
    assert set(got.grads) == set(plain.grads) and len(got.grads) > 0
    for k, v in plain.grads.items():
        assert v is not None and float(v.abs().max()) > 0, k
        assert torch.equal(got.grads[k], v), k


@pytest.mark.parametrize("keys", [{}, {"loss_type": "l2"}, {"loss_type": None}])
def test_defaults_are_the_unconfigured_step(keys):
    c = _case()
    plain = c["plain"]
    got = StepCapture(c["model"], c["d"], config(**keys))
    assert got.launches == plain.launches and len(plain.launches) > 0
    assert not any(n in NEW_KERNELS or "robust" in n for n in got.launches)
    _same_step(got, plain)


def test_robust_step_forward_only_writes_no_gradient():
    c = _case()
    full = StepCapture(c["model"], c["d"], config(**ROBUST_KEYS))
    fwd = StepCapture(c["model"], c["d"], config(**ROBUST_KEYS), backward=False)
    assert torch.equal(fwd.loss, full.loss) and all(v is None for v in fwd.grads.values())
    assert torch.equal(fwd.ld["transformer_mse"], c["plain"].ld["transformer_mse"])


def test_validate_epoch_keeps_its_value_under_a_robust_config():
    from ltx_amd.scheduler import RectifiedFlowScheduler
    from ltx_amd.validation import validate_epoch
    c = _case()
    d, model = c["d"], c["model"]
    batch = {"latents": d["in.latents"], "ref_image_latents": d["in.ref_image_latents"],
             "pose_latents": d["in.pose_latents"]}
    vals = []
    try:
        for tc in (config(), config(**ROBUST_KEYS), config(loss_type="smooth_l1", huber_schedule="exponential")):
            torch.manual_seed(11)
            vals.append(validate_epoch(model, [batch, batch], RectifiedFlowScheduler(), model.patchifier, tc,
                                       d["in.prompt_embeds"], d["in.prompt_attention_mask"], DEV))
    finally:
        model.train()
    assert isinstance(vals[0], float) and vals[0] > 0 and vals[0] == vals[1] == vals[2]
