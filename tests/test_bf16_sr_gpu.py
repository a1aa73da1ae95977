"""Stochastically rounded bf16 weights with f32 moments on the MI355X (FusedAdamW / FusedProdigy
bf16_update="stochastic": ltx_adamw_multi_sr, ltx_prodigy_moments_multi's mixed mode,
ltx_prodigy_apply_multi_sr). Everything but the two statistical checks is bitwise:

  * AdamW against bf16_sr_utils.AdamWModel -- the project's f32 per-tensor step on the widened values, then
    training.stochastic_round_bf16 on the CPU -- plain, under a clip that bites and one that does not,
    with the EMA, with multi_tensor=False and with the group split in two;
  * 64 steps of a sixteenth of a bf16 spacing each: lost under round-to-nearest, kept in the mean here;
  * Prodigy against prodigy_utils.ProdigyStatement on the widened values, fed the device's d and dlr as
    tests/test_prodigy_gpu.py does, plain and with clip + EMA;
  * the tiny model through train_loop: resume, two runs of one seed, another seed;
  * the mode mismatch on load, and "nearest" as today's run.

Tensor sizes: bf16_sr_utils.BF16_SIZES (a vector is 8 elements, a chunk 2048) and one f32 tensor; the
model runs use the tiny config and helpers of tests/test_adapter_ckpt_gpu.py."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

from bf16_sr_utils import BF16_SIZES, AdamWModel, make_grads, make_params, sr_store
from prodigy_utils import ProdigyStatement
from test_adapter_ckpt_gpu import _build, _config, _same, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x5EED0123456789AB  # both key words in use
LR, WD = 1e-3, 0.01
NB = len(BF16_SIZES)
BF16 = torch.bfloat16


def _step(opt, ps, grads):
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    opt.step()


def _check_adamw(opt, ps, model, f32_twin, where):
    """the bf16 tensors against the model, the f32 tensor against its twin of an optimizer without the mode"""
    for i in range(NB):
        st = opt.state[ps[i]]
        assert ps[i].dtype == BF16 and st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32
        assert torch.equal(st["exp_avg"], model.exp_avg[i]), (where, i, "exp_avg")
        assert torch.equal(st["exp_avg_sq"], model.exp_avg_sq[i]), (where, i, "exp_avg_sq")
        bad = int((ps[i].detach().view(torch.int16) != model.p[i].view(torch.int16)).sum())
        assert bad == 0, (where, i, "param", BF16_SIZES[i], bad)
    (tp, topt), p = f32_twin, ps[NB]
    assert torch.equal(p, tp), (where, "f32 param")
    for key in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(opt.state[p][key], topt.state[tp][key]), (where, "f32", key)


def _f32_twin():
    from ltx_amd.training import FusedAdamW
    tp = make_params(1, DEV)[NB]
    return tp, FusedAdamW([tp], lr=LR, weight_decay=WD)


_PLAIN = {}


def _plain_run():
    """Three plain stochastic steps, run once and left unchanged: what the variants must reproduce.
    Returns per step the parameters and the two moments of every tensor."""
    from ltx_amd.training import FusedAdamW
    if not _PLAIN:
        ps = make_params(1, DEV)
        opt = FusedAdamW(ps, lr=LR, weight_decay=WD, bf16_update="stochastic", sr_seed=SEED)
        snaps = []
        for k in range(3):
            _step(opt, ps, make_grads(10 + k, DEV))
            snaps.append([(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                          for p in ps])
        _PLAIN["snaps"] = snaps
    return _PLAIN["snaps"]


def _same_as_plain(opt, ps, k, where):
    for i, (p, (wp, wm, wv)) in enumerate(zip(ps, _plain_run()[k])):
        assert torch.equal(p.detach(), wp), (where, k, i, "param")
        assert torch.equal(opt.state[p]["exp_avg"], wm) and torch.equal(opt.state[p]["exp_avg_sq"], wv), (where, k, i)


# ---------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------
def test_adamw_is_the_f32_step_then_the_stochastic_store_bitwise():
    from ltx_amd.training import FusedAdamW
    ps = make_params(1, DEV)
    opt = FusedAdamW(ps, lr=LR, weight_decay=WD, bf16_update="stochastic", sr_seed=SEED)
    model = AdamWModel(ps[:NB], SEED, LR, WD)
    tp, topt = _f32_twin()
    for k in range(3):
        grads = make_grads(10 + k, DEV)
        _step(opt, ps, grads)
        model.step(grads[:NB])
        _step(topt, [tp], grads[NB:])
        _check_adamw(opt, ps, model, (tp, topt), ("plain", k))
        _same_as_plain(opt, ps, k, "plain")
        assert all(opt.state[p]["step"] == k + 1 for p in ps)
    assert opt.grad_norm is None and opt.clip_coef is None
    group = opt.param_groups[0]
    assert group["bf16_update"] == "stochastic" and group["sr_seed"] == SEED


def test_a_bf16_parameter_needs_a_bf16_gradient():
    from ltx_amd.training import FusedAdamW, FusedProdigy
    for cls in (FusedAdamW, FusedProdigy):
        p = torch.nn.Parameter(torch.ones(8, dtype=BF16, device=DEV))
        opt = cls([p], bf16_update="stochastic")
        p.grad_dtype = None  # torch then lets a gradient of another dtype in
        p.grad = torch.ones(8, dtype=torch.float32, device=DEV)
        with pytest.raises(TypeError, match="bf16"):
            opt.step()
        assert torch.equal(p.detach(), torch.ones(8, dtype=BF16, device=DEV)) and not opt.state[p]


def test_a_clip_that_does_not_bite_is_the_plain_step_and_one_that_bites_scales_the_bf16_gradient():
    from ltx_amd.training import FusedAdamW
    ps = make_params(1, DEV)
    opt = FusedAdamW(ps, lr=LR, weight_decay=WD, max_grad_norm=1e30, bf16_update="stochastic", sr_seed=SEED)
    for k in range(3):
        _step(opt, ps, make_grads(10 + k, DEV))
        assert float(opt.clip_coef) == 1.0
        _same_as_plain(opt, ps, k, "huge max_grad_norm")
    ps = make_params(1, DEV)
    opt = FusedAdamW(ps, lr=LR, weight_decay=WD, max_grad_norm=0.5, bf16_update="stochastic", sr_seed=SEED)
    model = AdamWModel(ps[:NB], SEED, LR, WD)
    tp = make_params(1, DEV)[NB]
    fm, fv = torch.zeros_like(tp), torch.zeros_like(tp)
    from ltx_amd import ops
    for k in range(3):
        grads = make_grads(10 + k, DEV)
        _step(opt, ps, grads)
        coef = opt.clip_coef
        assert 0.0 < float(coef) < 1.0
        for p, g in zip(ps, grads):
            assert torch.equal(p.grad, g)  # scaled on the way in, never in memory
        model.step(grads[:NB], coef=coef)
        for i in range(NB):
            assert torch.equal(ps[i].detach(), model.p[i]), (k, i)
            assert torch.equal(opt.state[ps[i]]["exp_avg"], model.exp_avg[i]), (k, i)
            assert torch.equal(opt.state[ps[i]]["exp_avg_sq"], model.exp_avg_sq[i]), (k, i)
        # the f32 tensor: today's clipped step, the f32 per-tensor kernel on g * coef
        with torch.no_grad():
            ops.adamw_step(tp, grads[NB] * coef, fm, fv, LR, 0.9, 0.999, 1e-8, WD, k + 1)
        assert torch.equal(ps[NB].detach(), tp.detach()) and torch.equal(opt.state[ps[NB]]["exp_avg"], fm)


def test_with_the_ema_the_step_is_the_plain_one_and_the_shadow_follows_the_value_stored():
    from ltx_amd.training import EMASchedule, FusedAdamW
    sched = EMASchedule(0.999)
    ps = make_params(1, DEV)
    opt = FusedAdamW(ps, lr=LR, weight_decay=WD, ema=sched, bf16_update="stochastic", sr_seed=SEED)
    for k in range(3):
        prev = [opt.state[p]["ema"].clone() if k else p.detach().float().clone() for p in ps]
        _step(opt, ps, make_grads(10 + k, DEV))
        _same_as_plain(opt, ps, k, "ema")
        omd = torch.tensor(1.0 - sched.decay_at(k + 1), dtype=torch.float32, device=DEV)
        for i, p in enumerate(ps):
            shadow = opt.state[p]["ema"]
            want = prev[i].clone()
            want.sub_((want - p.detach().float()) * omd)  # three separately rounded f32 operations
            assert shadow.dtype == torch.float32 and torch.equal(shadow, want), (k, i)
    # and with the clip on top, still the plain bits when it does not bite
    ps = make_params(1, DEV)
    opt = FusedAdamW(ps, lr=LR, weight_decay=WD, ema=sched, max_grad_norm=1e30, bf16_update="stochastic", sr_seed=SEED)
    for k in range(3):
        _step(opt, ps, make_grads(10 + k, DEV))
        _same_as_plain(opt, ps, k, "ema + clip")


def test_launch_grouping_does_not_change_the_bits():
    """multi_tensor=False, one group split in two with the same hyper-parameters (the ordinal is the index
    in the concatenation of the groups), and gradients one element off the 16-byte boundary (the
    one-element path: the same lane of the same generator call)."""
    from ltx_amd.training import FusedAdamW
    ps = make_params(1, DEV)
    opt = FusedAdamW(ps, lr=LR, weight_decay=WD, multi_tensor=False, bf16_update="stochastic", sr_seed=SEED)
    for k in range(3):
        _step(opt, ps, make_grads(10 + k, DEV))
        _same_as_plain(opt, ps, k, "multi_tensor=False")
    ps = make_params(1, DEV)
    opt = FusedAdamW([{"params": ps[:3]}, {"params": ps[3:]}], lr=LR, weight_decay=WD, bf16_update="stochastic",
                     sr_seed=SEED)
    for k in range(3):
        _step(opt, ps, make_grads(10 + k, DEV))
        _same_as_plain(opt, ps, k, "two groups")
    ps = make_params(1, DEV)
    opt = FusedAdamW(ps, lr=LR, weight_decay=WD, bf16_update="stochastic", sr_seed=SEED)
    for k in range(3):
        for p, g in zip(ps, make_grads(10 + k, DEV)):
            buf = torch.empty(g.numel() + 1, dtype=g.dtype, device=DEV)
            p.grad = buf[1:].copy_(g)
            assert p.grad.data_ptr() % 16 != 0
        opt.step()
        _same_as_plain(opt, ps, k, "unaligned gradients")


def test_small_steps_accumulate():
    """65 536 bf16 ones, g = -1, lr = 2^-11 (a sixteenth of the spacing 2^-7 above 1), no weight decay, 64
    steps: AdamW's step under a constant gradient is lr / (1 + eps), so the f32 walk ends 4 spacings up.
    Round-to-nearest loses every step. Stochastically each step moves an element up one spacing with
    probability 1/16: per element the sum of 64 such draws, variance 64 * 15 / 256 spacings^2, and the
    mean over N elements has sigma = sqrt(64 * 15 / 256) / 256 = 0.0076 spacings; the CPU statement gives
    4.0014 spacings (+0.19 sigma)."""
    from ltx_amd.training import FusedAdamW
    n, ulp = 65536, 2.0 ** -7
    g = torch.full((n,), -1.0, dtype=BF16, device=DEV)
    pn = torch.nn.Parameter(torch.ones(n, dtype=BF16, device=DEV))
    ps = torch.nn.Parameter(torch.ones(n, dtype=BF16, device=DEV))
    near = FusedAdamW([pn], lr=2.0 ** -11, weight_decay=0.0, bf16_update="nearest")
    stoch = FusedAdamW([ps], lr=2.0 ** -11, weight_decay=0.0, bf16_update="stochastic", sr_seed=1)
    for _ in range(64):
        _step(near, [pn], [g])
        _step(stoch, [ps], [g])
    assert torch.equal(pn.detach(), torch.ones(n, dtype=BF16, device=DEV))  # the defect
    moved = (float(ps.detach().double().mean()) - 1.0) / ulp
    sigma = (64 * 15 / 256) ** 0.5 / 256
    print(f"mean(p) - 1 = {moved:.4f} spacings, {(moved - 4.0) / sigma:+.2f} sigma")
    assert abs(moved - 4.0) <= 5 * sigma
    assert near.state[pn]["exp_avg"].dtype == BF16 and stoch.state[ps]["exp_avg"].dtype == torch.float32


# ---------------------------------------------------------------------------------------------
# Prodigy
# ---------------------------------------------------------------------------------------------
SMALL = 1e-4  # test_prodigy_gpu.SMALL: the first steps are a few d0 long


def _drift_grads(seed, k, scale=1.0):
    """test_prodigy_gpu._drift_grads on this file's sizes: a fixed direction plus fresh noise of half its
    size, so <g, p0 - p> grows"""
    base, noise = make_grads(seed, DEV, scale), make_grads(1000 * seed + k + 1, DEV, 0.5 * scale)
    return [(b.float() + n.float()).to(b.dtype) for b, n in zip(base, noise)]


@pytest.mark.parametrize("variant", ["plain", "clip_ema", "decoupled_weight_decay"])
def test_prodigy_is_the_f32_statement_then_the_stochastic_store_bitwise(variant):
    """The statement runs on f32 copies float(p) with float(g) (under the clip float(bf16(float(g) * coef)))
    and is fed the device's d and dlr; after its step every widened bf16 tensor is stored through
    stochastic_round_bf16. exp_avg, exp_avg_sq, s (f32), p0 and the parameters are bitwise the device's; of
    the record, k / applied / dlr / d are the device's by construction, d_denom and d_numerator are f64
    sums of the same f32 terms in another order: within 2^-40 of the sum of the terms' magnitudes (fewer
    than 2^13 terms of 2^-53 relative error each)."""
    from ltx_amd.training import EMASchedule, FusedProdigy
    clip = variant == "clip_ema"
    sched = EMASchedule(0.999) if clip else None
    kw = dict(weight_decay=0.01, decouple=True) if variant == "decoupled_weight_decay" else {}
    ps = make_params(7, DEV, scale=SMALL)
    qs = [torch.nn.Parameter(p.detach().float().clone()) for p in ps]
    start = [p.detach().clone() for p in ps]
    opt = FusedProdigy(ps, max_grad_norm=0.5 if clip else None, ema=sched, bf16_update="stochastic", sr_seed=SEED, **kw)
    ref = ProdigyStatement(qs, **kw)
    num_bound, ds = 0.0, []
    for k in range(5):
        grads = _drift_grads(100, k, scale=0.1 * (k + 1))
        prev = [opt.state[p]["ema"].clone() if k else p.detach().float().clone() for p in ps] if clip else None
        _step(opt, ps, grads)
        rec = dict(zip(opt.RECORD, opt.record.tolist()))
        assert rec["applied"] == 1.0 and rec["k"] == k + 1
        G = [g.float() for g in grads]
        if clip:
            coef = opt.clip_coef
            assert 0.0 < float(coef) < 1.0
            G = [(g * coef).to(BF16).float() for g in G[:NB]] + [G[NB] * coef]
        terms = sum(float(((ref._state(q)["p0"] - q.detach()) * g).abs().double().sum()) for q, g in zip(qs, G))
        d_old = ref.d
        ref.step(G, override=(rec["d"], rec["dlr"]))
        with torch.no_grad():
            for i in range(NB):
                qs[i].copy_(sr_store(qs[i], SEED, i, k + 1).float())
        for i, (p, q) in enumerate(zip(ps, qs)):
            for key in ("exp_avg", "exp_avg_sq", "s"):
                a, b = opt.state[p][key], ref.state[q][key]
                assert a.dtype == torch.float32 and torch.equal(a, b), (variant, k, i, key, int((a != b).sum()))
            assert opt.state[p]["p0"].dtype == p.dtype and torch.equal(opt.state[p]["p0"], start[i])
            assert torch.equal(p.detach().float(), q.detach()), (variant, k, i, "param", int((p.float() != q).sum()))
        den = sum(float(ref.state[q]["s"].abs().double().sum()) for q in qs)
        assert abs(rec["d_denom"] - den) <= 2.0 ** -40 * den
        num_bound = ref.beta3 * num_bound + (d_old / ref.d0) * rec["dlr"] * terms
        assert abs(rec["d_numerator"] - ref.d_numerator) <= 2.0 ** -40 * num_bound, (k, rec["d_numerator"], ref.d_numerator)
        if clip:
            omd = torch.tensor(1.0 - sched.decay_at(k + 1), dtype=torch.float32, device=DEV)
            for i, p in enumerate(ps):
                want = prev[i].clone()
                want.sub_((want - p.detach().float()) * omd)
                assert torch.equal(opt.state[p]["ema"], want), (k, i)
        ds.append(rec["d"])
    print(variant, "d per step:", ds)
    assert all(not torch.equal(p.detach(), s0) for p, s0 in zip(ps[3:], start[3:]))  # the tensors moved


OFF_SIZES = [1, 7, 8, 9, 2047, 2049, 4096 + 13]


def _one_element_off(t):
    """a copy of `t` that starts one element (2 or 4 bytes) past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].copy_(t.detach())
    assert out.data_ptr() % 16 == t.element_size()
    return out


@pytest.mark.parametrize("kind", ["adamw", "prodigy"])
def test_tensors_one_element_off_the_16_byte_boundary_give_the_aligned_tensors_bits(kind):
    """Parameters and gradients that start one element off a 16-byte boundary take the one-element walk of
    ltx_adamw_multi_sr, of ltx_prodigy_moments_multi's mixed mode and of ltx_prodigy_apply_multi_sr (each with
    the clip and the shadow column); the aligned copies of the same values take the 16-byte walk with its
    single-element tail. Parameters, moments, s and shadows are bitwise the same after each of 3 steps."""
    from ltx_amd.training import EMASchedule, FusedAdamW, FusedProdigy
    cls, kw, scale = (FusedAdamW, dict(lr=LR, weight_decay=WD), 1.0) if kind == "adamw" else (FusedProdigy, {}, SMALL)
    pa = make_params(3, DEV, scale=scale, sizes=OFF_SIZES)
    pb = [torch.nn.Parameter(_one_element_off(p)) for p in pa]
    a, b = (cls(ps, max_grad_norm=0.5, ema=EMASchedule(0.999), bf16_update="stochastic", sr_seed=SEED, **kw)
            for ps in (pa, pb))
    for k in range(3):
        grads = make_grads(30 + k, DEV, sizes=OFF_SIZES)
        for x, y, g in zip(pa, pb, grads):
            x.grad, y.grad = g.clone(), _one_element_off(g)
            assert x.data_ptr() % 16 == 0 and x.grad.data_ptr() % 16 == 0
        a.step()
        b.step()
        assert 0.0 < float(a.clip_coef) < 1.0 and float(a.clip_coef) == float(b.clip_coef)
        for i, (x, y) in enumerate(zip(pa, pb)):
            assert torch.equal(x.detach(), y.detach()), (kind, k, i, "param")
            keys = [key for key, v in a.state[x].items() if torch.is_tensor(v)]
            assert "ema" in keys and "exp_avg_sq" in keys and ("s" in keys) == (kind == "prodigy")
            for key in keys:
                assert torch.equal(a.state[x][key], b.state[y][key]), (kind, k, i, key)
    start = make_params(3, DEV, scale=scale, sizes=OFF_SIZES)
    assert all(not torch.equal(x.detach(), p) for x, p in zip(pa[4:], start[4:]))  # the large tensors moved


# ---------------------------------------------------------------------------------------------
# the tiny model through train_loop
# ---------------------------------------------------------------------------------------------
def _run(tiny, out, epochs, extra, save=False, resume=None):
    """train_loop on fresh model / loader objects under torch.manual_seed(77) with the config attributes
    `extra`: (model, the optimizer train_loop built, logs, the caption projection after the first step)."""
    from ltx_amd import io, training
    made = []

    class Recording(training.FusedAdamW):  # train_loop keeps its optimizer to itself
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(training, "FusedAdamW", Recording)
        model = _build(tiny, {})
        loader = io.LatentLoader(tiny["ds"]["train"], 2, DEV, shuffle=True, seed=1)
        tc = _config(extra, learning_rate=1e-3, num_epochs=epochs, output_dir=str(out), save_every_n_epochs=1)
        if save:
            tc.save_adapters = True
        logs, first = [], {}

        def log(payload, step):
            logs.append((step, payload))
            if not first and "train/loss" in payload:
                first.update({n: p.detach().clone() for n, p in model.named_parameters()
                              if p.requires_grad and "caption_projection" in n})
        torch.manual_seed(77)
        training.train_loop(model, tc, loader, tiny["prompt"], tiny["mask"], log_fn=log, resume_from=resume)
    return model, made[0], logs, first


def _state(model, opt):
    names = {id(p): n for n, p in model.named_parameters()}
    params = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    moments = {}
    for p, st in opt.state.items():
        moments["exp_avg." + names[id(p)]], moments["exp_avg_sq." + names[id(p)]] = st["exp_avg"], st["exp_avg_sq"]
    return params, moments


STOCH = {"bf16_update": "stochastic", "bf16_sr_seed": 1234}
_RUNS = {}


def _first_epoch(tiny, tmp_path_factory, key):
    """One epoch with save_adapters under the config attributes of `key`, run once and left unchanged."""
    if key not in _RUNS:
        out = tmp_path_factory.mktemp("sr_first") / "out"
        extra = {"stoch": STOCH, "absent": {}, "nearest": {"bf16_update": "nearest"}}[key]
        _RUNS[key] = (out,) + _run(tiny, out, 1, extra, save=True)
    return _RUNS[key]


def _losses(logs, epoch):
    return [(s, p["train/loss"]) for s, p in logs if "train/loss" in p and p.get("train/epoch") == epoch]


def test_resumed_run_is_bitwise_the_uninterrupted_run(tiny, tmp_path_factory, tmp_path):
    import shutil
    model_a, opt_a, logs_a, first_a = _run(tiny, tmp_path / "a", 2, STOCH)
    out1, model_1, opt_1, logs_1, first_1 = _first_epoch(tiny, tmp_path_factory, "stoch")
    out_b = tmp_path / "b"
    shutil.copytree(out1, out_b)
    saved = load_file(str(out_b / "adapter_epoch_1" / "optimizer.safetensors"))
    names = {id(p): n for n, p in model_1.named_parameters()}
    bf16_names = [names[id(p)] for p in opt_1.state if p.dtype == BF16]
    assert bf16_names and all("caption_projection" in n for n in bf16_names)
    for n in bf16_names:  # the moments in their stored dtype
        assert saved["exp_avg." + n].dtype == saved["exp_avg_sq." + n].dtype == torch.float32
    with open(out_b / "adapter_epoch_1" / "train_state.json") as f:
        group = json.load(f)["optimizer"]["param_groups"][0]
    assert group["bf16_update"] == "stochastic" and group["sr_seed"] == 1234
    model_b, opt_b, logs_b, _ = _run(tiny, out_b, 2, STOCH, resume="auto")
    (pa, ma), (pb, mb) = _state(model_a, opt_a), _state(model_b, opt_b)
    _same(pa, pb)
    _same(ma, mb)
    assert _losses(logs_a, 1) == _losses(logs_b, 1) and len(_losses(logs_a, 1)) == 2
    assert _losses(logs_a, 0) == _losses(logs_1, 0)
    # two runs with one seed: the one-epoch run's first step is the two-epoch run's, bit for bit
    _same(first_a, first_1)


def test_another_seed_changes_caption_projection_bits_after_the_first_step(tiny, tmp_path_factory, tmp_path):
    _, _, _, logs_1, first_1 = _first_epoch(tiny, tmp_path_factory, "stoch")
    _, opt, logs, first = _run(tiny, tmp_path / "o", 1, dict(STOCH, bf16_sr_seed=1235))
    assert sorted(first) == sorted(first_1) and first
    assert any(not torch.equal(first[n], first_1[n]) for n in first)
    assert _losses(logs, 0)[0] == _losses(logs_1, 0)[0]  # the first step's loss precedes any rounding
    assert opt.sr_seed == 1235


def test_loading_another_mode_or_seed_raises_and_writes_nothing(tiny, tmp_path_factory):
    from ltx_amd import io
    from ltx_amd.training import FusedAdamW
    stoch_dir = _first_epoch(tiny, tmp_path_factory, "stoch")[0] / "adapter_epoch_1"
    near_dir = _first_epoch(tiny, tmp_path_factory, "absent")[0] / "adapter_epoch_1"
    for path, kw, match in ((near_dir, dict(bf16_update="stochastic", sr_seed=1234), "bf16_update"),
                            (stoch_dir, {}, "bf16_update"),
                            (stoch_dir, dict(bf16_update="stochastic", sr_seed=1235), "sr_seed")):
        model = _build(tiny, {})
        params = [p for p in model.parameters() if p.requires_grad]
        before = [p.detach().clone() for p in params]
        opt = FusedAdamW(params, lr=1e-3, **kw)
        groups = [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups]
        with pytest.raises(ValueError, match=match):
            io.load_adapter_checkpoint(model, str(path), optimizer=opt)
        assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
        assert len(opt.state) == 0
        assert [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups] == groups
    # the matching optimizer loads, and the moments arrive as f32
    model = _build(tiny, {})
    params = [p for p in model.parameters() if p.requires_grad]
    opt = FusedAdamW(params, lr=1e-3, bf16_update="stochastic", sr_seed=1234)
    io.load_adapter_checkpoint(model, str(stoch_dir), optimizer=opt)
    assert all(st["exp_avg"].dtype == torch.float32 for st in opt.state.values()) and len(opt.state) == len(params)


def test_nearest_is_todays_run(tiny, tmp_path_factory):
    """bf16_update: nearest against the keys absent: parameters, the bf16 moments, the param_groups keys
    and train_state.json"""
    out_a, model_a, opt_a, logs_a, _ = _first_epoch(tiny, tmp_path_factory, "absent")
    out_n, model_n, opt_n, logs_n, _ = _first_epoch(tiny, tmp_path_factory, "nearest")
    (pa, ma), (pn, mn) = _state(model_a, opt_a), _state(model_n, opt_n)
    _same(pa, pn)
    _same(ma, mn)
    assert any(v.dtype == BF16 for v in ma.values())
    assert [sorted(g) for g in opt_a.param_groups] == [sorted(g) for g in opt_n.param_groups]
    assert not {"bf16_update", "sr_seed"} & set(opt_n.param_groups[0])
    with open(out_a / "adapter_epoch_1" / "train_state.json") as fa, open(out_n / "adapter_epoch_1" / "train_state.json") as fn:
        assert fa.read() == fn.read()
    assert _losses(logs_a, 0) == _losses(logs_n, 0)
    assert sorted(os.listdir(out_a / "adapter_epoch_1")) == sorted(os.listdir(out_n / "adapter_epoch_1"))
