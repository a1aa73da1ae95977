"""Prodigy for the LoRA optimizer step on the MI355X (training.FusedProdigy: ltx_prodigy_moments_multi,
ltx_prodigy_d_update, ltx_prodigy_apply_multi), against tests/prodigy_utils.ProdigyStatement, the statement
in plain torch eager ops on the same device.

  * the two sums and the f64 update of the record: bitwise on inputs whose every product and sum is
    exact, within a bound worked out from the two f32 roundings per term on random ones, and bitwise
    between two calls;
  * exp_avg, exp_avg_sq, s and the parameters after every step: bitwise the statement's when it is fed
    the device's d and dlr (the sums have their own order, so d itself is not compared bitwise);
  * with clipping, with the EMA, with parameters that have no gradient, the launch sequence, no host sync;
  * the tiny model through train_loop: d is logged and grows, a resumed run is bitwise the uninterrupted
    one, and without the new keys the run is today's.

Tensor sizes are those of tests/test_optim_clip_gpu.py ([1, 2047, 2048, 2049, 5000], alternating f32 and
bf16: one element, one short of a chunk, a chunk, one over, several chunks with a ragged tail) and one
bf16 tensor of 300 x 2048 elements, so the one-block finish adds more than 256 partials; the model runs use
the tiny config and helpers of tests/test_adapter_ckpt_gpu.py."""
import ctypes
import json
import math
import os

import pytest
import torch
from safetensors.torch import load_file

from prodigy_utils import ProdigyStatement
from test_adapter_ckpt_gpu import CASES, _build, _config, _same, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 77
SIZES = [1, 2047, 2048, 2049, 5000, 300 * 2048]
DTYPES = [torch.float32, torch.bfloat16, torch.float32, torch.bfloat16, torch.float32, torch.bfloat16]
ENTRY_POINTS = {"ltx_prodigy_moments_multi", "ltx_prodigy_d_update", "ltx_prodigy_apply_multi"}
STATES = ("exp_avg", "exp_avg_sq", "s", "p0")
# Parameters of this size in the runs that watch d grow: the first steps are a few d0 = 1e-6 long, which a
# bf16 parameter near 1 cannot take (its spacing is 2^-8), and a tensor that does not move adds to the sum of
# |s| but not to <g, p0 - p>, which holds d at d0.
SMALL = 1e-4
FOUR = ["adapter_config.json", "adapter_model.safetensors", "optimizer.safetensors", "train_state.json"]


def _params(seed=0, sizes=SIZES, dtypes=DTYPES, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((scale * torch.randn(n, generator=g)).to(dt).to(DEV)) for n, dt in zip(sizes, dtypes)]


def _rand_grads(seed, scale=1.0, sizes=SIZES, dtypes=DTYPES):
    g = torch.Generator().manual_seed(seed)
    return [(scale * torch.randn(n, generator=g)).to(dt).to(DEV) for n, dt in zip(sizes, dtypes)]


def _drift_grads(seed, k, scale=1.0):
    """Step k's gradients of a run: a fixed direction (seed) plus fresh noise (seed, k) of half its size.
    Independent gradients would leave <g, p0 - p> a zero-mean sum and d at d0; these make it grow."""
    base, noise = _rand_grads(seed, scale), _rand_grads(1000 * seed + k + 1, 0.5 * scale)
    return [(b.float() + n.float()).to(b.dtype) for b, n in zip(base, noise)]


def _ints(seed, lo, hi, scale, sizes, dtypes):
    """integers in [lo, hi] times `scale` (a power of two): exact in f32 and in bf16"""
    g = torch.Generator().manual_seed(seed)
    return [(scale * torch.randint(lo, hi + 1, (n,), generator=g)).to(dt).to(DEV) for n, dt in zip(sizes, dtypes)]


def _step(opt, ps, grads):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.clone()
    opt.step()


def _record(opt):
    return dict(zip(opt.RECORD, opt.record.tolist()))


def _bits(values):
    return [float(v).hex() for v in values]


def _inject(opt, ps, grads, s, p0):
    """State as after earlier steps, set by hand (zero moments); returns the optimizer's items per dtype."""
    by_dtype = {}
    for i, p in enumerate(ps):
        opt.state[p] = st = {"step": 1, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p),
                             "s": s[i].clone(), "p0": p0[i].clone()}
        by_dtype.setdefault(p.dtype, []).append((p, grads[i], st))
    return by_dtype


def _pass1_and_update(opt, by_dtype, hyper, coef=None):
    """The two launches of the d update, called directly: pass 1 per dtype (the second dtype's partials
    behind the first's), then ltx_prodigy_d_update. Returns the partials as a [rows, 2] f64 tensor."""
    from ltx_amd import ops
    lr, b1, b2, b3, d0, d_coef, growth = hyper
    tables = [opt._items_table("prodigy", dt, items) + (1 if dt == torch.bfloat16 else 0,)
              for dt, items in by_dtype.items()]
    total = sum(n for _, n, _ in tables)
    part = torch.full((2 * total,), float("nan"), dtype=torch.float64, device=DEV)  # overwritten, never accumulated into
    off = 0
    for dev, nrows, is_bf16 in tables:
        ops.call("ltx_prodigy_moments_multi", ops._p(dev), nrows, is_bf16, ops._p(opt.record), lr, b1, b2, b3, d0,
                 0.0, 0, 0, None if coef is None else ops._p(coef), ctypes.c_void_p(part.data_ptr() + 16 * off), ops._s())
        off += nrows
    ops.call("ltx_prodigy_d_update", ops._p(part), total, ops._p(opt.record), lr, b1, b2, b3, d0, d_coef, growth, 0,
             ops._s())
    torch.cuda.synchronize()
    return part.view(total, 2)


# ---------------------------------------------------------------------------------------------
# the sums and the record
# ---------------------------------------------------------------------------------------------
# (name, d, record's d_max, record's d_numerator, growth_rate, zero gradients)
EXACT = [("first_step_d_equals_d0", 2.0 ** -20, 2.0 ** -20, 0.0, float("inf"), False),
         ("growth_rate_binds", 2.0 ** -10, 2.0 ** -10, 2.0 ** 24, 1.5, False),
         ("d_denom_zero", 2.0 ** -20, 2.0 ** -20, 0.0, float("inf"), True)]


@pytest.mark.parametrize("name, d, d_max, d_num, growth, zero", EXACT, ids=[e[0] for e in EXACT])
def test_exact_inputs_give_the_exact_sums_and_record(name, d, d_max, d_num, growth, zero):
    """g, p0 - p and s are small integers times powers of two and d, d0, lr, 1 - beta1, 1 - beta2, beta3
    are powers of two (beta2 = 0.75 on exp_avg_sq = 0), so every product and every partial sum is exact and
    any summation order gives the f64 sums bit for bit; the record then is the f64 formulae's. A second
    f32 tensor of 2100 x 2048 elements takes the finish past its first 8 x 256 rows."""
    from ltx_amd.training import FusedProdigy
    sizes, dtypes = SIZES + [2100 * 2048], DTYPES + [torch.float32]
    d0, lr, b1, b2, b3, d_coef = 2.0 ** -20, 1.0, 0.5, 0.75, 0.5, 1.0
    ps = _ints(1, -3, 3, 2.0 ** -4, sizes, dtypes)
    p0 = [p + q for p, q in zip(ps, _ints(2, -3, 3, 2.0 ** -3, sizes, dtypes))]
    grads = _ints(3, 0 if zero else -3, 0 if zero else 3, 1.0, sizes, dtypes)
    # s / 2 + (d / d0) dlr g must stay exact in bf16: s = 0 where that factor is 2^-20, quarters where it is 1
    s = _ints(4, 0, 0, 1.0, sizes, dtypes) if d == d0 else _ints(4, -3, 3, 0.25, sizes, dtypes)
    opt = FusedProdigy([torch.nn.Parameter(p) for p in ps], lr=lr, betas=(b1, b2), beta3=b3, d0=d0, growth_rate=growth)
    params = opt.param_groups[0]["params"]
    opt.ensure_record().copy_(torch.tensor([d, d_max, d_num, 0.0, 0.25, 0.0, 3.0, 1.0], dtype=torch.float64))
    by_dtype = _inject(opt, params, grads, s, p0)
    part = _pass1_and_update(opt, by_dtype, (lr, b1, b2, b3, d0, d_coef, growth))
    dlr = d * lr
    a3 = (d / d0) * dlr
    want_num = want_den = 0.0
    for p, g, s0, q0 in zip(params, grads, s, p0):
        st = opt.state[p]
        s_new = s0.double() * b3 + a3 * g.double()
        assert torch.equal(st["s"].double(), s_new) and st["s"].dtype == p.dtype
        assert torch.equal(st["exp_avg"].double(), d * (1 - b1) * g.double())
        assert torch.equal(st["exp_avg_sq"].double(), d * d * (1 - b2) * g.double() ** 2)
        want_num += float(((q0.double() - p.detach().double()) * g.double()).sum())
        want_den += float(s_new.abs().sum())
    assert not torch.isnan(part).any()
    assert float(part[:, 0].sum()).hex() == want_num.hex() and float(part[:, 1].sum()).hex() == want_den.hex()
    rec = _record(opt)
    if zero:
        assert want_den == 0.0
        want = {"d": d, "d_max": d_max, "d_numerator": d_num, "d_denom": 0.0, "d_hat": 0.25, "dlr": dlr, "k": 3.0,
                "applied": 0.0}
    else:
        assert want_den > 0.0 and want_num != 0.0
        numerator = b3 * d_num + (d / d0) * dlr * want_num
        d_hat = d_coef * numerator / want_den
        new_d = max(d, d_hat) if d == d0 else d
        new_max = max(d_max, d_hat)
        new_d = min(new_max, new_d * growth)
        want = {"d": new_d, "d_max": new_max, "d_numerator": numerator, "d_denom": want_den, "d_hat": d_hat,
                "dlr": dlr, "k": 4.0, "applied": 1.0}
        if name == "growth_rate_binds":
            assert new_d == 1.5 * d < new_max
    assert _bits(rec[k] for k in opt.RECORD) == _bits(want[k] for k in opt.RECORD), (rec, want)


def test_random_inputs_sum_error_bounds():
    """|SUM_dev - SUM_f64| <= 4 2^-24 sum |g_i| |p0_i - p_i|: per term the subtraction and the product
    round once each in f32 (unit roundoff 2^-24; for bf16 tensors the statement's R(p0 - p) is the term's
    factor and the f32 product of two bf16 values is exact), with margin 2; the f64 accumulation of ~10^6
    terms adds 10^6 2^-53, which is negligible against that. The same form with sum |s_i| for the
    denominator. d = d0 = 2^-20 and lr = 1 make (d / d0) dlr a power of two, so SUM_dev is the record's
    d_numerator scaled back exactly."""
    from ltx_amd.training import FusedProdigy
    d0, lr, b1, b2 = 2.0 ** -20, 1.0, 0.9, 0.999
    b3 = math.sqrt(b2)
    for seed, scale in ((2, 1.0), (3, 1e-3), (4, 300.0)):
        ps = [torch.nn.Parameter(p.detach()) for p in _params(seed)]
        p0 = _params(seed + 10)
        p0 = [p.detach() for p in p0]
        grads = _rand_grads(seed + 20, scale)
        s = _rand_grads(seed + 30, scale * 2.0 ** -20)
        opt = FusedProdigy(ps, lr=lr, betas=(b1, b2), d0=d0)
        opt.ensure_record()
        by_dtype = _inject(opt, ps, grads, s, p0)
        _pass1_and_update(opt, by_dtype, (lr, b1, b2, b3, d0, 1.0, float("inf")))
        rec = _record(opt)
        assert rec["applied"] == 1.0 and rec["dlr"] == d0
        num_dev, den_dev = rec["d_numerator"] * 2.0 ** 20, rec["d_denom"]
        num64 = bound = den64 = 0.0
        for p, g, q0 in zip(ps, grads, p0):
            diff = (q0 - p.detach()).double() if p.dtype == torch.bfloat16 else q0.double() - p.detach().double()
            num64 += float((diff * g.double()).sum())
            bound += float((diff.abs() * g.double().abs()).sum())
            den64 += float(opt.state[p]["s"].double().abs().sum())
        print(f"scale {scale}: num {num_dev!r} f64 {num64!r} err {abs(num_dev - num64):.3e} bound {4 * 2.0 ** -24 * bound:.3e}; "
              f"den {den_dev!r} f64 {den64!r} err {abs(den_dev - den64):.3e} bound {4 * 2.0 ** -24 * den64:.3e}")
        assert abs(num_dev - num64) <= 4 * 2.0 ** -24 * bound
        assert abs(den_dev - den64) <= 4 * 2.0 ** -24 * den64
        assert den64 > 0 and bound > 0


def test_two_calls_give_the_same_record_bitwise():
    """Two optimizers over other buffers, stepped on identical gradients, hold bitwise-identical records
    and parameters after each of 5 steps: d needs no collective under data parallelism."""
    from ltx_amd.training import FusedProdigy
    pa, pb = _params(5, scale=SMALL), _params(5, scale=SMALL)
    a, b = FusedProdigy(pa, max_grad_norm=1.0), FusedProdigy(pb, max_grad_norm=1.0)
    seen = []
    for k in range(5):
        grads = _drift_grads(50, k)
        _step(a, pa, grads)
        _step(b, pb, grads)
        assert _bits(a.record.tolist()) == _bits(b.record.tolist()), k
        for x, y in zip(pa, pb):
            assert torch.equal(x, y)
            for key in STATES:
                assert torch.equal(a.state[x][key], b.state[y][key]), (k, key)
        seen.append(float(a.d))
    assert seen[-1] > seen[0] >= 1e-6 and a.record[6].item() == 5.0
    # and the same gradients again on the same state of a third optimizer: pass 1 twice, same partials
    pc = _params(5, scale=SMALL)
    c = FusedProdigy(pc, max_grad_norm=1.0)
    for k in range(5):
        _step(c, pc, _drift_grads(50, k))
    assert _bits(c.record.tolist()) == _bits(a.record.tolist())


# ---------------------------------------------------------------------------------------------
# the elementwise arithmetic
# ---------------------------------------------------------------------------------------------
def _compare(opt, ps, ref, qs, where):
    for i, (p, q) in enumerate(zip(ps, qs)):
        if p not in opt.state and q not in ref.state:
            continue
        for key in STATES:
            a, b = opt.state[p][key], ref.state[q][key]
            assert a.dtype == p.dtype and torch.equal(a, b), (where, i, key, DTYPES[i], int((a != b).sum()))
        assert torch.equal(p, q), (where, i, "param", DTYPES[i], int((p != q).sum()))


CONFIGS = {"decouple": dict(weight_decay=0.01, decouple=True),
           "coupled_weight_decay": dict(weight_decay=0.01, decouple=False),
           "safeguard_warmup": dict(safeguard_warmup=True),
           "use_bias_correction": dict(use_bias_correction=True)}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_states_and_parameters_are_the_statements_bitwise(config):
    """After each of 6 steps with fresh seeded gradients the device record's d and dlr are fed to the
    statement, whose exp_avg, exp_avg_sq, s and parameters then must be the kernels' bit for bit, f32 and
    bf16. Every torch op of the statement is one correctly rounded IEEE operation on this device (add_
    with alpha, addcmul_ and addcdiv_ are one fused multiply-add on an f32 product or quotient), so no state
    needs a tolerance."""
    from ltx_amd.training import FusedProdigy
    kw = CONFIGS[config]
    ps, qs = _params(7, scale=SMALL), _params(7, scale=SMALL)
    start = [p.detach().clone() for p in ps]
    opt = FusedProdigy(ps, **kw)
    ref = ProdigyStatement(qs, **kw)
    ds = []
    for k in range(6):
        grads = _drift_grads(100, k, scale=0.1 * (k + 1))
        _step(opt, ps, grads)
        rec = _record(opt)
        assert rec["applied"] == 1.0 and rec["k"] == k + 1
        ref.step(grads, override=(rec["d"], rec["dlr"]))
        _compare(opt, ps, ref, qs, (config, k))
        ds.append(rec["d"])
    print(config, "d per step:", ds)
    assert ds[-1] > ds[0] and all(b >= a for a, b in zip(ds, ds[1:]))
    for i, p in enumerate(ps):
        assert torch.equal(opt.state[p]["p0"], start[i]) and opt.state[p]["step"] == 6
        assert not torch.equal(p, start[i]), (i, DTYPES[i])  # every tensor moved, the bf16 ones too


def _offset_views(tensors):
    """Copies of `tensors` that start one element into a buffer of their own: 4 (f32) or 2 (bf16) bytes past
    a 16-byte boundary, as a gradient that is a view into a reducer's bucket can be."""
    out = []
    for t in tensors:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        out.append(buf[1:].view(t.shape).copy_(t.detach()))
    return out


def test_tensors_off_the_16_byte_boundary_take_the_one_element_path_with_the_same_arithmetic():
    """Rows whose parameter or gradient is not 16-byte aligned are walked one element per lane in both
    passes (pass 2's with the EMA column too): the states, parameters and shadows are still the
    statement's, bitwise."""
    from ltx_amd.training import EMASchedule, FusedProdigy
    sched = EMASchedule(0.999)
    ps = [torch.nn.Parameter(v) for v in _offset_views(_params(12, scale=SMALL))]
    qs = _params(12, scale=SMALL)
    assert all(p.data_ptr() % 16 in (2, 4) for p in ps) and all(torch.equal(p, q) for p, q in zip(ps, qs))
    opt = FusedProdigy(ps, ema=sched)
    ref = ProdigyStatement(qs)
    for k in range(3):
        grads = _drift_grads(120, k)
        prev = [opt.state[p]["ema"].clone() if k else p.detach().float().clone() for p in ps]
        for p, g in zip(ps, _offset_views(grads)):
            p.grad = g
        assert all(p.grad.data_ptr() % 16 in (2, 4) for p in ps)
        opt.step()
        rec = _record(opt)
        ref.step(grads, override=(rec["d"], rec["dlr"]))
        _compare(opt, ps, ref, qs, ("offset", k))
        omd = torch.tensor(1.0 - sched.decay_at(k + 1), dtype=torch.float32, device=DEV)
        for i, p in enumerate(ps):
            want = prev[i].clone()
            want.sub_((want - p.detach().float()) * omd)
            assert torch.equal(opt.state[p]["ema"], want), (k, i)
    assert rec["d"] > 1e-6 and rec["k"] == 3.0


# ---------------------------------------------------------------------------------------------
# composition
# ---------------------------------------------------------------------------------------------
def test_with_clipping_pass_1_sees_the_scaled_gradient_and_grad_is_unchanged():
    from ltx_amd.training import FusedAdamW, FusedProdigy
    ps, qs, ts = _params(8, scale=SMALL), _params(8, scale=SMALL), _params(8, scale=SMALL)
    opt = FusedProdigy(ps, max_grad_norm=0.5)
    twin = FusedAdamW(ts, lr=1e-3, max_grad_norm=0.5)  # the clip record is FusedAdamW's
    ref = ProdigyStatement(qs)
    for k in range(3):
        grads = _drift_grads(200, k)
        _step(opt, ps, grads)
        _step(twin, ts, grads)
        assert float(opt.clip_coef) < 1.0
        assert _bits([opt.clip_sumsq.item(), opt.grad_norm.item(), opt.clip_coef.item()]) == \
            _bits([twin.clip_sumsq.item(), twin.grad_norm.item(), twin.clip_coef.item()])
        for p, g in zip(ps, grads):
            assert torch.equal(p.grad, g)
        rec = _record(opt)
        ref.step(grads, coef=opt.clip_coef, override=(rec["d"], rec["dlr"]))
        _compare(opt, ps, ref, qs, ("clip", k))
    unclipped = FusedProdigy(_params(8))
    _step(unclipped, unclipped.param_groups[0]["params"], _rand_grads(200))
    assert unclipped.grad_norm is None and unclipped.clip_coef is None


@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_with_the_ema_shadows_follow_the_unfused_arithmetic_and_the_rest_is_the_twins(max_norm):
    from ltx_amd.training import EMASchedule, FusedProdigy
    sched = EMASchedule(0.999)
    pe, pt = _params(3, scale=SMALL), _params(3, scale=SMALL)
    ema = FusedProdigy(pe, max_grad_norm=max_norm, ema=sched)
    twin = FusedProdigy(pt, max_grad_norm=max_norm)
    for k in range(4):
        n = k + 1
        grads = _drift_grads(40, k)
        prev = [ema.state[p]["ema"].clone() if k else p.detach().float().clone() for p in pe]
        _step(ema, pe, grads)
        _step(twin, pt, grads)
        assert ema.ema_steps == n and ema.ema_decay == sched.decay_at(n)
        assert _bits(ema.record.tolist()) == _bits(twin.record.tolist())
        omd = torch.tensor(1.0 - sched.decay_at(n), dtype=torch.float32, device=DEV)
        for i, (a, b) in enumerate(zip(pe, pt)):
            assert torch.equal(a, b), (k, i)
            for key in STATES:
                assert torch.equal(ema.state[a][key], twin.state[b][key]), (k, i, key)
            assert "ema" not in twin.state[b]
            shadow = ema.state[a]["ema"]
            assert shadow.dtype == torch.float32 and shadow.is_cuda
            want = prev[i].clone()
            want.sub_((want - a.detach().float()) * omd)
            assert torch.equal(shadow, want), (k, i, DTYPES[i])
    # the swap machinery is FusedAdamW's
    live = [p.detach().clone() for p in pe]
    with ema.ema_weights():
        for p, dt in zip(pe, DTYPES):
            assert torch.equal(p, ema.state[p]["ema"].to(dt))
        with pytest.raises(RuntimeError, match="swapped in"):
            ema.step()
    for p, was in zip(pe, live):
        assert torch.equal(p, was)


def test_parameters_without_a_gradient_keep_everything():
    from ltx_amd.training import FusedProdigy
    ps, qs = _params(4), _params(4)
    opt, ref = FusedProdigy(ps), ProdigyStatement(qs)
    for k in range(2):
        grads = _rand_grads(60 + k)
        _step(opt, ps, grads)
        rec = _record(opt)
        ref.step(grads, override=(rec["d"], rec["dlr"]))
    mask = (True, False, False, True, True, False)
    keep = [{key: opt.state[p][key].clone() for key in STATES} for p in ps]
    before = [p.detach().clone() for p in ps]
    grads = [g if m else None for g, m in zip(_rand_grads(62), mask)]
    _step(opt, ps, grads)
    rec = _record(opt)
    ref.step(grads, override=(rec["d"], rec["dlr"]))
    assert rec["k"] == 3.0
    for i, (p, m) in enumerate(zip(ps, mask)):
        assert opt.state[p]["step"] == (3 if m else 2)
        assert torch.equal(p, before[i]) != m
        for key in ("exp_avg", "exp_avg_sq", "s"):
            assert torch.equal(opt.state[p][key], keep[i][key]) != m, (i, key)
        assert torch.equal(opt.state[p]["p0"], keep[i]["p0"])
    _compare(opt, ps, ref, qs, "masked")
    # a parameter that first gets a gradient later takes its p0 then, before anything moves
    late = _params(4)
    opt = FusedProdigy(late)
    _step(opt, late, [g if i != 2 else None for i, g in enumerate(_rand_grads(63))])
    assert late[2] not in opt.state or not opt.state[late[2]]
    with torch.no_grad():
        late[2].add_(1.0)
    was = late[2].detach().clone()
    _step(opt, late, _rand_grads(64))
    assert torch.equal(opt.state[late[2]]["p0"], was) and opt.state[late[2]]["step"] == 1


def test_zero_lr_and_zero_gradient_steps():
    """lr == 0 launches nothing and changes nothing; a first step on zero gradients has d_denom == 0: the
    record says applied = 0 and no parameter moves."""
    from ltx_amd import ops
    from ltx_amd.training import FusedProdigy
    ps = _params(6)
    start = [p.detach().clone() for p in ps]
    opt = FusedProdigy(ps, lr=0.0, max_grad_norm=1.0)
    names = []
    real = ops.call
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
        gen = ops.weight_generation()
        _step(opt, ps, _rand_grads(1))
        assert names == [] and ops.weight_generation() == gen and opt.grad_norm is None
    assert all(not opt.state[p] for p in ps) and opt.record is None
    opt.param_groups[0]["lr"] = 1.0
    _step(opt, ps, [torch.zeros_like(p) for p in ps])
    rec = _record(opt)
    assert rec == {"d": 1e-6, "d_max": 1e-6, "d_numerator": 0.0, "d_denom": 0.0, "d_hat": 0.0, "dlr": 1e-6, "k": 0.0,
                   "applied": 0.0}
    for p, was in zip(ps, start):
        assert torch.equal(p, was) and not opt.state[p]["s"].any() and not opt.state[p]["exp_avg"].any()
    _step(opt, ps, _rand_grads(2))
    assert _record(opt)["applied"] == 1.0 and not torch.equal(ps[4], start[4])


def test_launch_sequence(monkeypatch):
    """Per step: the clip's norm launches and its coefficient launch when clipping, pass 1 per bucket, the
    d update, pass 2 per bucket -- a bucket of one tensor included -- and nothing else."""
    from ltx_amd import ops
    from ltx_amd.training import EMASchedule, FusedProdigy
    names = []
    real = ops.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(ops, "call", call)
    grads = [g if i not in (3, 5) else None for i, g in enumerate(_rand_grads(31))]  # bf16 is left with one tensor
    core = ["ltx_prodigy_moments_multi"] * 2 + ["ltx_prodigy_d_update"] + ["ltx_prodigy_apply_multi"] * 2
    clip = ["ltx_grad_sumsq_multi"] * 2 + ["ltx_grad_clip_coef"]
    for kw, want in (({}, core), ({"max_grad_norm": 1.0}, clip + core), ({"ema": EMASchedule(0.999)}, core),
                     ({"max_grad_norm": 1.0, "ema": EMASchedule(0.999)}, clip + core)):
        ps = _params(9)
        opt = FusedProdigy(ps, **kw)
        for _ in range(2):
            del names[:]
            gen = ops.weight_generation()
            _step(opt, ps, grads)
            assert names == want, kw
            assert ops.weight_generation() == gen + 1
    ps = _params(9)
    del names[:]
    _step(FusedProdigy(ps), ps, [g if i % 2 == 0 else None for i, g in enumerate(grads)])  # f32 only
    assert names == ["ltx_prodigy_moments_multi", "ltx_prodigy_d_update", "ltx_prodigy_apply_multi"]
    two = FusedProdigy(_params(9))
    two.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3, device=DEV))]})
    with pytest.raises(ValueError, match="one parameter group"):
        two.step()


def test_a_step_does_not_sync_with_the_host():
    from ltx_amd.training import EMASchedule, FusedProdigy
    ps = _params(11)
    opt = FusedProdigy(ps, max_grad_norm=1.0, ema=EMASchedule(0.999))
    grads = [_rand_grads(70 + k) for k in range(3)]
    for k in range(2):  # tables, partials and record warm
        _step(opt, ps, grads[k])
    for p, g in zip(ps, grads[2]):
        p.grad.copy_(g)  # the same buffers: the cached tables stay valid, as in a training loop
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
        d = opt.d  # a device tensor: no sync yet
        with pytest.raises(RuntimeError):
            float(d)  # reading it is the sync
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(opt.d) > 0 and _record(opt)["k"] == 3.0


# ---------------------------------------------------------------------------------------------
# the tiny model through train_loop
# ---------------------------------------------------------------------------------------------
PRODIGY = {"optimizer": "prodigy", "lr_scheduler": "cosine", "max_grad_norm": 1.0}


def _run(tiny, case, out, epochs, extra=None, lr=1.0, val=False, save=False, resume=None, record=None, on_log=None):
    """train_loop on fresh model / loader objects under torch.manual_seed(SEED) with the config attributes of
    CASES[case] and `extra`: (model, the optimizer train_loop built, logs)."""
    from ltx_amd import io, ops, training
    attrs, accum = CASES[case]
    made = []

    def recording(cls):
        class Recording(cls):  # train_loop keeps its optimizer to itself
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                made.append(self)
        return Recording
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(training, "FusedAdamW", recording(training.FusedAdamW))
        mp.setattr(training, "FusedProdigy", recording(training.FusedProdigy))
        if record is not None:
            real = ops.call
            mp.setattr(ops, "call", lambda name, *a: (record.append(name), real(name, *a))[1])
        model = _build(tiny, attrs)
        loader = io.LatentLoader(tiny["ds"]["train"], 2, DEV, shuffle=True, seed=1)
        vloader = io.LatentLoader(tiny["ds"]["val"], 2, DEV, shuffle=False) if val else None
        tc = _config(dict(attrs, **(extra or {})), learning_rate=lr, num_epochs=epochs,
                     gradient_accumulation_steps=accum, output_dir=str(out), save_every_n_epochs=1)
        if save:
            tc.save_adapters = True
        logs = []

        def log(payload, step):
            logs.append((step, payload))
            if on_log is not None:
                on_log(made[0], payload, step)
        torch.manual_seed(SEED)
        training.train_loop(model, tc, loader, tiny["prompt"], tiny["mask"], log_fn=log, val_dataloader=vloader,
                            resume_from=resume)
    return model, made[0], logs


def _same_file(a, b):
    """Byte for byte -- except that a safetensors file with string metadata lists those keys in no fixed
    order (two writes of the same content differ there), so such a file is compared as its metadata and its
    tensors, bitwise."""
    from safetensors import safe_open
    if a.read_bytes() == b.read_bytes():
        return
    assert str(a).endswith(".safetensors"), a
    with safe_open(str(a), "pt") as fa, safe_open(str(b), "pt") as fb:
        assert fa.metadata() and fa.metadata() == fb.metadata(), a
    _same(load_file(str(a)), load_file(str(b)))


def _all_state(model, opt):
    names = {id(p): n for n, p in model.named_parameters()}
    out = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    for p, st in opt.state.items():
        for key, v in st.items():
            if torch.is_tensor(v):
                out[f"{key}.{names[id(p)]}"] = v
    return out, {names[id(p)]: st["step"] for p, st in opt.state.items()}


def test_train_loop_with_prodigy_logs_d_and_d_grows(tiny, tmp_path):
    """optimizer: prodigy, learning_rate 1.0 (given as null), cosine schedule, clipping on, everything else
    at its default: the first 8 steps of a 50-step schedule. The bf16 caption projection (weights near
    0.03, spacing 2^-13) cannot take the first steps of a few d0 = 1e-6, so d sits at d0 while the f32
    adapters' share of the numerator accumulates, and leaves it at the fifth step."""
    from ltx_amd.training import FusedProdigy, LRSchedule
    seen = []

    def on_log(opt, payload, step):
        if "train/prodigy_d" in payload:
            seen.append((step, payload["train/prodigy_d"], opt.record[0].item(), payload["train/lr"], opt.record[5].item()))
    model, opt, logs = _run(tiny, "attn2", tmp_path / "out", 4, dict(PRODIGY, lr_total_steps=50), lr=None, on_log=on_log)
    assert isinstance(opt, FusedProdigy)
    steps = [p for _, p in logs if "train/loss" in p]
    assert len(steps) == 8 == len(seen) and all("train/prodigy_d" in p and "train/grad_norm" in p for p in steps)
    assert all(math.isfinite(p["train/loss"]) and math.isfinite(p["train/grad_norm"]) for p in steps)
    sched = LRSchedule("cosine", 1.0, 0, 50)  # learning_rate null: Prodigy's 1.0 times the cosine factor
    for n, (step, logged, device, lr, dlr) in enumerate(seen):
        assert step == n + 1 and logged == device and isinstance(logged, float)
        assert lr == sched.at(n)
    ds = [s[1] for s in seen]
    print("d per step:", ds)
    assert all(b >= a for a, b in zip(ds, ds[1:])) and ds[0] >= 1e-6 and ds[-1] > 1e-6
    assert _record(opt)["k"] == 8.0 and _record(opt)["applied"] == 1.0
    for p, st in opt.state.items():
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "p0", "s", "step"] and st["s"].dtype == p.dtype


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
def test_resumed_run_is_bitwise_the_uninterrupted_run(tiny, tmp_path, ema):
    # d0 = 1e-4: d moves at every step of these four, so the record the resumed run starts from matters
    extra = dict(PRODIGY, prodigy_d0=1e-4, **({"ema_decay": 0.999} if ema else {}))
    model_a, opt_a, logs_a = _run(tiny, "attn2", tmp_path / "a", 2, extra)
    out_b = tmp_path / "b"
    _, opt_1, logs_1 = _run(tiny, "attn2", out_b, 1, dict(extra, lr_total_steps=4), save=True)
    ckpt = out_b / "adapter_epoch_1"
    assert sorted(os.listdir(ckpt)) == sorted(FOUR + (["ema_model.safetensors"] if ema else []))
    with open(ckpt / "train_state.json") as f:
        block = json.load(f)["prodigy"]
    assert block["hyper"] == opt_1.hyper() and block["record"] == {k: v.hex() for k, v in _record(opt_1).items()}
    saved = load_file(str(ckpt / "optimizer.safetensors"))
    assert sum(k.startswith("s.") for k in saved) == sum(k.startswith("p0.") for k in saved) == len(opt_1.state) > 0
    model_b, opt_b, logs_b = _run(tiny, "attn2", out_b, 2, extra, resume="auto")
    (sa, na), (sb, nb) = _all_state(model_a, opt_a), _all_state(model_b, opt_b)
    _same(sa, sb)
    assert na == nb and set(na.values()) == {4}
    assert any(k.startswith("s.") for k in sa) and any(k.startswith("p0.") for k in sa)
    assert any(k.startswith("ema.") for k in sa) == ema
    assert _bits(opt_a.record.tolist()) == _bits(opt_b.record.tolist()) and _record(opt_b)["k"] == 4.0
    assert (opt_a.ema_steps, opt_a.ema_decay) == (opt_b.ema_steps, opt_b.ema_decay)
    assert len(logs_b) > 0 and logs_a[-len(logs_b):] == logs_b and logs_a[:len(logs_1)] == logs_1
    assert [s for s, p in logs_b if "train/prodigy_d" in p] == [3, 4]
    # the record moved during the second epoch
    assert _record(opt_b)["d"] > _record(opt_1)["d"] > 1e-4


def test_resume_refuses_the_other_kind_and_other_hyper_parameters(tiny, tmp_path):
    out = tmp_path / "p"
    _run(tiny, "attn2", out, 1, dict(PRODIGY, lr_total_steps=4), save=True)
    with pytest.raises(ValueError, match="Prodigy"):
        _run(tiny, "attn2", out, 2, lr=1e-3, resume="auto")
    with pytest.raises(ValueError, match="d_coef"):
        _run(tiny, "attn2", out, 2, dict(PRODIGY, prodigy_d_coef=2.0), resume="auto")
    out = tmp_path / "a"
    _run(tiny, "attn2", out, 1, lr=1e-3, save=True)
    with pytest.raises(ValueError, match="AdamW"):
        _run(tiny, "attn2", out, 2, PRODIGY, resume="auto")


def test_without_the_keys_the_run_is_todays(tiny, tmp_path):
    """`optimizer` absent, and `optimizer: adamw` with no other new key: the same entry points in the same
    order, none of them Prodigy's, and the same files byte for byte."""
    from ltx_amd.training import FusedAdamW
    runs = {}
    for name, extra in (("absent", {}), ("adamw", {"optimizer": "adamw"})):
        calls = []
        _, opt, logs = _run(tiny, "attn2", tmp_path / name, 1, extra, lr=1e-3, save=True, record=calls)
        assert isinstance(opt, FusedAdamW) and not hasattr(opt, "record")
        assert "ltx_adamw_multi" in calls and not ENTRY_POINTS & set(calls)
        assert not any("train/prodigy_d" in p for _, p in logs)
        g = opt.param_groups[0]
        assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 1e-2)
        assert all(sorted(st) == ["exp_avg", "exp_avg_sq", "step"] for st in opt.state.values())
        runs[name] = (calls, logs)
    assert runs["absent"] == runs["adamw"]
    a, b = tmp_path / "absent", tmp_path / "adamw"
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["adapter_epoch_1", "best_model_epoch_1.safetensors"]
    assert sorted(os.listdir(a / "adapter_epoch_1")) == FOUR
    for rel in ["best_model_epoch_1.safetensors"] + [os.path.join("adapter_epoch_1", f) for f in FOUR]:
        _same_file(a / rel, b / rel)
    with open(a / "adapter_epoch_1" / "train_state.json") as f:
        st = json.load(f)
    assert "prodigy" not in st and sorted(st["optimizer"]["param_groups"][0]) == ["betas", "eps", "lr", "weight_decay"]
    keys = [k for k in load_file(str(a / "adapter_epoch_1" / "optimizer.safetensors")) if not k.startswith("rng.")]
    assert keys and all(k.startswith(("exp_avg.", "exp_avg_sq.")) for k in keys)
    # ... and with the key the step is Prodigy's
    calls = []
    _run(tiny, "attn2", tmp_path / "on", 1, dict(PRODIGY, lr_total_steps=2), record=calls)
    assert calls.count("ltx_prodigy_d_update") == 2 and calls.count("ltx_prodigy_apply_multi") == 4
    assert "ltx_adamw_multi" not in calls and "ltx_adamw_multi_clip" not in calls
