"""GPU: global-norm gradient clipping and the warmup / decay schedule inside the fused Adam step (optim.AvAdam, av_adam_multi_ex)
against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam + LambdaLR on the same device, and float64 on the host for the norm."""
import copy
import math

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

# (70001,): two chunks and a tail that is no multiple of 4; (5,): tail only; (128, 1024): exactly two aligned chunks.  The fifth parameter's
# GRADIENT is a view one element into a larger buffer: not 16-byte aligned, so every kernel takes its scalar path (arena gradients can be so)
SHAPES = [(1000, 33), (70001,), (5,), (128, 1024), (4097,)]
LRS = (1e-4, 2e-5)
ULP = 2.0 ** -23


def _data(steps=3, seed=12):
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(*s, generator=g) for s in SHAPES]
    grads = [[torch.randn(*s, generator=g) for s in SHAPES] for _ in range(steps)]
    return p0, grads


def _params(p0):
    return [p.clone().cuda().requires_grad_(True) for p in p0]


def _groups(ps):
    return [{"params": ps[:2], "lr": LRS[0]}, {"params": ps[2:], "lr": LRS[1]}]


def _set_grads(ps, gs, drop=False, factor=1.0, view=True):
    """Gradients of one step; drop: parameter 2 gets none (a parameter without a gradient is skipped).  view: the last gradient is a
    (4097,) slice of a (4098,) buffer (for the fused optimizer; torch's gets a plain tensor)."""
    for i, (p, g) in enumerate(zip(ps, gs)):
        g = g.cuda() * factor
        if view and i == len(ps) - 1:
            buf = torch.zeros(g.numel() + 1, device="cuda")
            buf[1:] = g
            g = buf[1:]
            assert g.data_ptr() % 16 != 0
        p.grad = g
    if drop:
        ps[2].grad = None


def _norm64(gs, drop=False, factor=1.0):
    """sqrt(sum g.double()^2) on the host."""
    return math.sqrt(sum(float((g.double() * factor).pow(2).sum()) for i, g in enumerate(gs) if not (drop and i == 2)))


def _close_ulp(got, want):
    return abs(got - want) <= ULP * abs(want)


def test_norm_is_within_one_ulp_of_float64_and_reproducible():
    """Double accumulation: the reported norm is float32(sqrt(sum of exact squares)) up to the rounding of the double sum, far below
    one float32 ulp - derived, not measured.  Squares of 1e20 overflow fp32 but not the accumulator.  No atomics: same bits on every run."""
    optim = pkg("optim")
    p0, grads = _data()
    runs = []
    for _ in range(2):
        ps = _params(p0)
        opt = optim.AvAdam(_groups(ps), max_grad_norm=1.0)
        norms = []
        for step, gs in enumerate(grads):
            _set_grads(ps, gs, drop=step == 1)
            opt.step()
            norms.append(opt.last_grad_norm.clone())
            got, want = float(norms[-1]), _norm64(gs, drop=step == 1)
            print(f"step {step}: norm {got!r} float64 {want!r} rel {abs(got - want) / want:.3e}")
            assert _close_ulp(got, want), (step, got, want)
        assert opt.last_grad_norm.device.type == "cuda" and opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.dtype == torch.float32
        runs.append((norms, [p.detach().clone() for p in ps]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    big = [g.clone() for g in grads[0]]
    big[0].fill_(1e20)
    ps = _params(p0)
    opt = optim.AvAdam(_groups(ps), max_grad_norm=1.0)
    _set_grads(ps, big)
    opt.step()
    got, want = float(opt.last_grad_norm), _norm64(big)
    assert math.isfinite(got) and _close_ulp(got, want), (got, want)


def _shadows(ps, cache):
    return [cache.get(i, [ps[i]], torch.bfloat16, lambda i=i: ps[i].data.to(torch.bfloat16), flat=True) for i in (0, 1, 4)]


def test_below_the_threshold_nothing_changes():
    optim, shadow = pkg("optim"), pkg("utils.shadow")
    p0, grads = _data()
    top = max(_norm64(gs, drop=step == 1) for step, gs in enumerate(grads))
    pa, pb = _params(p0), _params(p0)
    ca, cb = shadow.ParamCache(), shadow.ParamCache()
    sa, sb = _shadows(pa, ca), _shadows(pb, cb)
    oa = optim.AvAdam(_groups(pa), max_grad_norm=10.0 * top)
    ob = optim.AvAdam(_groups(pb))
    for step, gs in enumerate(grads):
        _set_grads(pa, gs, drop=step == 1); _set_grads(pb, gs, drop=step == 1)
        oa.step(); ob.step()
        assert float(oa.last_clip_coef) == 1.0
        for a, b in zip(pa, pb):
            assert torch.equal(a.detach(), b.detach())
            assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
        for i, a, b in zip((0, 1, 4), sa, sb):
            assert torch.equal(a, b) and torch.equal(a, pa[i].data.to(torch.bfloat16).reshape(a.shape))
    assert ob.last_grad_norm is None and oa.fused_launches == ob.fused_launches == 3


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_above_the_threshold_is_torch_clip_grad_norm(grad_scale):
    optim = pkg("optim")
    p0, grads = _data()
    max_norm = 0.1 * grad_scale * min(_norm64(gs, drop=step == 1) for step, gs in enumerate(grads))
    pr, pa = _params(p0), _params(p0)
    o_ref = torch.optim.Adam(_groups(pr))
    o_av = optim.AvAdam(_groups(pa), max_grad_norm=max_norm)
    o_av.grad_scale = grad_scale
    for step, gs in enumerate(grads):
        _set_grads(pr, gs, drop=step == 1, factor=grad_scale, view=False)        # torch sees grad * grad_scale
        _set_grads(pa, gs, drop=step == 1)
        total = torch.nn.utils.clip_grad_norm_(pr, max_norm)
        o_ref.step(); o_av.step()
        coef_ref = min(1.0, float(torch.tensor(max_norm, dtype=torch.float32, device="cuda") / (total + 1e-6)))
        assert coef_ref < 0.11
        assert _close_ulp(float(o_av.last_grad_norm), _norm64(gs, drop=step == 1, factor=grad_scale))
        torch.testing.assert_close(float(o_av.last_clip_coef), coef_ref, rtol=1e-6, atol=0)
        for r, a in zip(pr, pa):
            torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7)


def _hf_lambda(warmup, total):
    def f(step):
        if step < warmup:
            return float(step) / float(max(1, warmup))
        if total == 0:
            return 1.0
        return max(0.0, float(total - step) / float(max(1, total - warmup)))
    return f


def test_under_the_grad_scaler_overflowing_steps_are_skipped_and_do_not_advance_the_schedule():
    """The protocol of test_grad_scaler_matches_torch_amp_on_injected_infs (tests/test_modules_gpu.py) with clipping and a schedule on: the
    norm pass is also the non-finite check."""
    optim = pkg("optim")
    p0, grads = _data(steps=9, seed=3)
    max_norm, warmup, total = 50.0, 3, 20                                      # norms are about sqrt(238175) = 488: always clipped
    pr, pa = _params(p0), _params(p0)
    o_ref = torch.optim.Adam(_groups(pr))
    sched = torch.optim.lr_scheduler.LambdaLR(o_ref, _hf_lambda(warmup, total))
    o_av = optim.AvAdam(_groups(pa), max_grad_norm=max_norm, warmup_steps=warmup, total_steps=total)
    s_ref = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    s_av = optim.AvGradScaler(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    scales = []
    for it, gs in enumerate(grads):
        sc_ref = float(s_ref.scale(torch.ones((), device="cuda")))
        sc_av = s_av.get_scale()
        assert sc_ref == sc_av, (it, sc_ref, sc_av)
        scales.append(sc_av)
        _set_grads(pr, gs, factor=sc_ref, view=False); _set_grads(pa, gs, factor=sc_av)
        if it in (2, 7):
            pr[1].grad[17] = float("inf"); pa[1].grad[17] = float("inf")
        if it == 3:
            pr[4].grad[0] = float("nan"); pa[4].grad[0] = float("nan")
        before = [p.detach().clone() for p in pa]
        s_ref.unscale_(o_ref)
        torch.nn.utils.clip_grad_norm_(pr, max_norm)
        s_ref.step(o_ref); s_ref.update()
        s_av.step(o_av); s_av.update()
        if it in (2, 3, 7):
            assert all(torch.equal(a.detach(), b) for a, b in zip(pa, before))   # skipped
        else:
            sched.step()                                                         # HF's Trainer: the schedule does not move on a skipped step
            assert _close_ulp(float(o_av.last_grad_norm), _norm64(gs)), it       # the un-scaled norm (the scale is a power of two: exact)
        for r, a in zip(pr, pa):
            torch.testing.assert_close(a.detach(), r.detach(), rtol=2e-6, atol=2e-7)
    assert scales == [1024.0, 1024.0, 1024.0, 512.0, 256.0, 256.0, 256.0, 512.0, 256.0]
    assert s_av.steps_taken() == 6
    assert o_av.schedule_step() == 6
    o_av.sync_steps(s_av)
    assert all(st["step"] == 6 for st in o_av.state.values())
    assert o_av.state_dict()[o_av.SCHEDULE_KEY] == 6


def test_without_a_scaler_non_finite_gradients_follow_torch():
    """One inf element: the norm is inf, the coefficient 0, inf * 0 = NaN in that element and 0 elsewhere - no exception, no skip."""
    optim = pkg("optim")
    p0, grads = _data(steps=2)
    pr, pa = _params(p0), _params(p0)
    o_ref = torch.optim.Adam(_groups(pr))
    o_av = optim.AvAdam(_groups(pa), max_grad_norm=1.0)
    for step, gs in enumerate(grads):
        _set_grads(pr, gs, view=False); _set_grads(pa, gs)
        if step == 1:
            pr[1].grad[65537] = float("inf"); pa[1].grad[65537] = float("inf")
        torch.nn.utils.clip_grad_norm_(pr, 1.0)
        o_ref.step(); o_av.step()
    assert math.isinf(float(o_av.last_grad_norm)) and float(o_av.last_clip_coef) == 0.0
    assert o_av.state[pa[0]]["step"] == 2
    for i, (r, a) in enumerate(zip(pr, pa)):
        assert torch.equal(torch.isnan(a.detach()), torch.isnan(r.detach()))
        assert int(torch.isnan(a.detach()).sum()) == (1 if i == 1 else 0)
        torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7, equal_nan=True)


def test_schedule_matches_lambdalr_without_plan_churn():
    optim = pkg("optim")
    warmup, total = 3, 7
    p0, grads = _data(steps=9, seed=21)
    pr, pa = _params(p0), _params(p0)
    o_ref = torch.optim.Adam(_groups(pr))
    sched = torch.optim.lr_scheduler.LambdaLR(o_ref, _hf_lambda(warmup, total))
    o_av = optim.AvAdam(_groups(pa), warmup_steps=warmup, total_steps=total)
    for k, gs in enumerate(grads):
        _set_grads(pr, gs, view=False); _set_grads(pa, gs)
        o_ref.step(); sched.step(); o_av.step()
        assert float(o_av.last_lr_mult) == float(np.float32(optim.lr_multiplier(k, warmup, total))), k
        assert float(o_av.last_clip_coef) == 1.0
        if k == 0:                                                              # multiplier 0: moments and step counts advance, parameters stay
            assert all(torch.equal(a.detach().cpu(), p) for a, p in zip(pa, p0))
            assert all(float(o_av.state[a]["exp_avg"].abs().max()) > 0 and o_av.state[a]["step"] == 1 for a in pa)
        for r, a in zip(pr, pa):
            torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7)
    assert o_av.schedule_step() == 9
    assert len(o_av._plans) == 1
    assert [g["lr"] for g in o_av.param_groups] == list(LRS)                    # the base rates stay in the groups


def test_resume_from_state_dict_continues_the_schedule():
    optim = pkg("optim")
    kw = dict(max_grad_norm=40.0, warmup_steps=3, total_steps=7)
    p0, grads = _data(steps=5, seed=8)
    pa = _params(p0)
    oa = optim.AvAdam(_groups(pa), **kw)
    for step, gs in enumerate(grads):
        _set_grads(pa, gs, drop=step == 1)
        oa.step()
    pb = _params(p0)
    ob = optim.AvAdam(_groups(pb), **kw)
    for step, gs in enumerate(grads[:4]):
        _set_grads(pb, gs, drop=step == 1)
        ob.step()
    sd = copy.deepcopy(ob.state_dict())
    assert sd[ob.SCHEDULE_KEY] == 4
    pc = [p.detach().clone().requires_grad_(True) for p in pb]
    oc = optim.AvAdam(_groups(pc), **kw)
    oc.load_state_dict(sd)
    assert oc.schedule_step() == 4
    _set_grads(pc, grads[4])
    oc.step()
    assert oc.schedule_step() == 5 and oc.state[pc[2]]["step"] == 4 and oc.state[pc[0]]["step"] == 5
    for a, c in zip(pa, pc):
        assert torch.equal(a.detach(), c.detach())
    torch.optim.Adam(_groups(_params(p0))).load_state_dict(sd)                  # torch's Adam ignores the extra key
    oc.reset_state()
    assert oc.schedule_step() == 0


def _with(t0, **kw):
    tr = pkg("model.trainer")
    t = tr.MultimodalTrainer(t0.visual_encoder, t0.audio_encoder, t0.fusion_module, t0.decoder1, t0.tokenizer, learning_rate=1e-4,
                             device="cuda", lambda_=0.1, **kw)
    t.fixed_projection = t0.fixed_projection
    return t


def test_trainer_clips_inside_the_fused_step():
    from test_step_gpu import build
    init = pkg("utils.init"); synth = pkg("dataset.synthetic")
    cfg = init.W2V2_TINY
    batch = synth.make_batch(2, 1.0, seed=5, ragged=True)

    def all_params(t):
        return [p for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1) for p in m.parameters()]

    plain = build(cfg, "fp32")
    loose = _with(build(cfg, "fp32"), max_grad_norm=1e9)
    o_plain, o_loose = plain.train_step(batch), loose.train_step(batch)
    assert "grad_norm" not in o_plain
    norm = float(o_loose["grad_norm"])
    assert math.isfinite(norm) and norm > 0 and float(loose.optimizer.last_clip_coef) == 1.0
    for a, b in zip(all_params(plain), all_params(loose)):
        assert torch.equal(a.detach(), b.detach())
    assert plain.optimizer.fused_launches == loose.optimizer.fused_launches == 1

    tight = _with(build(cfg, "fp32"), max_grad_norm=norm / 10)
    ref = build(cfg, "fp32")
    o_tight = tight.train_step(batch)
    # the same step on ``ref`` with torch's clipping between backward and the optimizer (train_step without a reducer or scaler)
    ref.optimizer.zero_grad(set_to_none=True)
    ref._head_arena.begin_step()
    begin = getattr(ref.audio_encoder.model, "begin_grad_step", None)
    if begin is not None:
        begin()
    out = ref.forward_losses(batch)
    out["total"].backward()
    ref._head_arena.finalize()
    total = torch.nn.utils.clip_grad_norm_([p for p in ref.parameters if p.grad is not None], norm / 10)
    ref.optimizer.step()
    torch.testing.assert_close(o_tight["grad_norm"], total, rtol=1e-5, atol=0)      # torch's norm is an fp32 sum: a few 1e-7 of its own
    torch.testing.assert_close(float(tight.optimizer.last_clip_coef), 0.1, rtol=1e-4, atol=0)
    for a, b in zip(all_params(tight), all_params(ref)):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-6, atol=1e-7)
    assert tight.optimizer.fused_launches == ref.optimizer.fused_launches == 1
