"""GPU: decoupled weight decay and the cosine schedule inside the fused Adam step (optim.AvAdam(weight_decay=..., lr_schedule="cosine"),
av_adam_multi_wd) against torch.optim.AdamW + LambdaLR (+ GradScaler, clip_grad_norm_, the lerp law of the EMA) on the same device, against
a float32 restatement of the decay, and against runs with the feature off."""
import copy
import math

import pytest
import torch

from conftest import pkg
from test_optim_clip_gpu import SHAPES, ULP, _close_ulp, _data, _norm64, _params, _set_grads, _shadows

pytestmark = pytest.mark.gpu

# the shapes of test_optim_clip_gpu.py: (70001,) two chunks and a tail that is no multiple of 4, (5,) tail only, (128, 1024) exactly two aligned
# chunks, and the last GRADIENT a view one element into a larger buffer (the scalar path).  Against torch every optimizer has decay_1d=True, so
# the 1-D shapes are decayed as torch.optim.AdamW decays them.
LRS = (1e-3, 2e-4)
ONE_D = [i for i, s in enumerate(SHAPES) if len(s) <= 1]
TWO_D = [i for i, s in enumerate(SHAPES) if len(s) > 1]


@pytest.fixture(autouse=True)
def _bf16_library():
    """The 16-bit shadows below are bfloat16: the library of the bf16 / fp32 modes writes them."""
    prec = pkg("precision")
    was = prec.get_precision()
    prec.set_precision("bf16")
    yield
    prec.set_precision(was)


def _groups(ps, wds=None, lrs=LRS):
    gs = [{"params": ps[:2], "lr": lrs[0]}, {"params": ps[2:], "lr": lrs[1]}]
    if wds is not None:
        for g, wd in zip(gs, wds):
            g["weight_decay"] = wd
    return gs


def _moments_close(o_av, pa, o_ref, pr, rtol, atol):
    """The moments against torch's.  hyper carries beta2 as a float32, so 1 - beta2 is 0.99998713e-3 where torch has 1e-3 in double:
    exp_avg_sq sits 1.3e-5 (relative) beside torch's, as it always has; with grad_scale = 0.5 that stays below atol."""
    pairs = [(o_av.state[a], o_ref.state[r]) for r, a in zip(pr, pa) if r in o_ref.state and "exp_avg" in o_ref.state[r]]
    worst = max(float((sa["exp_avg_sq"] - sr["exp_avg_sq"]).abs().max()) for sa, sr in pairs)
    print(f"exp_avg_sq: worst |got - torch| {worst:.3e}")
    for sa, sr in pairs:
        torch.testing.assert_close(sa["exp_avg"], sr["exp_avg"], rtol=rtol, atol=atol)
        torch.testing.assert_close(sa["exp_avg_sq"], sr["exp_avg_sq"], rtol=rtol, atol=atol)


def _cosine_lambda(warmup, total):
    """HF get_cosine_schedule_with_warmup's lambda (num_cycles = 0.5) up to ``total``, and 0 after it."""
    def f(step):
        if step < warmup:
            return float(step) / float(max(1, warmup))
        if step >= total:
            return 0.0
        progress = float(step - warmup) / float(max(1, total - warmup))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))
    return f


def test_decay_alone_is_one_float32_product():
    """lr = 2^-10 and lambda = 0.5: f = 1 - 2^-11 is exact in float32.  Zero gradients leave the moments at 0 and the update at 0, so the new
    parameter is the rounded product p * f, bit for bit, on the quad path, the tail and the scalar path alike."""
    optim = pkg("optim")
    p0, _ = _data(steps=1)
    ps = _params(p0)
    opt = optim.AvAdam(_groups(ps, lrs=(2.0 ** -10, 2.0 ** -10)), weight_decay=0.5, decay_1d=True)
    f = torch.tensor(1.0 - 2.0 ** -11, dtype=torch.float32, device="cuda")
    assert float(f) == 1.0 - 2.0 ** -11
    want = [p.cuda() for p in p0]
    zeros = [torch.zeros(*s) for s in SHAPES]
    for step in range(2):
        _set_grads(ps, zeros, drop=True)                             # parameter 2 gets no gradient
        opt.step()
        want = [w if i == 2 else w * f for i, w in enumerate(want)]
        for i, (p, w) in enumerate(zip(ps, want)):
            assert torch.equal(p.detach(), w), (step, i)
            if i == 2:
                assert p not in opt.state or not opt.state[p]        # untouched: not even a state
                continue
            assert not torch.equal(p.detach(), p0[i].cuda())
            assert int(opt.state[p]["exp_avg"].count_nonzero()) == 0 and int(opt.state[p]["exp_avg_sq"].count_nonzero()) == 0
            assert opt.state[p]["step"] == step + 1
    assert torch.equal(ps[2].detach(), p0[2].cuda()) and opt.fused_launches == 2
    assert opt._steps_dev.tolist()[:5] == [2, 2, 0, 2, 2]            # the device's own step counts


@pytest.mark.parametrize("wds", [(0.1, 0.0), (0.0, 0.05)], ids=["first_group", "second_group"])
def test_matches_torch_adamw(wds):
    optim = pkg("optim")
    p0, grads = _data(steps=3)
    pr, pa = _params(p0), _params(p0)
    o_ref = torch.optim.AdamW(_groups(pr, wds))
    o_av = optim.AvAdam(_groups(pa, wds), decay_1d=True)
    o_av.grad_scale = 0.5
    for step, gs in enumerate(grads):
        _set_grads(pr, gs, drop=step == 1, factor=0.5, view=False)    # torch sees grad * grad_scale
        _set_grads(pa, gs, drop=step == 1)
        o_ref.step(); o_av.step()
        for r, a in zip(pr, pa):
            torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7)
        _moments_close(o_av, pa, o_ref, pr, 1e-6, 1e-7)
    assert o_av.fused_launches == 3 and o_av.last_lr_mult is None     # no schedule: no state block
    # the decay is there: the same run without it ends elsewhere
    pb = _params(p0)
    o_b = optim.AvAdam(_groups(pb))
    o_b.grad_scale = 0.5
    for step, gs in enumerate(grads):
        _set_grads(pb, gs, drop=step == 1)
        o_b.step()
    decayed = range(2) if wds[0] else range(2, 5)
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a.detach(), b.detach()) == (i not in decayed), i


def test_warmup_and_cosine_match_adamw_with_lambdalr():
    optim = pkg("optim")
    warmup, total, wds = 2, 6, (0.1, 0.02)
    p0, grads = _data(steps=total + 3, seed=21)
    pr, pa = _params(p0), _params(p0)
    o_ref = torch.optim.AdamW(_groups(pr, wds))
    sched = torch.optim.lr_scheduler.LambdaLR(o_ref, _cosine_lambda(warmup, total))
    o_av = optim.AvAdam(_groups(pa, wds), decay_1d=True, lr_schedule="cosine", warmup_steps=warmup, total_steps=total)
    for k, gs in enumerate(grads):                                    # k = 0 .. total + 2
        before = [a.detach().clone() for a in pa]
        _set_grads(pr, gs, view=False); _set_grads(pa, gs)
        o_ref.step(); sched.step(); o_av.step()
        got, host = float(o_av.last_lr_mult), optim.lr_multiplier(k, warmup, total, schedule="cosine")
        print(f"k {k}: device multiplier {got!r} host {host!r} diff {abs(got - host):.3e}")
        # the device's cos may differ from the host's in the last place of a double, and 1 + cos cancels near the end: 2^-50 absolute
        assert abs(got - host) <= ULP * abs(host) + 2.0 ** -50, (k, got, host)
        if k == 0 or k >= total:                                      # multiplier 0: nothing moves and nothing decays
            assert got == 0.0 and all(torch.equal(a.detach(), b) for a, b in zip(pa, before)), k
        else:
            assert not any(torch.equal(a.detach(), b) for a, b in zip(pa, before)), k
        if k == 0:
            assert all(float(o_av.state[a]["exp_avg"].abs().max()) > 0 and o_av.state[a]["step"] == 1 for a in pa)
        for r, a in zip(pr, pa):
            torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7)
    assert o_av.schedule_step() == total + 3 and len(o_av._plans) == 1
    assert [g["lr"] for g in o_av.param_groups] == list(LRS)          # the base rates stay in the groups


def test_under_the_grad_scaler_a_skipped_step_decays_nothing():
    """The injected-inf protocol of tests/test_optim_clip_gpu.py: steps 2, 3 and 7 overflow."""
    optim = pkg("optim")
    warmup, total, wds = 2, 12, (0.1, 0.05)
    p0, grads = _data(steps=9, seed=3)
    pr, pa = _params(p0), _params(p0)
    o_ref = torch.optim.AdamW(_groups(pr, wds))
    sched = torch.optim.lr_scheduler.LambdaLR(o_ref, _cosine_lambda(warmup, total))
    o_av = optim.AvAdam(_groups(pa, wds), decay_1d=True, lr_schedule="cosine", warmup_steps=warmup, total_steps=total)
    s_ref = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    s_av = optim.AvGradScaler(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    taken = 0
    for it, gs in enumerate(grads):
        sc_ref = float(s_ref.scale(torch.ones((), device="cuda")))
        sc_av = s_av.get_scale()
        assert sc_ref == sc_av, (it, sc_ref, sc_av)
        _set_grads(pr, gs, factor=sc_ref, view=False); _set_grads(pa, gs, factor=sc_av)
        if it in (2, 7):
            pr[1].grad[17] = float("inf"); pa[1].grad[17] = float("inf")
        if it == 3:
            pr[4].grad[0] = float("nan"); pa[4].grad[0] = float("nan")
        before = [p.detach().clone() for p in pa]
        s_ref.step(o_ref); s_ref.update()
        s_av.step(o_av); s_av.update()
        if it in (2, 3, 7):
            assert all(torch.equal(a.detach(), b) for a, b in zip(pa, before)), it     # skipped: no bit of any parameter changes
        else:
            sched.step()                                                          # the schedule does not move on a skipped step
            got, host = float(o_av.last_lr_mult), optim.lr_multiplier(taken, warmup, total, schedule="cosine")
            assert abs(got - host) <= ULP * abs(host) + 2.0 ** -50, (it, got, host)
            taken += 1
        assert o_av.schedule_step() == taken, it
        for r, a in zip(pr, pa):
            torch.testing.assert_close(a.detach(), r.detach(), rtol=2e-6, atol=2e-7)
    assert taken == 6 and s_av.steps_taken() == 6
    o_av.sync_steps(s_av)
    assert all(st["step"] == 6 for st in o_av.state.values())


def test_with_clipping_the_decay_does_not_see_the_coefficient():
    """Against clip_grad_norm_ + AdamW.  Every step is clipped to about a tenth: a decay scaled by the coefficient would leave the decayed
    tensors off by 0.9 * lr * lambda = 4.5e-4 relative, far outside the tolerance."""
    optim = pkg("optim")
    wds = (0.5, 0.25)
    p0, grads = _data(steps=3)
    max_norm = 0.1 * min(_norm64(gs, drop=step == 1) for step, gs in enumerate(grads))
    pr, pa = _params(p0), _params(p0)
    o_ref = torch.optim.AdamW(_groups(pr, wds))
    o_av = optim.AvAdam(_groups(pa, wds), decay_1d=True, max_grad_norm=max_norm)
    for step, gs in enumerate(grads):
        _set_grads(pr, gs, drop=step == 1, view=False); _set_grads(pa, gs, drop=step == 1)
        torch.nn.utils.clip_grad_norm_(pr, max_norm)
        o_ref.step(); o_av.step()
        assert float(o_av.last_clip_coef) < 0.11 and float(o_av.last_lr_mult) == 1.0
        assert _close_ulp(float(o_av.last_grad_norm), _norm64(gs, drop=step == 1))
        for r, a in zip(pr, pa):
            torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7)


def test_the_average_and_the_shadow_follow_the_decayed_parameters():
    optim, shadow = pkg("optim"), pkg("utils.shadow")
    decay, wds = 0.9, (0.1, 0.05)
    p0, grads = _data(steps=4)
    pr, pa = _params(p0), _params(p0)
    cache = shadow.ParamCache()
    sh = _shadows(pa, cache)
    o_ref = torch.optim.AdamW(_groups(pr, wds))
    o_av = optim.AvAdam(_groups(pa, wds), decay_1d=True, ema_decay=decay)
    ema_ref = [None] * len(pr)
    for k, gs in enumerate(grads):
        drop = k == 2                                                 # parameter 2 then has an average and no gradient
        _set_grads(pr, gs, drop=drop, view=False); _set_grads(pa, gs, drop=drop)
        o_ref.step(); o_av.step()
        w = 1.0 - optim.ema_decay(k, decay)
        for i, r in enumerate(pr):
            ema_ref[i] = r.detach().clone() if ema_ref[i] is None else torch.lerp(ema_ref[i], r.detach(), w)
        for i, (r, a) in enumerate(zip(pr, pa)):
            torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7)
            torch.testing.assert_close(o_av.state[a]["ema"], ema_ref[i], rtol=1e-6, atol=1e-7)
        for i, s in zip((0, 1, 4), sh):
            assert torch.equal(s, pa[i].data.to(torch.bfloat16).reshape(s.shape)), (k, i)      # the cast of the NEW, decayed parameter
            assert shadow.lookup(pa[i]) is not None
    assert o_av.ema_step() == 4 and o_av.fused_launches == 4
    p_old, e_old, sh_old = [p.detach().clone() for p in pa], [o_av.state[p]["ema"].clone() for p in pa], [s.clone() for s in sh]
    o_av.swap_averaged()
    assert all(torch.equal(p.detach(), e) for p, e in zip(pa, e_old))
    o_av.swap_averaged()
    for p, po, eo in zip(pa, p_old, e_old):
        assert torch.equal(p.detach(), po) and torch.equal(o_av.state[p]["ema"], eo)
    assert all(torch.equal(s, so) for s, so in zip(sh, sh_old))


def _run(optim, p0, grads, groups=_groups, drop_at=1, **kw):
    ps = _params(p0)
    opt = optim.AvAdam(groups(ps), **kw)
    for step, gs in enumerate(grads):
        _set_grads(ps, gs, drop=step == drop_at)
        opt.step()
    return ps, opt


def _same(pa, oa, pb, ob, idx):
    return [torch.equal(pa[i].detach(), pb[i].detach()) and torch.equal(oa.state[pa[i]]["exp_avg"], ob.state[pb[i]]["exp_avg"])
            and torch.equal(oa.state[pa[i]]["exp_avg_sq"], ob.state[pb[i]]["exp_avg_sq"]) for i in idx]


def test_off_is_off():
    optim = pkg("optim")
    p0, grads = _data(steps=3)
    pa, oa = _run(optim, p0, grads)
    pb, ob = _run(optim, p0, grads, weight_decay=0, lr_schedule="linear")
    assert all(_same(pa, oa, pb, ob, range(5)))
    assert ob.last_lr_mult is None and ob.SCHEDULE_KEY not in ob.state_dict() and oa.fused_launches == ob.fused_launches == 3
    assert all(pl.wd is None for pl in ob._plans.values())            # every lambda 0: the launch passes NULL
    # groups whose lambda is 0, in an optimizer whose other group decays, are the plain run bit for bit
    pc, oc = _run(optim, p0, grads, groups=lambda ps: _groups(ps, (0.3, 0.0)), decay_1d=True)
    assert all(pl.wd is not None for pl in oc._plans.values())
    assert all(_same(pa, oa, pc, oc, range(2, 5)))
    assert not any(torch.equal(pa[i].detach(), pc[i].detach()) for i in range(2))
    assert all(torch.equal(oa.state[pa[i]]["exp_avg"], oc.state[pc[i]]["exp_avg"]) for i in range(2))     # the moments never see the parameter
    # ... and with the schedule on both sides
    kw = dict(warmup_steps=1, total_steps=5)
    pd, od = _run(optim, p0, grads, **kw)
    pe, oe = _run(optim, p0, grads, groups=lambda ps: _groups(ps, (0.3, 0.0)), decay_1d=True, **kw)
    assert all(_same(pd, od, pe, oe, range(2, 5))) and not any(torch.equal(pd[i].detach(), pe[i].detach()) for i in range(2))


def test_one_dimensional_tensors_are_not_decayed_unless_asked():
    optim = pkg("optim")
    p0, grads = _data(steps=3)
    pa, oa = _run(optim, p0, grads)
    pb, ob = _run(optim, p0, grads, weight_decay=0.1)
    assert ONE_D == [1, 2, 4] and TWO_D == [0, 3]
    assert all(_same(pa, oa, pb, ob, ONE_D))
    assert not any(torch.equal(pa[i].detach(), pb[i].detach()) for i in TWO_D)
    pc, oc = _run(optim, p0, grads, weight_decay=0.1, decay_1d=True)
    assert not any(torch.equal(pa[i].detach(), pc[i].detach()) for i in range(5))
    assert all(torch.equal(pb[i].detach(), pc[i].detach()) for i in TWO_D)


def test_resume_from_state_dict_continues_cosine_and_decay():
    optim = pkg("optim")
    kw = dict(weight_decay=0.1, decay_1d=True, lr_schedule="cosine", warmup_steps=2, total_steps=7)
    p0, grads = _data(steps=5, seed=8)
    pa, oa = _run(optim, p0, grads, **kw)
    pb, ob = _run(optim, p0, grads[:4], **kw)
    sd = copy.deepcopy(ob.state_dict())
    assert sd[ob.SCHEDULE_KEY] == 4 and all(g["weight_decay"] == 0.1 for g in sd["param_groups"])
    old = copy.deepcopy(sd)
    for g in old["param_groups"]:
        del g["weight_decay"]                                         # a state dict written before the key existed
    for state in (sd, old):
        pc = [p.detach().clone().requires_grad_(True) for p in pb]
        oc = optim.AvAdam(_groups(pc), **kw)
        oc.load_state_dict(state)
        assert oc.schedule_step() == 4
        _set_grads(pc, grads[4])
        oc.step()                                                     # runs at the constructor default where the key is missing
        assert oc.schedule_step() == 5 and oc.state[pc[2]]["step"] == 4 and oc.state[pc[0]]["step"] == 5
        assert float(oc.last_lr_mult) == float(oa.last_lr_mult)
        for a, c in zip(pa, pc):
            assert torch.equal(a.detach(), c.detach())
            assert torch.equal(oa.state[a]["exp_avg"], oc.state[c]["exp_avg"])
    torch.optim.AdamW(_groups(_params(p0))).load_state_dict(sd)       # torch's AdamW accepts the dict


def test_trainer_decays_matrices_inside_the_fused_step():
    from trainer_util import gpu_trainer
    init = pkg("utils.init"); synth = pkg("dataset.synthetic")
    cfg = init.W2V2_TINY
    batch = synth.make_batch(2, 1.0, seed=5, ragged=True)
    kw = dict(lr_schedule="cosine", warmup_steps=2, total_steps=6)
    a, b = gpu_trainer(cfg, "fp32", weight_decay=0.01, **kw), gpu_trainer(cfg, "fp32", weight_decay=0.01, **kw)
    plain = gpu_trainer(cfg, "fp32", weight_decay=0.0, **kw)
    assert a.optimizer.decay_1d is False and all(g["weight_decay"] == 0.01 for g in a.optimizer.param_groups)
    start = [p.detach().clone() for p in a.parameters]
    for step in range(4):
        oa, ob = a.train_step(batch), b.train_step(batch)
        assert torch.equal(oa["total"], ob["total"]), step
        if step == 0:                                                 # warmup step 0: multiplier 0, nothing moves, nothing decays
            assert all(torch.equal(p.detach(), s) for p, s in zip(a.parameters, start))
        if step < 2:
            plain.train_step(batch)
        if step == 1:
            # Step 1 is the first that moves anything, and all three trainers enter it with the same weights, so the same gradients: there the
            # 1-D parameters must equal the undecayed trainer's bit for bit.  From the next step on the matrices differ and with them every gradient.
            moved = [i for i, (p, s) in enumerate(zip(a.parameters, start)) if not torch.equal(p.detach(), s)]
            one_d = [i for i in moved if a.parameters[i].ndim <= 1]
            mats = [i for i in moved if a.parameters[i].ndim > 1]
            assert one_d and mats
            assert all(torch.equal(a.parameters[i].detach(), plain.parameters[i].detach()) for i in one_d)
            assert any(not torch.equal(a.parameters[i].detach(), plain.parameters[i].detach()) for i in mats)
    for p, q in zip(a.parameters, b.parameters):
        assert torch.equal(p.detach(), q.detach())
    assert a.optimizer.fused_launches == b.optimizer.fused_launches == 4 and a.optimizer.schedule_step() == 4
