"""GPU: the exponential moving average of the weights inside the fused Adam step (optim.AvAdam(ema_decay=...), av_adam_multi_ema), the
in-place exchange of parameters and averages (av_param_swap_multi), and evaluating / saving with the averaged weights - against the law
in float64, torch.optim.swa_utils.AveragedModel on the same device, and runs with the feature off."""
import copy

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

# the shapes of test_optim_clip_gpu.py - (70001,): two chunks and a tail that is no multiple of 4; (5,): tail only; (128, 1024): exactly two
# aligned chunks; the (4097,) parameter's GRADIENT is a view one element into a larger buffer - and a sixth PARAMETER that is itself a leaf made
# from such a view: p is not 16-byte aligned, so every kernel (Adam + EMA, swap) takes its scalar path for it
SHAPES = [(1000, 33), (70001,), (5,), (128, 1024), (4097,), (3001,)]
LRS = (1e-4, 2e-5)
ULP = 2.0 ** -23
SHADOWED = (0, 1, 4, 5)


@pytest.fixture(autouse=True)
def _bf16_library():
    """The 16-bit shadows below are bfloat16: the library of the bf16 / fp32 modes writes them."""
    prec = pkg("precision")
    was = prec.get_precision()
    prec.set_precision("bf16")
    yield
    prec.set_precision(was)


def _data(steps=5, seed=12):
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(*s, generator=g) for s in SHAPES]
    grads = [[torch.randn(*s, generator=g) for s in SHAPES] for _ in range(steps)]
    return p0, grads


def _offset_leaf(x):
    buf = torch.zeros(x.numel() + 1, device="cuda")
    buf[1:] = x.reshape(-1)
    p = buf[1:].detach().requires_grad_()
    assert p.is_leaf and p.data_ptr() % 16 != 0
    return p


def _params(p0, plain=False):
    """plain: ordinary tensors throughout (torch's side)."""
    ps = [p.clone().cuda().requires_grad_(True) for p in p0[:5]]
    ps.append(p0[5].clone().cuda().requires_grad_(True) if plain else _offset_leaf(p0[5].cuda()))
    return ps


def _like(ps):
    """Fresh leaves with the values and the alignment of ``ps``."""
    return [_offset_leaf(p.detach()) if p.data_ptr() % 16 else p.detach().clone().requires_grad_(True) for p in ps]


def _groups(ps):
    return [{"params": ps[:2], "lr": LRS[0]}, {"params": ps[2:], "lr": LRS[1]}]


def _set_grads(ps, gs, drop=False, factor=1.0, view=True):
    """Gradients of one step; drop: parameter 2 gets none.  view: the (4097,) gradient is a slice of a (4098,) buffer."""
    for i, (p, g) in enumerate(zip(ps, gs)):
        g = g.cuda() * factor
        if view and i == 4:
            buf = torch.zeros(g.numel() + 1, device="cuda")
            buf[1:] = g
            g = buf[1:]
            assert g.data_ptr() % 16 != 0
        p.grad = g
    if drop:
        ps[2].grad = None


def _emas(opt, ps):
    return [opt.state[p]["ema"].clone() for p in ps]


def _lerp64(ema, p, w):
    """torch.lerp written out, in float64 on fp32 inputs."""
    ema, p = ema.double(), p.double()
    return ema + w * (p - ema) if w < 0.5 else p - (p - ema) * (1.0 - w)


@pytest.mark.parametrize("decay,warmup", [(0.999, False), (0.5, False), (0.9, True)])
def test_every_update_is_the_law_within_three_roundings(decay, warmup):
    """Each EMA update against the law in float64 on the same fp32 inputs, with w = 1 - float(last_ema_decay).  The bound is derived: the
    kernel rounds the subtraction, the product and the sum (w and 1 - w add at most half an ulp of a term below max(|ema|, |p|)), so
    |got - want| <= 3 * 2^-23 * max(|ema|, |p_new|) elementwise.  0.999: the w < 0.5 branch; 0.5 and the warmup: the other one.
    Parameter 2 gets no gradient in steps 1 and 3.  After update 0 its average equals the parameter, so in step 1 the law maps it onto
    itself; in step 3 the average lags the parameter and must move although the Adam launch does not see the tensor."""
    optim = pkg("optim")
    p0, grads = _data(steps=5)
    ps = _params(p0)
    opt = optim.AvAdam(_groups(ps), ema_decay=decay, ema_warmup=warmup)
    worst = worst_lerp = 0.0
    for k, gs in enumerate(grads):
        drop = k in (1, 3)
        _set_grads(ps, gs, drop=drop)
        prev = [opt.state[p]["ema"].clone() if "ema" in opt.state[p] else p.detach().clone() for p in ps]
        p2 = ps[2].detach().clone()
        opt.step()
        d = float(opt.last_ema_decay)
        assert d == float(np.float32(optim.ema_decay(k, decay, warmup))), (k, d)
        w = 1.0 - d
        for i, p in enumerate(ps):
            got, pn = opt.state[p]["ema"], p.detach()
            assert got.dtype == torch.float32 and got.shape == p.shape
            bound = 3 * ULP * torch.maximum(prev[i].abs(), pn.abs()).double()
            err = (got.double() - _lerp64(prev[i], pn, w)).abs()
            assert bool((err <= bound).all()), (k, i, float((err / bound.clamp_min(1e-300)).max()))
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            ref = torch.lerp(prev[i], pn, float(np.float32(w)))
            worst_lerp = max(worst_lerp, float(((ref.double() - _lerp64(prev[i], pn, w)).abs() / bound.clamp_min(1e-300)).max()))
            if k == 0:
                assert torch.equal(got, pn)                         # d_0 = 0: the first update copies the parameters exactly
        if drop:
            assert torch.equal(ps[2].detach(), p2)                  # no gradient: Adam left the parameter alone
            if k == 3:
                assert not torch.equal(opt.state[ps[2]]["ema"], prev[2])      # ... and its average still moved towards it
    print(f"decay {decay} warmup {warmup}: worst |got - want| / bound {worst:.3f} (torch.lerp on the device: {worst_lerp:.3f})")
    assert opt.ema_step() == 5 and opt.fused_launches == 5


@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_matches_torch_adam_with_averaged_model(decay):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    optim = pkg("optim")
    p0, grads = _data(steps=5)
    pr, pa = _params(p0, plain=True), _params(p0)

    class Holder(torch.nn.Module):
        def __init__(self, ps):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(p.detach()) for p in ps])

    model = Holder(pr)
    pr = list(model.ps)
    o_ref = torch.optim.Adam(_groups(pr))
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
    o_av = optim.AvAdam(_groups(pa), ema_decay=decay)
    for step, gs in enumerate(grads):
        _set_grads(pr, gs, drop=step == 1, view=False); _set_grads(pa, gs, drop=step == 1)
        o_ref.step(); avg.update_parameters(model); o_av.step()
        for r, e, a in zip(pr, avg.module.ps, pa):
            torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7)
            torch.testing.assert_close(o_av.state[a]["ema"], e.detach(), rtol=1e-6, atol=1e-7)
    assert int(avg.n_averaged) == o_av.ema_step() == 5


def _shadows(ps, cache):
    return [cache.get(i, [ps[i]], torch.bfloat16, lambda i=i: ps[i].data.to(torch.bfloat16), flat=True) for i in SHADOWED]


@pytest.mark.parametrize("kw", [{}, dict(max_grad_norm=40.0, warmup_steps=2, total_steps=9)], ids=["plain", "clip_schedule"])
def test_with_the_average_on_nothing_else_changes(kw):
    optim, shadow = pkg("optim"), pkg("utils.shadow")
    p0, grads = _data(steps=4)
    for dropping in (True, False):
        pa, pb = _params(p0), _params(p0)
        ca, cb = shadow.ParamCache(), shadow.ParamCache()
        sa, sb = _shadows(pa, ca), _shadows(pb, cb)
        oa = optim.AvAdam(_groups(pa), ema_decay=0.9, **kw)
        ob = optim.AvAdam(_groups(pb), **kw)
        for step, gs in enumerate(grads):
            drop = dropping and step == 1
            _set_grads(pa, gs, drop=drop); _set_grads(pb, gs, drop=drop)
            oa.step(); ob.step()
            for a, b in zip(pa, pb):
                assert torch.equal(a.detach(), b.detach())
                assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
                assert oa.state[a]["step"] == ob.state[b]["step"] and "ema" not in ob.state[b]
            for i, a, b in zip(SHADOWED, sa, sb):
                assert torch.equal(a, b) and torch.equal(a, pa[i].data.to(torch.bfloat16).reshape(a.shape))
                assert shadow.lookup(pa[i]) is not None
        assert oa.fused_launches == ob.fused_launches == 4
        assert ob.last_ema_decay is None and ob.EMA_KEY not in ob.state_dict()
        if kw:
            assert torch.equal(oa.last_grad_norm, ob.last_grad_norm) and oa.schedule_step() == ob.schedule_step() == 4
        if not dropping:
            assert len(oa._plans) == len(ob._plans) == 1            # a fixed gradient pattern: one plan, nothing uploaded again


@pytest.mark.parametrize("max_norm", [0.0, 50.0], ids=["check_pass", "norm_pass"])
def test_under_the_grad_scaler_overflowing_steps_leave_the_average_alone(max_norm):
    """The injected-inf protocol of test_under_the_grad_scaler_... (tests/test_optim_clip_gpu.py): steps 2, 3 and 7 overflow.  The device skips
    the EMA with the step and does not count it - whether the non-finite check is its own pass or the norm pass."""
    optim = pkg("optim")
    p0, grads = _data(steps=9, seed=3)
    pa = _params(p0)
    o_av = optim.AvAdam(_groups(pa), ema_decay=0.9, max_grad_norm=max_norm)
    s_av = optim.AvGradScaler(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    taken = 0
    for it, gs in enumerate(grads):
        _set_grads(pa, gs, factor=s_av.get_scale())
        if it in (2, 7):
            pa[1].grad[17] = float("inf")
        if it == 3:
            pa[4].grad[0] = float("nan")
        before = _emas(o_av, pa) if it else None
        s_av.step(o_av); s_av.update()
        after = _emas(o_av, pa)
        if it in (2, 3, 7):
            assert all(torch.equal(a, b) for a, b in zip(after, before)), it
        else:
            taken += 1
            assert float(o_av.last_ema_decay) == float(np.float32(optim.ema_decay(taken - 1, 0.9))), it
            if it:
                assert not any(torch.equal(a, b) for a, b in zip(after, before)), it
        assert all(bool(torch.isfinite(a).all()) for a in after)
    assert s_av.steps_taken() == 6 and o_av.ema_step() == 6
    assert o_av.state_dict()[o_av.EMA_KEY] == 6


def test_swap_exchanges_parameters_averages_and_shadows_in_place():
    optim, shadow = pkg("optim"), pkg("utils.shadow")
    p0, grads = _data(steps=3)
    ps = _params(p0)
    lone = torch.randn(17, device="cuda").requires_grad_(True)         # never gets a gradient: no average, its averaged value is itself
    opt = optim.AvAdam([{"params": ps[:2], "lr": LRS[0]}, {"params": ps[2:] + [lone], "lr": LRS[1]}], ema_decay=0.5)
    cache = shadow.ParamCache()
    sh = _shadows(ps, cache)
    built = []

    def derived():
        built.append(1)
        return ps[3].data.to(torch.bfloat16).t().contiguous()

    for step, gs in enumerate(grads):
        _set_grads(ps, gs, drop=step == 1)
        opt.step()
    assert "ema" not in opt.state.get(lone, {})
    first = cache.get("t3", [ps[3]], torch.bfloat16, derived)
    assert len(built) == 1 and cache.get("t3", [ps[3]], torch.bfloat16, derived) is first and len(built) == 1
    p_old, e_old = [p.detach().clone() for p in ps], _emas(opt, ps)
    sh_old = [s.clone() for s in sh]
    assert not any(torch.equal(p, e) for p, e in zip(p_old, e_old))
    lone_old, lone_ver = lone.detach().clone(), lone._version

    def check_swapped():
        for i, p in enumerate(ps):
            assert torch.equal(p.detach(), e_old[i]) and torch.equal(opt.state[p]["ema"], p_old[i])
        for i, s in zip(SHADOWED, sh):
            assert torch.equal(s, ps[i].data.to(torch.bfloat16).reshape(s.shape))
            assert shadow.lookup(ps[i]) is not None                                     # written by the launch and marked fresh ...
            assert cache.get(i, [ps[i]], torch.bfloat16, lambda: 1 / 0, flat=True) is s   # ... so nothing is cast again
        assert torch.equal(lone.detach(), lone_old) and lone._version == lone_ver

    def check_restored():
        for i, p in enumerate(ps):
            assert torch.equal(p.detach(), p_old[i]) and torch.equal(opt.state[p]["ema"], e_old[i])
        for s, o in zip(sh, sh_old):
            assert torch.equal(s, o)
        assert torch.equal(lone.detach(), lone_old) and lone._version == lone_ver

    opt.swap_averaged()
    check_swapped()
    second = cache.get("t3", [ps[3]], torch.bfloat16, derived)              # a derived entry rebuilds from the new parameter
    assert len(built) == 2 and torch.equal(second, e_old[3].to(torch.bfloat16).t())
    _set_grads(ps, grads[0])
    with pytest.raises(RuntimeError, match="averaged"):
        opt.step()
    check_swapped()                                                         # the refused step touched nothing
    opt.swap_averaged()
    check_restored()
    assert len(built) == 2 and torch.equal(cache.get("t3", [ps[3]], torch.bfloat16, derived), first) and len(built) == 3
    with opt.averaged():
        check_swapped()
    check_restored()
    with pytest.raises(KeyError):
        with opt.averaged():
            raise KeyError("inside")
    check_restored()
    opt.step()                                                              # swapped back: stepping works again
    assert opt.ema_step() == 4


def test_resume_from_state_dict_continues_the_average():
    optim = pkg("optim")
    kw = dict(ema_decay=0.9, ema_warmup=True)
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
    assert sd[ob.EMA_KEY] == 4
    pc = _like(pb)
    oc = optim.AvAdam(_groups(pc), **kw)
    oc.load_state_dict(sd)
    assert oc.ema_step() == 4
    _set_grads(pc, grads[4])
    oc.step()
    assert oc.ema_step() == 5 and float(oc.last_ema_decay) == float(np.float32(optim.ema_decay(4, 0.9, True))) == float(oa.last_ema_decay)
    for a, c in zip(pa, pc):
        assert torch.equal(a.detach(), c.detach())
        assert torch.equal(oa.state[a]["ema"], oc.state[c]["ema"])
    torch.optim.Adam(_groups(_params(p0, plain=True))).load_state_dict(sd)     # torch's Adam accepts the dict
    oc.reset_state()
    assert oc.ema_step() == 0 and not oc.state


def _with(t0, **kw):
    tr = pkg("model.trainer")
    t = tr.MultimodalTrainer(t0.visual_encoder, t0.audio_encoder, t0.fusion_module, t0.decoder1, t0.tokenizer, learning_rate=1e-4,
                             device="cuda", lambda_=0.1, **kw)
    t.fixed_projection = t0.fixed_projection
    return t


def _modules(t):
    return (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1)


def _all_params(t):
    return [p for m in _modules(t) for p in m.parameters()]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_trainer_evaluates_and_saves_with_the_averaged_weights(precision, tmp_path):
    from test_step_gpu import build
    init = pkg("utils.init"); synth = pkg("dataset.synthetic"); ckpt = pkg("checkpoint")
    cfg = init.W2V2_TINY
    batch = synth.make_batch(2, 1.0, seed=5, ragged=True)
    t = _with(build(cfg, precision), ema_decay=0.5, eval_ema=True)
    control = _with(build(cfg, precision), ema_decay=0.5)               # never evaluates
    for _ in range(3):
        t.train_step(batch); control.train_step(batch)
    opt = t.optimizer
    assert opt.ema_step() == 3 and float(opt.last_ema_decay) == 0.5
    averaged = [opt.state[p]["ema"].clone() if "ema" in opt.state.get(p, {}) else p.detach().clone() for p in _all_params(t)]
    n_avg = sum("ema" in opt.state.get(p, {}) for p in _all_params(t))
    assert 0 < n_avg < len(averaged)                                    # the frozen parameters have no average
    before = [p.detach().clone() for p in _all_params(t)]
    assert any(not torch.equal(a, b) for a, b in zip(averaged, before))
    modes = [(sm, sm.training) for m in _modules(t) for sm in m.modules()]
    loss_ema, _ = t.evaluate([batch])
    path = str(tmp_path / "averaged.pt")
    ckpt.save_checkpoint(0, t, path, averaged=True)
    for sm, was in modes:                                               # evaluate() leaves the modules in eval mode
        sm.training = was
    for p, b in zip(_all_params(t), before):
        assert torch.equal(p.detach(), b)

    # the next step is the one of a trainer that never evaluated
    o_t, o_c = t.train_step(batch), control.train_step(batch)
    assert torch.equal(o_t["total"], o_c["total"])
    for a, b in zip(_all_params(t), _all_params(control)):
        assert torch.equal(a.detach(), b.detach())
    for a, b in zip(_all_params(t), _all_params(control)):
        if "ema" in opt.state.get(a, {}):
            assert torch.equal(opt.state[a]["ema"], control.optimizer.state[b]["ema"])

    # a twin whose parameters were overwritten with the averages from outside (buffers - BatchNorm statistics - are the trained ones)
    twin = build(cfg, precision)
    ck = torch.load(path, map_location="cuda", weights_only=True)
    assert ck["optimizer"]["av_ema_step"] == 3
    for m, key in zip(_modules(twin), ("visual_encoder", "audio_encoder", "fusion", "decoder1")):
        m.load_state_dict(ck[key])                                      # buffers (and parameters, overwritten next)
    with torch.no_grad():
        for p, a in zip(_all_params(twin), averaged):
            p.data.copy_(a)
    loss_twin, _ = twin.evaluate([batch])
    assert loss_twin == loss_ema, (loss_twin, loss_ema)

    # the averaged checkpoint has the ordinary layout: it loads into a fresh trainer and gives that loss
    fresh = build(cfg, precision)
    assert ckpt.load_checkpoint(fresh, path, audio_encoder=True) == 1
    for p, a in zip(_all_params(fresh), averaged):
        assert torch.equal(p.detach(), a)
    loss_fresh, _ = fresh.evaluate([batch])
    assert loss_fresh == loss_ema, (loss_fresh, loss_ema)
    plain = build(cfg, precision)
    with pytest.raises(ValueError):
        ckpt.save_checkpoint(0, plain, str(tmp_path / "no.pt"), averaged=True)
