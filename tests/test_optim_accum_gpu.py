"""GPU: gradient accumulation on the device (optim.AvAdam.accumulate, av_grad_accum_multi; MultimodalTrainer(accum_steps=...)) against
torch's own accumulation on the same device, against the plain fused step on the summed gradients, float64 on the host for the norm, and
against runs with the feature off."""
import pytest
import torch

from conftest import pkg
from test_optim_clip_gpu import SHAPES, _close_ulp, _data, _groups, _norm64, _params, _set_grads, _shadows

pytestmark = pytest.mark.gpu

# the shapes of test_optim_clip_gpu.py: (70001,) two chunks and a tail that is no multiple of 4, (5,) tail only, (128, 1024) exactly two aligned
# chunks, and the last GRADIENT a view one element into a larger buffer (the scalar path of the accumulate kernel; its accumulator is aligned).
NEG_ZERO = -2 ** 31                                                   # the bits of -0.0 as an int32


@pytest.fixture(autouse=True)
def _bf16_library():
    """The 16-bit shadows below are bfloat16: the library of the bf16 / fp32 modes writes them."""
    prec = pkg("precision")
    was = prec.get_precision()
    prec.set_precision("bf16")
    yield
    prec.set_precision(was)


def _torch_sums(micro, dropped=()):
    """a = g_0.clone(); a += g_1; ... per parameter on the device, in micro-step order, as autograd accumulates into .grad.  ``dropped``:
    (micro-step, parameter) pairs without a gradient.  None for a parameter that never got one."""
    sums = [None] * len(SHAPES)
    for k, gs in enumerate(micro):
        for i, g in enumerate(gs):
            if (k, i) in dropped:
                continue
            if sums[i] is None:
                sums[i] = g.cuda().clone()
            else:
                sums[i] += g.cuda()
    return sums


def _accumulate(opt, ps, micro, dropped=(), factor=1.0, poke=None):
    for k, gs in enumerate(micro):
        _set_grads(ps, gs, factor=factor)
        for kk, i in dropped:
            if kk == k:
                ps[i].grad = None
        if poke is not None:
            poke(k)
        opt.accumulate()


def _same_state(oa, pa, ob, pb, keys=("exp_avg", "exp_avg_sq")):
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a.detach(), b.detach()), i
        assert (a in oa.state and bool(oa.state[a])) == (b in ob.state and bool(ob.state[b])), i
        for key in keys:
            if b in ob.state and ob.state[b]:
                assert torch.equal(oa.state[a][key], ob.state[b][key]), (i, key)


def test_the_accumulator_is_torchs_sum_bit_for_bit():
    optim = pkg("optim")
    p0, micro = _data(steps=3)
    micro[0][1][3] = -0.0                                             # quad path, first chunk
    micro[0][1][65537] = float("inf")                                 # second chunk
    micro[0][1][70000] = float("nan")                                 # the tail
    micro[1][4][0] = -0.0; micro[1][4][4096] = -0.0                   # the view: the scalar path
    micro[0][4][0] = -0.0                                             # -0.0 + -0.0 = -0.0 there after micro-step 1; -0.0 + x elsewhere
    ps = _params(p0)
    opt = optim.AvAdam(_groups(ps))
    assert opt.accum_pending == 0 and opt._accum == {}
    for k in range(3):
        _set_grads(ps, micro[k], drop=k == 0)                         # parameter 2: its first contribution is micro-step 1, a copy
        assert ps[4].grad.data_ptr() % 16 != 0
        opt.accumulate()
        assert opt.accum_pending == k + 1
        want = _torch_sums(micro[:k + 1], dropped={(0, 2)})
        for i, (p, w) in enumerate(zip(ps, want)):
            if w is None:
                assert p not in opt._accum and (k, i) == (0, 2)
                continue
            a = opt._accum[p]
            assert a.dtype == torch.float32 and a.is_contiguous() and a.shape == p.shape and a.data_ptr() % 16 == 0
            nan = torch.isnan(w)
            assert torch.equal(torch.isnan(a), nan), (k, i)
            assert torch.equal(a[~nan], w[~nan]), (k, i)
            assert int(nan.sum()) == (1 if i == 1 else 0)
            if k == 0 or (k == 1 and i == 2):                         # a copy: every bit, the sign of a zero included
                assert torch.equal(a.view(torch.int32)[~nan], w.view(torch.int32)[~nan]), (k, i)
        a1, a4 = opt._accum[ps[1]].view(torch.int32), opt._accum[ps[4]].view(torch.int32)
        if k == 0:
            assert int(a1[3]) == NEG_ZERO and int(a4[0]) == NEG_ZERO
            assert float(opt._accum[ps[1]][65537]) == float("inf")
        if k == 1:
            assert int(a4[0]) == NEG_ZERO                             # the sum of two negative zeros keeps the sign
            assert int(a4[4096]) == int(want[4].view(torch.int32)[4096]) != NEG_ZERO      # x + -0.0 = x
    assert opt.fused_launches == 0 and not opt.state                  # nothing has stepped
    assert len(opt._accum_plans) == 3                                 # copy without parameter 2; adds with its copy; adds
    for p, w in zip(ps, p0):
        assert torch.equal(p.detach().cpu(), w)


def test_a_step_on_accumulated_gradients_is_the_plain_step_on_their_sum():
    optim, shadow = pkg("optim"), pkg("utils.shadow")
    p0, micro = _data(steps=3)
    pa, pb = _params(p0), _params(p0)
    ca, cb = shadow.ParamCache(), shadow.ParamCache()
    sa, sb = _shadows(pa, ca), _shadows(pb, cb)
    oa, ob = optim.AvAdam(_groups(pa)), optim.AvAdam(_groups(pb))
    oa.grad_scale = 0.5
    ob.grad_scale = 0.5 / 3
    _accumulate(oa, pa, micro, dropped={(0, 2)})
    for p in pa:
        p.grad = None                                                 # the step runs on what contributed, whatever p.grad is now
    # plain contiguous tensors: the accumulators are aligned whatever the gradients were, and both sides take the same path
    _set_grads(pb, _torch_sums(micro, dropped={(0, 2)}), view=False)
    assert oa.accum_pending == 3
    oa.step(); ob.step()
    assert oa.accum_pending == 0 and not oa._accum_open and ob.accum_pending == 0 and ob._accum == {}
    _same_state(oa, pa, ob, pb)
    for a, b in zip(pa, pb):
        assert oa.state[a]["step"] == ob.state[b]["step"] == 1
    for i, a, b in zip((0, 1, 4), sa, sb):
        assert torch.equal(a, b) and torch.equal(a, pa[i].data.to(torch.bfloat16).reshape(a.shape)), i
    assert oa.fused_launches == ob.fused_launches == 1
    assert oa._steps_dev.tolist()[:5] == ob._steps_dev.tolist()[:5] == [1] * 5
    assert not any(torch.equal(a.detach().cpu(), w) for a, w in zip(pa, p0))


@pytest.mark.parametrize("n", [2, 4])
def test_it_is_torchs_accumulation(n):
    """torch's .grad is g_0 / N, then += g_k / N; N a power of two, so sum(g_k / N) and sum(g_k) / N are the same floats.  The gradients are
    standard normal draws halved (exact), the size torch sees in tests/test_optim_wd_gpu.py::test_matches_torch_adamw: hyper carries beta2 as
    a float32, so exp_avg_sq sits 1.3e-5 (relative) beside torch's, and (1.3e-5 - rtol) * 1e-3 * g^2 stays below atol only while |g| < 2.9,
    which a mean of two standard normal draws over 240 000 elements does not."""
    optim = pkg("optim")
    p0, grads = _data(steps=2 * n, seed=31)
    grads = [[g * 0.5 for g in gs] for gs in grads]
    pr, pa = _params(p0), _params(p0)
    o_ref = torch.optim.Adam(_groups(pr))
    o_av = optim.AvAdam(_groups(pa))
    assert o_av.grad_scale == 1.0 and o_av.accum_mean
    for step in range(2):
        micro = grads[step * n:(step + 1) * n]
        for k, gs in enumerate(micro):
            for r, g in zip(pr, gs):
                g = g.cuda() / n
                if k == 0:
                    r.grad = g
                else:
                    r.grad += g
        _accumulate(o_av, pa, micro)
        assert o_av.accum_pending == n
        o_ref.step(); o_av.step()
        worst = 0.0
        for r, a in zip(pr, pa):
            torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7)
            sa, sr = o_av.state[a], o_ref.state[r]
            worst = max(worst, float((sa["exp_avg_sq"] - sr["exp_avg_sq"]).abs().max()))
            torch.testing.assert_close(sa["exp_avg"], sr["exp_avg"], rtol=1e-6, atol=1e-7)
            torch.testing.assert_close(sa["exp_avg_sq"], sr["exp_avg_sq"], rtol=1e-6, atol=1e-7)
            assert sa["step"] == step + 1
        print(f"N {n} step {step}: exp_avg_sq worst |got - torch| {worst:.3e}")
    assert o_av.fused_launches == 2 and o_av.accum_pending == 0


def test_a_parameter_that_contributed_in_part_takes_one_step_on_what_it_got():
    """LayerDrop.  The reference optimizer steps on torch's sums with the same grad_scale / N."""
    optim = pkg("optim")
    p0, micro = _data(steps=6, seed=4)
    none = {(k, 2) for k in range(3)}
    pa, pb = _params(p0), _params(p0)
    oa, ob = optim.AvAdam(_groups(pa)), optim.AvAdam(_groups(pb))
    ob.grad_scale = 1.0 / 3
    # cycle 0: parameter 2 contributes in none of the micro-steps
    _accumulate(oa, pa, micro[:3], dropped=none)
    oa.step()
    _set_grads(pb, [s if s is not None else g for s, g in zip(_torch_sums(micro[:3], dropped=none), micro[0])], view=False)
    pb[2].grad = None
    ob.step()
    assert torch.equal(pa[2].detach().cpu(), p0[2])
    assert (pa[2] not in oa.state or not oa.state[pa[2]]) and pa[2] not in oa._accum
    assert oa._steps_dev.tolist()[:5] == [1, 1, 0, 1, 1]
    _same_state(oa, pa, ob, pb)
    # cycle 1: in one of three
    some = {(0, 2), (2, 2)}
    _accumulate(oa, pa, micro[3:], dropped=some)
    oa.step()
    _set_grads(pb, _torch_sums(micro[3:], dropped=some), view=False)
    ob.step()
    assert oa._steps_dev.tolist()[:5] == [2, 2, 1, 2, 2]              # the device's own step counts
    assert [oa.state[p]["step"] for p in pa] == [2, 2, 1, 2, 2]
    assert not torch.equal(pa[2].detach().cpu(), p0[2])
    _same_state(oa, pa, ob, pb)
    assert oa.fused_launches == ob.fused_launches == 2 and oa.accum_pending == 0


def test_clipping_schedule_and_ema_are_per_optimizer_step():
    optim = pkg("optim")
    n, scale = 3, 0.5
    p0, grads = _data(steps=2 * n, seed=9)
    ps = _params(p0)
    opt = optim.AvAdam(_groups(ps), max_grad_norm=1.0, warmup_steps=2, total_steps=10, ema_decay=0.9)
    opt.grad_scale = scale
    for cycle in range(2):
        micro = grads[cycle * n:(cycle + 1) * n]
        _accumulate(opt, ps, micro)
        opt.step()
        sum64 = [sum(g.double() for g in gs) for gs in zip(*micro)]
        got, want = float(opt.last_grad_norm), _norm64(sum64, factor=scale / n)
        print(f"cycle {cycle}: norm {got!r} float64 {want!r} rel {abs(got - want) / want:.3e}")
        assert _close_ulp(got, want), (cycle, got, want)
        assert float(opt.last_clip_coef) < 1.0
        assert float(opt.last_lr_mult) == optim.lr_multiplier(cycle, 2, 10)
        assert opt.schedule_step() == cycle + 1 and opt.ema_step() == cycle + 1
        assert float(opt.last_ema_decay) == float(torch.tensor(optim.ema_decay(cycle, 0.9), dtype=torch.float32))
    assert opt.fused_launches == 2 and [opt.state[p]["step"] for p in ps] == [2] * 5


def test_under_the_grad_scaler_an_overflow_discards_the_whole_cycle():
    optim = pkg("optim")
    kw = dict(total_steps=10, ema_decay=0.9)                          # no warmup: the first step taken moves the parameters
    skw = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=100)
    p0, grads = _data(steps=6, seed=3)
    ps = _params(p0)
    opt = optim.AvAdam(_groups(ps), **kw)
    sc = optim.AvGradScaler(init_scale=1024.0, **skw)

    def poke(k):
        if k == 1:
            ps[1].grad[17] = float("inf")

    _accumulate(opt, ps, grads[:3], factor=1024.0, poke=poke)
    assert opt.accum_pending == 3
    sc.step(opt); sc.update()
    assert opt.accum_pending == 0 and not opt._accum_open             # closed: the host does not know that the device skipped the step
    for p, w in zip(ps, p0):
        assert torch.equal(p.detach().cpu(), w)
        assert int(opt.state[p]["exp_avg"].count_nonzero()) == 0 and int(opt.state[p]["exp_avg_sq"].count_nonzero()) == 0
        assert torch.equal(opt.state[p]["ema"].cpu(), w)
    assert opt.schedule_step() == 0 and opt.ema_step() == 0 and opt._steps_dev.tolist()[:5] == [0] * 5
    assert sc.get_scale() == 512.0 and sc.steps_taken() == 0
    # the next, clean cycle: where a fresh optimizer with the backed-off scale ends
    _accumulate(opt, ps, grads[3:], factor=512.0)
    sc.step(opt); sc.update()
    pf = _params(p0)
    of = optim.AvAdam(_groups(pf), **kw)
    sf = optim.AvGradScaler(init_scale=512.0, **skw)
    _accumulate(of, pf, grads[3:], factor=512.0)
    sf.step(of); sf.update()
    _same_state(opt, ps, of, pf, keys=("exp_avg", "exp_avg_sq", "ema"))
    assert not any(torch.equal(p.detach().cpu(), w) for p, w in zip(ps, p0))
    assert opt.schedule_step() == of.schedule_step() == 1 and opt.ema_step() == of.ema_step() == 1
    assert opt._steps_dev.tolist()[:5] == of._steps_dev.tolist()[:5] == [1] * 5
    assert sc.get_scale() == sf.get_scale() == 512.0 and sc.steps_taken() == sf.steps_taken() == 1


def test_off_is_off():
    optim = pkg("optim")
    p0, grads = _data(steps=3)
    runs = []
    for kw in ({}, dict(accum_mean=True), dict(accum_mean=False)):    # without accumulate() the argument is never read
        ps = _params(p0)
        opt = optim.AvAdam(_groups(ps), **kw)
        for step, gs in enumerate(grads):
            _set_grads(ps, gs, drop=step == 1)
            opt.step()
            assert opt.accum_pending == 0
        assert opt._accum == {} and opt._accum_plans == {} and not opt._accum_open and opt._accum_keep is None
        assert set(opt.state_dict()) == {"state", "param_groups"}
        runs.append((ps, opt))
    (pa, oa), rest = runs[0], runs[1:]
    for pb, ob in rest:
        _same_state(oa, pa, ob, pb)
        assert oa.fused_launches == ob.fused_launches == 3


def test_the_sum_instead_of_the_mean_and_reset_state():
    optim = pkg("optim")
    p0, micro = _data(steps=2)
    pa, pb = _params(p0), _params(p0)
    oa, ob = optim.AvAdam(_groups(pa), accum_mean=False), optim.AvAdam(_groups(pb))
    _accumulate(oa, pa, micro)
    oa.reset_state()                                                  # closes the open cycle; the accumulators stay
    assert oa.accum_pending == 0 and not oa._accum_open and len(oa._accum) == 5
    for p in pa:
        p.grad = None
    oa.step()                                                         # nothing contributed, no gradient: nothing to do
    assert oa.fused_launches == 0
    _accumulate(oa, pa, micro)
    oa.step()
    _set_grads(pb, _torch_sums(micro), view=False)
    ob.step()                                                         # grad_scale 1: the sum
    _same_state(oa, pa, ob, pb)


# ---- the trainer ----
def _all_params(t):
    return [p for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1) for p in m.parameters()]


def _batches(n):
    synth = pkg("dataset.synthetic")
    return [synth.make_batch(2, 1.0, seed=5 + i, ragged=True) for i in range(n)]


def _forward_backward(t, batch):
    """train_step without a reducer or scaler, up to the optimizer (the lines of test_trainer_clips_inside_the_fused_step)."""
    t.optimizer.zero_grad(set_to_none=True)
    t._head_arena.begin_step()
    begin = getattr(t.audio_encoder.model, "begin_grad_step", None)
    if begin is not None:
        begin()
    out = t.forward_losses(batch)
    out["total"].backward()
    t._head_arena.finalize()


def test_trainer_steps_once_per_two_micro_batches():
    from test_step_gpu import build
    cfg = pkg("utils.init").W2V2_TINY
    b0, b1 = _batches(2)
    acc = build(cfg, "fp32", accum_steps=2)
    start = [p.detach().clone() for p in _all_params(acc)]
    o0 = acc.train_step(b0)
    assert o0["stepped"] is False and "grad_norm" not in o0
    assert acc.optimizer.fused_launches == 0 and acc.optimizer.accum_pending == 1
    assert all(torch.equal(p.detach(), s) for p, s in zip(_all_params(acc), start))
    o1 = acc.train_step(b1)
    assert o1["stepped"] is True and acc.optimizer.fused_launches == 1 and acc.optimizer.accum_pending == 0
    assert not torch.equal(o0["total"], o1["total"])
    # the reference: both backward passes by hand, the first gradients cloned, the second added, one step on the mean
    ref = build(cfg, "fp32")
    _forward_backward(ref, b0)
    first = {p: p.grad.clone() for p in ref.parameters if p.grad is not None}
    _forward_backward(ref, b1)
    assert first and {id(p) for p in first} == {id(p) for p in ref.parameters if p.grad is not None}
    for p, g in first.items():
        g += p.grad
        p.grad = g
    ref.optimizer.grad_scale = 0.5
    ref.optimizer.step()
    moved = 0
    for a, b, s in zip(_all_params(acc), _all_params(ref), start):    # not bit for bit: the vector-zone column sums use atomics
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-6, atol=1e-7)
        moved += not torch.equal(a.detach(), s)
    assert 0 < moved <= len(first)


def test_trainer_with_one_step_per_batch_is_the_trainer_without_the_argument():
    from test_step_gpu import build
    cfg = pkg("utils.init").W2V2_TINY
    (b0,) = _batches(1)
    one, plain = build(cfg, "fp32", accum_steps=1), build(cfg, "fp32")
    oa, ob = one.train_step(b0), plain.train_step(b0)
    assert "stepped" not in oa and "stepped" not in ob
    assert one.optimizer.fused_launches == plain.optimizer.fused_launches == 1
    assert one.optimizer.accum_pending == 0 and one.optimizer._accum == {}
    for a, b in zip(_all_params(one), _all_params(plain)):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-6, atol=1e-7)


def test_train_epoch_flushes_the_open_cycle():
    from test_step_gpu import build
    cfg = pkg("utils.init").W2V2_TINY
    t = build(cfg, "fp32", accum_steps=2)
    t.train_epoch(_batches(3))                                        # a full cycle, then one micro-step that the flush steps on its own
    assert t.optimizer.fused_launches == 2 and t.optimizer.accum_pending == 0
    assert t.flush_accumulated() is False


def test_train_epoch_logs_the_norm_only_once_a_step_has_been_taken(capsys):
    """With clipping on, batch 0 of the first epoch is a micro-step before any optimizer step: there is no norm to print yet, and nothing raises."""
    from test_step_gpu import build
    cfg = pkg("utils.init").W2V2_TINY
    t = build(cfg, "fp32", accum_steps=2, max_grad_norm=1.0)
    batches = _batches(3)
    t.train_epoch(batches)
    first = capsys.readouterr().out
    assert "Error at batch" not in first and "[Batch 0] CTC1" in first and "grad norm" not in first
    assert t.optimizer.fused_launches == 2 and t.optimizer.accum_pending == 0
    assert float(t.optimizer.last_grad_norm) > 0 and float(t.optimizer.last_clip_coef) <= 1.0
    t.train_epoch(batches)                                            # now batch 0 shows the last optimizer step's norm
    second = capsys.readouterr().out
    assert "Error at batch" not in second and "[Batch 0] grad norm:" in second
    assert t.optimizer.fused_launches == 4 and t.optimizer.accum_pending == 0


def test_load_state_dict_closes_an_open_cycle():
    optim = pkg("optim")
    p0, micro = _data(steps=2)
    pa, pb = _params(p0), _params(p0)
    oa, ob = optim.AvAdam(_groups(pa)), optim.AvAdam(_groups(pb))
    _accumulate(oa, pa, micro[:1])
    assert oa.accum_pending == 1
    oa.load_state_dict(ob.state_dict())                               # the open cycle belonged to the state that was replaced
    assert oa.accum_pending == 0 and not oa._accum_open
    _set_grads(pa, micro[1]); _set_grads(pb, micro[1])
    oa.step(); ob.step()                                              # a plain step on p.grad, at grad_scale 1, not on the stale accumulators
    _same_state(oa, pa, ob, pb)
