"""CPU: the learning-rate schedule law, the trainer's clipping / schedule options and the argument checks of av_adam_multi_ex
(nothing is launched without a GPU)."""
import ctypes

import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer as _trainer


def _hf_lambda(warmup, total):
    """transformers.optimization.get_linear_schedule_with_warmup's lambda, written out; total == 0: get_constant_schedule_with_warmup's."""
    def f(step):
        if step < warmup:
            return float(step) / float(max(1, warmup))
        if total == 0:
            return 1.0
        return max(0.0, float(total - step) / float(max(1, total - warmup)))
    return f


@pytest.mark.parametrize("warmup,total", [(3, 7), (3, 0), (0, 5), (0, 0)])
def test_lr_multiplier_is_lambdalr_with_the_hf_lambda(warmup, total):
    optim = pkg("optim")
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([p], lr=1.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, _hf_lambda(warmup, total))
    got, want = [], []
    for k in range(10):
        want.append(opt.param_groups[0]["lr"])                     # the rate optimizer step k runs at
        got.append(optim.lr_multiplier(k, warmup, total))
        opt.step(); sched.step()
    assert got == want, (got, want)
    if (warmup, total) == (3, 7):
        assert got == [0, 1 / 3, 2 / 3, 1, .75, .5, .25, 0, 0, 0]
    if (warmup, total) == (0, 0):
        assert got == [1.0] * 10


def _opts(t):
    o = t.optimizer
    assert (o.max_grad_norm, o.warmup_steps, o.total_steps) == (t.max_grad_norm, t.warmup_steps, t.total_steps)
    return o.max_grad_norm, o.warmup_steps, o.total_steps


def test_trainer_clips_and_schedules_only_when_asked(monkeypatch):
    for v in ("AVAMD_CLIP_NORM", "AVAMD_WARMUP_STEPS", "AVAMD_TOTAL_STEPS"):
        monkeypatch.delenv(v, raising=False)
    t = _trainer()
    assert _opts(t) == (0.0, 0, 0) and not t.optimizer.clipping and not t.optimizer.scheduled
    assert t.optimizer.SCHEDULE_KEY not in t.optimizer.state_dict()
    monkeypatch.setenv("AVAMD_CLIP_NORM", "1.0"); monkeypatch.setenv("AVAMD_WARMUP_STEPS", "10"); monkeypatch.setenv("AVAMD_TOTAL_STEPS", "50")
    t = _trainer()
    assert _opts(t) == (1.0, 10, 50) and t.optimizer.clipping and t.optimizer.scheduled
    assert _opts(_trainer(max_grad_norm=0.0, warmup_steps=0, total_steps=0)) == (0.0, 0, 0)     # an explicit argument wins over the variable
    assert _opts(_trainer(max_grad_norm=2.5)) == (2.5, 10, 50)
    for v in ("AVAMD_CLIP_NORM", "AVAMD_WARMUP_STEPS", "AVAMD_TOTAL_STEPS"):
        monkeypatch.delenv(v)
    assert _opts(_trainer(max_grad_norm=0.5, warmup_steps=3, total_steps=7)) == (0.5, 3, 7)
    assert _opts(_trainer(warmup_steps=3)) == (0.0, 3, 0)
    for bad in (dict(max_grad_norm=-1.0), dict(max_grad_norm=float("nan")), dict(warmup_steps=-1), dict(total_steps=3, warmup_steps=3)):
        with pytest.raises(ValueError):
            _trainer(**bad)


def test_adam_multi_ex_reports_bad_arguments():
    L = pkg("_lib")
    lib = L.lib()
    buf = (ctypes.c_double * 8)()
    P = ctypes.addressof(buf)                                      # non-null, 16-byte aligned enough for the checks; never dereferenced

    def call(tables=P, max_norm=0.0, warmup=0, total=0, ws=P, ws_bytes=64, state=P, n_chunks=4):
        return lib.av_adam_multi_ex(tables, tables, tables, tables, tables, n_chunks, 65536, tables, tables, 2, 1.0, None, 1.0, 1.0, 1,
                                    max_norm, warmup, total, ws, ws_bytes, state, None)

    assert P % 16 == 0
    assert call(tables=None, max_norm=1.0) != 0 and b"bad args" in lib.av_last_error()
    assert call(max_norm=-1.0) != 0 and b"max_norm" in lib.av_last_error()
    assert call(max_norm=float("nan")) != 0 and b"max_norm" in lib.av_last_error()
    assert call(warmup=3, total=3) != 0 and b"total_steps" in lib.av_last_error()
    assert call(warmup=5, total=2) != 0 and b"total_steps" in lib.av_last_error()
    assert call(warmup=-1) != 0 and b"warmup_steps" in lib.av_last_error()
    assert call(max_norm=1.0, ws=None) != 0 and b"workspace" in lib.av_last_error()
    assert call(max_norm=1.0, ws_bytes=31) != 0 and b"workspace" in lib.av_last_error()      # 4 chunks need 32 bytes
    assert call(max_norm=1.0, state=None) != 0 and b"state block" in lib.av_last_error()
    assert call(warmup=3, state=None) != 0 and b"state block" in lib.av_last_error()
    n = ctypes.c_longlong(0)
    assert lib.av_grad_norm_workspace_bytes(4, ctypes.byref(n)) == 0 and n.value == 32
    assert lib.av_grad_norm_workspace_bytes(-1, ctypes.byref(n)) != 0
    assert lib.av_grad_norm_workspace_bytes(4, None) != 0
