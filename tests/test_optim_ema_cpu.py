"""CPU: the EMA decay law, the trainer's EMA switches and the argument checks of av_adam_multi_ema / av_param_swap_multi
(nothing is launched without a GPU)."""
import ctypes

import pytest

from conftest import pkg
from trainer_util import cpu_trainer as _trainer


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_ema_decay_is_the_written_out_law(decay, warmup):
    optim = pkg("optim")
    for k in range(31):
        if k == 0:
            want = 0.0                                              # the first update copies the parameters
        elif warmup:
            want = min(decay, (1 + k) / (10 + k))
        else:
            want = decay
        assert optim.ema_decay(k, decay, warmup) == want, (k, decay, warmup)
    if warmup and decay == 0.999:
        assert [optim.ema_decay(k, decay, True) for k in (1, 2, 30)] == [2 / 11, 3 / 12, 31 / 40]
    if warmup and decay == 0.5:
        assert optim.ema_decay(7, decay, True) == 8 / 17 and optim.ema_decay(8, decay, True) == 0.5       # 9/18 reaches the decay


def test_check_ema_rejects_bad_decays():
    optim = pkg("optim")
    assert optim.check_ema(0.0, False) == (0.0, False) and optim.check_ema(0.999, 1) == (0.999, True)
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            optim.check_ema(bad, False)
        with pytest.raises(ValueError):
            optim.AvAdam([__import__("torch").zeros(1, requires_grad=True)], ema_decay=bad)


def _opts(t):
    o = t.optimizer
    assert (o.ema_decay, o.ema_warmup) == (t.ema_decay, t.ema_warmup) and o.averaging == (o.ema_decay > 0)
    return o.ema_decay, o.ema_warmup, t.eval_ema


VARS = ("AVAMD_EMA_DECAY", "AVAMD_EMA_WARMUP", "AVAMD_EVAL_EMA")


def test_trainer_averages_only_when_asked(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    t = _trainer()
    assert _opts(t) == (0.0, False, False)
    sd = t.optimizer.state_dict()
    assert t.optimizer.EMA_KEY == "av_ema_step" and "av_ema_step" not in sd       # EMA off: the dict is the one it was
    monkeypatch.setenv("AVAMD_EMA_DECAY", "0.999"); monkeypatch.setenv("AVAMD_EMA_WARMUP", "1"); monkeypatch.setenv("AVAMD_EVAL_EMA", "1")
    assert _opts(_trainer()) == (0.999, True, True)
    assert _opts(_trainer(ema_decay=0.5, ema_warmup=False, eval_ema=False)) == (0.5, False, False)   # an explicit argument wins
    assert _opts(_trainer(ema_decay=0.9)) == (0.9, True, True)
    with pytest.raises(ValueError):
        _trainer(ema_decay=0.0)                                     # the variable still asks for eval_ema: nothing to evaluate
    assert _opts(_trainer(ema_decay=0.0, eval_ema=False)) == (0.0, True, False)
    for v in VARS:
        monkeypatch.delenv(v)
    assert _opts(_trainer(ema_decay=0.99, eval_ema=True)) == (0.99, False, True)
    assert _opts(_trainer(ema_warmup=True)) == (0.0, True, False)
    t = _trainer(ema_decay=0.99)
    assert t.optimizer.state_dict()["av_ema_step"] == 0 and t.optimizer.ema_step() == 0 and t.optimizer.last_ema_decay is None
    for bad in (dict(eval_ema=True), dict(eval_ema=True, ema_decay=0.0), dict(ema_decay=-0.5), dict(ema_decay=1.0),
                dict(ema_decay=float("nan"))):
        with pytest.raises(ValueError):
            _trainer(**bad)


def test_adam_multi_ema_reports_bad_arguments():
    L = pkg("_lib")
    lib = L.lib()
    buf = (ctypes.c_double * 8)()
    P = ctypes.addressof(buf)                                      # non-null, aligned enough for the checks; never dereferenced

    def call(tables=P, max_norm=0.0, state=P, ema_ptrs=P, only=P, n_only=1, decay=0.9, warmup=0, ema_state=P):
        return lib.av_adam_multi_ema(tables, tables, tables, tables, tables, 4, 65536, tables, tables, 2, 1.0, None, 1.0, 1.0, 1,
                                     max_norm, 0, 0, P, 64, state, ema_ptrs, only, only, only, only, n_only, decay, warmup, ema_state, None)

    assert P % 16 == 0
    assert call(tables=None) != 0 and b"av_adam_multi_ema: bad args" in lib.av_last_error()
    assert call(max_norm=-1.0) != 0 and b"max_norm" in lib.av_last_error()             # the checks of av_adam_multi_ex still hold
    assert call(max_norm=1.0, state=None) != 0 and b"state block" in lib.av_last_error()
    for bad in (-0.1, 1.0, 2.0, float("nan")):
        assert call(decay=bad) != 0 and b"ema_decay must be in [0, 1)" in lib.av_last_error()
    assert call(ema_ptrs=None) != 0 and b"EMA pointer table" in lib.av_last_error()
    assert call(only=None) != 0 and b"EMA-only tables" in lib.av_last_error()
    assert call(n_only=-1) != 0 and b"EMA-only tables" in lib.av_last_error()
    assert call(ema_state=None) != 0 and b"EMA state block" in lib.av_last_error()
    assert call(ema_state=P + 2) != 0 and b"4-byte aligned" in lib.av_last_error()
    assert call(decay=0.0) != 0 and b"EMA tables without" in lib.av_last_error()        # decay 0 means off: tables make no sense
    assert call(decay=0.0, ema_ptrs=None, only=None, n_only=1) != 0 and b"EMA tables without" in lib.av_last_error()


def test_param_swap_multi_reports_bad_arguments():
    L = pkg("_lib")
    lib = L.lib()
    buf = (ctypes.c_double * 8)()
    P = ctypes.addressof(buf)
    for args in ((None, P, P, P, 1, 65536), (P, None, P, P, 1, 65536), (P, P, None, P, 1, 65536), (P, P, P, None, 1, 65536),
                 (P, P, P, P, -1, 65536), (P, P, P, P, 1, 0)):
        assert lib.av_param_swap_multi(*args, None) != 0 and b"av_param_swap_multi: bad args" in lib.av_last_error()
    assert lib.av_param_swap_multi(P, P, P, P, 0, 65536, None) == 0                     # nothing to swap: no launch


def test_both_libraries_export_the_ema_entry_points():
    import os
    L = pkg("_lib")
    here = os.path.dirname(os.path.abspath(L.__file__))
    for name in ("libavhip.so", "libavhip_f16.so"):
        lib = ctypes.CDLL(os.path.join(here, name))
        assert hasattr(lib, "av_adam_multi_ema") and hasattr(lib, "av_param_swap_multi"), name
    assert len(L.SIGNATURES["av_adam_multi_ema"]) == len(L.SIGNATURES["av_adam_multi_ex"]) + 9
    assert len(L.SIGNATURES["av_param_swap_multi"]) == 7
