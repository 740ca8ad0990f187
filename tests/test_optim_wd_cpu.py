"""CPU: the cosine schedule law, the weight-decay / schedule options of the trainer and of optim.AvAdam, and the argument checks of
av_adam_multi_wd (nothing is launched without a GPU)."""
import ctypes
import math
import os

import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer as _trainer


def _hf_cosine_lambda(warmup, total, num_cycles=0.5):
    """transformers.optimization.get_cosine_schedule_with_warmup's lambda, written out."""
    def f(step):
        if step < warmup:
            return float(step) / float(max(1, warmup))
        progress = float(step - warmup) / float(max(1, total - warmup))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))
    return f


@pytest.mark.parametrize("warmup,total", [(3, 7), (0, 5), (2, 3), (10, 50), (1, 1000)])
def test_cosine_lr_multiplier_is_lambdalr_with_the_hf_lambda(warmup, total):
    optim = pkg("optim")
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([p], lr=1.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, _hf_cosine_lambda(warmup, total))
    for k in range(total + 1):                                      # every k in 0..total
        want = opt.param_groups[0]["lr"]                            # the rate optimizer step k runs at
        assert optim.lr_multiplier(k, warmup, total, schedule="cosine") == want, (k, want)
        opt.step(); sched.step()
    assert optim.lr_multiplier(total, warmup, total, schedule="cosine") == 0.0
    for k in (total + 1, total + 2, 2 * total, 3 * total + 1):      # HF's lambda rises again there; this one stays at 0
        assert optim.lr_multiplier(k, warmup, total, schedule="cosine") == 0.0, k
    if (warmup, total) == (3, 7):
        assert optim.lr_multiplier(3, 3, 7, schedule="cosine") == 1.0
        assert optim.lr_multiplier(5, 3, 7, schedule="cosine") == 0.5 * (1.0 + math.cos(math.pi * 0.5))
        assert abs(optim.lr_multiplier(5, 3, 7, schedule="cosine") - 0.5) < 1e-16


@pytest.mark.parametrize("warmup,total", [(3, 7), (3, 0), (0, 5), (0, 0)])
def test_linear_lr_multiplier_is_what_it_was(warmup, total):
    optim = pkg("optim")

    def was(k):                                                     # the law before the schedule argument, statement for statement
        if k < warmup:
            return k / warmup
        if total == 0:
            return 1.0
        return max(0.0, (total - k) / (total - warmup))

    for k in range(12):
        assert optim.lr_multiplier(k, warmup, total) == optim.lr_multiplier(k, warmup, total, schedule="linear") == was(k)
    assert optim.lr_multiplier(4, warmup_steps=3, total_steps=7, schedule="linear") == 0.75


def test_lr_multiplier_rejects_bad_schedules():
    optim = pkg("optim")
    for bad in ("cos", "", None, 1):
        with pytest.raises(ValueError):
            optim.lr_multiplier(1, 3, 7, schedule=bad)
    for warmup, total in ((0, 0), (3, 0), (3, 3), (5, 2)):
        with pytest.raises(ValueError):
            optim.lr_multiplier(1, warmup, total, schedule="cosine")


def test_both_libraries_export_av_adam_multi_wd():
    L = pkg("_lib")
    here = os.path.dirname(os.path.abspath(L.__file__))
    for name in ("libavhip.so", "libavhip_f16.so"):
        lib = ctypes.CDLL(os.path.join(here, name))
        assert hasattr(lib, "av_adam_multi_wd"), name
    ema, wd = L.SIGNATURES["av_adam_multi_ema"], L.SIGNATURES["av_adam_multi_wd"]
    assert len(wd) == len(ema) + 2
    assert wd[:len(ema) - 1] == ema[:-1] and wd[-3:] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]     # ..., weight_decay, lr_schedule, stream


def test_adam_multi_wd_reports_bad_arguments():
    L = pkg("_lib")
    lib = L.lib()
    buf = (ctypes.c_double * 8)()
    P = ctypes.addressof(buf)                                      # non-null, aligned enough for the checks; never dereferenced

    def call(tables=P, max_norm=0.0, warmup=0, total=0, state=P, ema_ptrs=None, decay=0.0, ema_state=None, wd=P, schedule=0):
        return lib.av_adam_multi_wd(tables, tables, tables, tables, tables, 4, 65536, tables, tables, 2, 1.0, None, 1.0, 1.0, 1,
                                    max_norm, warmup, total, P, 64, state, ema_ptrs, None, None, None, None, 0, decay, 0, ema_state,
                                    wd, schedule, None)

    def failed(status, *words):
        msg = lib.av_last_error()
        return status != 0 and b"av_adam_multi_wd" in msg and all(w in msg for w in words)

    assert P % 16 == 0
    for off in (1, 2, 3):
        assert failed(call(wd=P + off), b"weight_decay", b"4-byte aligned")
    for bad in (-1, 2, 7):
        assert failed(call(schedule=bad, warmup=2, total=6), b"lr_schedule")
    assert failed(call(schedule=1), b"cosine", b"total_steps")                          # cosine without total_steps
    assert failed(call(schedule=1, warmup=3), b"cosine", b"total_steps")
    assert failed(call(schedule=1, warmup=2, total=6, state=None), b"cosine", b"state block")
    # the existing checks hold under the new name
    assert failed(call(tables=None), b"bad args")
    assert failed(call(max_norm=-1.0), b"max_norm")
    assert failed(call(warmup=3, total=3), b"total_steps")
    assert failed(call(schedule=1, warmup=3, total=3), b"total_steps")
    assert failed(call(max_norm=1.0, state=None), b"state block")
    assert failed(call(warmup=3, state=None), b"state block")
    assert failed(call(decay=1.5), b"ema_decay must be in [0, 1)")
    assert failed(call(decay=0.0, ema_ptrs=P), b"EMA tables without")
    assert failed(call(decay=0.9, ema_ptrs=None), b"EMA pointer table")
    assert failed(call(decay=0.9, ema_ptrs=P, ema_state=None), b"EMA state block")


VARS = ("AVAMD_WEIGHT_DECAY", "AVAMD_LR_SCHEDULE", "AVAMD_WARMUP_STEPS", "AVAMD_TOTAL_STEPS")


def _opts(t):
    o = t.optimizer
    assert (o.lr_schedule, o.warmup_steps, o.total_steps) == (t.lr_schedule, t.warmup_steps, t.total_steps)
    assert all(g["weight_decay"] == t.weight_decay for g in o.param_groups) and len(o.param_groups) == 4
    assert o.decay_1d is False                                      # the trainer keeps the 1-D rule on
    return t.weight_decay, t.lr_schedule, t.total_steps


def test_trainer_decays_and_follows_the_cosine_only_when_asked(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    assert _opts(_trainer()) == (0.0, "linear", 0)
    monkeypatch.setenv("AVAMD_WEIGHT_DECAY", "0.01"); monkeypatch.setenv("AVAMD_LR_SCHEDULE", "cosine")
    with pytest.raises(ValueError):
        _trainer()                                                  # cosine without total_steps
    monkeypatch.setenv("AVAMD_TOTAL_STEPS", "50")
    assert _opts(_trainer()) == (0.01, "cosine", 50)                # the variables are parsed
    assert _opts(_trainer(weight_decay=0.0, lr_schedule="linear")) == (0.0, "linear", 50)      # an explicit argument wins over the variable
    assert _opts(_trainer(weight_decay=0.1)) == (0.1, "cosine", 50)
    assert _opts(_trainer(lr_schedule="linear", total_steps=0)) == (0.01, "linear", 0)
    with pytest.raises(ValueError):
        _trainer(total_steps=0)                                     # the variable still asks for the cosine
    monkeypatch.setenv("AVAMD_LR_SCHEDULE", "cosin")
    with pytest.raises(ValueError):
        _trainer()
    monkeypatch.setenv("AVAMD_LR_SCHEDULE", "linear"); monkeypatch.setenv("AVAMD_WEIGHT_DECAY", "-0.5")
    with pytest.raises(ValueError):
        _trainer()
    monkeypatch.setenv("AVAMD_WEIGHT_DECAY", "much")
    with pytest.raises(ValueError):
        _trainer()
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    assert _opts(_trainer(weight_decay=0.01, lr_schedule="cosine", warmup_steps=2, total_steps=6)) == (0.01, "cosine", 6)
    for bad in (dict(weight_decay=-0.01), dict(weight_decay=float("nan")), dict(weight_decay=float("inf")), dict(lr_schedule="tri-stage"),
                dict(lr_schedule="cosine"), dict(lr_schedule="cosine", warmup_steps=4), dict(lr_schedule="cosine", warmup_steps=4, total_steps=4)):
        with pytest.raises(ValueError):
            _trainer(**bad)


def test_options_table_has_the_two_rows():
    options = pkg("model.options")
    assert options.OPTIONS["weight_decay"][0] == "AVAMD_WEIGHT_DECAY" and options.OPTIONS["weight_decay"][2] == "0"
    assert options.OPTIONS["lr_schedule"][0] == "AVAMD_LR_SCHEDULE" and options.OPTIONS["lr_schedule"][2] == "linear"
    options.check_schedule("linear", 0); options.check_schedule("cosine", 1)
    for bad in (("cosine", 0), ("exp", 10)):
        with pytest.raises(ValueError):
            options.check_schedule(*bad)


def _leaves():
    return [torch.zeros(3, 2, requires_grad=True), torch.zeros(4, requires_grad=True)]


def test_avadam_constructor_and_groups_are_validated():
    optim = pkg("optim")
    o = optim.AvAdam(_leaves())
    assert o.defaults["weight_decay"] == 0.0 and o.param_groups[0]["weight_decay"] == 0.0
    assert o.lr_schedule == "linear" and o.decay_1d is False and not o.scheduled
    w, b = _leaves()
    o = optim.AvAdam([{"params": [w], "weight_decay": 0.25}, {"params": [b]}], weight_decay=0.5, decay_1d=True, lr_schedule="cosine",
                     warmup_steps=2, total_steps=6)
    assert [g["weight_decay"] for g in o.param_groups] == [0.25, 0.5]                   # a per-group key, the constructor's value as default
    assert o.lr_schedule == "cosine" and o.decay_1d is True and o.scheduled
    assert o.state_dict()["param_groups"][0]["weight_decay"] == 0.25
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            optim.AvAdam(_leaves(), weight_decay=bad)
        with pytest.raises(ValueError):
            optim.AvAdam([{"params": _leaves(), "weight_decay": bad}])
        with pytest.raises(ValueError):
            optim.check_weight_decay(bad)
        o = optim.AvAdam(_leaves()[:1])
        with pytest.raises(ValueError):
            o.add_param_group({"params": _leaves()[1:], "weight_decay": bad})
    assert optim.check_weight_decay(0) == 0.0 and optim.check_weight_decay("0.5") == 0.5
    for bad in ("cos", "Cosine", "", None, 0):
        with pytest.raises(ValueError):
            optim.AvAdam(_leaves(), lr_schedule=bad, total_steps=5)
    for kw in ({}, dict(warmup_steps=3), dict(warmup_steps=3, total_steps=3)):
        with pytest.raises(ValueError):
            optim.AvAdam(_leaves(), lr_schedule="cosine", **kw)     # cosine without total_steps above the warmup
    assert optim.check_lr_schedule("linear", 0, 0) == 0 and optim.check_lr_schedule("cosine", 2, 6) == 1


def test_a_state_dict_without_the_key_loads_and_falls_back_to_the_constructor_default():
    optim = pkg("optim")
    o = optim.AvAdam(_leaves(), weight_decay=0.125)
    sd = o.state_dict()
    for g in sd["param_groups"]:
        del g["weight_decay"]                                       # as written before weight_decay existed
    fresh = optim.AvAdam(_leaves(), weight_decay=0.125)
    fresh.load_state_dict(sd)
    assert all(g.get("weight_decay", fresh.defaults["weight_decay"]) == 0.125 for g in fresh.param_groups)
    assert fresh._collect() == ([], None, None)                     # no gradients: nothing to launch, and no KeyError on a missing key
