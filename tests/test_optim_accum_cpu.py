"""CPU: the accum_steps option of the trainer, the argument checks of av_grad_accum_multi (nothing is launched without a GPU) and the
checkpoint's refusal of an open accumulation cycle."""
import ctypes
import os
import types

import pytest

from conftest import pkg
from trainer_util import cpu_trainer as _trainer

VAR = "AVAMD_ACCUM_STEPS"


def test_options_row_resolves_argument_over_variable_over_default(monkeypatch):
    options = pkg("model.options")
    assert options.OPTIONS["accum_steps"][0] == VAR and options.OPTIONS["accum_steps"][2] == "1"
    monkeypatch.delenv(VAR, raising=False)
    assert options.resolve("accum_steps", None) == 1 and _trainer().accum_steps == 1
    monkeypatch.setenv(VAR, "4")
    assert options.resolve("accum_steps", None) == 4 and _trainer().accum_steps == 4
    assert options.resolve("accum_steps", 2) == 2 and _trainer(accum_steps=2).accum_steps == 2
    assert _trainer(accum_steps=1).accum_steps == 1                # an explicit argument wins over the variable
    monkeypatch.setenv(VAR, "many")
    with pytest.raises(ValueError):
        _trainer()


def test_values_below_one_are_refused(monkeypatch):
    options = pkg("model.options")
    monkeypatch.delenv(VAR, raising=False)
    for bad in (0, -1, -8):
        with pytest.raises(ValueError):
            options.check_accum(bad)
        with pytest.raises(ValueError):
            _trainer(accum_steps=bad)
    options.check_accum(1); options.check_accum(64)
    monkeypatch.setenv(VAR, "0")
    with pytest.raises(ValueError):
        _trainer()
    assert _trainer(accum_steps=3).accum_steps == 3                # the argument is looked at, not the variable


def test_one_step_per_batch_opens_no_cycle_and_has_no_accumulator(monkeypatch):
    monkeypatch.delenv(VAR, raising=False)
    for t in (_trainer(), _trainer(accum_steps=1), _trainer(accum_steps=4)):
        o = t.optimizer
        assert o.accum_pending == 0 and o.accum_mean is True
        assert o._accum == {} and o._accum_plans == {} and not o._accum_open
        assert t.flush_accumulated() is False                      # no open cycle: nothing to step
    sd = _trainer(accum_steps=4).optimizer.state_dict()
    assert set(sd) == {"state", "param_groups"} and sd["state"] == {}       # torch-Adam's format: nothing of the accumulation is in it


def test_both_libraries_export_av_grad_accum_multi():
    L = pkg("_lib")
    here = os.path.dirname(os.path.abspath(L.__file__))
    for name in ("libavhip.so", "libavhip_f16.so"):
        lib = ctypes.CDLL(os.path.join(here, name))
        assert hasattr(lib, "av_grad_accum_multi"), name
    sig = L.SIGNATURES["av_grad_accum_multi"]
    assert len(sig) == 8
    assert sig == [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]       # five tables, n_chunks, chunk_elems, stream


def test_grad_accum_multi_reports_bad_arguments():
    L = pkg("_lib")
    lib = L.lib()
    buf = (ctypes.c_double * 8)()
    P = ctypes.addressof(buf)                                      # non-null; never dereferenced

    def call(tables=(P, P, P, P, P), n_chunks=4, chunk_elems=65536):
        return lib.av_grad_accum_multi(*tables, n_chunks, chunk_elems, None)

    def failed(status):
        return status != 0 and b"av_grad_accum_multi: bad args" in lib.av_last_error()

    for i in range(5):                                             # ptrs, mode, sizes, chunk_tensor, chunk_start
        assert failed(call(tables=tuple(None if j == i else P for j in range(5)))), i
    assert failed(call(n_chunks=-1))
    assert failed(call(chunk_elems=0))
    assert failed(call(chunk_elems=-4))
    assert failed(call(n_chunks=0, chunk_elems=0))                 # the checks come before the early return


def test_no_chunks_is_ok_without_a_device():
    L = pkg("_lib")
    lib = L.lib()
    buf = (ctypes.c_double * 8)()
    P = ctypes.addressof(buf)
    assert lib.av_grad_accum_multi(P, P, P, P, P, 0, 65536, None) == 0


def test_checkpoint_refuses_an_open_cycle(monkeypatch):
    ckpt = pkg("checkpoint")
    monkeypatch.delenv(VAR, raising=False)
    t = _trainer(accum_steps=2)
    assert set(ckpt.KEYS) <= set(ckpt.checkpoint_dict(0, t))       # at a cycle boundary a checkpoint is what it is
    t.optimizer.accum_pending = 1
    with pytest.raises(ValueError, match=r"flush_accumulated\(\)"):
        ckpt.checkpoint_dict(0, t)
    with pytest.raises(ValueError, match=r"flush_accumulated\(\)"):
        ckpt.save_checkpoint(0, t, os.devnull)
    t.optimizer.accum_pending = 0
    assert ckpt.checkpoint_dict(3, t)["epoch"] == 3
    # an optimizer without the attribute (a plain torch one) is saved as before
    plain = types.SimpleNamespace(optimizer=types.SimpleNamespace(state_dict=lambda: {"state": {}}), visual_encoder=t.visual_encoder,
                                  audio_encoder=t.audio_encoder, fusion_module=t.fusion_module, decoder1=t.decoder1)
    assert ckpt.checkpoint_dict(1, plain)["optimizer"] == {"state": {}}


def test_load_state_dict_and_reset_state_close_an_open_cycle():
    import torch
    optim = pkg("optim")
    for close in (lambda o: o.load_state_dict(o.state_dict()), lambda o: o.reset_state()):
        w = torch.zeros(3, requires_grad=True)
        o = optim.AvAdam([w])
        o.accum_pending = 2; o._accum_open.add(id(w))                 # as two accumulate() calls leave them; no GPU is needed
        close(o)
        assert o.accum_pending == 0 and not o._accum_open
