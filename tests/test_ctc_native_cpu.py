"""CPU: the device CTC loss is part of the C-ABI of both libraries, rejects bad arguments with a status + message, has no CPU fallback,
and is OFF unless asked for (``native_ctc=True`` or AVAMD_NATIVE_CTC=1): the default CTC stays nn.CTCLoss, as BASELINE north_star says."""
import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer as _trainer

NAMES = ("av_ctc_loss_fwd", "av_ctc_loss_bwd")


def _libs():
    L = pkg("_lib"); P = pkg("precision")
    old = P.get_precision()
    out = []
    try:
        for mode, suffix in (("fp32", "libavhip.so"), ("fp16", "libavhip_f16.so")):
            P.set_precision(mode)
            lib = L.lib()
            assert lib._name.endswith(suffix)
            out.append(lib)
    finally:
        P.set_precision(old)
    return out


def test_both_symbols_exported_by_both_libraries_and_bound():
    L = pkg("_lib")
    for lib in _libs():
        for n in NAMES:
            assert n in L.SIGNATURES, n
            fn = getattr(lib, n)
            assert fn.argtypes is not None and len(fn.argtypes) == len(L.SIGNATURES[n])


def test_argument_errors_are_statuses_with_a_message():
    P = 4096                                     # any non-null address: argument checks come before a launch, nothing is dereferenced
    for lib in _libs():
        # (log_probs, stride_b, stride_t, targets, target_ld, input_lengths, target_lengths, B, T, V, S_max, blank, zero_infinity, nll, alpha, beta, stream)
        assert lib.av_ctc_loss_fwd(None, 80, 8, P, 2, P, P, 2, 10, 8, 5, 0, 1, P, None, None, None) != 0
        assert b"null" in lib.av_last_error()
        assert lib.av_ctc_loss_fwd(P, 80, 8, P, 2, P, P, 2, 10, 8, 5, 8, 1, P, None, None, None) != 0           # blank >= V
        assert b"blank" in lib.av_last_error()
        assert lib.av_ctc_loss_fwd(P, 80, 8, P, 2, P, P, 2, 0, 8, 5, 0, 1, P, None, None, None) != 0            # T < 1
        assert b"bad shape" in lib.av_last_error()
        assert lib.av_ctc_loss_fwd(P, 80, 4, P, 2, P, P, 2, 10, 8, 5, 0, 1, P, None, None, None) != 0           # time stride < row
        assert b"strides" in lib.av_last_error()
        assert lib.av_ctc_loss_fwd(P, 80, 8, P, 1, P, P, 2, 10, 8, 5, 0, 1, P, None, None, None) != 0           # target_ld < Lmax
        assert b"target_ld" in lib.av_last_error()
        assert lib.av_ctc_loss_fwd(P, 80, 8, P, 2, P, P, 2, 10, 8, 5, 0, 1, P, None, P, None) != 0              # beta without alpha
        assert lib.av_ctc_loss_bwd(P, 80, 8, P, 2, P, P, 2, 10, 8, 5, 0, P, P, P, P, None, None) != 0           # grad missing
        assert b"null" in lib.av_last_error()
        assert lib.av_ctc_loss_bwd(P, 80, 8, P, 2, P, P, 2, 10, 8, 5, -1, P, P, P, P, P, None) != 0
        assert b"blank" in lib.av_last_error()


def test_ops_ctc_loss_has_no_cpu_fallback_and_rejects_1d_targets():
    ops = pkg("ops")
    lp = torch.log_softmax(torch.randn(5, 2, 8), -1)
    tg = torch.tensor([[1, 2], [2, 1]])
    il, tl = torch.tensor([5, 5]), torch.tensor([2, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ctc_loss(lp, tg, il, tl)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg("model.decoder").CTCDecoder(16, 8, 0, native_ctc=True)(torch.zeros(2, 5, 16), tg, il, tl)


def test_native_ctc_is_off_by_default_and_follows_the_environment(monkeypatch):
    dm = pkg("model.decoder")
    monkeypatch.delenv("AVAMD_NATIVE_CTC", raising=False)
    assert dm.CTCDecoder(16, 8, 0).native_ctc is False
    t = _trainer()
    assert t.native_ctc is False and isinstance(t.ctc_loss, torch.nn.CTCLoss)
    monkeypatch.setenv("AVAMD_NATIVE_CTC", "0")
    assert dm.CTCDecoder(16, 8, 0).native_ctc is False and _trainer().native_ctc is False
    monkeypatch.setenv("AVAMD_NATIVE_CTC", "1")
    assert dm.CTCDecoder(16, 8, 0).native_ctc is True and _trainer().native_ctc is True
    # an explicit argument wins over the variable, in both directions
    assert dm.CTCDecoder(16, 8, 0, native_ctc=False).native_ctc is False and _trainer(native_ctc=False).native_ctc is False
    monkeypatch.delenv("AVAMD_NATIVE_CTC")
    assert dm.CTCDecoder(16, 8, 0, native_ctc=True).native_ctc is True and _trainer(native_ctc=True).native_ctc is True
