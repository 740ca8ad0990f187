"""CPU: the n-best CTC entry points are part of the C-ABI of both libraries and reject bad arguments with a status + message before any
launch; ops.ctc_nbest_nll has no CPU fallback; mwer.mwer_loss on host tensors follows the law of tests/mwer_ref.py (float64 torch) and
has the structure the law promises (a gradient that sums to zero over the list, nothing from equal errors, nothing and no NaN from an
utterance without hypotheses); the trainer's MWER term is off unless asked for."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mwer_ref
from conftest import pkg
from test_ctc_native_cpu import _libs, _trainer

NAMES = ("av_ctc_nbest_fwd", "av_ctc_nbest_bwd")
EPS32 = float(np.finfo(np.float32).eps)


def test_both_symbols_in_header_signatures_and_both_libraries():
    import os
    L = pkg("_lib")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "av_hip.h"), encoding="utf-8").read()
    for n in NAMES:
        assert ("int " + n + "(") in header, n
        assert n in L.SIGNATURES, n
    for lib in _libs():
        for n in NAMES:
            fn = getattr(lib, n)
            assert fn.argtypes is not None and len(fn.argtypes) == len(L.SIGNATURES[n])


def test_argument_errors_are_statuses_with_a_message():
    P = 4096                                     # any non-null address: argument checks come before a launch, nothing is dereferenced
    # (log_probs, stride_b, stride_t, hyp_ids, hyp_ld_b, hyp_ld_n, hyp_lens, input_lengths, B, N, T, V, S_max, blank, nll, alpha, beta, stream)
    good = [P, 80, 8, P, 8, 2, P, P, 2, 4, 10, 8, 5, 0, P, None, None, None]
    fwd_cases = [
        ({0: None}, b"null"), ({3: None}, b"null"), ({6: None}, b"null"), ({7: None}, b"null"), ({14: None}, b"null"),
        ({16: P}, b"log_beta without log_alpha"),
        ({9: 0}, b"hypotheses"), ({9: 65}, b"hypotheses"),
        ({8: 0}, b"bad shape"), ({8: 65536}, b"grid limit"), ({10: 0}, b"bad shape"), ({11: 0}, b"bad shape"),
        ({13: 8}, b"blank"), ({13: -1}, b"blank"),
        ({12: 4}, b"odd"), ({12: 0}, b"odd"),
        ({5: 1}, b"hyp_ld_n"),
        ({4: 7}, b"hyp_ld_b"),
        ({2: 4}, b"strides"), ({1: 79}, b"strides"),
        ({12: 2001, 5: 1000, 4: 4000}, b"LDS"),
    ]
    for lib in _libs():
        for change, word in fwd_cases:
            a = list(good)
            for k, v in change.items():
                a[k] = v
            assert lib.av_ctc_nbest_fwd(*a) != 0, change
            assert word in lib.av_last_error(), (change, lib.av_last_error())
        # (the same inputs ..., blank, nll, alpha, beta, grad_nll, grad, stream)
        bgood = good[:14] + [P, P, P, P, P, None]
        for k in (0, 3, 6, 7, 14, 15, 16, 17, 18):
            a = list(bgood); a[k] = None
            assert lib.av_ctc_nbest_bwd(*a) != 0, k
            assert b"null" in lib.av_last_error()
        for change, word in [({9: 65}, b"hypotheses"), ({8: 65536}, b"grid limit"), ({13: 8}, b"blank"), ({12: 4}, b"odd"), ({5: 1}, b"hyp_ld_n"),
                             ({4: 7}, b"hyp_ld_b"), ({2: 4}, b"strides"),
                             ({11: 20000, 2: 20000, 1: 200000}, b"LDS"),                       # one [V + S_max] row alone is past 64 KiB
                             ({9: 64, 12: 401, 5: 200, 4: 12800}, b"LDS")]:                    # 3 N Lmax label ints are
            a = list(bgood)
            for k, v in change.items():
                a[k] = v
            assert lib.av_ctc_nbest_bwd(*a) != 0, change
            assert word in lib.av_last_error(), (change, lib.av_last_error())


def test_ops_ctc_nbest_nll_has_no_cpu_fallback():
    ops = pkg("ops")
    lp = torch.log_softmax(torch.randn(2, 5, 8), -1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ctc_nbest_nll(lp, torch.ones((2, 3, 2), dtype=torch.int32), torch.full((2, 3), 2), torch.tensor([5, 5]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg("beam_search").nbest_on_device(lp, 4, 0, nbest=2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the host law, B = 3, N = 4, T = 12, V = 7
# ---------------------------------------------------------------------------------------------------------------------------------
B, N, T, V, BLANK = 3, 4, 12, 7, 0


def _case(seed=3):
    g = torch.Generator().manual_seed(seed)
    lp = F.log_softmax(torch.randn(B, T, V, generator=g) * 1.5, -1)
    refs = torch.randint(1, V, (B, 6), generator=g)
    return lp, refs, torch.tensor([6, 4, 2]), torch.tensor([12, 9, 5])


def _ref_loss(lp, refs, rl, il, ids, lens, reduction="mean"):
    counts = pkg("error_rate").error_counts(refs, ids, rl, lens, ref_skip=BLANK, hyp_skip=BLANK)[:, :, 0]
    x = lp.double().requires_grad_()
    loss, det = mwer_ref.mwer(x, ids, lens, il, BLANK, counts[..., :3].sum(-1), counts[..., 3] >= 0, reduction)
    loss.sum().backward()
    return loss.detach(), x.grad, det


def _tol(d64, errors):
    """float32 rounding of the float64 value: nll is a sum of T terms (|nll| eps T / 2 absolute), the posterior is exp of differences of
    nll, the risk a sum of N products with errors up to Emax."""
    return 8 * EPS32 * T * float(d64["nll"][torch.isfinite(d64["nll"])].abs().max()) * max(float(errors.max()), 1.0)


def test_host_mwer_loss_equals_the_float64_reference():
    mw = pkg("mwer")
    lp, refs, rl, il = _case()
    x = lp.clone().requires_grad_()
    loss, det = mw.mwer_loss(x, refs, rl, il, BLANK, nbest=N, beam_width=6, level="token", return_details=True)
    loss.backward()
    loss = loss.detach()
    assert det["ids"].shape == (B, N, T) and det["lens"].shape == (B, N) and int((det["lens"] >= 0).sum()) == B * N
    want, g64, d64 = _ref_loss(lp, refs, rl, il, det["ids"], det["lens"])
    tol = _tol(d64, det["errors"])
    print(f"\nhost mwer: loss {float(loss):.7f} ref {float(want):.7f} |d| {abs(float(loss) - float(want)):.2e} (tol {tol:.2e})")
    assert abs(float(loss) - float(want)) < tol
    assert float((det["posterior"].double() - d64["posterior"]).abs().max()) < tol
    assert float((x.grad.double() - g64).abs().max()) < tol
    assert torch.equal(det["errors"], pkg("error_rate").error_counts(refs, det["ids"], rl, det["lens"], ref_skip=0, hyp_skip=0)[:, :, 0, :3].sum(-1))
    for red in ("sum", "none"):
        got = mw.mwer_loss(lp, refs, rl, il, BLANK, nbest=N, beam_width=6, level="token", reduction=red)
        assert float((got.double() - _ref_loss(lp, refs, rl, il, det["ids"], det["lens"], red)[0]).abs().max()) < tol * B


def test_risk_gradient_sums_to_zero_and_equal_errors_give_nothing():
    mw = pkg("mwer")
    g = torch.Generator().manual_seed(11)
    nll = (torch.rand(B, N, generator=g) * 20 + 1).requires_grad_()
    errors = torch.randint(0, 9, (B, N), generator=g)
    counted = torch.ones(B, N, dtype=torch.bool)
    risk, post, live = mw.risk_from_nll(nll, errors, counted)
    risk.sum().backward()
    d_logit = -nll.grad                                              # d risk / d (-nll)
    assert float(d_logit.abs().max()) > 1e-3
    assert float(d_logit.sum(1).abs().max()) < 16 * EPS32 * float(errors.max())
    assert float((post.detach().sum(1) - 1).abs().max()) < 8 * EPS32
    nll.grad = None
    risk, _, _ = mw.risk_from_nll(nll, torch.full((B, N), 5), counted)
    risk.sum().backward()
    assert float(risk.detach().abs().max()) < 16 * EPS32 * 5 and float(nll.grad.abs().max()) < 16 * EPS32 * 5


def test_equal_errors_through_the_whole_host_law():
    mw = pkg("mwer")
    lp, _, _, il = _case()
    # every hypothesis is the same distance from the reference: one token each, none of them the reference's
    ids = torch.tensor([[[1], [2], [3], [4]]] * B, dtype=torch.int32)
    lens = torch.ones((B, N), dtype=torch.long)
    refs, rl = torch.full((B, 1), 6), torch.ones(B, dtype=torch.long)
    x = lp.clone().requires_grad_()
    loss, det = mw.mwer_loss(x, refs, rl, il, BLANK, level="token", hyps=(ids, lens), return_details=True)
    loss.backward()
    assert torch.equal(det["errors"], torch.ones((B, N), dtype=det["errors"].dtype))
    assert abs(float(loss.detach())) < 16 * EPS32 and float(x.grad.abs().max()) < 16 * EPS32


def test_all_out_utterance_gives_zero_and_no_nan_and_hyps_are_used_verbatim():
    mw = pkg("mwer")
    lp, refs, rl, il = _case()
    # utterance 1: absent, an id outside [0, V), longer than the id block, and [2, 2, 2, 2, 2] at T_b = 9 exactly feasible -> make T_b = 8
    il = torch.tensor([12, 8, 5])
    ids = torch.tensor([[[1, 2, 3, 0, 0], [4, 4, 1, 0, 0], [5, 0, 0, 0, 0], [0, 0, 0, 0, 0]],
                        [[1, 2, 3, 0, 0], [1, 9, 3, 0, 0], [1, 2, 3, 4, 5], [2, 2, 2, 2, 2]],
                        [[3, 0, 0, 0, 0], [3, 3, 0, 0, 0], [1, 2, 0, 0, 0], [6, 6, 6, 0, 0]]], dtype=torch.int32)
    lens = torch.tensor([[3, 3, 1, 0], [-1, 3, 6, 5], [1, 2, 2, 3]])
    x = lp.clone().requires_grad_()
    loss, det = mw.mwer_loss(x, refs, rl, il, BLANK, level="token", hyps=(ids, lens), reduction="none", return_details=True)
    loss.sum().backward()
    assert det["ids"] is not None and torch.equal(det["ids"].cpu().to(torch.int32), ids) and torch.equal(det["lens"].cpu().long(), lens)
    assert bool(torch.isinf(det["nll"][1]).all()) and bool(torch.isfinite(det["nll"][0]).all())
    loss = loss.detach()
    assert float(loss[1]) == 0.0 and float(x.grad[1].abs().max()) == 0.0 and float(det["posterior"][1].abs().max()) == 0.0
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(x.grad).all())
    assert float(x.grad[0].abs().max()) > 0 and float(x.grad[2].abs().max()) > 0
    # utterance 2: [6, 6, 6] needs 5 frames = T_b: in; [3, 3] and the others too
    assert bool(torch.isfinite(det["nll"][2]).all())
    want, g64, d64 = _ref_loss(lp, refs, rl, il, ids, lens, "none")
    tol = _tol(d64, det["errors"])
    assert float((loss.double() - want).abs().max()) < tol and float((x.grad.double() - g64).abs().max()) < tol
    assert torch.equal(torch.isinf(d64["nll"]), torch.isinf(det["nll"]))
    with pytest.raises(ValueError, match="table"):
        mw.mwer_loss(lp, refs, rl, il, BLANK, level="word")
    with pytest.raises(ValueError, match="level"):
        mw.mwer_loss(lp, refs, rl, il, BLANK, level="sentence")


# ---------------------------------------------------------------------------------------------------------------------------------
def test_trainer_mwer_is_off_by_default_follows_the_environment_and_validates(monkeypatch):
    for k in ("AVAMD_MWER_WEIGHT", "AVAMD_MWER_NBEST", "AVAMD_MWER_BEAM"):
        monkeypatch.delenv(k, raising=False)
    t = _trainer()
    assert t.mwer_weight == 0 and t.mwer_nbest == 4 and t.mwer_beam == 8 and t.mwer_level == "word" and t._mwer_table is None
    monkeypatch.setenv("AVAMD_MWER_WEIGHT", "0.25"); monkeypatch.setenv("AVAMD_MWER_NBEST", "3"); monkeypatch.setenv("AVAMD_MWER_BEAM", "5")
    t = _trainer()
    assert t.mwer_weight == 0.25 and t.mwer_nbest == 3 and t.mwer_beam == 5
    t = _trainer(mwer_weight=0.0, mwer_nbest=2, mwer_beam=2, mwer_level="token")           # explicit arguments win
    assert t.mwer_weight == 0 and t.mwer_nbest == 2 and t.mwer_beam == 2 and t.mwer_level == "token"
    for bad in (dict(mwer_weight=-0.1), dict(mwer_weight=math.inf), dict(mwer_weight=math.nan), dict(mwer_nbest=0), dict(mwer_nbest=9, mwer_beam=8),
                dict(mwer_nbest=4, mwer_beam=65), dict(mwer_level="sentence")):
        with pytest.raises(ValueError, match="mwer"):
            _trainer(**bad)
