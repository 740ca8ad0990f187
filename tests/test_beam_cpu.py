"""CPU: CTC prefix beam search (beam_search.prefix_beam_search, host path = float32 numpy restatement of the law of csrc/ctc_beam.hip)
against brute force, against the float64 reference law of tests/beam_ref.py and against greedy decoding; the C-ABI's argument errors in
both libraries; the trainer keeps the greedy decode unless asked."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer as _trainer
import beam_ref as R


def _decode(lp, W, blank=0, **kw):
    return pkg("beam_search").prefix_beam_search(torch.from_numpy(np.asarray(lp)), beam_width=W, blank=blank, **kw)


def test_brute_force_t4_v3():
    """T = 4, two labels, W = 31: nothing can be pruned, so the top hypothesis is the labelling with the largest exact likelihood among all
    31 labellings of length <= 4, and its score is that likelihood."""
    labellings = [l for n in range(5) for l in itertools.product((1, 2), repeat=n)]
    assert len(labellings) == 31
    for seed in range(20):
        lp = R.make_log_probs(1000 + seed, 4, 3)
        ll = [R.exact_loglik(lp, l, 0) for l in labellings]
        best = int(np.argmax(ll))
        ids, scores = _decode(lp, 31, nbest=31, return_scores=True)
        assert ids[0][0] == list(labellings[best]), (seed, ids[0][0], labellings[best])
        assert abs(scores[0][0] - ll[best]) <= 1e-5, (seed, scores[0][0], ll[best])
        for i, s in zip(ids[0], scores[0]):                                  # every kept hypothesis carries ALL its alignments at this size
            if np.isfinite(s):
                assert abs(s - R.exact_loglik(lp, i, 0)) <= 1e-5, (seed, i)


@pytest.mark.parametrize("T,V,W,n", [(60, 40, 5, 16), (40, 12, 8, 16), (199, 800, 5, 4)])
def test_host_path_against_the_reference_law(T, V, W, n):
    lps = [R.make_log_probs(7000 + 100 * W + s, T, V) for s in range(n)]
    refs = R.references(lps, W, 0, workers=8 if V >= 800 else 1)
    got = []
    for lp in lps:
        ids, scores = _decode(lp, W, nbest=W, return_scores=True)
        got.append((ids[0], scores[0]))
    R.check_agreement(got, refs, f"host T={T} V={V} W={W}")


def test_lengths_equal_truncated_rows_and_zero_length():
    T, V, W = 30, 20, 4
    lp = np.stack([R.make_log_probs(50 + b, T, V, blank=3) for b in range(4)])
    lens = [30, 0, 17, 1]
    ids, scores = _decode(lp, W, blank=3, lengths=torch.tensor(lens), nbest=W, return_scores=True)
    for b, n in enumerate(lens):
        if n == 0:
            assert ids[b] == [[]] and scores[b] == [0.0]
            continue
        i1, s1 = _decode(lp[b, :n], W, blank=3, nbest=W, return_scores=True)
        assert ids[b] == i1[0] and scores[b] == s1[0]
    assert _decode(lp, W, blank=3, lengths=lens) == [i[0] for i in ids]      # a plain list of lengths, nbest = 1


def test_minus_infinity_column_gives_no_nan():
    lp = R.make_log_probs(5, 25, 9)
    lp[:, 4] = -np.inf
    lp[3, 0] = -np.inf                                                       # and one frame that cannot emit blank
    for W in (3, 8, 16):                                                     # W + 1 > V - 1 at 8 and 16: every token is expanded, -inf ones too
        ids, scores = _decode(lp, W, nbest=W, return_scores=True)
        assert not any(np.isnan(s) for s in scores[0])
        assert np.isfinite(scores[0][0]) and 4 not in ids[0][0]
        assert all(a >= b for a, b in zip(scores[0], scores[0][1:]))


def test_nbest_one_is_the_head_of_nbest_w():
    lp = np.stack([R.make_log_probs(300 + b, 50, 30) for b in range(3)])
    full, fs = _decode(lp, 6, nbest=6, return_scores=True)
    one, s1 = _decode(lp, 6, return_scores=True)
    assert one == [f[0] for f in full] and s1 == [s[0] for s in fs]
    assert _decode(lp[0], 6) == [one[0]]                                     # [T, V] is a batch of one
    with pytest.raises(ValueError):
        _decode(lp, 6, nbest=7)
    with pytest.raises(ValueError):
        _decode(lp, 65)


def _greedy_cases(n=30, T=60, V=40, W=5):
    """The first n seeds, counted from 0, on which the float64 reference LAW ITSELF does not lose to greedy decoding.  Beam search is not
    guaranteed to beat greedy: at W = 5 the prefix of the per-frame argmax path can be pruned, and with this generator the reference law's
    best hypothesis has a lower exact likelihood than the greedy one on 4 of the seeds 0..89 (2, 10, 56, 76; by 0.004 to 0.1 nat).  No
    implementation of the law can pass "never lower" there, so those seeds are set aside - by the reference alone, never by the code
    under test - and printed."""
    bs = pkg("beam_search")
    cases, skipped, seed = [], [], 0
    while len(cases) < n:
        lp = R.make_log_probs(seed, T, V)
        greedy = bs.greedy_batch(torch.from_numpy(lp)[None], 0)[0]
        lg = R.exact_loglik(lp, greedy, 0)
        if R.exact_loglik(lp, R.ref_pbs(lp.astype(np.float64), W, 0)[0][0], 0) >= lg - 1e-6:
            cases.append((seed, lp, lg))
        else:
            skipped.append(seed)
        seed += 1
    print(f"[beam vs greedy] seeds set aside because the reference law itself is below greedy: {skipped}")
    return cases


def test_likelihood_never_below_greedy_and_often_above():
    higher = 0
    for seed, lp, lg in _greedy_cases():
        lb = R.exact_loglik(lp, _decode(lp, 5)[0], 0)
        assert lb >= lg - 1e-6, (seed, lb, lg)
        higher += lb > lg
    print(f"[beam vs greedy] strictly higher exact likelihood in {higher} of 30")
    assert higher >= 10, higher


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


def test_abi_argument_errors_in_both_libraries():
    P = 4096                                     # any non-null address: argument checks come before a launch, nothing is dereferenced
    B, T, V = 2, 10, 8
    for lib in _libs():
        need = ctypes.c_longlong(0)
        assert lib.av_ctc_beam_workspace_bytes(B, T, V, 5, ctypes.byref(need)) == 0 and need.value > 0
        assert lib.av_ctc_beam_workspace_bytes(B, T, V, 5, None) != 0
        assert lib.av_ctc_beam_workspace_bytes(B, T, V, 65, ctypes.byref(need)) != 0
        n = need.value
        # (log_probs, stride_b, stride_t, lengths, out_ids, out_len, out_score, workspace, workspace_bytes, B, T, V, blank, beam_width, nbest, stream)
        for bad in range(5):
            a = [P, T * V, V, None, P, P, P, P, n, B, T, V, 0, 5, 1, None]
            a[(0, 4, 5, 6, 7)[bad]] = None
            assert lib.av_ctc_beam_search(*a) != 0 and b"null" in lib.av_last_error()
        for W in (0, 65):
            assert lib.av_ctc_beam_search(P, T * V, V, None, P, P, P, P, 1 << 30, B, T, V, 0, W, 1, None) != 0
            assert b"beam_width" in lib.av_last_error()
        assert lib.av_ctc_beam_search(P, T * V, V, None, P, P, P, P, n, B, T, V, 0, 5, 6, None) != 0
        assert b"nbest" in lib.av_last_error()
        assert lib.av_ctc_beam_search(P, T * V, V, None, P, P, P, P, n, B, T, V, 0, 5, 0, None) != 0
        assert lib.av_ctc_beam_search(P, T * V, V, None, P, P, P, P, n - 1, B, T, V, 0, 5, 1, None) != 0
        assert b"workspace" in lib.av_last_error()
        assert lib.av_ctc_beam_frame_pass(P, T * V, V, None, P, n - 1, B, T, V, 0, 5, None) != 0
        assert b"workspace" in lib.av_last_error()
        assert lib.av_ctc_beam_search(P, T * V, V, None, P, P, P, P, n, B, T, V, V, 5, 1, None) != 0
        assert b"blank" in lib.av_last_error()
        assert lib.av_ctc_beam_search(P, T * V, V, None, P, P, P, P, 1 << 40, B, 4097, V, 0, 5, 1, None) != 0
        assert b"bad shape" in lib.av_last_error()
        assert lib.av_ctc_beam_search(P, T * V, V, None, P, P, P, P, n, B, T, 1, 0, 5, 1, None) != 0
        assert lib.av_ctc_beam_search(P, T * V, V - 1, None, P, P, P, P, n, B, T, V, 0, 5, 1, None) != 0
        assert b"strides" in lib.av_last_error()


def test_trainer_decodes_greedily_unless_asked(monkeypatch):
    monkeypatch.delenv("AVAMD_EVAL_BEAM", raising=False)
    assert _trainer().eval_beam_width == 0
    monkeypatch.setenv("AVAMD_EVAL_BEAM", "8")
    assert _trainer().eval_beam_width == 8
    assert _trainer(eval_beam_width=0).eval_beam_width == 0                  # an explicit argument wins over the variable
    monkeypatch.delenv("AVAMD_EVAL_BEAM")
    assert _trainer(eval_beam_width=4).eval_beam_width == 4
    with pytest.raises(ValueError):
        _trainer(eval_beam_width=-1)
