"""CPU: CTC segmentation.  The package's host path (segmentation.ctc_segment on host tensors, float32 numpy) equals the cell-by-cell law of
tests/segment_ref.py bit for bit on the test matrix, with every combination of free ends; with fixed ends it is align.forced_align bit
for bit; a constructed recording with speech in the middle is found with score 0.0 exactly; the C-ABI of both libraries rejects bad
arguments with a status and a message; the options table."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer
import segment_ref as R

NAMES = ("av_ctc_segment_workspace_bytes", "av_ctc_segment")
FIELDS = ("states", "spans", "token_scores", "score", "frame_scores", "utt_spans", "utt_means", "utt_scores")


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


def _bits(x):
    x = np.asarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _ref_padded(lp, tg, il, tl, ut, blank, free, w):
    """segment_ref.law per item, padded to the package's shapes."""
    B, T, _ = lp.shape
    Lmax, U = tg.shape[1], ut.shape[1]
    out = {"states": np.full((B, T), -1, np.int32), "spans": np.full((B, Lmax, 2), -1, np.int32), "token_scores": np.zeros((B, Lmax), np.float32),
           "score": np.zeros(B, np.float32), "frame_scores": np.zeros((B, T), np.float32), "utt_spans": np.full((B, U, 2), -1, np.int32),
           "utt_means": np.zeros((B, U), np.float32), "utt_scores": np.zeros((B, U), np.float32)}
    for b in range(B):
        Tb, Lb = int(il[b]), int(tl[b])
        r = R.law(lp[b, :Tb], tg[b, :Lb], blank, free, [tuple(x) for x in ut[b].tolist()], w)
        out["states"][b, :Tb] = r["states"]
        out["frame_scores"][b, :Tb] = r["frame_scores"]
        if Lb:
            out["spans"][b, :Lb] = r["spans"]
            out["token_scores"][b, :Lb] = r["token_scores"]
        out["score"][b] = r["score"]
        if U:
            out["utt_spans"][b] = r["utt_spans"]
            out["utt_means"][b] = r["utt_means"]
            out["utt_scores"][b] = r["utt_scores"]
    return out


@pytest.mark.parametrize("blank", [0, 3])
@pytest.mark.parametrize("free", [0, 1, 2, 3])
def test_host_path_equals_the_cell_by_cell_law_bit_for_bit(blank, free):
    S = pkg("segmentation")
    T, V, Lmax = 37, 5, 12
    lp, tg, il, tl, ut, items = R.matrix(T, V, Lmax, blank)
    for w in (1, 4, 30):
        got = S.ctc_segment(torch.from_numpy(lp), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl), blank=blank,
                            utterances=torch.from_numpy(ut), free_start=bool(free & 1), free_end=bool(free & 2), score_window=w)
        want = _ref_padded(lp, tg, il, tl, ut, blank, free, w)
        for name, g in zip(FIELDS, got):
            g = g.numpy()
            assert g.dtype == want[name].dtype and g.shape == want[name].shape, (name, g.dtype, g.shape)
            assert np.array_equal(_bits(g), _bits(want[name])), (free, w, name, g, want[name])
    # the matrix is what it says: the tight item has a single path, the short one none, and the utterances hit every branch
    assert np.isfinite(got.score.numpy()).tolist() == [True, True, True, True, True, False]               # a free end saves no frame
    usp = got.utt_spans.numpy()
    assert (usp[0, 0] >= 0).all() and (usp[0, 1] >= 0).all() and usp[0, 1, 0] > usp[0, 0, 1]              # a gap of one token between them
    assert (usp[:, 2:] == -1).all() and (usp[1] == -1).all() and (usp[5] == -1).all() and (usp[2, 0] == (0, 1)).all()
    on = usp[..., 0] >= 0
    assert (got.utt_scores.numpy()[on] <= got.utt_means.numpy()[on] + 1e-6).all()                         # the least window mean


@pytest.mark.parametrize("T,V,Lmax", [(37, 5, 12), (100, 800, 30)])
@pytest.mark.parametrize("blank", [0, 3])
def test_fixed_ends_are_forced_align_bit_for_bit(T, V, Lmax, blank):
    S = pkg("segmentation"); A = pkg("align")
    lp, tg, il, tl, ut, _ = R.matrix(T, V, Lmax, blank)
    args = (torch.from_numpy(lp), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl))
    got = S.ctc_segment(*args, blank=blank, utterances=torch.from_numpy(ut))
    want = A.forced_align(*args, blank=blank)
    for name, g, w in zip(FIELDS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g.numpy()), _bits(w.numpy())), name
    # [T, B, V] input, default lengths, no utterances
    got_t = S.ctc_segment(args[0].transpose(0, 1), *args[1:], blank=blank, batch_first=False)
    assert all(torch.equal(x, y) for x, y in zip(got_t[:5], got[:5])) and got_t.utt_spans.shape == (6, 0, 2)
    one = S.ctc_segment(args[0][:1], args[1][:1], blank=blank)
    assert torch.equal(one.states, got.states[:1]) and torch.equal(one.score, got.score[:1])


def test_speech_in_the_middle_of_a_recording_is_found_with_free_ends():
    """A known path over frames [a, g) with probability 0.9 on the path's class; outside, 0.9 on a class that is neither the blank nor in
    the transcript.  With both ends free the path is an argmax path over exactly those frames: score 0.0.  (No emission is above 0, so a
    free end lies on the FIRST frame on which the last label is complete - the known path gives its last label one frame.)"""
    S = pkg("segmentation")
    T, V, blank, other = 60, 8, 0, 7
    target = [1, 2, 2, 3]
    a = 11
    frames = [1, 1, 1, 0, 2, 2, 0, 2, 0, 0, 3]                              # the ids of frames a ..; the last label frame is a + 10
    known = [(a, a + 3), (a + 4, a + 6), (a + 7, a + 8), (a + 10, a + 11)]
    g = a + len(frames)
    ids = [other] * a + frames + [other] * (T - g)
    p = np.full((T, V), 0.1 / (V - 1), np.float32)
    p[np.arange(T), ids] = 0.9
    lp = torch.from_numpy(np.log(p))[None]
    tg = torch.tensor([target])
    both = S.ctc_segment(lp, tg, blank=blank, utterances=[[[0, 2], [2, 4]]], free_start=True, free_end=True, score_window=4)
    assert float(both.score[0]) == 0.0 and np.signbit(both.score[0].numpy()) == np.signbit(np.float32(0.0))
    st = both.states[0].tolist()
    assert [t for t in range(T) if st[t] >= 0] == list(range(a, g))
    assert both.spans[0].tolist() == [list(x) for x in known]
    assert bool((both.frame_scores[0] == 0).all()) and bool((both.token_scores[0] == 0).all())
    assert both.utt_spans[0].tolist() == [[a, a + 6], [a + 7, a + 11]] and both.utt_means[0].tolist() == [0.0, 0.0] and both.utt_scores[0].tolist() == [0.0, 0.0]
    fixed = S.ctc_segment(lp, tg, blank=blank)
    assert float(fixed.score[0]) < 0.0 and bool((fixed.states[0] >= 0).all())
    # one free end alone reaches the other end of the recording through frames that cost
    start_only = S.ctc_segment(lp, tg, blank=blank, free_start=True)
    end_only = S.ctc_segment(lp, tg, blank=blank, free_end=True)
    assert float(start_only.score[0]) < 0.0 and int(start_only.states[0, T - 1]) >= 0 and int(start_only.states[0, 0]) == -1
    assert float(end_only.score[0]) < 0.0 and int(end_only.states[0, 0]) >= 0 and int(end_only.states[0, T - 1]) == -1


def test_utterance_segments_and_argument_checks():
    S = pkg("segmentation")
    seg = S.Segmentation(None, None, None, None, None, torch.tensor([[[5, 30], [-1, -1], [40, 50]]], dtype=torch.int32),
                         torch.tensor([[-0.5, 0.0, -1.0]]), torch.tensor([[-2.0, 0.0, -1.5]]))
    rows = S.utterance_segments(seg, [["a", "b", "c"]], frame_rate=25.0)
    assert rows == [[{"text": "a", "start": 0.2, "end": 1.2, "score": -2.0, "mean": -0.5}, {"text": "c", "start": 1.6, "end": 2.0, "score": -1.5, "mean": -1.0}]]
    with pytest.raises(ValueError, match="texts"):
        S.utterance_segments(seg, [["a"], ["b"]])
    lp = torch.log_softmax(torch.randn(2, 6, 5), -1)
    tg = torch.tensor([[1, 2], [2, 1]])
    with pytest.raises(ValueError, match="score_window"):
        S.ctc_segment(lp, tg, score_window=0)
    with pytest.raises(ValueError, match="utterances"):
        S.ctc_segment(lp, tg, utterances=torch.zeros((2, 1, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="rows"):
        S.ctc_segment(lp, tg[:1])


# ---- the C-ABI ----
def test_both_symbols_exported_by_both_libraries_and_bound():
    L = pkg("_lib")
    assert len(L.SIGNATURES["av_ctc_segment_workspace_bytes"]) == 4 and len(L.SIGNATURES["av_ctc_segment"]) == 27
    for lib in _libs():
        for n in NAMES:
            fn = getattr(lib, n)
            assert fn.argtypes is not None and list(fn.argtypes) == list(L.SIGNATURES[n])


def test_argument_errors_are_statuses_with_a_message():
    P = 4096                                     # any non-null address: argument checks come before a launch, nothing is dereferenced
    for lib in _libs():
        need = ctypes.c_longlong(-1)
        assert lib.av_ctc_segment_workspace_bytes(2, 10, 5, ctypes.byref(need)) == 0 and need.value == 2 * 1 * 5 * 4     # 2 bits per (t, s)
        assert lib.av_ctc_segment_workspace_bytes(2, 17, 5, ctypes.byref(need)) == 0 and need.value == 2 * 2 * 5 * 4
        assert lib.av_ctc_segment_workspace_bytes(2, 90000, 16383, ctypes.byref(need)) == 0 and need.value == 2 * 5625 * 16383 * 4      # > 2^31: 64-bit
        assert lib.av_ctc_segment_workspace_bytes(2, 10, 5, None) != 0 and b"null" in lib.av_last_error()
        assert lib.av_ctc_segment_workspace_bytes(2, 0, 5, ctypes.byref(need)) != 0 and b"bad shape" in lib.av_last_error()
        assert lib.av_ctc_segment_workspace_bytes(2, 10, 4, ctypes.byref(need)) != 0 and b"odd" in lib.av_last_error()
        assert lib.av_ctc_segment_workspace_bytes(2, 10, 16385, ctypes.byref(need)) != 0 and b"limit" in lib.av_last_error()
        # (log_probs, stride_b, stride_t, targets, target_ld, input_lengths, target_lengths, utterances, B, T, V, S_max, U, blank, free,
        #  score_window, out_state, out_span, out_token_score, out_score, out_frame_score, out_utt_span, out_utt_mean, out_utt_score,
        #  workspace, workspace_bytes, stream)
        f = lib.av_ctc_segment

        def call(**kw):
            a = dict(lp=P, sb=80, st=8, tg=P, ld=2, il=P, tl=P, ut=P, B=2, T=10, V=8, S=5, U=3, blank=0, free=0, w=30, state=P, span=P, tok=P,
                     score=P, frame=P, usp=P, umean=P, uscore=P, ws=P, wsb=40, stream=None)
            a.update(kw)
            return f(*a.values())
        for name in ("lp", "tg", "il", "tl", "state", "score", "frame", "ws", "span", "tok", "ut", "usp", "umean", "uscore"):
            assert call(**{name: None}) != 0 and b"av_ctc_segment: null" in lib.av_last_error(), name
        for name in ("B", "T"):
            assert call(**{name: 0}) != 0 and b"bad shape" in lib.av_last_error(), name
        assert call(S=4) != 0 and b"odd" in lib.av_last_error()                                   # even S_max
        assert call(S=16385, ld=8192, wsb=1 << 30) != 0 and b"limit" in lib.av_last_error()       # S_max above the limit
        assert call(V=0) != 0 and b"V = 0" in lib.av_last_error()
        assert call(V=12001, st=12001, sb=10 * 12001) != 0 and b"V = 12001" in lib.av_last_error()
        for blank in (-1, 8):
            assert call(blank=blank) != 0 and b"blank" in lib.av_last_error()
        for free in (-1, 4):
            assert call(free=free) != 0 and b"free" in lib.av_last_error()
        assert call(w=0) != 0 and b"score_window" in lib.av_last_error()
        assert call(U=-1) != 0 and b"utterances" in lib.av_last_error()
        assert call(ld=1) != 0 and b"target_ld" in lib.av_last_error()
        assert call(st=4) != 0 and b"strides" in lib.av_last_error()
        assert call(sb=8) != 0 and b"strides" in lib.av_last_error()
        assert call(wsb=39) != 0 and b"workspace" in lib.av_last_error() and b"too small" in lib.av_last_error()
        assert call(ws=P + 2) != 0 and b"workspace" in lib.av_last_error() and b"aligned" in lib.av_last_error()


def test_ops_ctc_segment_and_the_trainer_have_no_cpu_fallback():
    lp = torch.log_softmax(torch.randn(2, 5, 8), -1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg("ops").ctc_segment(lp, torch.tensor([[1, 2], [2, 1]]), torch.tensor([5, 5]), torch.tensor([2, 2]))
    t = cpu_trainer()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.align_long({}, "A", "B")


# ---- the options table ----
def test_options_argument_beats_variable_beats_default(monkeypatch):
    O = pkg("model.options")
    assert O.OPTIONS["segment_window"][:3:2] == ("AVAMD_SEGMENT_WINDOW", "30") and O.OPTIONS["segment_free"][:3:2] == ("AVAMD_SEGMENT_FREE", "0")
    monkeypatch.delenv("AVAMD_SEGMENT_WINDOW", raising=False); monkeypatch.delenv("AVAMD_SEGMENT_FREE", raising=False)
    assert O.resolve("segment_window", None) == 30 and O.resolve("segment_free", None) == 0
    monkeypatch.setenv("AVAMD_SEGMENT_WINDOW", "12"); monkeypatch.setenv("AVAMD_SEGMENT_FREE", "3")
    assert O.resolve("segment_window", None) == 12 and O.resolve("segment_free", None) == 3
    assert O.resolve("segment_window", 5) == 5 and O.resolve("segment_free", 1) == 1
    t = cpu_trainer()
    assert (t.segment_window, t.segment_free) == (12, 3)
    t = cpu_trainer(segment_window=7, segment_free=2)
    assert (t.segment_window, t.segment_free) == (7, 2)
    O.check_segmentation(1, 0); O.check_segmentation(30, 3)
    for bad in ((0, 0), (30, 4), (30, -1)):
        with pytest.raises(ValueError, match="segment_"):
            O.check_segmentation(*bad)
    with pytest.raises(ValueError, match="segment_free"):
        cpu_trainer(segment_free=4)
