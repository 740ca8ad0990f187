"""CPU: CTC forced alignment is part of the C-ABI of both libraries and rejects bad arguments with a status + message; the package's host
path (align.forced_align on host tensors, float32 numpy) against brute force, against the float64 law of tests/align_ref.py, and on
all-tie inputs; word_segments on hand-made spans; MultimodalTrainer.align has no CPU fallback."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer as _trainer
import align_ref as R

NAMES = ("av_ctc_align_workspace_bytes", "av_ctc_align")


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
    assert len(L.SIGNATURES["av_ctc_align_workspace_bytes"]) == 4 and len(L.SIGNATURES["av_ctc_align"]) == 19
    for lib in _libs():
        for n in NAMES:
            fn = getattr(lib, n)
            assert fn.argtypes is not None and list(fn.argtypes) == list(L.SIGNATURES[n])


def test_argument_errors_are_statuses_with_a_message():
    P = 4096                                     # any non-null address: argument checks come before a launch, nothing is dereferenced
    for lib in _libs():
        need = ctypes.c_longlong(-1)
        assert lib.av_ctc_align_workspace_bytes(2, 10, 5, ctypes.byref(need)) == 0 and need.value == 2 * 1 * 5 * 4       # 2 bits per (t, s)
        assert lib.av_ctc_align_workspace_bytes(2, 17, 5, ctypes.byref(need)) == 0 and need.value == 2 * 2 * 5 * 4
        assert lib.av_ctc_align_workspace_bytes(2, 10, 5, None) != 0 and b"null" in lib.av_last_error()
        assert lib.av_ctc_align_workspace_bytes(2, 4097, 5, ctypes.byref(need)) != 0 and b"bad shape" in lib.av_last_error()
        assert lib.av_ctc_align_workspace_bytes(2, 10, 4, ctypes.byref(need)) != 0 and b"odd" in lib.av_last_error()
        # (log_probs, stride_b, stride_t, targets, target_ld, input_lengths, target_lengths, B, T, V, S_max, blank,
        #  out_state, out_span, out_token_score, out_score, workspace, workspace_bytes, stream)
        f = lib.av_ctc_align
        assert f(None, 80, 8, P, 2, P, P, 2, 10, 8, 5, 0, P, P, P, P, P, 40, None) != 0
        assert b"null" in lib.av_last_error()
        assert f(P, 80, 8, P, 2, P, P, 2, 10, 8, 5, 0, P, None, P, P, P, 40, None) != 0                 # spans missing with Lmax = 2
        assert b"null" in lib.av_last_error()
        assert f(P, 80, 8, P, 2, P, P, 2, 10, 8, 5, 0, P, P, P, P, None, 40, None) != 0                 # workspace missing
        assert b"null" in lib.av_last_error()
        assert f(P, 80, 8, P, 2, P, P, 2, 10, 8, 5, 8, P, P, P, P, P, 40, None) != 0                    # blank >= V
        assert b"blank" in lib.av_last_error()
        assert f(P, 80, 8, P, 2, P, P, 2, 10, 8, 5, -1, P, P, P, P, P, 40, None) != 0
        assert b"blank" in lib.av_last_error()
        assert f(P, 80, 8, P, 2, P, P, 2, 0, 8, 5, 0, P, P, P, P, P, 40, None) != 0                     # T < 1
        assert b"bad shape" in lib.av_last_error()
        assert f(P, 4097 * 8, 8, P, 2, P, P, 2, 4097, 8, 5, 0, P, P, P, P, P, 1 << 30, None) != 0       # T > 4096
        assert b"bad shape" in lib.av_last_error()
        assert f(P, 80, 8, P, 2, P, P, 2, 10, 8, 4, 0, P, P, P, P, P, 40, None) != 0                    # even S_max
        assert b"odd" in lib.av_last_error()
        assert f(P, 80, 4, P, 2, P, P, 2, 10, 8, 5, 0, P, P, P, P, P, 40, None) != 0                    # time stride < row
        assert b"strides" in lib.av_last_error()
        assert f(P, 8, 8, P, 2, P, P, 2, 10, 8, 5, 0, P, P, P, P, P, 40, None) != 0                     # neither [B][T][V] nor [T][B][V]
        assert b"strides" in lib.av_last_error()
        assert f(P, 80, 8, P, 1, P, P, 2, 10, 8, 5, 0, P, P, P, P, P, 40, None) != 0                    # target_ld < Lmax
        assert b"target_ld" in lib.av_last_error()
        assert f(P, 80, 8, P, 2, P, P, 2, 10, 8, 5, 0, P, P, P, P, P, 39, None) != 0                    # one byte short
        assert b"workspace" in lib.av_last_error() and b"too small" in lib.av_last_error()
        assert f(P, 80, 8, P, 2, P, P, 2, 10, 8, 5, 0, P, P, P, P, P + 2, 40, None) != 0
        assert b"workspace" in lib.av_last_error() and b"aligned" in lib.av_last_error()
        assert f(P, 80000, 8, P, 1000, P, P, 2, 10, 8, 2001, 0, P, P, P, P, P, 1 << 30, None) != 0      # the lattice row does not fit
        assert b"LDS" in lib.av_last_error()


def test_ops_ctc_align_has_no_cpu_fallback():
    lp = torch.log_softmax(torch.randn(5, 2, 8), -1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg("ops").ctc_align(lp, torch.tensor([[1, 2], [2, 1]]), torch.tensor([5, 5]), torch.tensor([2, 2]))


def _host(lp, target, blank=0, Tb=None, Lmax=None):
    """The package's host path on one utterance -> (states [T_b], spans, token scores, score) as numpy."""
    A = pkg("align")
    L = len(target)
    Lmax = L if Lmax is None else Lmax
    tg = torch.zeros((1, Lmax), dtype=torch.long)
    tg[0, :L] = torch.tensor(target, dtype=torch.long)
    al = A.forced_align(torch.from_numpy(np.ascontiguousarray(lp))[None], tg, None if Tb is None else torch.tensor([Tb]), torch.tensor([L]),
                        blank=blank)
    assert al.states.dtype == torch.int32 and al.spans.dtype == torch.int32 and al.token_scores.dtype == torch.float32
    assert al.score.dtype == torch.float32 and al.states.shape == (1, lp.shape[0]) and al.spans.shape == (1, Lmax, 2)
    return al.states[0].numpy(), al.spans[0].numpy(), al.token_scores[0].numpy(), al.score[0].numpy()


@pytest.mark.parametrize("target", [[1, 2], [1, 1]])
def test_host_path_against_brute_force(target):
    """T = 5, V = 3: the score equals the best of all 3^5 frame paths that collapse to the target, and the returned path is one of them."""
    for seed in range(30):
        lp = R.make_log_probs(2000 + seed, 5, 3)
        states, spans, tok, score = _host(lp, target)
        want = R.brute_force(lp, target, 0)
        assert np.isfinite(want)
        assert R.collapse(R.emitted(states, target, 0), 0) == target, (seed, states)
        got64 = R.path_score64(lp, states, target, 0)
        assert abs(got64 - want) <= 1e-12, (seed, got64, want)
        assert abs(float(score) - want) <= 5 * 2.0 ** -23 * abs(want), (seed, score, want)      # the float32 score of that path
        s64, _, _, sc64 = R.law(lp.astype(np.float64), target, 0)
        assert abs(float(sc64) - want) <= 1e-12, (seed, sc64, want)                              # the float64 law finds the same optimum


def test_host_float32_path_against_the_float64_law():
    """200 random cases, T 20-119, V in {8, 40, 800}, labels from 5 classes.  |score32 - score64| <= T 2^-23 |score64| (one fp32 rounding
    per frame on a partial sum no larger in magnitude than the final one: twice that margin), the float32 path re-scored in float64 is
    within the same bound of the optimum, and the host path equals the float32 law bit for bit."""
    rng = np.random.default_rng(7)
    worst, same = 0.0, 0
    for case in range(200):
        T = int(rng.integers(20, 120))
        V = (8, 40, 800)[case % 3]
        L = int(rng.integers(1, T // 3 + 1))
        lp, target = R.make_case(5000 + case, T, V, L)
        s64, _, _, sc64 = R.law(lp.astype(np.float64), target, 0)
        s32, sp32, tk32, sc32 = R.law(lp, target, 0)
        states, spans, tok, score = _host(lp, target)
        assert s64 is not None and s32 is not None
        assert states.tolist() == s32 and spans.tolist() == [list(x) for x in sp32]
        assert tok.view(np.int32).tolist() == np.array(tk32, np.float32).view(np.int32).tolist()
        assert score.view(np.int32) == np.float32(sc32).view(np.int32)
        bound = T * 2.0 ** -23 * abs(float(sc64))
        assert abs(float(score) - float(sc64)) <= bound, (case, score, sc64, bound)
        rescored = R.path_score64(lp, states, target, 0)
        assert abs(rescored - float(sc64)) <= bound, (case, rescored, sc64, bound)
        worst = max(worst, abs(float(score) - float(sc64)) / bound)
        same += states.tolist() == s64
    print(f"[align host] 200 cases: float32 path equals the float64 path in {same}, worst |score32 - score64| = {worst:.3f} of the bound")


def test_uniform_log_probs_follow_the_tie_rule():
    """Every path ties: the stay wins every tie and S-2 wins the final one, so the path leaves a state at the last possible frame going
    backwards - the first label for one frame, then the second label to the end, no blank."""
    lp = np.full((6, 4), np.log(np.float32(0.25)), np.float32)
    states, spans, tok, score = _host(lp, [1, 2])
    assert states.tolist() == [1, 3, 3, 3, 3, 3]
    assert spans.tolist() == [[0, 1], [1, 6]]
    c = np.float32(lp[0, 0])
    acc = np.float32(0.0)
    for _ in range(5):
        acc = np.float32(acc + c)
    assert tok.tolist() == [float(c), float(acc)] and float(score) == float(np.float32(acc + c))
    assert R.law(lp, [1, 2], 0)[0] == [1, 3, 3, 3, 3, 3]
    # a repeated label cannot skip: the blank between the two is on the path for exactly one frame
    states, spans, _, _ = _host(lp, [1, 1])
    assert states.tolist() == [1, 2, 3, 3, 3, 3] and spans.tolist() == [[0, 1], [2, 6]]


def test_host_path_lengths_infeasible_items_and_padding():
    A = pkg("align")
    T, V, Lmax = 12, 6, 4
    lp = torch.from_numpy(np.stack([R.make_log_probs(70 + b, T, V) for b in range(7)]))
    tg = torch.tensor([[1, 2, 3, 4], [1, 1, 1, 0], [1, 2, 0, 0], [1, 0, 2, 0], [1, 6, 0, 0], [2, 2, 2, 2], [3, 0, 0, 0]])
    il = torch.tensor([12, 5, 0, 12, 12, 6, 99])
    tl = torch.tensor([4, 3, 0, 3, 2, 4, -3])
    al = A.forced_align(lp, tg, il, tl, blank=0)
    # item 0: plain; 1: three equal labels in exactly 5 frames (a single path); 2: no frames, no labels (feasible, score 0, empty path);
    # 3: a label equal to the blank; 4: a label >= V; 5: four equal labels need 7 frames, one short; 6: lengths clamped to [0, T] / [0, Lmax]
    assert al.states[1].tolist() == [1, 2, 3, 4, 5] + [-1] * 7 and al.spans[1].tolist() == [[0, 1], [2, 3], [4, 5], [-1, -1]]
    assert float(al.score[2]) == 0.0 and bool((al.states[2] == -1).all()) and bool((al.spans[2] == -1).all())
    for b in (3, 4, 5):
        assert float(al.score[b]) == float("-inf") and bool((al.states[b] == -1).all()) and bool((al.spans[b] == -1).all())
        assert bool((al.token_scores[b] == 0).all())
    assert bool((al.states[6] == 0).all()) and float(al.score[6]) == float(lp[6, :, 0].numpy().cumsum(dtype=np.float32)[-1])
    ids = A.token_path(al, tg, 0)
    assert ids.dtype == torch.int64 and ids[1].tolist() == [1, 0, 1, 0, 1] + [-1] * 7 and bool((ids[3] == -1).all())
    assert R.collapse([i for i in ids[0].tolist() if i >= 0], 0) == [1, 2, 3, 4]
    # [T, B, V] input and default lengths
    al_t = A.forced_align(lp.transpose(0, 1), tg, il, tl, blank=0, batch_first=False)
    assert all(torch.equal(x, y) for x, y in zip(al, al_t))
    al_d = A.forced_align(lp[:1], tg[:1])
    assert torch.equal(al_d.states, al.states[:1]) and torch.equal(al_d.score, al.score[:1])


def test_word_segments_on_hand_made_spans():
    A = pkg("align")
    tok = pkg("utils.tokenizer").SyntheticTokenizer(800)
    sp, a, b, c = tok.token_to_id["▁"], 5, 6, 7
    ids = [sp, a, b, sp, sp, c, sp]                                  # "▁AB▁▁C▁": leading / trailing space pieces and two in a row
    spans = [[0, 1], [1, 3], [3, 4], [5, 6], [6, 7], [8, 10], [10, 11], [-1, -1]]
    scores = [-0.1, -0.25, -0.5, -0.1, -0.1, -1.0, -0.1, 0.0]
    w = A.word_segments(tok, ids, torch.tensor(spans, dtype=torch.int32), torch.tensor(scores), frame_rate=25.0)
    assert [x["word"] for x in w] == [tok.id_to_token[a] + tok.id_to_token[b], tok.id_to_token[c]]
    assert w[0]["start"] == 1 / 25.0 and w[0]["end"] == 4 / 25.0 and abs(w[0]["score"] - (-0.75 / 3)) < 1e-7
    assert w[1]["start"] == 8 / 25.0 and w[1]["end"] == 10 / 25.0 and abs(w[1]["score"] - (-1.0 / 2)) < 1e-7
    assert tok.decode(ids).split() == [x["word"] for x in w]
    assert A.word_segments(tok, ids, spans, scores, frame_rate=50.0)[1]["start"] == 8 / 50.0
    assert A.word_segments(tok, ids, [[-1, -1]] * 8, [0.0] * 8) == []            # infeasible utterance
    assert A.word_segments(tok, [], [[-1, -1]] * 8, [0.0] * 8) == []             # empty transcript
    assert A.word_segments(tok, [sp, sp], [[0, 1], [1, 2]], [-0.1, -0.1]) == []  # nothing but spaces


def test_trainer_align_has_no_cpu_fallback():
    synth = pkg("dataset.synthetic")
    t = _trainer()
    modes = [m.training for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.align(synth.make_batch(2, 1.0, seed=1))
    assert [m.training for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1)] == modes
