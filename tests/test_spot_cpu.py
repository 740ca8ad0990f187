"""CPU: CTC keyword spotting.  The package's host law (spot.keyword_spot on host tensors, float32 numpy) against the independent float64
reference of tests/spot_ref.py within a bound derived from rounding, on planted occurrences (exact), on the properties of the hit list and
on degenerate inputs; the two entry points are part of the C-ABI of both libraries and reject bad arguments with a status and a message;
the options table."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer
import spot_ref as R

NAMES = ("av_ctc_spot_workspace_bytes", "av_ctc_spot")
NEG = float("-inf")


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


def _spot(lp, keywords, **kw):
    S = pkg("spot")
    s = S.keyword_spot(torch.from_numpy(np.ascontiguousarray(lp))[None] if isinstance(lp, np.ndarray) else lp, keywords, **kw)
    assert s.hits.dtype == torch.int32 and s.scores.dtype == torch.float32 and s.counts.dtype == torch.int32
    return s


def _listed(s, b=0, k=0):
    n = int(s.counts[b, k])
    assert bool((s.hits[b, k, n:] == -1).all()) and bool((s.scores[b, k, n:] == NEG).all())
    return [(int(s.hits[b, k, r, 0]), int(s.hits[b, k, r, 1]), float(s.scores[b, k, r])) for r in range(n)]


# ---- the host law against the float64 reference ----
def test_host_law_against_the_float64_reference():
    """240 seeded cases, T in [1, 40], V in [3, 9], L in [1, 4], a random blank, logit scales 0.5, 3 and 8.  |e32[t] - e64[t]| <= 2^-23 (t + 2)
    sum_{u <= t} max_s |c64[u][s]| (spot_ref.bound: one rounding of c, at most t + 1 additions whose partial sums are bounded by the sum of
    |c|, a factor of two of margin), e32 is -inf exactly where e64 is, and the carried start is consistent: the float64 score of the best
    path restricted to [es[t], t] is within twice the bound of the float64 optimum."""
    S = pkg("spot")
    rng = np.random.default_rng(2024)
    worst = worst_start = 0.0
    for case in range(240):
        T, V, L = int(rng.integers(1, 41)), int(rng.integers(3, 10)), int(rng.integers(1, 5))
        blank = int(rng.integers(0, V))
        y = [int(i) for i in rng.choice([v for v in range(V) if v != blank], size=L)]
        lp = R.make_log_probs(9000 + case, T, V, (0.5, 3.0, 8.0)[case % 3])
        e32, es = S._host_end_series(lp, [y], T, blank)
        e32, es = e32[0], es[0]
        assert e32.dtype == np.float32 and es.dtype == np.int32
        E = R.end_scores64(lp, y, blank)
        e64, bd = E.max(axis=0), R.bound(lp, y, blank)
        assert (np.isneginf(e32) == np.isneginf(e64)).all(), case
        for t in np.flatnonzero(np.isfinite(e64)):
            err = abs(float(e32[t]) - e64[t])
            assert err <= bd[t], (case, t, e32[t], e64[t], bd[t])
            assert 0 <= es[t] <= t, (case, t, es[t])
            gap = e64[t] - E[es[t], t]
            assert gap <= 2 * bd[t], (case, t, es[t], gap, bd[t])
            if bd[t] > 0:
                worst, worst_start = max(worst, err / bd[t]), max(worst_start, gap / (2 * bd[t]))
    print(f"[spot host] 240 cases: worst |e32 - e64| = {worst:.3f} of the bound, worst start gap = {worst_start:.3f} of twice the bound")


# ---- planted occurrences ----
@pytest.mark.parametrize("keyword", [[3, 5, 5, 7], [5, 5], [3]])
def test_planted_occurrences_are_found_exactly(keyword):
    """Posteriors whose argmax path holds the keyword three times between fillers of other labels: with min_score = 0.0 the hits are exactly
    the planted (first frame of y_1's run, end frame of y_L's run) intervals and every score is bit-equal to 0.0.  [3, 5, 5, 7] and [5, 5]
    repeat a label, which forces the blank between the two; [3] is the one-state lattice."""
    trials = 50 if keyword == [3, 5, 5, 7] else 10
    for trial in range(trials):
        lp, path, spans = R.planted(100 * len(keyword) + trial, keyword, 3, 10, 0, [0, 1, 2, 4, 6, 8, 9])
        s = _spot(lp, [keyword], blank=0, max_hits=8, min_score=0.0)
        got = _listed(s)
        assert sorted((a, b) for a, b, _ in got) == spans, (trial, got, spans, path)
        assert [(a, b) for a, b, _ in got] == spans[::-1]                     # all tie at 0.0: the greater end frame first
        assert all(np.float32(sc).view(np.int32) == 0 for _, _, sc in got)     # +0.0, bit for bit


# ---- properties of the hit list ----
def test_hits_are_disjoint_descending_and_cut_by_count_and_score():
    rng = np.random.default_rng(5)
    some = 0
    for case in range(40):
        T, V = int(rng.integers(20, 60)), 6
        lp = R.make_log_probs(300 + case, T, V, 3.0)
        kws = [[1], [2, 3], [4, 4], [1, 2, 5]]
        s8 = _spot(lp, kws, blank=0, max_hits=8)
        s1 = _spot(lp, kws, blank=0, max_hits=1)
        for k in range(len(kws)):
            h = _listed(s8, 0, k)
            assert len(h) <= 8 and int(s1.counts[0, k]) == min(1, len(h))
            assert all(0 <= a < b <= T for a, b, _ in h)
            assert all(x[2] >= y[2] for x, y in zip(h, h[1:]))
            assert all(a1 >= b2 or a2 >= b1 for i, (a1, b1, _) in enumerate(h) for a2, b2, _ in h[i + 1:])
            assert _listed(s1, 0, k) == h[:1]
            if len(h) >= 2:
                some += 1
                thr = h[len(h) // 2][2]
                cut = _spot(lp, kws, blank=0, max_hits=8, min_score=thr)
                assert _listed(cut, 0, k) == [x for x in h if x[2] >= thr]
                assert _listed(_spot(lp, kws, blank=0, max_hits=8, min_score=h[0][2] + 1.0), 0, k) == []     # scores are <= 0
    assert some > 40


# ---- degenerate inputs ----
def test_lengths_are_clamped_and_an_empty_utterance_has_no_hits():
    T, V = 14, 6
    lp = torch.from_numpy(np.stack([R.make_log_probs(70 + b, T, V) for b in range(4)]))
    kws = [[1, 2], [3]]
    s = _spot(lp, kws, input_lengths=torch.tensor([0, 99, -3, 9]), blank=0, max_hits=3)
    full = _spot(lp, kws, blank=0, max_hits=3)
    assert s.counts[0].tolist() == [0, 0] and s.counts[2].tolist() == [0, 0] and bool((s.hits[0] == -1).all())
    assert all(torch.equal(x[1], y[1]) for x, y in zip(s, full))
    short = _spot(lp[3:, :9], kws, blank=0, max_hits=3)
    assert all(torch.equal(x[3], y[0]) for x, y in zip(s, short))
    assert int(full.counts.sum()) > 0
    # a [T, B, V] input is the transposed call
    tbv = _spot(lp.transpose(0, 1).contiguous(), kws, input_lengths=[0, 99, -3, 9], blank=0, max_hits=3, batch_first=False)
    assert all(torch.equal(x, y) for x, y in zip(s, tbv))


def test_invalid_keywords_tensor_rows_count_zero_and_lists_raise():
    S = pkg("spot")
    T, V, blank = 12, 6, 2
    lp = torch.from_numpy(R.make_log_probs(1, T, V))[None]
    ids = torch.tensor([[1, 3, 0], [1, blank, 3], [1, 6, 0], [-1, 0, 0], [4, 0, 0], [5, 0, 0]])
    lens = torch.tensor([2, 3, 2, 1, 0, -2])
    s = _spot(lp, (ids, lens), blank=blank, max_hits=2)
    assert s.counts[0, 1:].tolist() == [0, 0, 0, 0, 0] and int(s.counts[0, 0]) > 0
    assert bool((s.hits[0, 1:] == -1).all()) and bool((s.scores[0, 1:] == NEG).all())
    one = _spot(lp, [[1, 3]], blank=blank, max_hits=2)
    assert all(torch.equal(x[0, :1], y[0]) for x, y in zip(s, one))
    long_ = _spot(lp, (ids[:1], torch.tensor([99])), blank=blank, max_hits=2)          # a length above Lmax is clamped to it
    assert all(torch.equal(x, y) for x, y in zip(long_, _spot(lp, [[1, 3, 0]], blank=blank, max_hits=2)))
    assert torch.equal(_spot(lp, ids[:1, :2], blank=blank, max_hits=2).hits, one.hits)  # a bare tensor: every row Lmax long
    for bad, word in (([[1, blank]], "blank"), ([[1, 6]], "outside"), ([[-1]], "outside"), ([[]], "empty"), ([[1] * 33], "more than 32")):
        with pytest.raises(ValueError, match=word) as err:
            S.keyword_spot(lp, bad, blank=blank)
        assert repr(bad[0]) in str(err.value)
    for kw in (dict(max_hits=0), dict(max_hits=9), dict(min_score=float("nan")), dict(blank=V)):
        with pytest.raises(ValueError):
            S.keyword_spot(lp, [[1]], **{"blank": blank, **kw})


def test_minus_infinity_entries_and_rows():
    S = pkg("spot")
    lp, path, spans = R.planted(77, [3, 5], 2, 8, 0, [1, 2, 4, 6])
    lp = lp.copy()
    lp[:, 7] = -np.inf                                                 # a class that is never possible
    hole = spans[1][0]
    lp[hole, :] = -np.inf                                              # the first frame of the second occurrence: no finite maximum
    s = _spot(lp, [[3, 5], [7]], blank=0, max_hits=8, min_score=0.0)
    got = _listed(s)
    want = [spans[0]] if path[hole + 1] != 3 else [spans[0], (hole + 1, spans[1][1])]
    assert sorted((a, b) for a, b, _ in got) == want and int(s.counts[0, 1]) == 0
    e, es = S._host_end_series(lp, [[3, 5]], lp.shape[0], 0)
    assert e[0, hole] == -np.inf and not np.isnan(e).any()
    everything = _spot(lp, [[3, 5]], blank=0, max_hits=8)             # no hit lies across the hole
    assert all(b <= hole or a > hole for a, b, _ in _listed(everything))
    allneg = _spot(np.full((5, 4), -np.inf, np.float32), [[1]], blank=0)
    assert int(allneg.counts[0, 0]) == 0


# ---- inputs and helpers ----
def test_context_bias_and_its_phrases_are_one_input():
    B = pkg("bias")
    lp = torch.from_numpy(np.stack([R.make_log_probs(40 + b, 30, 9) for b in range(2)]))
    cb = B.ContextBias.from_phrases([[1, 2], [3], [4, 4, 5]], vocab_size=9, blank=0)
    a, b = _spot(lp, cb, blank=0), _spot(lp, cb.phrases, blank=0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a.hits.shape == (2, 3, 4, 2)
    ids = torch.tensor([[1, 2, 0], [3, 0, 0], [4, 4, 5]])
    c = _spot(lp, (ids, [2, 1, 3]), blank=0)
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_hit_segments_times_and_names():
    S = pkg("spot")
    hits = torch.full((2, 2, 3, 2), -1, dtype=torch.int32)
    scores = torch.full((2, 2, 3), NEG)
    counts = torch.tensor([[2, 0], [1, 1]], dtype=torch.int32)
    hits[0, 0, 0] = torch.tensor([10, 20]); hits[0, 0, 1] = torch.tensor([50, 55]); scores[0, 0, :2] = torch.tensor([-1.0, -2.5])
    hits[1, 0, 0] = torch.tensor([0, 4]); scores[1, 0, 0] = 0.0
    hits[1, 1, 0] = torch.tensor([7, 8]); scores[1, 1, 0] = -0.5
    seg = S.hit_segments(S.Spots(hits, scores, counts), ["alpha", "beta"], frame_rate=25.0)
    assert seg[0] == [{"keyword": "alpha", "start": 0.4, "end": 0.8, "score": -1.0, "per_frame": -0.1},
                      {"keyword": "alpha", "start": 2.0, "end": 2.2, "score": -2.5, "per_frame": -0.5}]
    assert seg[1] == [{"keyword": "alpha", "start": 0.0, "end": 4 / 25.0, "score": 0.0, "per_frame": 0.0},
                      {"keyword": "beta", "start": 7 / 25.0, "end": 8 / 25.0, "score": -0.5, "per_frame": -0.5}]
    assert S.hit_segments(S.Spots(hits, scores, counts), ["alpha", "beta"], frame_rate=50.0)[1][1]["start"] == 7 / 50.0
    with pytest.raises(ValueError, match="names"):
        S.hit_segments(S.Spots(hits, scores, counts), ["alpha"])


# ---- the C-ABI ----
def test_both_symbols_exported_by_both_libraries_and_bound():
    L = pkg("_lib")
    assert len(L.SIGNATURES["av_ctc_spot_workspace_bytes"]) == 4 and len(L.SIGNATURES["av_ctc_spot"]) == 21
    for lib in _libs():
        for n in NAMES:
            fn = getattr(lib, n)
            assert fn.argtypes is not None and list(fn.argtypes) == list(L.SIGNATURES[n])


def test_argument_errors_are_statuses_with_a_message():
    P = 4096                                     # any non-null address: argument checks come before a launch, nothing is dereferenced
    inf = float("-inf")
    for lib in _libs():
        need = ctypes.c_longlong(-1)
        assert lib.av_ctc_spot_workspace_bytes(2, 10, 3, ctypes.byref(need)) == 0 and need.value == 4 * 2 * 10 * (1 + 2 * 3)
        assert lib.av_ctc_spot_workspace_bytes(64, 100, 100, ctypes.byref(need)) == 0 and need.value == 4 * 64 * 100 * 201
        assert lib.av_ctc_spot_workspace_bytes(2, 10, 3, None) != 0 and b"null" in lib.av_last_error()
        for shape in ((0, 10, 3), (2, 0, 3), (2, 10, 0)):
            assert lib.av_ctc_spot_workspace_bytes(*shape, ctypes.byref(need)) != 0 and b"bad shape" in lib.av_last_error()
        # (log_probs, stride_b, stride_t, input_lengths, keywords, kw_ld, kw_lengths, B, T, V, K, L_max, blank, N, min_score,
        #  out_hits, out_scores, out_counts, workspace, workspace_bytes, stream)
        f = lib.av_ctc_spot
        ws = 4 * 2 * 10 * 7

        def call(**kw):
            a = dict(lp=P, sb=80, st=8, il=None, kw=P, ld=4, kl=P, B=2, T=10, V=8, K=3, L=4, blank=0, N=4, ms=inf, hits=P, scores=P, counts=P,
                     ws=P, wsb=ws, stream=None)
            a.update(kw)
            return f(*a.values())
        for name in ("lp", "kw", "kl", "hits", "scores", "counts", "ws"):
            assert call(**{name: None}) != 0 and b"av_ctc_spot: null" in lib.av_last_error(), name
        for name in ("B", "T", "V", "K"):
            assert call(**{name: 0}) != 0 and b"bad shape" in lib.av_last_error(), name
        for blank in (-1, 8):
            assert call(blank=blank) != 0 and b"blank" in lib.av_last_error()
        for Lmax in (0, 33):
            assert call(L=Lmax, ld=40) != 0 and b"L_max" in lib.av_last_error()
        assert call(ld=3) != 0 and b"kw_ld" in lib.av_last_error()
        for N in (0, 9):
            assert call(N=N) != 0 and b"hits per keyword" in lib.av_last_error()
        assert call(ms=float("nan")) != 0 and b"NaN" in lib.av_last_error()
        assert call(st=4) != 0 and b"strides" in lib.av_last_error()
        assert call(wsb=ws - 1) != 0 and b"workspace" in lib.av_last_error() and b"too small" in lib.av_last_error()
        assert call(ws=P + 2) != 0 and b"workspace" in lib.av_last_error() and b"aligned" in lib.av_last_error()


def test_the_rejected_stride_pairs_of_the_row_law_are_rejected_by_name():
    """The six pairs of tests/test_ctc_rows_law_cpu.py, which cover neither [B][T][V] nor [T][B][V] at B 2, T 4, V 8."""
    P, BIG = 4096, 1 << 40
    rejected = ((8, 8), (31, 8), (8, 15), (7, 32), (-32, 8), (2 ** 62, 2 ** 62))
    for lib in _libs():
        for sb, st in rejected:
            assert lib.av_ctc_spot(P, sb, st, None, P, 2, P, 2, 4, 8, 3, 2, 0, 4, 0.0, P, P, P, P, BIG, None) != 0, (sb, st)
            msg = lib.av_last_error()
            assert b"strides" in msg and b"av_ctc_spot" in msg, (sb, st, msg)


def test_ops_ctc_spot_and_the_trainer_have_no_cpu_fallback():
    lp = torch.log_softmax(torch.randn(2, 5, 8), -1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg("ops").ctc_spot(lp, torch.tensor([[1, 2]]), torch.tensor([2]))
    t = cpu_trainer()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.spot(pkg("dataset.synthetic").make_batch(1, 1.0, seed=1), [[5, 6]])


# ---- the options table ----
def test_options_argument_beats_variable_beats_default(monkeypatch):
    O = pkg("model.options")
    monkeypatch.delenv("AVAMD_SPOT_MIN_SCORE", raising=False); monkeypatch.delenv("AVAMD_SPOT_MAX_HITS", raising=False)
    assert O.resolve("spot_min_score", None) == NEG and O.resolve("spot_max_hits", None) == 4
    monkeypatch.setenv("AVAMD_SPOT_MIN_SCORE", "-7.5"); monkeypatch.setenv("AVAMD_SPOT_MAX_HITS", "2")
    assert O.resolve("spot_min_score", None) == -7.5 and O.resolve("spot_max_hits", None) == 2
    assert O.resolve("spot_min_score", -1) == -1.0 and O.resolve("spot_max_hits", 6) == 6
    t = cpu_trainer()
    assert (t.spot_min_score, t.spot_max_hits) == (-7.5, 2)
    t = cpu_trainer(spot_min_score=-3.0, spot_max_hits=8)
    assert (t.spot_min_score, t.spot_max_hits) == (-3.0, 8)
    O.check_spot(NEG, 1); O.check_spot(0.0, 8)
    for bad in ((0.0, 0), (0.0, 9), (float("nan"), 4)):
        with pytest.raises(ValueError, match="spot_"):
            O.check_spot(*bad)
    with pytest.raises(ValueError, match="spot_max_hits"):
        cpu_trainer(spot_max_hits=9)
