"""CPU: the laws of longform.py (window plan, stitch, cut points, segments) against tests/longform_ref.py, the greedy identity of the
segment decode, and the long_* options of the trainer."""
import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer
import longform_ref as R


def _lf():
    return pkg("longform")


def test_plan_exhaustive():
    """Every W <= 16, every admissible S, every F <= 3 W + 5."""
    LF = _lf()
    n = 0
    for W in range(1, 17):
        for S in range(0, (W - 1) // 2 + 1):
            hop = W - 2 * S
            assert hop >= 1
            for F in range(1, 3 * W + 6):
                p = LF.plan_windows(F, W, S)
                starts, cuts, width = R.plan(F, W, S)
                assert (p.starts, p.cuts, p.width, p.hop, p.frames) == (starts, cuts, width, hop, F), (W, S, F)
                if F <= W:
                    assert p.starts == [0] and p.cuts == [0, F] and p.width == F and p.coverage == 1       # one window, not padded
                else:
                    assert p.count == -(-(F - W) // hop) + 1 and p.width == W
                    assert all(a < b for a, b in zip(p.starts, p.starts[1:]))
                    assert p.starts[-1] + W == F                                                       # the last window ends with the recording
                    assert all(s == min(k * hop, F - W) for k, s in enumerate(p.starts))
                assert all(a < b for a, b in zip(p.cuts, p.cuts[1:])) and p.cuts[0] == 0 and p.cuts[-1] == F
                for k, s in enumerate(p.starts):                                                       # every owned frame lies inside its window
                    assert s <= p.cuts[k] and p.cuts[k + 1] <= s + p.width, (W, S, F, k)
                assert p.coverage == R.coverage(F, W, S)
                assert p.audio_window(p.count - 1) == (640 * p.starts[-1], 640 * (p.starts[-1] + p.width))
                n += 1
    assert n == 2700
    for bad in ((0, 0), (4, -1), (4, 2), (5, 3)):
        with pytest.raises(ValueError):
            LF.plan_windows(10, *bad)
    with pytest.raises(ValueError):
        LF.plan_windows(0, 4, 1)


@pytest.mark.parametrize("W,S,F", [(12, 0, 29), (12, 2, 29), (12, 4, 61), (12, 4, 13), (12, 2, 12), (12, 2, 1), (5, 1, 17)])
def test_centre_stitch_is_the_owners_rows(W, S, F):
    LF = _lf()
    p = LF.plan_windows(F, W, S)
    win = R.make_windows(F, 2, p.count, p.width, 7)
    got = LF.stitch(torch.from_numpy(win), p).numpy()
    assert got.dtype == np.float32 and got.shape == (2, F, 7)
    for t in range(F):
        k = R.owner(F, W, S, t)
        assert p.cuts[k] <= t < p.cuts[k + 1]
        assert np.array_equal(got[:, t], win[:, k, t - p.starts[k]])
    assert np.array_equal(got.astype(np.float64), R.stitch(win, F, W, S, "centre"))
    with pytest.raises(ValueError):
        LF.stitch(torch.from_numpy(win), p, "middle")
    with pytest.raises(ValueError):
        LF.stitch(torch.zeros(2, p.count + 1, p.width, 7), p)


def _lse(x):
    m = x.max(-1)
    return m + np.log(np.exp(x - m[..., None]).sum(-1))


@pytest.mark.parametrize("W,S,F", [(12, 0, 29), (12, 2, 29), (12, 4, 61), (12, 4, 29), (12, 4, 13), (12, 2, 12), (9, 3, 40)])
def test_average_stitch(W, S, F):
    """Rows stay distributions.  Bound: every element is M + log(acc); acc carries at most 6 float32 roundings and an exp, the log and the
    final sum one each, the inputs are rounded once - below 2^-23 (max |x| + 8) in all, and a row's logsumexp errs no more than its elements."""
    LF = _lf()
    p = LF.plan_windows(F, W, S)
    V = 37
    win = R.make_windows(100 + F, 2, p.count, p.width, V)
    got = LF.stitch(torch.from_numpy(win), p, "average").numpy()
    bound = 2.0 ** -23 * (float(np.abs(win).max()) + 8.0)
    lse = np.abs(_lse(got.astype(np.float64)))
    print(f"[longform cpu] average W={W} S={S} F={F}: coverage {p.coverage}, |logsumexp| {lse.max():.2e}, bound {bound:.2e}")
    assert lse.max() <= bound
    want = R.stitch(win, F, W, S, "average")
    assert np.abs(got - want).max() <= bound
    row, _ = p.sources("average")
    single = (row >= 0).sum(1) == 1
    assert single.any() or S > 0
    for t in np.nonzero(single)[0]:                                                                    # bit copies
        assert np.array_equal(got[:, t].view(np.int32), win.reshape(2, -1, V)[:, row[t, 0]].view(np.int32))
    assert (row >= 0).sum(1).max() == p.coverage == R.coverage(F, W, S)


def test_average_stitch_edge_values_and_coverage_limit():
    LF = _lf()
    W, S, F, V = 12, 4, 29, 5
    p = LF.plan_windows(F, W, S)
    assert p.coverage == 4
    win = R.make_windows(3, 1, p.count, p.width, V)
    t = 10                                                                                            # under windows 0, 1, 2
    ks = [k for k, s in enumerate(p.starts) if s <= t < s + W]
    assert len(ks) >= 3
    for k in ks:
        win[0, k, t - p.starts[k], 1] = -np.inf                                                        # -inf in every source: -inf
    win[0, ks[0], t - p.starts[ks[0]], 2] = -np.inf                                                    # -inf in one source: finite
    win[0, ks[1], t - p.starts[ks[1]], 3] = np.nan                                                     # a NaN source: NaN
    got = LF.stitch(torch.from_numpy(win), p, "average").numpy()
    want = R.stitch(win, F, W, S, "average")
    assert got[0, t, 1] == -np.inf and np.isfinite(got[0, t, 2]) and np.isnan(got[0, t, 3])
    ok = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == -np.inf, want == -np.inf)
    assert np.abs(got[ok] - want[ok]).max() <= 2.0 ** -23 * (float(np.abs(win[np.isfinite(win)]).max()) + 8.0)
    # five windows over a frame: W = 12, hop = 2
    q = LF.plan_windows(40, 12, 5)
    assert q.coverage > 4
    with pytest.raises(ValueError, match=r"smallest hop .* is 4\b"):
        LF.stitch(torch.zeros(1, q.count, 12, V), q, "average")
    assert LF.stitch(torch.zeros(1, q.count, 12, V), q, "centre").shape == (1, 40, V)
    assert LF.min_average_hop(12) == 4 and LF.min_average_hop(100) == 34


def _log_probs(F, V, seed):
    return torch.log_softmax(2 * torch.randn(2, F, V, generator=torch.Generator().manual_seed(seed)), -1)


@pytest.mark.parametrize("F", [1, 12, 13, 25, 26, 29, 45, 46, 61, 150])
def test_cut_points_against_the_ref(F):
    """segment 30, radius 5: N = 20.  F = 26 is the first length with a boundary (20 + 5 < 26, its zone ends at F - 1), F = 25 the last without."""
    LF = _lf()
    V, blank, segment, radius = 6, 2, 30, 5
    lp = _log_probs(F, V, F)
    nb = LF.boundaries(F, segment, radius)
    assert nb == R.boundaries(F, segment, radius) == max(0, (F - 6) // 20)
    if nb:
        lo = 15
        lp[0, lo:lo + 11, blank] = -0.25                                   # a tie over the whole zone: the first frame
        lp[1, lo + 2, blank] = float("nan")                                # a NaN is never the cut
        lp[1, lo + 3, blank] = lp[1, lo + 6, blank] = 0.0                  # a tie of two: the first
    cuts = LF.cut_points(lp, blank, segment, radius)
    assert cuts.dtype == torch.int32 and tuple(cuts.shape) == (2, nb + 2)
    for s in range(2):
        assert cuts[s].tolist() == R.cut_points(lp[s, :, blank].numpy(), segment, radius), (F, s)
        c = cuts[s].tolist()
        assert c[0] == 0 and c[-1] == F and all(1 <= b - a <= segment for a, b in zip(c, c[1:]))
    if nb:
        assert int(cuts[0, 1]) == 15 and int(cuts[1, 1]) == 18
    seg, ln = LF.split_segments(lp, cuts, segment)
    assert seg.dtype == torch.float32 and tuple(seg.shape) == (2 * (nb + 1), segment, V) and ln.dtype == torch.int64
    for s in range(2):
        want, wl = R.segments(lp[s].numpy(), cuts[s].tolist(), segment)
        assert np.array_equal(seg[s * (nb + 1):(s + 1) * (nb + 1)].numpy().view(np.int32), want.view(np.int32))
        assert ln[s * (nb + 1):(s + 1) * (nb + 1)].tolist() == wl


def test_cut_points_all_nan_zone_and_bad_arguments():
    LF = _lf()
    lp = _log_probs(50, 4, 1)
    lp[0, 15:26, 0] = float("nan")                                         # every frame of the zone ranks as -inf: the first
    lp[1, 15:26, 0] = float("-inf")
    cuts = LF.cut_points(lp, 0, 30, 5)
    assert cuts[:, 1].tolist() == [15, 15]
    assert cuts[0].tolist() == R.cut_points(lp[0, :, 0].numpy(), 30, 5)
    for seg, rad in ((30, 8), (409, 5), (30, -1), (0, 0)):
        with pytest.raises(ValueError):
            LF.cut_points(lp, 0, seg, rad)
    with pytest.raises(ValueError):
        LF.cut_points(lp, 4, 30, 5)
    assert LF.cut_points(lp, 0, 408, 101).shape == (2, 2)                   # N = 206 >= 203


def _greedy_joined(C, LF, lp, blank, segment, radius):
    cuts = LF.cut_points(lp, blank, segment, radius)
    seg, ln = LF.split_segments(lp, cuts, segment)
    g = C.greedy_timed(seg, blank, ln)
    ids, spans, conf = [], [], []
    for j in range(seg.shape[0]):
        n, c = int(g.lengths[j]), int(cuts[0, j])
        ids += g.ids[j, :n].tolist()
        spans += (g.spans[j, :n] + c).tolist()
        conf += g.token_conf[j, :n].view(torch.int32).tolist()
    return cuts, ids, spans, conf


def test_greedy_identity():
    """Every zone holds an argmax-blank frame: the segments' greedy ids, spans (+ c_j) and token confidences, joined, are those of the whole."""
    C = pkg("confidence"); LF = _lf()
    F, V, blank, segment, radius = 150, 9, 0, 30, 5
    for seed in range(6):
        gen = torch.Generator().manual_seed(seed)
        x = 2 * torch.randn(1, F, V, generator=gen)
        rep = torch.randint(1, 6, (F,), generator=gen)                     # runs of equal argmax frames, some of them blank
        sym = torch.randint(0, V, (F,), generator=gen)
        t = 0
        while t < F:
            x[0, t:t + int(rep[t]), int(sym[t])] += 12.0
            t += int(rep[t])
        for j in range(1, LF.boundaries(F, segment, radius) + 1):
            x[0, j * 20 - 5 + (seed + j) % 11, blank] += 40.0              # one certain blank frame somewhere in the zone
        lp = torch.log_softmax(x, -1)
        arg = lp[0].argmax(-1)
        for j in range(1, LF.boundaries(F, segment, radius) + 1):          # the condition of the identity, on the inputs
            assert bool((arg[j * 20 - 5:j * 20 + 6] == blank).any())
        cuts, ids, spans, conf = _greedy_joined(C, LF, lp, blank, segment, radius)
        assert all(int(arg[c]) == blank for c in cuts[0, 1:-1].tolist())
        whole = C.greedy_timed(lp, blank)
        n = int(whole.lengths[0])
        assert n > 20 and ids == whole.ids[0, :n].tolist()
        assert spans == whole.spans[0, :n].tolist()
        assert conf == whole.token_conf[0, :n].view(torch.int32).tolist()


def test_greedy_double_emission_without_a_blank_frame():
    """A run of one token over a whole zone: the cut takes the best blank posterior inside the run, and the run is emitted on both sides."""
    C = pkg("confidence"); LF = _lf()
    F, V, blank = 40, 5, 0
    x = torch.zeros(1, F, V)
    x[0, :, blank] = 6.0
    x[0, 3:6, 2] = 9.0
    x[0, 12:30, 3] = 9.0                                                   # covers the zone [15, 25]
    x[0, 21, blank] = 8.0                                                  # the best blank posterior of the zone, still below the token
    x[0, 33:35, 4] = 9.0
    lp = torch.log_softmax(x, -1)
    assert not bool((lp[0, 15:26].argmax(-1) == blank).any())
    cuts, ids, spans, _ = _greedy_joined(C, LF, lp, blank, 30, 5)
    assert cuts[0].tolist() == [0, 21, 40]
    whole = C.greedy_timed(lp, blank)
    assert whole.ids[0, :3].tolist() == [2, 3, 4] and whole.spans[0, 1].tolist() == [12, 30]
    assert ids == [2, 3, 3, 4] and spans == [[3, 6], [12, 21], [21, 30], [33, 35]]


def test_options(monkeypatch):
    options = pkg("model.options")
    want = {"long_window": ("AVAMD_LONG_WINDOW", 100), "long_stride": ("AVAMD_LONG_STRIDE", 12), "long_policy": ("AVAMD_LONG_POLICY", "centre"),
            "long_batch": ("AVAMD_LONG_BATCH", 16), "long_segment": ("AVAMD_LONG_SEGMENT", 400), "long_radius": ("AVAMD_LONG_RADIUS", 50)}
    for name, (var, default) in want.items():
        monkeypatch.delenv(var, raising=False)
        assert options.OPTIONS[name][0] == var and options.resolve(name, None) == default
    options.check_longform(100, 12, "centre", 16, 400, 50)
    options.check_longform(12, 4, "average", 1, 30, 5)
    bad = [(0, 0, "centre", 16, 400, 50),          # window >= 1
           (100, -1, "centre", 16, 400, 50),       # stride >= 0
           (100, 50, "centre", 16, 400, 50),       # hop >= 1
           (100, 12, "middle", 16, 400, 50),       # policy
           (100, 40, "average", 16, 400, 50),      # hop 20 < 34: more than 4 sources
           (100, 12, "centre", 0, 400, 50),        # batch >= 1
           (100, 12, "centre", 16, 409, 50),       # segment <= 408
           (100, 12, "centre", 16, 400, 100),      # N = 200 < 201
           (100, 12, "centre", 16, 400, -1)]       # radius >= 0
    for args in bad:
        with pytest.raises(ValueError):
            options.check_longform(*args)
    t = cpu_trainer()
    assert (t.long_window, t.long_stride, t.long_policy, t.long_batch, t.long_segment, t.long_radius) == (100, 12, "centre", 16, 400, 50)
    monkeypatch.setenv("AVAMD_LONG_WINDOW", "50"); monkeypatch.setenv("AVAMD_LONG_POLICY", "average")
    t = cpu_trainer(long_stride=5)
    assert (t.long_window, t.long_stride, t.long_policy) == (50, 5, "average")
    with pytest.raises(ValueError):
        cpu_trainer(long_stride=25)
    with pytest.raises(ValueError):
        cpu_trainer(long_segment=500)
    monkeypatch.delenv("AVAMD_LONG_WINDOW"); monkeypatch.delenv("AVAMD_LONG_POLICY")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu_trainer().transcribe_long({"audio": torch.zeros(640), "lip1": torch.zeros(1, 1, 96, 96), "lip2": torch.zeros(1, 1, 96, 96)})
