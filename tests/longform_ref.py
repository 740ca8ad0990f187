"""The laws of longform.py restated in plain Python and float64, independently of it: the window plan, the two stitch policies, the cut
points and the segments.  Loops over frames and windows, no tables."""
import math

import numpy as np


def plan(F, W, S):
    """-> (starts, cuts, width): windows [s, s + width), window k owns [cuts[k], cuts[k + 1])."""
    hop = W - 2 * S
    assert W >= 1 and S >= 0 and hop >= 1 and F >= 1
    if F <= W:
        return [0], [0, F], F
    starts = [0]
    while starts[-1] + W < F:                              # one more window as long as the recording is not covered to its end
        starts.append(min(len(starts) * hop, F - W))
    cuts = [0] + [(a + b + W) // 2 for a, b in zip(starts, starts[1:])] + [F]
    return starts, cuts, W


def coverage(F, W, S):
    starts, _, width = plan(F, W, S)
    return max(sum(1 for s in starts if s <= t < s + width) for t in range(F))


def owner(F, W, S, t):
    _, cuts, _ = plan(F, W, S)
    return max(k for k in range(len(cuts) - 1) if cuts[k] <= t)


def stitch(win, F, W, S, policy):
    """win [Sp, nw, width, V] (any float dtype) -> float64 [Sp, F, V]."""
    win = np.asarray(win, np.float64)
    starts, cuts, width = plan(F, W, S)
    Sp, nw, wd, V = win.shape
    assert nw == len(starts) and wd == width
    out = np.empty((Sp, F, V), np.float64)
    for t in range(F):
        if policy == "centre":
            k = owner(F, W, S, t)
            out[:, t] = win[:, k, t - starts[k]]
            continue
        ks = [k for k, s in enumerate(starts) if s <= t < s + width]
        w = [min(t - starts[k] + 1, starts[k] + width - t) for k in ks]
        for sp in range(Sp):
            for v in range(V):
                x = [win[sp, k, t - starts[k], v] for k in ks]
                if any(math.isnan(a) for a in x):
                    out[sp, t, v] = math.nan
                elif max(x) == -math.inf:
                    out[sp, t, v] = -math.inf
                elif len(x) == 1:
                    out[sp, t, v] = x[0]
                else:
                    M = max(x)
                    out[sp, t, v] = M + math.log(sum(wk / sum(w) * math.exp(a - M) for wk, a in zip(w, x))) if M != math.inf else math.inf
    return out


def boundaries(F, segment, radius):
    N = segment - 2 * radius
    assert radius >= 0 and N >= 2 * radius + 1
    j = 0
    while (j + 1) * N + radius < F:
        j += 1
    return j


def cut_points(col, segment, radius):
    """One speaker's blank column [F] -> list of nb + 2 cuts.  The compare is on the float32 values."""
    col = [float(np.float32(c)) for c in col]
    F, N = len(col), segment - 2 * radius
    cuts = [0]
    for j in range(1, boundaries(F, segment, radius) + 1):
        best, bt = None, None
        for t in range(j * N - radius, j * N + radius + 1):
            if not 1 <= t <= F - 1:
                continue
            x = -math.inf if math.isnan(col[t]) else col[t]
            if best is None or x > best:
                best, bt = x, t
        cuts.append(bt)
    return cuts + [F]


def segments(lp, cuts, segment):
    """lp [F, V], cuts of one speaker -> (seg [len(cuts) - 1, segment, V] float32, lengths)."""
    lp = np.asarray(lp, np.float32)
    seg = np.zeros((len(cuts) - 1, segment, lp.shape[1]), np.float32)
    for j, (a, b) in enumerate(zip(cuts, cuts[1:])):
        for i in range(b - a):
            seg[j, i] = lp[a + i]
    return seg, [b - a for a, b in zip(cuts, cuts[1:])]


def make_windows(seed, Sp, nw, width, V, scale=3.0):
    """Normal log-softmax rows, float32 [Sp, nw, width, V]."""
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((Sp, nw, width, V))).astype(np.float64)
    x = x - np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)) - x.max(-1, keepdims=True)
    return x.astype(np.float32)
