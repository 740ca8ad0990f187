"""An independent float64 reference of CTC keyword spotting, written for the tests.  It is deliberately NOT a restatement of the carried-start
walk of spot.py / csrc/ctc_spot.hip: per start frame it runs a plain Viterbi over the keyword's lattice with no start tracking, which gives
E[s][t] = the best score of a path that enters y_1 at frame s and ends in y_L at frame t; the end series is e64[t] = max_s E[s][t]."""
import numpy as np


def make_log_probs(seed, T, V, scale=3.0):
    """float32 [T, V] log-softmax of seeded normal logits times ``scale``."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, V)) * scale
    x = x - x.max(axis=1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)


def lattice(y, blank):
    """-> (class of each of the S = 2 L - 1 states, whether the transition from two states back exists)."""
    L = len(y)
    lab = [blank] * (2 * L - 1)
    lab[0::2] = [int(i) for i in y]
    skip = [s >= 2 and s % 2 == 0 and lab[s] != lab[s - 2] for s in range(2 * L - 1)]
    return lab, skip


def costs64(lp, y, blank):
    """float64 [T, S]: lp[t][label_s] - max_v lp[t][v] of the float32 input, computed in float64."""
    lab, _ = lattice(y, blank)
    x = np.asarray(lp, np.float64)
    return x[:, lab] - x.max(axis=1, keepdims=True)


def end_scores64(lp, y, blank):
    """E float64 [T, T]: E[s][t] as above, -inf for t < s."""
    lab, skip = lattice(y, blank)
    S, T = len(lab), lp.shape[0]
    c = costs64(lp, y, blank)
    E = np.full((T, T), -np.inf)
    for s0 in range(T):
        d = np.full(S, -np.inf)
        d[0] = c[s0, 0]
        E[s0, s0] = d[S - 1]
        for t in range(s0 + 1, T):
            new = np.full(S, -np.inf)
            for s in range(S):
                best = d[s]
                if s >= 1:
                    best = max(best, d[s - 1])
                if skip[s]:
                    best = max(best, d[s - 2])
                new[s] = best + c[t, s]
            d = new
            E[s0, t] = d[S - 1]
    return E


def bound(lp, y, blank):
    """float64 [T]: 2^-23 (t + 2) sum_{u <= t} max_s |c64[u][s]| - one rounding of c, at most t + 1 additions whose partial sums are bounded
    by the sum of |c|, and a factor of two of margin."""
    a = np.abs(costs64(lp, y, blank)).max(axis=1)
    return 2.0 ** -23 * (np.arange(lp.shape[0]) + 2) * np.cumsum(a)


def planted(seed, keyword, occurrences, V, blank, others, big=12.0):
    """Posteriors whose argmax path is known: fillers of labels from ``others`` (none of them in the keyword) around ``occurrences`` copies of
    the keyword, each label a run of 1 - 3 frames, a blank run between equal neighbours and sometimes between different ones.  The path's
    label has logit ``big`` plus noise in [0, 1), every other class noise alone.
    -> (float32 log-probs [T, V], the frame path, [(first frame of y_1's run, end frame of y_L's run)] per occurrence)."""
    rng = np.random.default_rng(seed)
    path, spans = [], []

    def run(label):
        path.extend([int(label)] * int(rng.integers(1, 4)))

    def filler():
        for _ in range(int(rng.integers(1, 4))):
            run(others[int(rng.integers(0, len(others)))])
    for _ in range(occurrences):
        filler()
        first = len(path)
        for j, c in enumerate(keyword):
            if j and (keyword[j - 1] == c or rng.integers(0, 2)):
                run(blank)
            run(c)
        spans.append((first, len(path)))
    filler()
    T = len(path)
    x = rng.random((T, V))
    x[np.arange(T), path] += big
    x = x - x.max(axis=1, keepdims=True)
    lp = (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)
    assert lp.argmax(axis=1).tolist() == path
    return lp, path, spans
