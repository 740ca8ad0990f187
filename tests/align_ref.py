"""Shared by tests/test_align_cpu.py and tests/test_align_gpu.py: the law of CTC forced alignment restated cell by cell (float64 = the
reference, float32 = the exact restatement the device and the package's host path must equal bit for bit), a brute force over all V^T
frame paths for tiny cases, the float64 score of a given path, and the input generator.  numpy only.

The law: extended label row l' of S = 2 L + 1 states (blank, l1, blank, ..., lL, blank), skip s-2 -> s where l'_s != l'_{s-2};
d[0][0] = lp[0][blank], d[0][1] = lp[0][l1], the rest -inf; d[t][s] = max(d[t-1][s], d[t-1][s-1], skip ? d[t-1][s-2] : -inf) + lp[t][l'_s];
ties go to the smaller move; the final state is S-1 only if strictly better than S-2.  Infeasible: a label outside [0, V) or equal to the
blank, or a final score of -inf."""
import itertools

import numpy as np

from beam_ref import make_log_probs  # noqa: F401  (re-exported: the peaky posterior generator)


def law(lp, target, blank):
    """lp [T_b, V] in float64 or float32 (the arithmetic runs in that dtype), target = the L_b labels -> (states list or None, spans,
    token scores, score); None / [] / [] / -inf for an infeasible utterance.  Written for clarity: plain loops, one cell at a time."""
    Z = lp.dtype.type
    NEG = Z(-np.inf)
    T, V = lp.shape
    target = [int(c) for c in target]
    if any(c < 0 or c >= V or c == blank for c in target):
        return None, [], [], NEG
    if T == 0:
        return ([], [], [], Z(0.0)) if not target else (None, [], [], NEG)
    ext = [blank]
    for c in target:
        ext += [c, blank]
    S = len(ext)
    d = [NEG] * S
    d[0] = lp[0, ext[0]]
    if S > 1:
        d[1] = lp[0, ext[1]]
    back = [[0] * S]
    for t in range(1, T):
        nd, mv = [NEG] * S, [0] * S
        for s in range(S):
            best, m = d[s], 0
            if s >= 1 and d[s - 1] > best:
                best, m = d[s - 1], 1
            if s >= 2 and ext[s] != ext[s - 2] and d[s - 2] > best:
                best, m = d[s - 2], 2
            nd[s] = Z(best + lp[t, ext[s]])
            mv[s] = m
        d = nd
        back.append(mv)
    s = 0 if S == 1 else (S - 1 if d[S - 1] > d[S - 2] else S - 2)
    score = d[s]
    if score == NEG:
        return None, [], [], NEG
    states = [0] * T
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= back[t][s]
    spans, tok = [], []
    for j, c in enumerate(target):
        fr = [t for t in range(T) if states[t] == 2 * j + 1]
        assert fr and fr == list(range(fr[0], fr[-1] + 1)), (j, fr)
        acc = Z(0.0)
        for t in fr:
            acc = Z(acc + lp[t, c])
        spans.append((fr[0], fr[-1] + 1))
        tok.append(acc)
    return states, spans, tok, score


def collapse(ids, blank):
    out, prev = [], None
    for i in ids:
        if i != prev and i != blank:
            out.append(int(i))
        prev = i
    return out


def emitted(states, target, blank):
    """Frame ids of a state path."""
    return [blank if s % 2 == 0 else int(target[s // 2]) for s in states]


def path_score64(lp, states, target, blank):
    """Log-probability of a state path, summed in float64 in frame order."""
    acc = 0.0
    for t, c in enumerate(emitted(states, target, blank)):
        acc += float(lp[t, c])
    return acc


def brute_force(lp, target, blank):
    """Best score over ALL V^T frame paths that collapse to ``target`` (float64) -> score (-inf if none)."""
    T, V = lp.shape
    lp = lp.astype(np.float64)
    best = -np.inf
    for ids in itertools.product(range(V), repeat=T):
        if collapse(ids, blank) == list(target):
            best = max(best, float(sum(lp[t, c] for t, c in enumerate(ids))))
    return best


def repeats(target):
    return sum(1 for a, b in zip(target, target[1:]) if a == b)


def make_case(seed, T, V, L, blank=0, classes=5):
    """(float32 [T, V] log-probs from the peaky generator, L labels drawn from ``classes`` non-blank classes so that repeats abound)."""
    rng = np.random.default_rng(seed)
    pool = [c for c in range(V) if c != blank][:classes]
    return make_log_probs(seed, T, V, blank), [int(pool[int(rng.integers(len(pool)))]) for _ in range(L)]
