"""Shared by tests/test_segment_cpu.py and tests/test_segment_gpu.py: the law of CTC segmentation (segmentation.py's docstring) restated
cell by cell - plain Python loops, np.float32 scalars, nothing shared with the package - and the case builders of both files.  numpy only.

The law: the lattice of align_ref.law; emissions lp[t][l'_s] with fixed ends, lp[t][l'_s] - max_v lp[t][v] (all -inf where the maximum is
not finite) with a free end on either side; a fresh start (move 3) at states 0 and 1 of frames t >= 1 only if 0 beats the ordinary moves
strictly; the end at the first frame with the greatest c[t] = better of d[t][S-1], d[t][S-2]; frame scores, token scores, and per utterance
the mean frame score and the least mean of its windows."""
import numpy as np

from beam_ref import make_log_probs  # noqa: F401  (re-exported: the peaky posterior generator)

Z = np.float32
NEG = Z(-np.inf)


def law(lp, target, blank, free, utterances, w):
    """lp float32 [T_b, V], target = the L_b labels, utterances = list of (begin, end) -> dict of the eight outputs of one item, all of
    length T_b / L_b / U (the caller pads).  One cell at a time."""
    T, V = lp.shape
    target = [int(c) for c in target]
    L = len(target)
    U = len(utterances)
    out = {"states": [-1] * T, "spans": [(-1, -1)] * L, "token_scores": [Z(0.0)] * L, "score": NEG, "frame_scores": [Z(0.0)] * T,
           "utt_spans": [(-1, -1)] * U, "utt_means": [Z(0.0)] * U, "utt_scores": [Z(0.0)] * U}
    if any(c < 0 or c >= V or c == blank for c in target):
        return out
    if T == 0:
        if L == 0:
            out["score"] = Z(0.0)
        return out
    ext = [blank]
    for c in target:
        ext += [c, blank]
    S = len(ext)

    def emission(t, s):
        x = Z(lp[t, ext[s]])
        if not free:
            return x
        m = NEG
        for v in range(V):
            if lp[t, v] > m:                                                   # a NaN never wins
                m = Z(lp[t, v])
        if not np.isfinite(m):
            return NEG
        with np.errstate(invalid="ignore"):
            return Z(x - m)

    def ending(d):
        if S == 1:
            return d[0], 0
        return (d[S - 1], S - 1) if d[S - 1] > d[S - 2] else (d[S - 2], S - 2)

    with np.errstate(invalid="ignore"):
        d = [NEG] * S
        d[0] = emission(0, 0)
        if S > 1:
            d[1] = emission(0, 1)
        back = [[0] * S]
        end_c, end_s = ending(d)
        end_t = 0
        for t in range(1, T):
            nd, mv = [NEG] * S, [0] * S
            for s in range(S):
                best, m = d[s], 0
                if s >= 1 and d[s - 1] > best:
                    best, m = d[s - 1], 1
                if s >= 2 and ext[s] != ext[s - 2] and d[s - 2] > best:
                    best, m = d[s - 2], 2
                if (free & 1) and s < 2 and Z(0.0) > best:
                    best, m = Z(0.0), 3
                nd[s] = Z(best + emission(t, s))
                mv[s] = m
            d = nd
            back.append(mv)
            c, s = ending(d)
            if free & 2:
                if c > end_c:
                    end_c, end_s, end_t = c, s, t
            elif t == T - 1:
                end_c, end_s, end_t = c, s, t
    if end_c == NEG:
        return out
    out["score"] = Z(end_c)
    t, s = end_t, end_s
    while True:
        out["states"][t] = s
        out["frame_scores"][t] = emission(t, s)
        if back[t][s] == 3 or t == 0:
            break
        s -= back[t][s]
        t -= 1

    def total(a, z):
        acc = Z(0.0)
        for i in range(a, z):
            acc = Z(acc + out["frame_scores"][i])
        return acc

    for j in range(L):
        fr = [i for i in range(T) if out["states"][i] == 2 * j + 1]
        if fr:
            assert fr == list(range(fr[0], fr[-1] + 1)), (j, fr)
            out["spans"][j] = (fr[0], fr[-1] + 1)
            out["token_scores"][j] = total(fr[0], fr[-1] + 1)
    for u, (b0, e0) in enumerate(utterances):
        if not 0 <= b0 < e0 <= L:
            continue
        f, g = out["spans"][b0][0], out["spans"][e0 - 1][1]
        if f < 0 or g <= f:
            continue
        out["utt_spans"][u] = (f, g)
        out["utt_means"][u] = Z(total(f, g) / Z(g - f))
        low = None
        k = f
        while k < g:
            z = min(k + w, g)
            mean = Z(total(k, z) / Z(z - k))
            if low is None or mean < low:
                low = mean
            k = z
        out["utt_scores"][u] = low
    return out


def repeats(target):
    return sum(1 for a, b in zip(target, target[1:]) if a == b)


def labels(rng, pool, L, reps):
    """L labels from ``pool`` with exactly ``reps`` equal neighbours."""
    same = set(rng.choice(L - 1, size=reps, replace=False).tolist()) if reps else set()
    out = [int(pool[int(rng.integers(len(pool)))])]
    for i in range(1, L):
        out.append(out[-1] if (i - 1) in same else int(rng.choice([c for c in pool if c != out[-1]])))
    assert repeats(out) == reps
    return out


def matrix(T, V, Lmax, blank):
    """The items of the test matrix at one shape -> (lp float32 [6, T, V], targets int64 [6, Lmax] padded with the blank, input lengths,
    target lengths, utterances int32 [6, 5, 2]).  Items: T frames with Lmax labels | 0 frames, no labels | 1 frame, 1 label | T-1 frames,
    all labels equal | T/2 frames exactly tight (T_b = L_b + repeats: a single path) | T/2 frames, one short (infeasible).  Utterances of
    every item: the first third of Lmax, a range after a gap, an empty range, (-1, -1), a range that ends past Lmax (past every L_b)."""
    rng = np.random.default_rng(T * 1009 + V * 7 + blank)
    pool = [c for c in range(V) if c != blank][:5]
    h = T // 2
    tight_L = min(Lmax, (h + 1) // 2 + h // 6)
    assert h - tight_L + 1 <= tight_L - 1
    items = [(T, labels(rng, pool, Lmax, min(Lmax // 5, T - Lmax))), (0, []), (1, [pool[1]]), (T - 1, [pool[2]] * min(Lmax, T // 2)),
             (h, labels(rng, pool, tight_L, h - tight_L)), (h, labels(rng, pool, tight_L, h - tight_L + 1))]
    B = len(items)
    lp = np.stack([make_log_probs(71000 + T + 17 * b + blank, T, V, blank) for b in range(B)])
    tg = np.full((B, Lmax), blank, np.int64)
    for b, (_, lab) in enumerate(items):
        tg[b, :len(lab)] = lab
    il = np.array([x[0] for x in items], np.int64)
    tl = np.array([len(x[1]) for x in items], np.int64)
    a = max(Lmax // 3, 1)
    ut = np.tile(np.array([[0, a], [a + 1, min(a + 1 + a, Lmax)], [2, 2], [-1, -1], [Lmax - 1, Lmax + 1]], np.int32), (B, 1, 1))
    ut[2, 0] = (0, 1)                                                           # the one-label item has an utterance of its own
    return lp, tg, il, tl, ut, items
