"""Shared by tests/test_beam_bias_cpu.py and tests/test_beam_bias_gpu.py: the phrase law of contextual biasing restated directly on tuples
(the longest suffix that is a prefix of some phrase is found by scanning the phrase list: no trie, no failure links), the dict restatement
of the biased fused CTC prefix beam search in the dtype of its input (float64 = the reference, float32 = the error yardstick; the n-gram
part is tests/lm_ref.py's, by import), and the choice of phrase sets from the unbiased n-best.  Written for clarity, not speed.  numpy only
at import time, so that worker processes can compute references without loading torch."""
import concurrent.futures as cf
import multiprocessing as mp

import numpy as np

import lm_ref as LR


def step(phrases, state, c):
    """(k, tail) -> the state after token c.  tail <- the longest suffix of tail + (c) that is a prefix of some phrase; a tail that is a
    phrase is banked."""
    k, tail = state
    s = tail + (c,)
    best = ()
    for i in range(len(s)):                                                   # longest suffix first
        suf = s[i:]
        if any(p[:len(suf)] == suf for p in phrases):
            best = suf
            break
    if best in phrases:
        return k + len(best), ()
    return k, best


def walk(phrases, ids):
    """[(k, |tail|)] after each token of ids."""
    phrases = set(map(tuple, phrases))
    out, st = [], (0, ())
    for c in ids:
        st = step(phrases, st, int(c))
        out.append((st[0], len(st[1])))
    return out


def ref_pbs_bias(lp, W, blank, D, alpha, beta, tokens, phrases, w):
    """The biased fused law in the dtype of ``lp`` (numpy [T, V]) -> [(ids, score, g_lm, k)], best first after finalisation.  D = lm_ref.lm_dict
    of the language model or None (g_lm = 0 throughout); alpha, beta, w are the float32 values the device is given.
    g(l) = g_lm(l) + w * (k + |tail|) ranks the entries during the search, g_fin = g_lm + w * k after the last frame (stable)."""
    la = np.logaddexp
    Z = lp.dtype.type
    NEG = Z(-np.inf)
    a, b, wz = Z(np.float32(alpha)), Z(np.float32(beta)), Z(np.float32(w))
    phrases = set(map(tuple, phrases))
    V = lp.shape[1]
    K = min(tokens, V - 1)
    beams, glm, st = {(): (Z(0.0), NEG)}, {(): Z(0.0)}, {(): (0, ())}
    g = lambda l: glm[l] + wz * Z(st[l][0] + len(st[l][1]))
    key = lambda kv: (-(la(*kv[1]) + g(kv[0])), len(kv[0]), kv[0])
    for row in lp:
        top = sorted((c for c in range(V) if c != blank and not np.isnan(row[c])), key=lambda c: (-row[c], c))[:K]
        nxt = {}

        def add(k, pb, pnb):
            o = nxt.get(k, (NEG, NEG)); nxt[k] = (la(o[0], pb), la(o[1], pnb))
        for l, (pb, pnb) in beams.items():
            tot = la(pb, pnb)
            add(l, tot + row[blank], pnb + row[l[-1]] if l else NEG)
            live = [k[-1] for k in beams if len(k) == len(l) + 1 and k[:-1] == l]
            for c in sorted(set(top) | set(live)):
                k = l + (c,)
                if k not in glm:
                    glm[k] = glm[l] if D is None else glm[l] + (a * LR.dict_score(D, l, c, Z) + b)
                    st[k] = step(phrases, st[l], c)
                add(k, NEG, (pb if l and l[-1] == c else tot) + row[c])
        beams = dict(sorted(nxt.items(), key=key)[:W])
        glm, st = {k: glm[k] for k in beams}, {k: st[k] for k in beams}
    ranked = sorted(beams.items(), key=key)                                   # the order before finalisation
    fin = lambda kv: la(*kv[1]) + (glm[kv[0]] + wz * Z(st[kv[0]][0]))
    ranked = sorted(ranked, key=lambda kv: -fin(kv))                          # stable: ties go to the entry that ranked earlier
    return [(list(k), float(fin((k, v))), float(glm[k]), st[k][0]) for k, v in ranked]


def _ref_one(args):
    return ref_pbs_bias(*args)


def _run(jobs, workers):
    """ref_pbs_bias over a list of argument tuples; ``workers`` > 1 spreads the runs over fresh (spawned) processes."""
    if workers <= 1:
        return [_ref_one(j) for j in jobs]
    with cf.ProcessPoolExecutor(max_workers=min(workers, len(jobs)), mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(_ref_one, jobs))


def references(lps, W, blank, D, alpha, beta, tokens, phrases, w, workers=1):
    """[(float64 n-best, float32 n-best)] of (ids, score, g_lm, k) for a list of float32 [T_b, V] arrays."""
    out = _run([(lp.astype(dt), W, blank, D, alpha, beta, tokens, phrases, w) for lp in lps for dt in (np.float64, np.float32)], workers)
    return list(zip(out[0::2], out[1::2]))


def unbiased(lps, W, blank, D, alpha, beta, tokens, workers=1):
    """The float64 n-best ids of the same search without phrases: what the phrase sets are drawn from."""
    out = _run([(lp.astype(np.float64), W, blank, D, alpha, beta, tokens, [], 0.0) for lp in lps], workers)
    return [[tuple(h[0]) for h in nb] for nb in out]


def draw_phrases(nbest, V, seed, per_utterance=3, absent=3, blank=0):
    """A phrase set from the unbiased n-best lists: per utterance ``per_utterance`` substrings of length 2..5 of hypotheses of random rank
    (the lower ranks included: those are the ones a positive weight can promote), plus ``absent`` random phrases of length 4 that occur
    in no hypothesis at all."""
    rng = np.random.default_rng(seed)
    out = []
    for hyps in nbest:
        pool = [h for h in hyps if len(h) >= 2]
        for _ in range(per_utterance if pool else 0):
            h = pool[int(rng.integers(len(pool)))]
            n = int(rng.integers(2, min(5, len(h)) + 1))
            i = int(rng.integers(0, len(h) - n + 1))
            out.append(tuple(h[i:i + n]))
    every = [h for hyps in nbest for h in hyps]
    nb = [c for c in range(V) if c != blank]
    while absent > 0:
        p = tuple(nb[int(x)] for x in rng.integers(len(nb), size=4))
        if not any(h[i:i + 4] == p for h in every for i in range(len(h) - 3)):
            out.append(p)
            absent -= 1
    return sorted(set(out))


def for_agreement(refs):
    """references(...) in the form beam_ref.check_agreement takes: (ids, score) pairs."""
    return [([(h[0], h[1]) for h in r64], [(h[0], h[1]) for h in r32]) for r64, r32 in refs]
