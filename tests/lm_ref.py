"""Shared by tests/test_beam_lm_cpu.py and tests/test_beam_lm_gpu.py: a seeded token corpus, the n-gram model as a dict (n-gram tuple ->
(logp, backoff), float64 copies of the stored float32 values) with the backoff walk written on tuples, and the dict restatement of CTC
prefix beam search with shallow fusion (prefixes as tuples, g per prefix, per frame the K best acoustic tokens plus the live extensions) in
the dtype of its input: float64 = the reference, float32 = the error yardstick.  Written for clarity, not speed.  numpy only at import
time, so that worker processes can compute references without loading torch."""
import concurrent.futures as cf
import multiprocessing as mp

import numpy as np


def make_corpus(seed, sentences, V, blank=0, lo=3, hi=14):
    """Token sentences with structure an n-gram model can learn: the first token is uniform over the non-blank ids; each next token is, with
    probability 0.7, one of three fixed successors of the previous one, else uniform."""
    rng = np.random.default_rng(seed)
    nb = [c for c in range(V) if c != blank]
    succ = {c: [nb[int(x)] for x in rng.integers(len(nb), size=3)] for c in nb}
    out = []
    for _ in range(sentences):
        s = [nb[int(rng.integers(len(nb)))]]
        for _ in range(int(rng.integers(lo, hi)) - 1):
            s.append(succ[s[-1]][int(rng.integers(3))] if rng.random() < 0.7 else nb[int(rng.integers(len(nb)))])
        out.append(s)
    return out


def lm_dict(lm):
    """An lm.NGramLM as plain data: {"order", "V", "bos", "unk", "grams": {tuple: (logp, backoff)}} with float64 copies of its values."""
    grams = {}
    for w in np.flatnonzero(lm.uni_present):
        grams[(int(w),)] = (float(lm.uni[w, 0]), float(lm.uni[w, 1]))
    for key, (lp, bo) in lm.table.items():
        g, k = [], key
        while k:
            g.append((k & 0xFFFF) - 1)
            k >>= 16
        grams[tuple(reversed(g))] = (float(lp), float(bo))
    return {"order": lm.order, "V": lm.vocab_size, "bos": lm.bos, "unk": float(lm.unk_logp), "grams": grams}


def dict_score(D, context, c, Z=np.float64):
    """s(c | context) by the law: the longest stored n-gram ending in c, the backoffs of the contexts that were tried before it."""
    N, grams = D["order"], D["grams"]
    ctx = tuple(context)
    if D["bos"] and len(ctx) < N - 1:
        ctx = (D["V"],) + ctx
    ctx = ctx[len(ctx) - min(len(ctx), N - 1):]
    acc = Z(0.0)
    for m in range(len(ctx), 0, -1):
        h = ctx[len(ctx) - m:]
        e = grams.get(h + (c,))
        if e is not None:
            return acc + Z(e[0])
        e = grams.get(h)
        if e is not None:
            acc = acc + Z(e[1])
    e = grams.get((c,))
    return acc + Z(e[0] if e is not None else D["unk"])


def ref_pbs_lm(lp, W, blank, D, alpha, beta, tokens):
    """The fused law in the dtype of ``lp`` (numpy [T, V]) -> [(ids, score, g)], best first.  alpha and beta are the float32 values the
    device is given.  g(l + c) = g(l) + (alpha s(c | l) + beta), each operation in the dtype; ranking by (p_b (+) p_nb) + g."""
    la = np.logaddexp
    Z = lp.dtype.type
    NEG = Z(-np.inf)
    a, b = Z(np.float32(alpha)), Z(np.float32(beta))
    V = lp.shape[1]
    K = min(tokens, V - 1)
    beams, g = {(): (Z(0.0), NEG)}, {(): Z(0.0)}
    key = lambda kv: (-(la(*kv[1]) + g[kv[0]]), len(kv[0]), kv[0])
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
                if k not in g:
                    g[k] = g[l] + (a * dict_score(D, l, c, Z) + b)
                add(k, NEG, (pb if l and l[-1] == c else tot) + row[c])
        beams = dict(sorted(nxt.items(), key=key)[:W])
        g = {k: g[k] for k in beams}
    return [(list(k), float(la(*v) + g[k]), float(g[k])) for k, v in sorted(beams.items(), key=key)]


def _ref_one(args):
    return ref_pbs_lm(*args)


def references(lps, W, blank, D, alpha, beta, tokens, workers=1):
    """[(float64 n-best, float32 n-best)] of (ids, score, g) triples for a list of float32 [T_b, V] arrays; ``workers`` > 1 spreads the
    runs over fresh (spawned) processes."""
    jobs = [(lp.astype(dt), W, blank, D, alpha, beta, tokens) for lp in lps for dt in (np.float64, np.float32)]
    if workers <= 1:
        out = [_ref_one(j) for j in jobs]
    else:
        with cf.ProcessPoolExecutor(max_workers=min(workers, len(jobs)), mp_context=mp.get_context("spawn")) as ex:
            out = list(ex.map(_ref_one, jobs))
    return list(zip(out[0::2], out[1::2]))


def for_agreement(refs):
    """references(...) in the form beam_ref.check_agreement takes: (ids, score) pairs."""
    return [([(i, s) for i, s, _ in r64], [(i, s) for i, s, _ in r32]) for r64, r32 in refs]


def float32_alone_agrees(refs):
    """The condition on the inputs: the float32 restatement has the float64 one's top hypothesis in every utterance, so the one top-1
    difference in 16 that the agreement rule allows is left to the code under test."""
    return all(r64[0][0] == r32[0][0] for r64, r32 in refs)
