"""Shared by tests/test_beam_cpu.py and tests/test_beam_gpu.py: the seeded posterior generator, the reference restatement of CTC prefix
beam search (full-vocabulary expansion, prefixes in a dict - written for clarity, not speed), the exact CTC likelihood and the agreement
rule.  numpy only at import time, so that worker processes can compute references without loading torch."""
import concurrent.futures as cf
import multiprocessing as mp

import numpy as np

SCORE_FLOOR = 1e-4          # floor of the score tolerance
SCORE_FACTOR = 8.0          # x the float32-vs-float64 error of the reference law on the same input: merge order and libm differ on the device


def make_log_probs(seed, T, V, blank=0):
    """Peaky synthetic posterior, float32 [T, V]: runs of 1-3 frames of a random token (+4.0, and +4 U(0,1) on one random distractor per
    run frame) separated by gaps of 0-3 blank frames (+4.0 on blank), over 2 randn noise; log_softmax in float32."""
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((T, V))).astype(np.float32)
    nb = [c for c in range(V) if c != blank]
    t = 0
    while t < T:
        tok = nb[int(rng.integers(len(nb)))]
        for _ in range(int(rng.integers(1, 4))):
            if t >= T:
                break
            x[t, tok] += np.float32(4.0)
            x[t, nb[int(rng.integers(len(nb)))]] += np.float32(4.0 * rng.random())
            t += 1
        for _ in range(int(rng.integers(0, 4))):
            if t >= T:
                break
            x[t, blank] += np.float32(4.0)
            t += 1
    m = x.max(axis=1, keepdims=True)
    e = x - m
    return (e - np.log(np.exp(e).sum(axis=1, keepdims=True, dtype=np.float32))).astype(np.float32)


def ref_pbs(lp, W, blank):
    """The law, in the dtype of ``lp`` (numpy [T, V]; float64 = the reference, float32 = the error yardstick) -> [(ids, score)], best first."""
    la = np.logaddexp
    Z = lp.dtype.type
    NEG = Z(-np.inf)
    beams = {(): (Z(0.0), NEG)}
    key = lambda kv: (-la(*kv[1]), len(kv[0]), kv[0])
    for row in lp:
        nxt = {}

        def add(k, pb, pnb):
            o = nxt.get(k, (NEG, NEG)); nxt[k] = (la(o[0], pb), la(o[1], pnb))
        for l, (pb, pnb) in beams.items():
            tot = la(pb, pnb)
            add(l, tot + row[blank], pnb + row[l[-1]] if l else NEG)
            for c in range(len(row)):
                if c != blank:
                    add(l + (c,), NEG, (pb if l and l[-1] == c else tot) + row[c])
        beams = dict(sorted(nxt.items(), key=key)[:W])
    return [(list(k), float(la(*v))) for k, v in sorted(beams.items(), key=key)]


def _ref_one(args):
    lp, W, blank = args
    return ref_pbs(lp, W, blank)


def references(lps, W, blank, workers=1):
    """[(float64 n-best, float32 n-best)] for a list of float32 [T_b, V] arrays; ``workers`` > 1 spreads the runs over fresh (spawned)
    processes - the reference expands the whole vocabulary for every entry and takes seconds per utterance at V = 800."""
    jobs = [(lp.astype(dt), W, blank) for lp in lps for dt in (np.float64, np.float32)]
    if workers <= 1:
        out = [_ref_one(j) for j in jobs]
    else:
        with cf.ProcessPoolExecutor(max_workers=min(workers, len(jobs)), mp_context=mp.get_context("spawn")) as ex:
            out = list(ex.map(_ref_one, jobs))
    return list(zip(out[0::2], out[1::2]))


def exact_loglik(lp, ids, blank):
    """log p(ids | lp) summed over ALL alignments, float64 (= -F.ctc_loss)."""
    import torch
    import torch.nn.functional as F
    x = torch.as_tensor(np.asarray(lp), dtype=torch.float64)[:, None, :]
    tg = torch.tensor([list(ids)], dtype=torch.long).reshape(1, len(ids))
    nll = F.ctc_loss(x, tg, torch.tensor([x.shape[0]]), torch.tensor([len(ids)]), blank=blank, reduction="sum", zero_infinity=False)
    return -float(nll)


def check_agreement(got, refs, what):
    """The agreement rule.  got: per utterance (id lists, scores) of the code under test with nbest = W; refs: references(...).
    Top-1 ids equal the float64 reference's in all but at most 1 utterance in 16, and a differing one is a genuine near-tie: it is in the
    reference's n-best list with a reference score within the tolerance of the reference's best.  Scores of hypotheses whose ids match
    (rank by rank) are within max(1e-4, 8 x e32), e32 = the float32 reference's own error against float64 on these inputs.
    Returns (largest score error, tolerance, top-1 mismatches) and prints them."""
    e32 = 0.0
    for r64, r32 in refs:
        s64 = {tuple(i): s for i, s in r64}
        for i, s in r32:
            if tuple(i) in s64 and np.isfinite(s64[tuple(i)]):
                e32 = max(e32, abs(s - s64[tuple(i)]))
    tol = max(SCORE_FLOOR, SCORE_FACTOR * e32)
    worst, mismatches, compared = 0.0, 0, 0
    for u, ((ids, scores), (r64, _)) in enumerate(zip(got, refs)):
        assert len(ids) == len(scores) == len(r64), (what, u, len(ids), len(r64))
        assert all(not np.isnan(s) for s in scores), (what, u)
        if ids[0] != r64[0][0]:
            mismatches += 1
            s64 = {tuple(i): s for i, s in r64}
            assert tuple(ids[0]) in s64, f"{what}: utterance {u}: top hypothesis {ids[0]} is not in the reference's n-best list"
            assert abs(s64[tuple(ids[0])] - r64[0][1]) <= tol, (what, u, s64[tuple(ids[0])], r64[0][1], tol)
        for k, (i, s) in enumerate(zip(ids, scores)):
            if i == r64[k][0] and np.isfinite(r64[k][1]):
                compared += 1
                worst = max(worst, abs(s - r64[k][1]))
    print(f"[beam agreement] {what}: utterances={len(got)} top-1 mismatches={mismatches} matched hypotheses={compared} "
          f"max|score - ref|={worst:.3e} e32={e32:.3e} tol={tol:.3e}")
    assert mismatches <= len(got) // 16, f"{what}: {mismatches} top-1 mismatches in {len(got)} utterances"
    assert compared >= len(got) - mismatches, f"{what}: only {compared} hypotheses matched the reference rank by rank"
    assert worst <= tol, f"{what}: score error {worst:.3e} > {tol:.3e}"
    return worst, tol, mismatches
