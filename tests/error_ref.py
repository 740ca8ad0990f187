"""Independent reference for the error counts of error_rate.py / csrc/error_counts.hip, written the slow, obvious way: strings from
``Tokenizer.decode`` / ``beam_search.fast_decode``, symbols from ``.split()`` / ``list()``, the recurrence over Python tuples
(cost, S, D, I) compared as tuples, and an exhaustive enumerator of every alignment for tiny inputs.  Shares no code with the package."""
import os

from conftest import ROOT, pkg

VOCAB = os.path.join(ROOT, "tests", "golden", "tokenizer800.vocab")


def counts(r, h):
    """(S, D, I, R) of the alignment with the smallest (cost, S, D) between two sequences of hashable symbols."""
    prev = [(j, 0, 0, j) for j in range(len(h) + 1)]                          # (cost, S, D, I): j insertions
    for i in range(1, len(r) + 1):
        cur = [(i, 0, i, 0)]
        for j in range(1, len(h) + 1):
            c, s, d, n = prev[j - 1]
            diag = (c, s, d, n) if r[i - 1] == h[j - 1] else (c + 1, s + 1, d, n)
            c, s, d, n = prev[j]
            dele = (c + 1, s, d + 1, n)
            c, s, d, n = cur[j - 1]
            ins = (c + 1, s, d, n + 1)
            cur.append(min(diag, dele, ins))                                   # tuple order: cost, then S, then D
        prev = cur
    c, s, d, n = prev[-1]
    assert c == s + d + n
    return (s, d, n, len(r))


def enumerate_counts(r, h):
    """The same by brute force: every alignment path, best (cost, S, D) over all of them."""
    best = [None]

    def walk(i, j, s, d, n):
        if i == len(r) and j == len(h):
            k = (s + d + n, s, d)
            if best[0] is None or k < best[0]:
                best[0] = k
            return
        if i < len(r) and j < len(h):
            walk(i + 1, j + 1, s + (r[i] != h[j]), d, n)
        if i < len(r):
            walk(i + 1, j, s, d + 1, n)
        if j < len(h):
            walk(i, j + 1, s, d, n + 1)
    walk(0, 0, 0, 0, 0)
    c, s, d = best[0]
    return (s, d, c - s - d, len(r))


def tokenizer():
    return pkg("utils.tokenizer").Tokenizer(VOCAB)


def ref_text(tok, ids):
    return tok.decode([int(i) for i in ids])


def hyp_text(tok, ids):
    return pkg("beam_search").fast_decode([int(i) for i in ids], tok)


def text_counts(ref: str, hyp: str):
    """{"char": (S, D, I, R), "word": ...} of two decoded strings."""
    return {"char": counts(list(ref), list(hyp)), "word": counts(ref.split(), hyp.split())}


_VOCAB_CASES = []


def vocab_cases(tok):
    """(name, reference ids, hypothesis ids) through tokenizer800.vocab, built once: the same words spelt with other pieces, ids out of
    range, the blank on either side, leading / trailing / doubled spaces, texts that strip to nothing, and random sequences."""
    if _VOCAB_CASES:
        return _VOCAB_CASES
    import numpy as np
    V, blank, sp = tok.vocab_size, tok.blank_id, tok.token_to_id["▁"]
    pid = tok.token_to_id
    spelt = lambda s: tok.encode(s)                                            # one id per character
    sent = "우리나라 사회 문제"
    pieces = [pid["▁우리나라"], pid["▁사회"], pid["▁문제"]]
    assert all(len(tok.id_to_token[i]) > 1 for i in pieces) and tok.decode(pieces) == sent and tok.unk_id not in spelt(sent)
    cases = [
        ("same words, other pieces", spelt(sent), pieces),
        ("other pieces, the other way", pieces, spelt(sent)),
        ("one word differs", spelt("우리나라 사회 문제"), [pid["▁우리나라"], pid["▁그"], pid["▁문제"]]),
        ("word split in two", spelt("우리나라 사회"), [pid["▁우리나라"], pid["▁사"], sp, pid["회"]]),
        ("ids out of range", [-5] + spelt(sent) + [V, 10000], [V + 3] + pieces[:2] + [-1, 2 ** 31 - 1] + pieces[2:]),
        ("blank in the hypothesis", spelt(sent), [blank, pieces[0], blank, blank, pieces[1], pieces[2], blank]),
        ("blank in the reference", spelt("사회") + [blank] + spelt(" 문제"), [pid["▁사회"], blank, pid["▁문제"]]),
        ("leading, trailing, doubled spaces", [sp, sp] + spelt("사회") + [sp, sp] + spelt("문제") + [sp], [sp] + pieces[1:] + [sp, sp, sp]),
        ("doubled space against one", spelt("사회") + [sp, sp] + spelt("문제"), spelt("사회 문제")),
        ("reference strips to nothing", [sp, sp], pieces),
        ("hypothesis strips to nothing", spelt(sent), [sp, blank, sp]),
        ("both strip to nothing", [sp], [blank, sp, sp]),
        ("both empty", [], []),
        ("empty reference", [], pieces),
        ("empty hypothesis", pieces, []),
        ("equal", pieces, pieces),
    ]
    rng = np.random.default_rng(800)
    for k, (lr, lh) in enumerate([(90, 85), (40, 64), (63, 65), (17, 3), (70, 70)]):
        r = rng.integers(sp, V, size=lr)
        r[rng.random(lr) < 0.3] = sp
        h = r.copy()[:lh] if lh <= lr else np.concatenate([r, rng.integers(sp, V, size=lh - lr)])
        edit = rng.random(len(h)) < 0.25
        h[edit] = rng.integers(blank, V, size=int(edit.sum()))               # some become the blank: skipped in a hypothesis
        cases.append((f"random {k}", r.tolist(), h.tolist()))
    _VOCAB_CASES.extend(cases)
    return _VOCAB_CASES


def id_counts(tok, ref_ids, hyp_ids):
    """[token, char, word] x (S, D, I, R) the way evaluate() reads its sequences: the reference through ``decode`` (nothing skipped), the
    hypothesis through ``fast_decode`` (the blank skipped); token level: the ids that contribute a piece."""
    V, blank = tok.vocab_size, tok.blank_id
    rk = [int(i) for i in ref_ids if 0 <= int(i) < V]
    hk = [int(i) for i in hyp_ids if 0 <= int(i) < V and int(i) != blank]
    t = text_counts(ref_text(tok, ref_ids), hyp_text(tok, hyp_ids))
    return [counts(rk, hk), t["char"], t["word"]]
