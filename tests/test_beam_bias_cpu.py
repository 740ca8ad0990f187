"""CPU: contextual phrase biasing (bias.py: ContextBias; beam_search.prefix_beam_search(bias=...)) without a GPU: the automaton against
the brute-force law of tests/bias_ref.py, its failure links and edge table, the constructor's errors, the host search against the biased
float64 law under the agreement rule of tests/beam_ref.py, the w = 0 identities, finalisation, the argument checks of both libraries and
the trainer's configuration."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer as _trainer
import beam_ref as R
import bias_ref as BR
import lm_ref as LR

V40 = 40
A, B_, C = 1, 2, 3                                                            # the three symbols of the automaton tests; 0 is the blank


def _cb(phrases, V=4, blank=0):
    return pkg("bias").ContextBias.from_phrases(phrases, vocab_size=V, blank=blank)


def _phrase_sets():
    """30 sets over 3 symbols.  Each holds a phrase with a proper prefix, a suffix and an infix of it, the overlapping pair ab / bc, random
    phrases and a 32-token phrase; every third set also holds a single-token phrase (which banks every occurrence of its token)."""
    rng = np.random.default_rng(11)
    sets = []
    for s in range(30):
        rnd = lambda n: tuple(int(x) for x in rng.integers(1, 4, size=n))
        long = rnd(int(rng.integers(4, 7)))
        ps = {long, long[:int(rng.integers(1, len(long) - 1)) + 1], long[-2:], long[1:-1], (A, B_), (B_, C), rnd(32)}
        ps |= {rnd(int(rng.integers(1, 5))) for _ in range(int(rng.integers(2, 5)))}
        if s % 3 == 0:
            ps.add((int(rng.integers(1, 4)),))
        sets.append(sorted(ps))
    return sets


def test_count_is_the_brute_force_law():
    """3000 random sequences of length <= 12 over 3 symbols, 100 per phrase set: k and |tail| after every token."""
    rng = np.random.default_rng(12)
    seen_k = seen_tail = 0
    for ps in _phrase_sets():
        cb = _cb(ps)
        assert any(len(p) == 32 for p in ps) and any(p != q and q[:len(p)] == p for p in ps for q in ps)
        for _ in range(100):
            ids = [int(x) for x in rng.integers(1, 4, size=int(rng.integers(0, 13)))]
            got, want = cb.count(ids), BR.walk(ps, ids)
            assert got.shape == (len(ids), 2) and got.dtype == np.int32
            assert [tuple(r) for r in got.tolist()] == want, (ps, ids)
            assert cb.banked(ids) == (want[-1][0] if want else 0)
            seen_k += bool(want and want[-1][0]); seen_tail += any(t for _, t in want)
        long = next(p for p in ps if len(p) == 32)
        ids = list(long) + [A, B_, C]
        assert [tuple(r) for r in cb.count(ids).tolist()] == BR.walk(ps, ids)
    assert seen_k > 1000 and seen_tail > 1000
    # the blank and ids outside the vocabulary match nothing and end a running match
    cb = _cb([(A, B_, C)])
    assert cb.count([A, B_, 0, C, A, B_, 9, C, A, B_, -1, A, B_, C]).tolist() == [[0, 1], [0, 2], [0, 0], [0, 0], [0, 1], [0, 2], [0, 0], [0, 0],
                                                                              [0, 1], [0, 2], [0, 0], [0, 1], [0, 2], [3, 0]]


def test_the_two_quirks_of_the_law():
    """A phrase that is a proper prefix of another always wins; a phrase strictly inside a longer partial match that fails is not credited."""
    cb = _cb([(A, B_), (A, B_, C)])
    assert cb.count([A, B_, C]).tolist() == [[0, 1], [2, 0], [2, 0]]
    cb = _cb([(C, A, B_, C), (A, B_)])
    assert cb.count([C, A, B_, A]).tolist() == [[0, 1], [0, 2], [0, 3], [0, 1]]
    assert cb.count([A, B_, C, A, B_, C]).tolist() == [[0, 1], [2, 0], [2, 1], [2, 2], [2, 3], [6, 0]]
    assert BR.walk([(C, A, B_, C), (A, B_)], [C, A, B_, A]) == [(0, 1), (0, 2), (0, 3), (0, 1)]


def _paths(cb):
    paths = {0: ()}
    todo = [0]
    while todo:
        n = todo.pop()
        for c, ch in cb.children[n].items():
            paths[ch] = paths[n] + (c,)
            todo.append(ch)
    return paths


def test_failure_links_are_the_deepest_proper_suffix():
    for ps in _phrase_sets()[:10]:
        cb = _cb(ps)
        paths = _paths(cb)
        node_of = {p: n for n, p in paths.items()}
        assert len(paths) == len(cb.children) == len(cb.fail) and len(node_of) == len(paths)
        for n, p in paths.items():
            want = next((node_of[p[i:]] for i in range(1, len(p) + 1) if p[i:] in node_of), 0)
            assert cb.fail[n] == want and cb.depth[n] == len(p) and cb.terminal[n] == (p in set(ps)), (ps, p)


def test_edge_table_layout():
    """Power-of-two size, load <= 0.5, key 0 = empty, every edge found within the recorded probe bound by linear probing from
    splitmix64(key); nodes = (failure link, depth | terminal << 16)."""
    LM = pkg("lm")
    rng = np.random.default_rng(3)
    cb = _cb([tuple(int(x) for x in rng.integers(1, V40, size=int(rng.integers(1, 9)))) for _ in range(300)], V=V40)
    nodes, tab, slots, bound = cb.host_tables()
    edges = {(n << 16) | (c + 1): ch for n, kids in enumerate(cb.children) for c, ch in kids.items()}
    assert nodes.shape == (len(cb.children), 2) and nodes.dtype == np.int32 and tab.shape == (slots, 2) and tab.dtype == np.int64
    assert slots & (slots - 1) == 0 and 2 * len(edges) <= slots < 4 * len(edges)
    keys = tab[:, 0].view(np.uint64)
    vals = np.ascontiguousarray(tab[:, 1]).view(np.int32).reshape(slots, 2)
    assert int((keys != 0).sum()) == len(edges) and not vals[:, 1].any()
    longest = 0
    for key, ch in edges.items():
        i = LM.splitmix64(key) & (slots - 1)
        for run in range(1, bound + 1):
            if int(keys[i]) == key:
                break
            assert keys[i] != 0
            i = (i + 1) & (slots - 1)
        assert int(keys[i]) == key and vals[i, 0] == ch
        longest = max(longest, run)
    assert longest == bound
    assert nodes[:, 0].tolist() == cb.fail and (nodes[:, 1] & 0xFFFF).tolist() == cb.depth and (nodes[:, 1] >> 16).tolist() == [int(x) for x in cb.terminal]
    assert cb.host_tables(slots=4 * slots)[2] == 4 * slots
    with pytest.raises(ValueError):
        cb.host_tables(slots=slots // 2)
    assert _cb([]).host_tables()[0].tolist() == [[0, 0]]                     # no phrases: the root alone


def test_from_phrases_errors_duplicates_and_nested():
    CB = pkg("bias").ContextBias
    tok = pkg("utils.tokenizer").SyntheticTokenizer(800)
    ga, na = chr(0xAC00), chr(0xAC01)
    cb = CB.from_phrases([ga + na, " " + ga, ga + na, [5, 6, 7], (5, 6)], tok)
    assert cb.phrases == [(5, 6), (4, 5), (5, 6, 7)] and cb.vocab_size == 800 and cb.blank == tok.blank_id
    assert cb.nested == [(5, 6)]                                             # a contiguous part of (5, 6, 7): reported, not an error
    assert CB.from_phrases([[5, 6, 7, 8], [6, 7], [7, 8], [5], [9]], vocab_size=20, blank=0).nested == [(5,), (6, 7), (7, 8)]
    for bad, word in (("", "empty"), ([], "empty"), (ga * 33, "more than 32"), ([5, tok.blank_id], "blank"), ("a" + ga, "<unk>"),
                      ([5, 800], "outside"), ([-1], "outside")):
        with pytest.raises(ValueError, match=word) as e:
            CB.from_phrases([ga, bad], tok)
        assert repr(bad) in str(e.value)
    assert len(CB.from_phrases([ga * 32], tok).phrases[0]) == 32
    with pytest.raises(ValueError):
        CB.from_phrases([[1, 2]])                                            # no tokenizer and no vocabulary
    with pytest.raises(ValueError):
        CB.from_phrases(["ab"], vocab_size=10, blank=0)                      # text without a tokenizer


def test_from_file(tmp_path):
    CB = pkg("bias").ContextBias
    tok = pkg("utils.tokenizer").SyntheticTokenizer(800)
    ga, na = chr(0xAC00), chr(0xAC01)
    path = tmp_path / "phrases.txt"
    path.write_text(f"# names\n{ga}{na}\n\n   \n {na}{ga}\n#{ga}\n{ga}{na}\r\n", encoding="utf-8")
    cb = CB.from_file(path, tok)
    assert cb.phrases == [(5, 6), (4, 6, 5)]
    path.write_text(f"{ga}x\n", encoding="utf-8")
    with pytest.raises(ValueError, match="<unk>"):
        CB.from_file(str(path), tok)


# ---- the host search ----
_LMS = {}


def _lm(order=3):
    if order not in _LMS:
        _LMS[order] = pkg("lm").NGramLM.from_corpus(LR.make_corpus(V40 + order, 400, V40), V40, 0, order=order)
    return _LMS[order]


def _search(lp, W, **kw):
    return pkg("beam_search").prefix_beam_search(torch.from_numpy(lp)[None], W, 0, nbest=W, return_scores=True, **kw)


SEED0 = 700                                                                   # chosen on the CPU reference: see _host_case


def _host_case(T, W, K, with_lm, w):
    """16 utterances of V 40, a phrase set drawn from the unbiased float64 n-best of the same inputs (plus phrases that never occur) and
    both references.  The seeds are fixed; that the float32 restatement alone agrees with the float64 one on them (the condition on the
    inputs, as in tests/test_beam_lm_gpu.py) is asserted here."""
    lm = _lm() if with_lm else None
    D = None if lm is None else LR.lm_dict(lm)
    alpha, beta = (0.5, 0.25) if with_lm else (0.0, 0.0)
    lps = [R.make_log_probs(SEED0 + T + s, T, V40) for s in range(16)]
    nbest = BR.unbiased(lps, W, 0, D, alpha, beta, K, workers=8)
    phrases = BR.draw_phrases(nbest, V40, seed=T + W)
    refs = BR.references(lps, W, 0, D, alpha, beta, K, phrases, w, workers=8)
    assert LR.float32_alone_agrees(refs), "these inputs hold a near-tie that the float32 law itself resolves differently: pick other seeds"
    return lm, alpha, beta, lps, nbest, phrases, refs


@pytest.mark.parametrize("w", [2.0, -1.0])
@pytest.mark.parametrize("with_lm", [True, False])
@pytest.mark.parametrize("T,W,K", [(60, 5, 6), (40, 8, 20)])
def test_host_path_against_the_reference_law(T, W, K, with_lm, w):
    """The agreement rule of beam_ref with the biased float64 law as the reference; where the hypotheses match rank by rank, the counts
    are equal and g_lm is within float32 rounding; every returned count is the law's k of its hypothesis.  Biasing is not vacuous: it
    changes the winner of at least one utterance."""
    lm, alpha, beta, lps, nbest, phrases, refs = _host_case(T, W, K, with_lm, w)
    cb = _cb(phrases, V=V40)
    fusion = dict(lm=lm, lm_weight=alpha, token_bonus=beta) if with_lm else {}
    got, changed = [], 0
    for lp, (r64, _), nb in zip(lps, refs, nbest):
        ids, scores, g, counts = _search(lp, W, tokens=K, bias=cb, bias_weight=w, **fusion)
        got.append((ids[0], scores[0]))
        changed += tuple(ids[0][0]) != nb[0]
        for k, i in enumerate(ids[0]):
            assert counts[0][k] == (BR.walk(phrases, i)[-1][0] if i else 0)
            if i == r64[k][0]:
                assert counts[0][k] == r64[k][3]
                assert abs(g[0][k] - r64[k][2]) <= 1e-5 * max(1.0, abs(r64[k][2])), (i, g[0][k], r64[k][2])
        if not with_lm:
            assert all(x == 0.0 for x in g[0])
    R.check_agreement(got, BR.for_agreement(refs), f"host bias T={T} W={W} K={K} lm={with_lm} w={w}")
    print(f"[beam bias] the top hypothesis differs from the unbiased search in {changed} of 16")
    assert changed >= 1


@pytest.mark.parametrize("W", [1, 5, 16])
def test_zero_weight_is_the_search_without_phrases(W):
    """w = 0: with a language model the ids, scores and g of the fused search; without one and with tokens = W + 1 (the default) those of
    the plain search, and g is 0; the counts are still the law's k of every emitted hypothesis."""
    bs = pkg("beam_search")
    lm = _lm()
    lp = torch.from_numpy(np.stack([R.make_log_probs(300 + b, 50, V40) for b in range(4)]))
    kw = dict(lengths=torch.tensor([50, 0, 17, 49]), nbest=W, return_scores=True)
    fusion = dict(lm=lm, lm_weight=0.7, token_bonus=0.25, tokens=7)
    nest = lambda out: [[[x] for x in col] for col in out] if W == 1 else out    # nbest = 1 returns one hypothesis per utterance, not a list
    plain, fused = nest(bs.prefix_beam_search(lp, W, 0, **kw)), nest(bs.prefix_beam_search(lp, W, 0, **kw, **fusion))
    phrases = sorted({tuple(h[i:i + 3]) for u in plain[0] for h in u for i in range(0, max(len(h) - 2, 0), 4)} | {(1, 2)})
    cb = _cb(phrases, V=V40)
    b0 = nest(bs.prefix_beam_search(lp, W, 0, **kw, bias=cb, bias_weight=0.0))
    b1 = nest(bs.prefix_beam_search(lp, W, 0, **kw, **fusion, bias=cb, bias_weight=0.0))
    bits = lambda col: [np.array(u, np.float64).tobytes() for u in col]
    assert b0[0] == plain[0] and bits(b0[1]) == bits(plain[1]) and all(x == 0.0 for u in b0[2] for x in u)
    assert b1[0] == fused[0] and bits(b1[1]) == bits(fused[1]) and bits(b1[2]) == bits(fused[2])
    banked = 0
    for got in (b0, b1):
        for hyps, ks in zip(got[0], got[3]):
            assert len(hyps) == len(ks) and [cb.banked(h) for h in hyps] == ks
            banked += sum(ks)
    assert banked > 0
    assert b0[0][1] == [[]] and b0[1][1] == [0.0] and b0[3][1] == [0]         # length 0: the empty hypothesis, score 0, count 0
    assert bs.prefix_beam_search(lp, W, 0, lengths=kw["lengths"], bias=cb, bias_weight=0.0) == bs.prefix_beam_search(lp, W, 0, lengths=kw["lengths"])


def finalisation_case():
    """Three frames over {blank, 1, 2, 3}: token 1, a blank, then 3 (p 0.5) or 2 (p 0.4).  With the phrase (1, 2, 3) and w = 1 the prefix
    (1, 2) leads during the search on the refundable credit of its partial match (ln 0.4 + 2 > ln 0.5) and loses the lead to (1, 3) when
    that credit is taken back.  -> (log-probs float32 [3][4], phrases, w)."""
    p = np.array([[0.02, 0.94, 0.02, 0.02], [0.94, 0.02, 0.02, 0.02], [0.05, 0.05, 0.40, 0.50]], np.float64)
    return np.log(p).astype(np.float32), [(1, 2, 3)], 1.0


def test_finalisation_takes_the_refundable_credit_back():
    lp, phrases, w = finalisation_case()
    cb = _cb(phrases)
    ids, scores, g, counts = _search(lp, 4, bias=cb, bias_weight=w)
    ids, scores, counts = ids[0], scores[0], counts[0]
    assert ids[0] == [1, 3] and ids[1] == [1, 2] and counts[:2] == [0, 0] and all(x >= y for x, y in zip(scores, scores[1:]))
    assert scores[1] + 2 * w > scores[0]                                     # before finalisation (1, 2) was ahead: its m was 2
    ref = BR.ref_pbs_bias(lp.astype(np.float64), 4, 0, None, 0.0, 0.0, 5, phrases, w)
    assert [r[0] for r in ref[:2]] == [[1, 3], [1, 2]] and abs(ref[0][1] - scores[0]) < 1e-5
    # a completed phrase keeps its credit: with (1, 2) itself in the set it is banked and stays first
    ids2, scores2, _, counts2 = _search(lp, 4, bias=_cb([(1, 2)]), bias_weight=w)
    assert ids2[0][0] == [1, 2] and counts2[0][0] == 2 and abs(scores2[0][0] - (scores[1] + 2 * w)) < 1e-5
    # and without phrases (1, 3) leads throughout
    assert _search(lp, 4)[0][0][0] == [1, 3]


def test_argument_errors():
    bs = pkg("beam_search")
    lp = torch.from_numpy(R.make_log_probs(1, 10, V40))[None]
    cb = _cb([(1, 2)], V=V40)
    with pytest.raises(ValueError, match="bias_weight needs bias"):
        bs.prefix_beam_search(lp, 4, 0, bias_weight=2.0)
    with pytest.raises(ValueError, match="need lm="):
        bs.prefix_beam_search(lp, 4, 0, tokens=5)                            # tokens alone still needs lm= or bias=
    with pytest.raises(ValueError, match="need lm="):
        bs.prefix_beam_search(lp, 4, 0, bias=cb, lm_weight=0.7)
    with pytest.raises(ValueError, match="phrases are over"):
        bs.prefix_beam_search(lp, 4, 0, bias=_cb([(1, 2)], V=41))
    with pytest.raises(ValueError, match="phrases are over"):
        bs.prefix_beam_search(lp, 4, 0, bias=_cb([(1, 2)], V=V40, blank=3))
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="finite"):
            bs.prefix_beam_search(lp, 4, 0, bias=cb, bias_weight=bad)
    with pytest.raises(ValueError, match="tokens"):
        bs.prefix_beam_search(lp, 4, 0, bias=cb, tokens=66)
    assert bs.prefix_beam_search(lp, 4, 0, bias=cb, tokens=9) == bs.prefix_beam_search(lp, 4, 0, bias=cb, tokens=9, bias_weight=1.0)
    with pytest.raises(ValueError, match="on the GPU"):
        cb.count_batch(torch.zeros((2, 3), dtype=torch.int32))


def _libs():
    L = pkg("_lib"); P = pkg("precision")
    old = P.get_precision()
    out = []
    try:
        for mode in ("fp32", "fp16"):
            P.set_precision(mode)
            out.append(L.lib())
    finally:
        P.set_precision(old)
    return out


def test_abi_argument_errors_in_both_libraries():
    P = 4096                                     # any non-null 16-byte aligned address: argument checks come before a launch
    B, T, V = 2, 10, 8
    for lib in _libs():
        need = ctypes.c_longlong(0)
        assert lib.av_ctc_beam_lm_workspace_bytes(B, T, V, 5, 6, ctypes.byref(need)) == 0
        n = need.value
        # (log_probs, stride_b, stride_t, lengths, out_ids, out_len, out_score, out_lm_score, out_bias_count, workspace, workspace_bytes,
        #  B, T, V, blank, beam_width, nbest, tokens, lm_unigrams, lm_table, lm_slots, lm_order, lm_vocab, lm_bos, lm_probe_bound, lm_weight,
        #  token_bonus, bias_nodes, bias_edges, bias_node_count, bias_slots, bias_probe_bound, bias_weight, stream)
        good = [P, T * V, V, None, P, P, P, P, P, P, n, B, T, V, 0, 5, 1, 6, P, P, 16, 3, V, V, 4, 0.5, 0.0, P, P, 3, 16, 2, 1.0, None]
        cases = {0: (None, b"null"), 7: (None, b"null"), 8: (None, b"null"), 9: (None, b"null"), 10: (n - 1, b"workspace"), 14: (V, b"blank"),
                 15: (65, b"beam_width"), 16: (6, b"nbest"), 17: (66, b"tokens"), 18: (None, b"null language-model"), 20: (12, b"power of two"),
                 21: (5, b"lm_order"), 22: (V + 1, b"vocabulary"), 25: (float("nan"), b"finite"), 27: (None, b"null bias"),
                 28: (None, b"null bias"), 29: (0, b"bias_node_count"), 30: (12, b"bias_slots"), 31: (17, b"bias_probe_bound"),
                 32: (float("inf"), b"bias_weight"), 2: (V - 1, b"strides")}
        for where, (value, word) in cases.items():
            a = list(good)
            a[where] = value
            assert lib.av_ctc_beam_search_bias(*a) != 0 and word in lib.av_last_error(), (where, lib.av_last_error())
        a = list(good); a[28] = P + 8
        assert lib.av_ctc_beam_search_bias(*a) != 0 and b"aligned" in lib.av_last_error()
        nolm = list(good); nolm[18:27] = [None, None, 0, 0, 0, -1, 0, float("nan"), 0.0]         # no language model: its arguments are ignored
        nolm[11] = 0                                                                             # B = 0: checked, nothing launched
        assert lib.av_ctc_beam_search_bias(*nolm) == 0, lib.av_last_error()
        nolm[32] = float("nan")
        assert lib.av_ctc_beam_search_bias(*nolm) != 0 and b"bias_weight" in lib.av_last_error()
        # (ids, lens, out, B, Lmax, V, blank, bias_nodes, bias_edges, bias_node_count, bias_slots, bias_probe_bound, stream)
        good = [P, None, P, 2, 5, V, 0, P, P, 3, 16, 2, None]
        for where, value, word in ((0, None, b"null"), (2, None, b"null"), (4, 0, b"bad shape"), (5, 70000, b"65533"), (6, V, b"blank"),
                                   (7, None, b"null bias"), (9, 0, b"bias_node_count"), (10, 24, b"bias_slots"), (11, 0, b"bias_probe_bound"),
                                   (2, P + 4, b"aligned")):
            a = list(good)
            a[where] = value
            assert lib.av_context_bias_count(*a) != 0 and word in lib.av_last_error(), (where, lib.av_last_error())
        a = list(good); a[3] = 0
        assert lib.av_context_bias_count(*a) == 0                             # B = 0: nothing to do


def test_trainer_takes_phrases_only_when_asked(monkeypatch, tmp_path):
    for name in ("AVAMD_EVAL_BEAM", "AVAMD_EVAL_LM", "AVAMD_EVAL_BIAS", "AVAMD_EVAL_BIAS_WEIGHT"):
        monkeypatch.delenv(name, raising=False)
    t = _trainer()
    assert t.eval_bias is None and t.eval_bias_weight == 1.0 and t.eval_beam_width == 0
    tok = pkg("utils.tokenizer").SyntheticTokenizer(800)
    cb = pkg("bias").ContextBias.from_phrases([chr(0xAC00) + chr(0xAC05)], tok)
    with pytest.raises(ValueError, match="eval_bias needs eval_beam_width"):
        _trainer(eval_bias=cb)                                               # phrases with the greedy decode
    t = _trainer(eval_bias=cb, eval_beam_width=4, eval_bias_weight=2.5)
    assert t.eval_bias is cb and t.eval_bias_weight == 2.5 and t.eval_lm is None
    path = tmp_path / "phrases.txt"
    path.write_text(f"# hot words\n{chr(0xAC00)}{chr(0xAC05)}\n {chr(0xAC07)}\n", encoding="utf-8")
    monkeypatch.setenv("AVAMD_EVAL_BIAS", str(path)); monkeypatch.setenv("AVAMD_EVAL_BEAM", "8"); monkeypatch.setenv("AVAMD_EVAL_BIAS_WEIGHT", "0.75")
    t = _trainer()
    assert t.eval_beam_width == 8 and t.eval_bias_weight == 0.75 and t.eval_bias.phrases == [(5, 10), (4, 12)]
    assert _trainer(eval_bias_weight=3.0).eval_bias_weight == 3.0            # an explicit argument wins over the variable
    assert _trainer(eval_bias=cb).eval_bias is cb
    monkeypatch.setenv("AVAMD_EVAL_BEAM", "0")
    with pytest.raises(ValueError):
        _trainer()
