"""CPU: the token n-gram model (lm.NGramLM: estimation, ARPA round trip, the scoring law against the dict restatement of tests/lm_ref.py,
the hash table's layout) and CTC prefix beam search with its shallow fusion on the host path (beam_search.prefix_beam_search(lm=...))
against the float64 law under the agreement rule of tests/beam_ref.py; the C-ABI's argument errors in both libraries; the trainer's
switches."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer as _trainer
import beam_ref as R
import lm_ref as LR

V40 = 40


def _corpus():
    return LR.make_corpus(1, 400, V40)


def _lm(order=3, bos=True):
    return pkg("lm").NGramLM.from_corpus(_corpus(), V40, 0, order=order, bos=bos)


def _decode(lp, W, lm, **kw):
    return pkg("beam_search").prefix_beam_search(torch.from_numpy(np.asarray(lp)), beam_width=W, blank=0, lm=lm, **kw)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("bos", [True, False])
def test_from_corpus_sums_to_one_for_every_context(order, bos):
    """Interpolated absolute discounting in float64: for every context of the corpus (and for unseen ones, through the backoff walk) the
    probabilities of the non-blank tokens sum to 1 within 1e-12 - including <s>, which at V = 40 and 400 sentences has seen every token:
    the case in which Katz's quotient divides by zero."""
    est = pkg("lm").estimate_interpolated(_corpus(), V40, 0, order, 0.75, bos)
    nb = range(1, V40)
    if bos and order >= 2:
        assert all((V40, w) in est for w in nb), "the corpus does not saturate <s>"

    def p(h, w):
        if not h:
            return est[(w,)][0]
        if h + (w,) in est:
            return est[h + (w,)][0]
        return (est[h][1] if h in est else 1.0) * p(h[1:], w)
    contexts = {g[:-1] for g in est if len(g) > 1} | {(), (5,), (7, 7, 7)[:max(order - 1, 0)]}
    worst = max(abs(sum(p(h, w) for w in nb) - 1.0) for h in contexts)
    print(f"[lm normalisation] order {order} bos {bos}: {len(contexts)} contexts, max |sum - 1| = {worst:.2e}")
    assert worst <= 1e-12


def test_katz_would_divide_by_zero_here():
    """What the interpolated form avoids: <s> has seen every non-blank token, so the seen lower-order mass is 1 and Katz's denominator 0."""
    est = pkg("lm").estimate_interpolated(_corpus(), V40, 0, 2, 0.75, True)
    seen = [w for w in range(1, V40) if (V40, w) in est]
    assert abs(1.0 - sum(est[(w,)][0] for w in seen)) <= 1e-12


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("bos", [True, False])
def test_score_is_the_law_and_arpa_round_trips(order, bos):
    """NGramLM.score equals the dict restatement in float32 bit for bit and the float64 one within float32 rounding, on contexts shorter
    and longer than N - 1, seen and unseen; to_arpa -> from_arpa gives the same float32 values."""
    LM = pkg("lm")
    lm = _lm(order, bos)
    D = LR.lm_dict(lm)
    rng = np.random.default_rng(3)
    for k in range(400):
        n = k % 6
        ctx = [int(x) for x in rng.integers(1, V40, size=n)]
        if k % 2:                                                            # a context the corpus holds
            s = _corpus()[k % 400]
            ctx = s[:min(n, len(s) - 1)]
        c = int(rng.integers(1, V40))
        a = lm.score(ctx, c)
        assert a.dtype == np.float32 and np.isfinite(a)
        assert a.tobytes() == np.float32(LR.dict_score(D, ctx, c, np.float32)).tobytes(), (ctx, c)
        assert abs(float(a) - float(LR.dict_score(D, ctx, c, np.float64))) <= 4 * order * np.finfo(np.float32).eps * 30.0
    back = LM.NGramLM.from_arpa(lm.to_arpa(), lambda w: int(w), vocab_size=V40, blank=0)
    assert (back.order, back.bos, back.vocab_size) == (lm.order, lm.bos, lm.vocab_size)
    assert back.table == lm.table and np.array_equal(back.uni, lm.uni) and back.unk_logp == lm.unk_logp


def test_arpa_specials_and_unknown_tokens(tmp_path):
    """log10 in the file, ln in memory; </s> n-grams are dropped, <unk> sets the score of a token without a unigram, a file is read by path."""
    LM = pkg("lm")
    text = "\n".join(["\\data\\", "ngram 1=5", "ngram 2=3", "", "\\1-grams:", "-2.0\t<unk>", "-99\t<s>\t-0.5", "-1.0\t</s>", "-0.5\ta\t-0.25",
                      "-0.75\tb", "", "\\2-grams:", "-0.1\t<s> a", "-0.2\ta b", "-0.3\tb </s>", "", "\\end\\", ""])
    ids = {"a": 1, "b": 2}
    path = tmp_path / "tiny.arpa"
    path.write_text(text, encoding="utf-8")
    for src in (text, path, str(path)):
        lm = LM.NGramLM.from_arpa(src, ids, vocab_size=4, blank=0)
        assert lm.order == 2 and lm.bos and len(lm.table) == 2
        ln10 = np.log(10.0)
        assert lm.score([], 1) == np.float32(-0.1 * ln10)                    # <s> a
        assert lm.score([1], 2) == np.float32(-0.2 * ln10)
        assert lm.score([2], 1) == np.float32(0.0) + np.float32(-0.5 * ln10)  # b has no backoff
        assert lm.score([1], 1) == np.float32(-0.25 * ln10) + np.float32(-0.5 * ln10)
        assert lm.score([1], 3) == np.float32(-0.25 * ln10) + np.float32(-2.0 * ln10)   # 3 has no unigram: <unk>
        assert lm.score([], 2) == np.float32(-0.5 * ln10) + np.float32(-0.75 * ln10)
    assert LM.NGramLM.from_arpa(text.replace("-2.0\t<unk>\n", "").replace("ngram 1=5", "ngram 1=4"), ids, vocab_size=4).unk_logp == np.float32(-10 * np.log(10.0))
    with pytest.raises(ValueError):
        LM.NGramLM.from_arpa(text, {"a": 1}, vocab_size=4)                   # b is not in the vocabulary


def test_hash_table_layout():
    """Power-of-two size, load <= 0.5, every key found within the recorded probe bound by linear probing from splitmix64(key)."""
    LM = pkg("lm")
    lm = _lm(4)
    uni, tab, slots, bound = lm.host_tables()
    assert uni.shape == (V40 + 1, 2) and uni.dtype == np.float32 and tab.shape == (slots, 2) and tab.dtype == np.int64
    assert slots & (slots - 1) == 0 and 2 * len(lm.table) <= slots < 4 * len(lm.table)
    keys = tab[:, 0].view(np.uint64)
    vals = np.ascontiguousarray(tab[:, 1]).view(np.float32).reshape(slots, 2)
    assert int((keys != 0).sum()) == len(lm.table)
    longest = 0
    for key, (lp, bo) in lm.table.items():
        i = LM.splitmix64(key) & (slots - 1)
        for run in range(1, bound + 1):
            if int(keys[i]) == key:
                break
            assert keys[i] != 0
            i = (i + 1) & (slots - 1)
        assert int(keys[i]) == key and vals[i, 0] == lp and vals[i, 1] == bo
        longest = max(longest, run)
    assert longest == bound
    assert LM.pack_key([0, 5, 39]) == (1 << 32) | (6 << 16) | 40 and LM.unpack_key(LM.pack_key([0, 5, 39])) == (0, 5, 39)
    assert lm.start_ctx == V40 + 1 and _lm(3, bos=False).start_ctx == 0 and _lm(1).start_ctx == 0
    assert lm.host_tables(slots=4 * slots)[2] == 4 * slots
    with pytest.raises(ValueError):
        lm.host_tables(slots=slots // 2)


@pytest.mark.parametrize("order,bos,W,K,alpha,beta", [(3, True, 5, 6, 0.5, 0.0), (4, True, 8, 20, 0.8, 1.0), (2, False, 5, 3, 0.5, 0.0),
                                                      (1, True, 4, 5, 0.8, 1.0)])
def test_host_path_against_the_reference_law(order, bos, W, K, alpha, beta):
    """16 utterances, T 60, V 40: the agreement rule of beam_ref with the fused float64 law as the reference, and g within float32
    rounding of the reference's.  In how many utterances the language model changes the winner is printed; it must be at least one."""
    lm = _lm(order, bos)
    lps = [R.make_log_probs(500 + s, 60, V40) for s in range(16)]
    refs = LR.references(lps, W, 0, LR.lm_dict(lm), alpha, beta, K)
    assert LR.float32_alone_agrees(refs)
    got, gs = [], []
    for lp in lps:
        ids, scores, g = _decode(lp, W, lm, lm_weight=alpha, token_bonus=beta, tokens=K, nbest=W, return_scores=True)
        got.append((ids[0], scores[0])); gs.append(g[0])
    R.check_agreement(got, LR.for_agreement(refs), f"host lm order={order} bos={bos} W={W} K={K} alpha={alpha} beta={beta}")
    for (ids, _), g, (r64, _) in zip(got, gs, refs):
        for k, (i, gk) in enumerate(zip(ids, g)):
            if i == r64[k][0]:
                assert abs(gk - r64[k][2]) <= 1e-5 * max(1.0, abs(r64[k][2])), (i, gk, r64[k][2])
    plain = [pkg("beam_search").prefix_beam_search(torch.from_numpy(lp), W, 0)[0] for lp in lps]
    changed = sum(p != i[0] for p, (i, _) in zip(plain, got))
    print(f"[beam lm] the top hypothesis differs from the search without a language model in {changed} of 16")
    assert changed >= 1


@pytest.mark.parametrize("W", [1, 5, 16])
def test_zero_weights_are_the_search_without_a_language_model(W):
    """alpha = 0, beta = 0, tokens = W + 1 (the default): ids and score bits of prefix_beam_search without lm; g is 0."""
    lm = _lm(3)
    lp = np.stack([R.make_log_probs(300 + b, 50, V40) for b in range(4)])
    lens = torch.tensor([50, 0, 17, 49])
    bs = pkg("beam_search")
    i0, s0 = bs.prefix_beam_search(torch.from_numpy(lp), W, 0, lengths=lens, nbest=W, return_scores=True)
    i1, s1, g1 = bs.prefix_beam_search(torch.from_numpy(lp), W, 0, lengths=lens, nbest=W, return_scores=True, lm=lm, lm_weight=0.0)
    assert i0 == i1
    if W == 1:                                                               # nbest = 1 returns one hypothesis per utterance, not a list of them
        s0, s1, g1 = [[s] for s in s0], [[s] for s in s1], [[g] for g in g1]
    for a, b, g in zip(s0, s1, g1):
        assert np.array(a, np.float64).tobytes() == np.array(b, np.float64).tobytes() and all(x == 0.0 for x in g)
    assert bs.prefix_beam_search(torch.from_numpy(lp), W, 0, lengths=lens, lm=lm, lm_weight=0.0) == bs.prefix_beam_search(
        torch.from_numpy(lp), W, 0, lengths=lens)


def test_g_is_the_sum_of_the_law_over_the_tokens_and_tokens_prunes():
    lm = _lm(3)
    lp = R.make_log_probs(11, 60, V40)
    a, b = np.float32(0.8), np.float32(1.0)
    ids, scores, g = _decode(lp, 6, lm, lm_weight=0.8, token_bonus=1.0, nbest=6, return_scores=True)
    for i, gk in zip(ids[0], g[0]):
        want = np.float32(0.0)
        for k, c in enumerate(i):
            want = want + (a * lm.score(i[:k], c) + b)
        assert np.float32(gk) == want
    assert all(x >= y for x, y in zip(scores[0], scores[0][1:]))
    one = _decode(lp, 6, lm, tokens=1)                                       # one token per frame: only the acoustic argmax may extend
    best = [int(np.argmax(np.where(np.arange(V40) == 0, -np.inf, lp[t]))) for t in range(60)]
    assert all(c in best for c in one[0])


def test_argument_errors():
    lm = _lm(2)
    LM = pkg("lm")
    lp = R.make_log_probs(1, 10, V40)
    for kw in (dict(tokens=0), dict(tokens=66), dict(lm_weight=float("nan")), dict(token_bonus=float("inf"))):
        with pytest.raises(ValueError):
            _decode(lp, 4, lm, **kw)
    with pytest.raises(ValueError):
        _decode(R.make_log_probs(1, 10, V40 + 1), 4, lm)                     # another vocabulary
    with pytest.raises(ValueError):
        pkg("beam_search").prefix_beam_search(torch.from_numpy(lp), 4, 3, lm=lm)   # another blank
    for kw in (dict(tokens=5), dict(lm_weight=0.3), dict(token_bonus=1.0)):   # without lm these would be silently ignored
        with pytest.raises(ValueError):
            pkg("beam_search").prefix_beam_search(torch.from_numpy(lp), 4, 0, **kw)
    with pytest.raises(ValueError):
        LM.NGramLM.from_corpus([[1, 2]], V40, 0, order=5)
    with pytest.raises(ValueError):
        LM.NGramLM.from_corpus([[1, 0]], V40, 0)                             # the blank in a sentence
    with pytest.raises(ValueError):
        LM.NGramLM.from_corpus([[1, 2]], 65534, 0)
    with pytest.raises(ValueError):
        LM.NGramLM(2, V40, 0, {}, {(1, V40): (-1.0, 0.0)})                   # bos predicted
    with pytest.raises(ValueError):
        lm.score([1], V40)
    tok = pkg("utils.tokenizer").SyntheticTokenizer(800)                     # ids 0, 1, 2 are spelled <unk>, <s>, </s>: ARPA's own names
    with pytest.raises(ValueError):
        LM.NGramLM.from_corpus([[0, 7, 8]], 800, tok.blank_id, order=2).to_arpa(tok.id_to_token)


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
        assert lib.av_ctc_beam_lm_workspace_bytes(B, T, V, 5, 6, ctypes.byref(need)) == 0 and need.value > 0
        plain = ctypes.c_longlong(0)
        assert lib.av_ctc_beam_workspace_bytes(B, T, V, 5, ctypes.byref(plain)) == 0 and need.value == plain.value
        assert lib.av_ctc_beam_lm_workspace_bytes(B, T, V, 5, 6, None) != 0
        assert lib.av_ctc_beam_lm_workspace_bytes(B, T, V, 5, 66, ctypes.byref(need)) != 0
        assert lib.av_ctc_beam_lm_workspace_bytes(B, T, V, 5, 0, ctypes.byref(need)) != 0
        n = need.value
        # (log_probs, stride_b, stride_t, lengths, out_ids, out_len, out_score, out_lm_score, workspace, workspace_bytes, B, T, V, blank,
        #  beam_width, nbest, tokens, lm_unigrams, lm_table, lm_slots, lm_order, lm_vocab, lm_bos, lm_probe_bound, lm_weight, token_bonus, stream)
        good = [P, T * V, V, None, P, P, P, P, P, n, B, T, V, 0, 5, 1, 6, P, P, 16, 3, V, V, 4, 0.5, 0.0, None]
        for where, word in ((0, b"null"), (4, b"null"), (7, b"null"), (8, b"null"), (17, b"null"), (18, b"null"), (9, b"workspace"),
                            (13, b"blank"), (14, b"beam_width"), (15, b"nbest"), (16, b"tokens"), (19, b"power of two"), (20, b"lm_order"),
                            (21, b"vocabulary"), (22, b"lm_bos"), (23, b"lm_probe_bound"), (24, b"finite"), (2, b"strides")):
            a = list(good)
            a[where] = {0: None, 4: None, 7: None, 8: None, 17: None, 18: None, 9: n - 1, 13: V, 14: 65, 15: 6, 16: 66, 19: 12, 20: 5,
                        21: V + 1, 22: 3, 23: 17, 24: float("nan"), 2: V - 1}[where]
            assert lib.av_ctc_beam_search_lm(*a) != 0 and word in lib.av_last_error(), (where, lib.av_last_error())
        a = list(good); a[18] = P + 8
        assert lib.av_ctc_beam_search_lm(*a) != 0 and b"aligned" in lib.av_last_error()
        # (ids, lens, out, B, Lmax, lm_unigrams, lm_table, lm_slots, lm_order, lm_vocab, lm_bos, lm_probe_bound, stream)
        assert lib.av_ngram_score(None, None, P, 2, 5, P, P, 16, 3, V, V, 4, None) != 0 and b"null" in lib.av_last_error()
        assert lib.av_ngram_score(P, None, P, 2, 0, P, P, 16, 3, V, V, 4, None) != 0 and b"bad shape" in lib.av_last_error()
        assert lib.av_ngram_score(P, None, P, 2, 5, P, P, 16, 0, V, V, 4, None) != 0 and b"lm_order" in lib.av_last_error()
        assert lib.av_ngram_score(P, None, P, 2, 5, P, P, 16, 3, 70000, -1, 4, None) != 0 and b"lm_vocab" in lib.av_last_error()
        assert lib.av_ngram_score(P, None, P, 0, 5, P, P, 16, 3, V, -1, 4, None) == 0                     # B = 0: nothing to do


def test_workspace_sizes_are_the_closed_forms_in_both_libraries():
    """One layout for both searches: top lists of the frame pass at width wf, then the arena sized for max(W, wf); wf = W without a
    language model, max(tokens - 1, 1) with one (below, equal to and above W)."""
    for lib in _libs():
        for B in (0, 3):
            for T in (1, 37):
                for W in (1, 8, 64):
                    got = ctypes.c_longlong(-1)
                    assert lib.av_ctc_beam_workspace_bytes(B, T, 50, W, ctypes.byref(got)) == 0
                    assert got.value == 8 * B * T * (W + 1) + 8 * B * T * W, (B, T, W, got.value)
                    for tokens in (1, 2, 9, 40, 65):
                        wf = max(tokens - 1, 1)
                        got = ctypes.c_longlong(-1)
                        assert lib.av_ctc_beam_lm_workspace_bytes(B, T, 50, W, tokens, ctypes.byref(got)) == 0
                        assert got.value == 8 * B * T * (wf + 1) + 8 * B * T * max(W, wf), (B, T, W, tokens, got.value)


def test_trainer_uses_a_language_model_only_when_asked(monkeypatch, tmp_path):
    for name in ("AVAMD_EVAL_BEAM", "AVAMD_EVAL_LM", "AVAMD_EVAL_LM_WEIGHT", "AVAMD_EVAL_TOKEN_BONUS"):
        monkeypatch.delenv(name, raising=False)
    t = _trainer()
    assert t.eval_lm is None and t.eval_beam_width == 0 and t.eval_lm_weight == 0.5 and t.eval_token_bonus == 0.0
    tok = pkg("utils.tokenizer").SyntheticTokenizer(800)
    corpus = [[c if c >= 5 else c + 5 for c in s] for s in LR.make_corpus(2, 50, 800, blank=tok.blank_id, lo=3, hi=8)]   # no special pieces: ARPA reserves <s>, </s>, <unk>
    lm = pkg("lm").NGramLM.from_corpus(corpus, 800, tok.blank_id, order=2)
    with pytest.raises(ValueError):
        _trainer(eval_lm=lm)                                                 # a language model with the greedy decode
    t = _trainer(eval_lm=lm, eval_beam_width=4, eval_lm_weight=0.7, eval_token_bonus=0.25)
    assert t.eval_lm is lm and (t.eval_lm_weight, t.eval_token_bonus) == (0.7, 0.25)
    path = tmp_path / "lm.arpa"
    path.write_text(lm.to_arpa(tok.id_to_token), encoding="utf-8")
    monkeypatch.setenv("AVAMD_EVAL_LM", str(path)); monkeypatch.setenv("AVAMD_EVAL_BEAM", "8")
    monkeypatch.setenv("AVAMD_EVAL_LM_WEIGHT", "0.3"); monkeypatch.setenv("AVAMD_EVAL_TOKEN_BONUS", "1.5")
    t = _trainer()
    assert t.eval_beam_width == 8 and (t.eval_lm_weight, t.eval_token_bonus) == (0.3, 1.5)
    assert t.eval_lm.table == lm.table and t.eval_lm.blank == tok.blank_id
    assert np.array_equal(t.eval_lm.uni[5:], lm.uni[5:])                     # the special pieces' own unigrams are not carried by the file
    assert _trainer(eval_lm_weight=0.9).eval_lm_weight == 0.9                # an explicit argument wins over the variable
    monkeypatch.setenv("AVAMD_EVAL_BEAM", "0")
    with pytest.raises(ValueError):
        _trainer()
