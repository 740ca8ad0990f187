"""GPU: contextual phrase biasing on the device in both libraries: av_context_bias_count against the host law, the biased search
(csrc/ctc_beam.hip, beam_search.prefix_beam_search(bias=...)) against the biased float64 law of tests/bias_ref.py under the agreement rule of
tests/beam_ref.py, against av_ctc_beam_search_lm and av_ctc_beam_search at weight zero, against the package's host path, for determinism
and output padding, on the finalisation case, and as the opt-in of MultimodalTrainer.evaluate()."""
import numpy as np
import pytest
import torch

from conftest import pkg
import beam_ref as R
import bias_ref as BR
import lm_ref as LR
from test_beam_bias_cpu import finalisation_case

pytestmark = pytest.mark.gpu

PAD = 24                    # the device input is a [B, T, V] view of a [B, T, V + PAD] block whose padding holds NaN: strided, and never read


@pytest.fixture(params=["fp32", "fp16"])
def library(request):
    """libavhip.so and libavhip_f16.so (decoding is float32 in both)."""
    P = pkg("precision")
    old = P.get_precision()
    P.set_precision(request.param)
    yield request.param
    P.set_precision(old)


def _strided(lp):
    B, T, V = lp.shape
    block = torch.full((B, T, V + PAD), float("nan"), dtype=torch.float32, device="cuda")
    block[:, :, :V] = torch.from_numpy(lp).cuda()
    view = block[:, :, :V]
    assert view.stride(1) == V + PAD and not view.is_contiguous()
    return view


_LMS = {}


def _lm(V, order=3):
    if (V, order) not in _LMS:
        _LMS[(V, order)] = pkg("lm").NGramLM.from_corpus(LR.make_corpus(V + order, 400, V), V, 0, order=order)
    return _LMS[(V, order)]


def _cb(phrases, V, blank=0):
    return pkg("bias").ContextBias.from_phrases(phrases, vocab_size=V, blank=blank)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---- (a) the automaton ----
def test_count_is_the_host_law(library):
    """B 16, Lmax 40, V 40: sequences made of phrases, parts of phrases and random tokens, with blanks and ids outside the vocabulary among
    them; lengths from 0 to beyond Lmax (clamped).  The ids are a view of a wider block: the columns past Lmax, and every position past an
    item's length, hold the token that would complete a phrase."""
    V, B, Lmax = 40, 16, 40
    rng = np.random.default_rng(21)
    rnd = lambda n: tuple(int(x) for x in rng.integers(1, V, size=n))
    long = rnd(32)
    single = next(c for c in range(3, V) if c not in long)
    phrases = [long, long[3:9], (single,), (1, 2), (2, 3), (1, 2, 3, 4)] + [rnd(int(rng.integers(2, 7))) for _ in range(40)]
    cb = _cb(phrases, V)
    assert cb.nested
    block = torch.full((B, Lmax + 8), 2, dtype=torch.int32)                   # 2 completes (1, 2)
    lens = []
    for b in range(B):
        row = list(long) if b == 1 else []                                    # the 32-token phrase, whole
        while len(row) < Lmax:
            p = cb.phrases[int(rng.integers(len(cb.phrases)))]
            kind = int(rng.integers(5))
            row += list(p) if kind < 2 else list(p[:-1]) if kind == 2 else list(rnd(3)) if kind == 3 else [int(rng.choice([0, -1, V, 70000, -2**31]))]
        n = [0, Lmax, Lmax + 5, 2**40, -3][b] if b < 5 else int(rng.integers(1, Lmax))
        lens.append(n)
        n = min(max(n, 0), Lmax)
        if n > 0:
            row[n - 1] = 1                                                   # ... so that the 2 after it would bank (1, 2)
        block[b, :n] = torch.tensor(row[:n], dtype=torch.int32)
    ids = block.cuda()[:, :Lmax]
    assert not ids.is_contiguous()
    got = cb.count_batch(ids, lens).cpu().numpy()
    want = np.zeros((B, Lmax, 2), np.int32)
    for b in range(B):
        n = min(max(lens[b], 0), Lmax)
        want[b, :n] = cb.count(block[b, :n].tolist())
        assert [tuple(x) for x in want[b, :n].tolist()] == BR.walk(cb.phrases, [c if 0 < c < V else -1 for c in block[b, :n].tolist()])
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert want[:, :, 0].max() >= 32 and want[:, :, 1].max() >= 4
    assert np.array_equal(cb.count_batch(ids).cpu().numpy()[1], want[1])      # no lens: Lmax


# ---- (b) the biased search against the float64 law ----
SHAPES = [(8, 60, 40, 5, 6), (16, 100, 800, 16, 17), (4, 40, 800, 64, 65)]
_CASES = {}


def _case(B, T, V, W, K, with_lm, w):
    """Inputs, ragged lengths, a phrase set drawn from the unbiased float64 n-best of the same inputs (plus phrases that never occur) and
    both references of one shape, computed once for both libraries.  The seeds are fixed; that the float32 restatement alone agrees with
    the float64 one on them (the condition on the inputs, as in tests/test_beam_lm_gpu.py) is asserted here."""
    key = (B, T, V, W, K, with_lm, w)
    if key not in _CASES:
        lp = np.stack([R.make_log_probs(52000 + 1000 * W + T + b, T, V) for b in range(B)])
        rng = np.random.default_rng(T * 131 + W)
        lens = [T if b % 3 == 0 else int(rng.integers(T // 3, T)) for b in range(B)]
        lm = _lm(V) if with_lm else None
        D = None if lm is None else LR.lm_dict(lm)
        alpha, beta = (0.5, 0.25) if with_lm else (0.0, 0.0)
        rows = [lp[b, :lens[b]] for b in range(B)]
        ukey = (B, T, V, W, K, with_lm)
        if ukey not in _CASES:
            _CASES[ukey] = BR.unbiased(rows, W, 0, D, alpha, beta, K, workers=16)
        phrases = BR.draw_phrases(_CASES[ukey], V, seed=T + W)
        refs = BR.references(rows, W, 0, D, alpha, beta, K, phrases, w, workers=16)
        assert LR.float32_alone_agrees(refs), "these inputs hold a near-tie that the float32 law itself resolves differently: pick other seeds"
        _CASES[key] = (lp, lens, lm, alpha, beta, phrases, refs, _CASES[ukey])
    return _CASES[key]


@pytest.mark.parametrize("w", [2.0, -1.0])
@pytest.mark.parametrize("with_lm", [True, False])
@pytest.mark.parametrize("B,T,V,W,K", SHAPES)
def test_device_against_the_reference_law(library, B, T, V, W, K, with_lm, w):
    """The gate of test_device_against_the_reference_law in tests/test_beam_lm_gpu.py (the agreement rule: tolerance max(1e-4, 8 e32), at
    most one near-tie in 16 utterances; g within 1e-5 relative where the hypotheses match) with nbest = W on strided input with ragged
    lengths.  Where a hypothesis matches the reference's rank by rank its count is the reference's, and every returned count is the law's
    k of its hypothesis.  Biasing changes the winner of at least one utterance."""
    lp, lens, lm, alpha, beta, phrases, refs, plain = _case(B, T, V, W, K, with_lm, w)
    cb = _cb(phrases, V)
    fusion = dict(lm=lm, lm_weight=alpha, token_bonus=beta) if with_lm else {}
    ids, scores, g, counts = pkg("beam_search").prefix_beam_search(_strided(lp), W, 0, lengths=torch.tensor(lens, device="cuda"), nbest=W,
                                                                   return_scores=True, tokens=K, bias=cb, bias_weight=w, **fusion)
    R.check_agreement(list(zip(ids, scores)), BR.for_agreement(refs), f"device bias {library} B={B} T={T} V={V} W={W} K={K} lm={with_lm} w={w}")
    matched = 0
    for u, (r64, _) in enumerate(refs):
        assert [cb.banked(i) for i in ids[u]] == counts[u]
        for k, i in enumerate(ids[u]):
            if i == r64[k][0]:
                matched += 1
                assert counts[u][k] == r64[k][3], (u, k, counts[u][k], r64[k][3])
                assert abs(g[u][k] - r64[k][2]) <= 1e-5 * max(1.0, abs(r64[k][2])), (u, k, g[u][k], r64[k][2])
        if not with_lm:
            assert all(x == 0.0 for x in g[u])
    assert matched >= B
    if w > 0:
        assert sum(map(sum, counts)) > 0                                     # a negative weight drives completed phrases out of the beam
    assert sum(tuple(ids[u][0]) != plain[u][0] for u in range(B)) >= 1


# ---- (c) weight zero: the searches without phrases ----
def _raw(lp, lens, W, nbest, tokens, lm=None, alpha=0.0, beta=0.0, cb=None, w=0.0):
    """The C entry points on pre-filled outputs -> host copies of (ids, lengths, scores[, g[, counts]]).  cb: av_ctc_beam_search_bias;
    else lm: av_ctc_beam_search_lm; else av_ctc_beam_search."""
    L = pkg("_lib"); ops = pkg("ops")
    B, T, V = lp.shape
    need = L.ll(0)
    if lm is None and cb is None:
        L.check(L.lib().av_ctc_beam_workspace_bytes(B, T, V, W, L.C.byref(need)))
    else:
        L.check(L.lib().av_ctc_beam_lm_workspace_bytes(B, T, V, W, tokens, L.C.byref(need)))
    ws = torch.empty(((need.value + 7) // 8,), dtype=torch.int64, device="cuda")
    out = torch.full((B, nbest, T), 12345, dtype=torch.int32, device="cuda")
    cnt = torch.full((B, nbest), 12345, dtype=torch.int32, device="cuda")
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda")
    gl = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda")
    kb = torch.full((B, nbest), 12345, dtype=torch.int32, device="cuda")
    head = (ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(lens), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc))
    d = None if lm is None else lm.to_device("cuda")
    lm_args = (None, None, 0, 0, 0, -1, 0, 0.0, 0.0) if d is None else (ops.ptr(d.unigrams), ops.ptr(d.table), d.slots, d.order, d.vocab_size,
                                                                        d.bos, d.probe_bound, alpha, beta)
    if cb is not None:
        db = cb.to_device("cuda")
        L.check(L.lib().av_ctc_beam_search_bias(*head, ops.ptr(gl), ops.ptr(kb), ops.ptr(ws), need.value, B, T, V, 0, W, nbest, tokens, *lm_args,
                                                ops.ptr(db.nodes), ops.ptr(db.edges), db.node_count, db.slots, db.probe_bound, w, ops.stream()),
                "av_ctc_beam_search_bias")
        res = (out, cnt, sc, gl, kb)
    elif lm is not None:
        L.check(L.lib().av_ctc_beam_search_lm(*head, ops.ptr(gl), ops.ptr(ws), need.value, B, T, V, 0, W, nbest, tokens, *lm_args, ops.stream()),
                "av_ctc_beam_search_lm")
        res = (out, cnt, sc, gl)
    else:
        L.check(L.lib().av_ctc_beam_search(*head, ops.ptr(ws), need.value, B, T, V, 0, W, nbest, ops.stream()), "av_ctc_beam_search")
        res = (out, cnt, sc)
    torch.cuda.synchronize()
    return tuple(x.cpu() for x in res)


def _phrases_of(out, cnt, V, seed):
    """Substrings of the emitted hypotheses (so that counts are not all zero) and a few random phrases."""
    rng = np.random.default_rng(seed)
    hyps = [out[b, k, :int(cnt[b, k])].tolist() for b in range(out.shape[0]) for k in range(min(out.shape[1], 3)) if int(cnt[b, k]) >= 3]
    ps = {tuple(h[i:i + 3]) for h in hyps for i in range(0, len(h) - 2, 5)}
    return sorted(ps | {tuple(int(x) for x in rng.integers(1, V, size=4)) for _ in range(5)})


@pytest.mark.parametrize("V,W", [(40, 5), (800, 64)])
def test_weight_zero_equals_the_searches_without_phrases(library, V, W):
    """w = 0, bit for bit (the int32 views): with a language model the ids, lengths, scores and g of av_ctc_beam_search_lm; without one
    and with tokens = W + 1 the ids, lengths and scores of av_ctc_beam_search, and g = 0.  The counts are still the law's k of every
    emitted hypothesis, and some are not zero."""
    B, T = 5, 90
    lp = _strided(np.stack([R.make_log_probs(77 + b, T, V) for b in range(B)]))
    lens = torch.tensor([90, 3, 0, 64, 89], device="cuda")
    lm = _lm(V)
    plain = _raw(lp, lens, W, W, W + 1)
    cb = _cb(_phrases_of(plain[0], plain[1], V, W), V)
    for base, got in ((plain, _raw(lp, lens, W, W, W + 1, cb=cb)),
                      (_raw(lp, lens, W, W, 7, lm, 0.7, 0.25), _raw(lp, lens, W, W, 7, lm, 0.7, 0.25, cb=cb))):
        for x, y in zip(base, got):
            assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32))
        if len(base) == 3:
            assert bool((got[3] == 0).all())
        out, cnt, kb = got[0], got[1], got[4]
        want = [[cb.banked(out[b, k, :int(cnt[b, k])].tolist()) if int(cnt[b, k]) >= 0 else 0 for k in range(W)] for b in range(B)]
        assert kb.tolist() == want and kb.sum() > 0


# ---- (d) host and device ----
@pytest.mark.parametrize("T,V,W,K,with_lm,w", [(60, 40, 5, 6, True, 2.0), (40, 40, 8, 20, False, -1.0), (50, 800, 6, 9, True, 2.0),
                                               (25, 9, 16, 17, False, 2.0)])
def test_host_and_device_paths_agree(library, T, V, W, K, with_lm, w):
    """Same law, same order, same tie rule: equal ids and counts, g equal bit for bit, scores within max(1e-4, 8 x the float32 law's own
    error) as in tests/test_beam_lm_gpu.py; V = 9 expands every token; lengths include 0 (the empty hypothesis, score 0, count 0) and 1."""
    bs = pkg("beam_search")
    B = 6
    lm = _lm(V) if with_lm else None
    D = None if lm is None else LR.lm_dict(lm)
    alpha, beta = (0.8, 1.0) if with_lm else (0.0, 0.0)
    fusion = dict(lm=lm, lm_weight=alpha, token_bonus=beta) if with_lm else {}
    lp = torch.from_numpy(np.stack([R.make_log_probs(400 + T + b, T, V) for b in range(B)]))
    lens = torch.tensor([T, 0, T // 2, 1, T - 1, T])
    rows = [lp[b, :int(lens[b])].numpy() for b in (0, 2, 4, 5)]
    phrases = BR.draw_phrases(BR.unbiased(rows, W, 0, D, alpha, beta, K), V, seed=T)
    cb = _cb(phrases, V)
    hi, hs, hg, hk = bs.prefix_beam_search(lp, W, 0, lengths=lens, nbest=W, return_scores=True, tokens=K, bias=cb, bias_weight=w, **fusion)
    di, ds, dg, dk = bs.prefix_beam_search(lp.cuda(), W, 0, lengths=lens.cuda(), nbest=W, return_scores=True, tokens=K, bias=cb, bias_weight=w,
                                           **fusion)
    refs = BR.references(rows, W, 0, D, alpha, beta, K, phrases, w)
    e32 = 0.0                                                                # as in beam_ref.check_agreement
    for r64, r32 in refs:
        s64 = {tuple(h[0]): h[1] for h in r64}
        e32 = max([e32] + [abs(h[1] - s64[tuple(h[0])]) for h in r32 if tuple(h[0]) in s64 and np.isfinite(s64[tuple(h[0])])])
    tol = max(R.SCORE_FLOOR, R.SCORE_FACTOR * e32)
    for b in range(B):
        fin = [k for k, s in enumerate(hs[b]) if np.isfinite(s)]               # entries without any alignment tie at -inf
        assert [di[b][k] for k in fin] == [hi[b][k] for k in fin], (b, di[b], hi[b])
        assert len(di[b]) == len(hi[b])
        assert [dk[b][k] for k in fin] == [hk[b][k] for k in fin]
        assert np.array_equal(_bits([dg[b][k] for k in fin]), _bits([hg[b][k] for k in fin]))
        assert all(abs(ds[b][k] - hs[b][k]) <= tol for k in fin), (b, ds[b], hs[b], tol)
    assert di[1] == [[]] and ds[1] == [0.0] and dg[1] == [0.0] and dk[1] == [0]
    assert w < 0 or sum(map(sum, dk)) > 0                                    # a negative weight drives completed phrases out of the beam
    assert bs.prefix_beam_search(lp.cuda(), W, 0, lengths=lens, tokens=K, bias=cb, bias_weight=w, **fusion) == [h[0] for h in hi]


# ---- (e) determinism and padding ----
@pytest.mark.parametrize("W,nbest,K,with_lm", [(5, 5, 6, True), (16, 7, 40, False), (64, 64, 65, True)])
def test_runs_are_bit_identical_and_outputs_are_padded(library, W, nbest, K, with_lm):
    B, T, V = 5, 120, 300
    lm = _lm(V) if with_lm else None
    lp = _strided(np.stack([R.make_log_probs(77 + b, T, V) for b in range(B)]))
    lens = torch.tensor([120, 3, 0, 64, 119], device="cuda")
    plain = _raw(lp, lens, W, min(W, 3), W + 1)
    cb = _cb(_phrases_of(plain[0], plain[1], V, W), V)
    a, b = _raw(lp, lens, W, nbest, K, lm, 0.5, 0.25, cb, 1.5), _raw(lp, lens, W, nbest, K, lm, 0.5, 0.25, cb, 1.5)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32))
    out, cnt, sc, gl, kb = a
    assert not torch.isnan(sc).any() and not torch.isnan(gl).any()
    for i in range(B):
        for k in range(nbest):
            n = int(cnt[i, k])
            assert -1 <= n <= int(lens[i])
            if n < 0:                                                        # fewer than nbest hypotheses exist (length 0: only the empty one)
                assert sc[i, k] == float("-inf") and gl[i, k] == 0.0 and kb[i, k] == 0 and bool((out[i, k] == -1).all())
                continue
            assert bool((out[i, k, n:] == -1).all()) and bool(((out[i, k, :n] >= 1) & (out[i, k, :n] < V)).all())
            assert int(kb[i, k]) == cb.banked(out[i, k, :n].tolist())
        valid = [k for k in range(nbest) if int(cnt[i, k]) >= 0]
        assert valid == list(range(len(valid))) and len(valid) >= 1
        s = sc[i, :len(valid)].tolist()
        assert all(x >= y for x, y in zip(s, s[1:])), s                       # non-increasing after finalisation
        assert len({tuple(out[i, k, :int(cnt[i, k])].tolist()) for k in valid}) == len(valid)            # hypotheses are distinct prefixes
    assert int(cnt[2, 0]) == 0 and float(sc[2, 0]) == 0.0 and float(gl[2, 0]) == 0.0 and int(kb[2, 0]) == 0 and bool((cnt[2, 1:] == -1).all())
    assert int(kb.sum()) > 0


# ---- (f) finalisation ----
def test_finalisation_on_the_device(library):
    """The constructed case of tests/test_beam_bias_cpu.py: (1, 2) leads on refundable credit and (1, 3) wins once it is taken back; the
    device gives the host path's order, counts and scores."""
    bs = pkg("beam_search")
    lp, phrases, w = finalisation_case()
    cb = _cb(phrases, 4)
    lp = torch.from_numpy(lp)[None]
    hi, hs, _, hk = bs.prefix_beam_search(lp, 4, 0, nbest=4, return_scores=True, bias=cb, bias_weight=w)
    di, ds, dg, dk = bs.prefix_beam_search(lp.cuda(), 4, 0, nbest=4, return_scores=True, bias=cb, bias_weight=w)
    assert di[0][:2] == [[1, 3], [1, 2]] and di == hi and dk == hk and dk[0][:2] == [0, 0]
    assert np.allclose(ds[0], hs[0], atol=1e-5, rtol=0) and ds[0][1] + 2 * w > ds[0][0]
    assert bs.prefix_beam_search(lp.cuda(), 4, 0, bias=_cb([(1, 2)], 4), bias_weight=w) == [[1, 2]]


# ---- (g) evaluate() ----
def test_evaluate_uses_the_phrases_only_when_asked(tmp_path):
    """evaluate() with eval_beam_width = 8 and nothing else set calls the search exactly as before (the same arguments, no bias among
    them) and returns what it returned; with eval_bias the bias object and its weight arrive, with and without eval_lm; eval_bias with
    the greedy decode is an error."""
    from test_dataset_gpu import _Tok, _make_corpus
    from test_step_gpu import build as build_trainer
    ds = pkg("dataset.multi_speaker_dataset"); cf = pkg("dataset.collate_fn").collate_fn; init = pkg("utils.init"); bs = pkg("beam_search")
    _, sents = _make_corpus(tmp_path)
    pairs = [(sents[0], sents[2]), (sents[1], sents[3]), (sents[2], sents[1]), (sents[3], sents[0])]
    loader = torch.utils.data.DataLoader(ds.FixedSentencePairDataset(pairs, _Tok()), batch_size=2, shuffle=False, collate_fn=cf, num_workers=0)
    t = build_trainer(init.W2V2_TINY, "fp32")
    assert t.eval_bias is None and t.eval_bias_weight == 1.0
    tok = t.tokenizer
    lm = pkg("lm").NGramLM.from_corpus(LR.make_corpus(3, 200, tok.vocab_size, blank=tok.blank_id), tok.vocab_size, tok.blank_id, order=3)
    seen, calls = [], []
    inner = t.forward_losses
    tr = pkg("model.trainer")
    search = tr.prefix_beam_search

    def recording(batch):
        out = inner(batch)
        seen.append((out["log_probs1"].detach().clone(), out["log_probs2"].detach().clone()))
        return out

    def counting(*a, **kw):
        calls.append((a[1:], kw))
        return search(*a, **kw)
    t.forward_losses = recording
    tr.prefix_beam_search = counting
    try:
        t.eval_beam_width = 8
        loss0, wer0 = t.evaluate(loader)
        assert calls == [((8, tok.blank_id), {})] * 4                        # two batches x two speakers: positional arguments only, as before
        want_plain = tuple([bs.fast_decode(i, tok) for lp in seen for i in bs.prefix_beam_search(lp[s], 8, tok.blank_id)] for s in (0, 1))
        assert t.last_decoded == want_plain
        first = [lp for lp in seen]
        hyps = [i for lp in seen for s in (0, 1) for i in bs.prefix_beam_search(lp[s], 8, tok.blank_id, nbest=3)]
        cb = pkg("bias").ContextBias.from_phrases(sorted({tuple(h[i:i + 3]) for u in hyps for h in u[1:] for i in range(0, len(h) - 2, 4)} | {(5, 6, 7)}),
                                                  vocab_size=tok.vocab_size, blank=tok.blank_id)
        del seen[:], calls[:]
        t.eval_bias, t.eval_bias_weight = cb, 2.5
        loss1, _ = t.evaluate(loader)
        assert calls == [((8, tok.blank_id), dict(bias=cb, bias_weight=2.5))] * 4
        want = tuple([bs.fast_decode(i, tok) for lp in seen for i in bs.prefix_beam_search(lp[s], 8, tok.blank_id, bias=cb, bias_weight=2.5)]
                     for s in (0, 1))
        assert t.last_decoded == want and len(want[0]) == len(want[1]) == 4
        assert all(torch.equal(a[s], b[s]) for a, b in zip(first, seen) for s in (0, 1))
        del seen[:], calls[:]
        t.eval_lm, t.eval_lm_weight, t.eval_token_bonus = lm, 0.8, 1.0
        loss2, _ = t.evaluate(loader)
        assert calls == [((8, tok.blank_id), dict(bias=cb, bias_weight=2.5, lm=lm, lm_weight=0.8, token_bonus=1.0))] * 4
        del seen[:], calls[:]
        t.eval_bias, t.eval_lm = None, None
        assert t.evaluate(loader) == (loss0, wer0) and calls == [((8, tok.blank_id), {})] * 4 and t.last_decoded == want_plain
    finally:
        tr.prefix_beam_search = search
    assert loss1 == loss0 and loss2 == loss0
    with pytest.raises(ValueError, match="eval_bias needs eval_beam_width"):
        pkg("model.trainer").MultimodalTrainer(t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1, tok, eval_bias=cb, eval_beam_width=0)
