"""GPU: the n-gram tables on the device (av_ngram_score against NGramLM.score, bit for bit) and CTC prefix beam search with shallow fusion
(csrc/ctc_beam.hip, beam_search.prefix_beam_search(lm=...)) in both libraries: against the fused float64 law of tests/lm_ref.py under the
agreement rule of tests/beam_ref.py, against av_ctc_beam_search at zero weights, against the package's host path, for determinism and
output padding, and as the opt-in decoder of MultimodalTrainer.evaluate()."""
import numpy as np
import pytest
import torch

from conftest import pkg
import beam_ref as R
import lm_ref as LR

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


def _lm(V, order, bos=True):
    if (V, order, bos) not in _LMS:
        _LMS[(V, order, bos)] = pkg("lm").NGramLM.from_corpus(LR.make_corpus(V + order, 400, V), V, 0, order=order, bos=bos)
    return _LMS[(V, order, bos)]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---- (a) the tables ----
def _score_all(lm, ids, lens, slots=None):
    """av_ngram_score on the tables of ``lm`` (optionally in a larger table) -> float32 [B][Lmax] on the host."""
    L = pkg("_lib"); ops = pkg("ops")
    d = lm.to_device("cuda", slots)
    ids_d = torch.tensor(ids, dtype=torch.int32, device="cuda")
    ln = torch.tensor(lens, dtype=torch.long, device="cuda")
    out = torch.full(ids_d.shape, 777.0, dtype=torch.float32, device="cuda")
    L.check(L.lib().av_ngram_score(ops.ptr(ids_d), ops.ptr(ln), ops.ptr(out), ids_d.shape[0], ids_d.shape[1], ops.ptr(d.unigrams), ops.ptr(d.table),
                                   d.slots, d.order, d.vocab_size, d.bos, d.probe_bound, ops.stream()), "av_ngram_score")
    return out.cpu().numpy()


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("bos", [True, False])
def test_ngram_score_is_bit_identical_to_the_host(library, order, bos):
    """Corpus sentences (seen n-grams, contexts growing from 0 to beyond N - 1) and random ones (unseen n-grams, every backoff depth),
    ragged lengths, more than one block of 256 tokens."""
    V = 40
    lm = _lm(V, order, bos)
    rng = np.random.default_rng(order)
    Lmax = 13
    rows = [s[:Lmax] for s in LR.make_corpus(V + order, 400, V)[:24]] + [[int(x) for x in rng.integers(1, V, size=Lmax)] for _ in range(24)]
    lens = [len(r) if k % 5 else max(0, len(r) - 3) for k, r in enumerate(rows)]
    ids = [r + [1] * (Lmax - len(r)) for r in rows]
    got = _score_all(lm, ids, lens)
    want = np.zeros_like(got)
    for b, r in enumerate(ids):
        for i in range(lens[b]):
            want[b, i] = lm.score(r[:i], r[i])
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(lm.score_batch(torch.tensor(ids, device="cuda"), lens).cpu().numpy()), _bits(want))


def test_ngram_score_with_long_probe_runs_and_unknown_tokens(library):
    """A table at load exactly 0.5 in which 24 of the 32 bigrams start probing at one slot (found by search over splitmix64), so that stored
    keys sit up to 24 probes from home; tokens without a unigram score unk_logp; an id outside the vocabulary gives NaN at its place and
    matches nothing as context."""
    LM = pkg("lm")
    V, slots = 3000, 64
    rng = np.random.default_rng(5)
    grams, home = {}, 0
    while len(grams) < 32:
        a, b = int(rng.integers(1, V)), int(rng.integers(1, V))
        h = LM.splitmix64(LM.pack_key([a, b])) & (slots - 1)
        want_home = sum(1 for g in grams if LM.splitmix64(LM.pack_key(g)) & (slots - 1) == 7) < 24
        if (h == 7) == want_home and (a, b) not in grams:
            grams[(a, b)] = (-float(rng.random()) - 0.5, -float(rng.random()))
    uni = {w: (-float(rng.random()) - 3.0, -float(rng.random())) for g in grams for w in g}
    lm = LM.NGramLM(2, V, 0, uni, grams, bos=False, unk_logp=-7.5)
    _, _, s, bound = lm.host_tables()
    assert s == slots and 2 * len(lm.table) == slots and bound >= 24
    rows = [list(g) + [int(rng.integers(1, V))] for g in grams] + [[int(rng.integers(1, V)) for _ in range(3)] for _ in range(32)]
    got = _score_all(lm, rows, [3] * len(rows))
    want = np.array([[lm.score(r[:i], r[i]) for i in range(3)] for r in rows], np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    assert (want == np.float32(-7.5)).any()                                  # some token had no unigram and no bigram
    bad = _score_all(lm, [[rows[0][0], V, rows[0][1]], [rows[0][0], -1, rows[0][1]]], [3, 3])
    assert np.isnan(bad[:, 1]).all() and np.array_equal(_bits(bad[:, 2]), _bits([lm.uni[rows[0][1], 0]] * 2))
    assert np.array_equal(_bits(bad[:, 0]), _bits([lm.uni[rows[0][0], 0]] * 2))


# ---- (b) the fused search against the float64 law ----
SHAPES = [(8, 60, 40, 5, 6, 3), (8, 60, 40, 8, 20, 4), (16, 100, 800, 5, 16, 3), (4, 40, 800, 64, 65, 2)]
WEIGHTS = [(0.5, 0.0), (0.8, 1.0)]
_CASES = {}


def _case(B, T, V, W, K, order, alpha, beta):
    """Inputs, ragged lengths and both references of one shape and one pair of weights, computed once for both libraries.  The seeds are
    fixed; that the float32 restatement alone agrees with the float64 one on them (the condition on the inputs) is asserted here."""
    key = (B, T, V, W, K, order, alpha, beta)
    if key not in _CASES:
        lp = np.stack([R.make_log_probs(20000 + 1000 * W + T + b, T, V) for b in range(B)])
        rng = np.random.default_rng(T * 131 + W)
        lens = [T if b % 3 == 0 else int(rng.integers(T // 3, T)) for b in range(B)]
        lm = _lm(V, order)
        refs = LR.references([lp[b, :lens[b]] for b in range(B)], W, 0, LR.lm_dict(lm), alpha, beta, K, workers=16)
        assert LR.float32_alone_agrees(refs), "these inputs hold a near-tie that the float32 law itself resolves differently: pick other seeds"
        _CASES[key] = (lp, lens, lm, refs)
    return _CASES[key]


@pytest.mark.parametrize("alpha,beta", WEIGHTS)
@pytest.mark.parametrize("B,T,V,W,K,order", SHAPES)
def test_device_against_the_reference_law(library, B, T, V, W, K, order, alpha, beta):
    """The agreement rule (tolerance max(1e-4, 8 e32), at most one near-tie in 16 utterances) with nbest = W on strided input with ragged
    lengths; g within float32 rounding of the reference's where the hypotheses match."""
    lp, lens, lm, refs = _case(B, T, V, W, K, order, alpha, beta)
    ids, scores, g = pkg("beam_search").prefix_beam_search(_strided(lp), W, 0, lengths=torch.tensor(lens, device="cuda"), nbest=W,
                                                           return_scores=True, lm=lm, lm_weight=alpha, token_bonus=beta, tokens=K)
    R.check_agreement(list(zip(ids, scores)), LR.for_agreement(refs),
                      f"device lm {library} B={B} T={T} V={V} W={W} K={K} order={order} alpha={alpha} beta={beta}")
    for u, (r64, _) in enumerate(refs):
        for k, i in enumerate(ids[u]):
            if i == r64[k][0]:
                assert abs(g[u][k] - r64[k][2]) <= 1e-5 * max(1.0, abs(r64[k][2])), (u, k, g[u][k], r64[k][2])


# ---- (c) zero weights: the search without a language model ----
def _raw(lp, lens, W, nbest, lm=None, tokens=None, alpha=0.0, beta=0.0):
    """The C entry points on pre-filled outputs -> host copies of (ids, lengths, scores[, g])."""
    L = pkg("_lib"); ops = pkg("ops")
    B, T, V = lp.shape
    need = L.ll(0)
    if lm is None:
        L.check(L.lib().av_ctc_beam_workspace_bytes(B, T, V, W, L.C.byref(need)))
    else:
        L.check(L.lib().av_ctc_beam_lm_workspace_bytes(B, T, V, W, tokens, L.C.byref(need)))
    ws = torch.empty(((need.value + 7) // 8,), dtype=torch.int64, device="cuda")
    out = torch.full((B, nbest, T), 12345, dtype=torch.int32, device="cuda")
    cnt = torch.full((B, nbest), 12345, dtype=torch.int32, device="cuda")
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda")
    if lm is None:
        L.check(L.lib().av_ctc_beam_search(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(lens), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                           ops.ptr(ws), need.value, B, T, V, 0, W, nbest, ops.stream()), "av_ctc_beam_search")
        torch.cuda.synchronize()
        return out.cpu(), cnt.cpu(), sc.cpu()
    d = lm.to_device("cuda")
    gl = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda")
    L.check(L.lib().av_ctc_beam_search_lm(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(lens), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                          ops.ptr(gl), ops.ptr(ws), need.value, B, T, V, 0, W, nbest, tokens, ops.ptr(d.unigrams),
                                          ops.ptr(d.table), d.slots, d.order, d.vocab_size, d.bos, d.probe_bound, alpha, beta, ops.stream()),
            "av_ctc_beam_search_lm")
    torch.cuda.synchronize()
    return out.cpu(), cnt.cpu(), sc.cpu(), gl.cpu()


@pytest.mark.parametrize("V,W,order", [(40, 5, 3), (300, 16, 4), (800, 64, 2), (9, 16, 3)])
def test_zero_weights_equal_the_search_without_a_language_model(library, V, W, order):
    """alpha = beta = 0 and tokens = W + 1: ids, lengths and score bits of av_ctc_beam_search (V = 9 at W = 16 expands every token)."""
    B, T = 5, 90
    lp = _strided(np.stack([R.make_log_probs(77 + b, T, V) for b in range(B)]))
    lens = torch.tensor([90, 3, 0, 64, 89], device="cuda")
    plain = _raw(lp, lens, W, W)
    fused = _raw(lp, lens, W, W, _lm(V, order), W + 1)
    for x, y in zip(plain, fused[:3]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert bool((fused[3] == 0).all())


# ---- (d) host and device ----
@pytest.mark.parametrize("T,V,W,K,order,bos,alpha,beta", [(60, 40, 5, 6, 3, True, 0.5, 0.0), (40, 40, 8, 20, 4, False, 0.8, 1.0),
                                                            (25, 9, 16, 17, 2, True, 0.5, 0.0), (50, 800, 6, 1, 3, True, 0.8, 1.0),
                                                            (30, 1500, 4, 9, 1, True, 0.5, 0.5)])
def test_host_and_device_paths_agree(library, T, V, W, K, order, bos, alpha, beta):
    """Same law, same order, same tie rule: equal ids, g equal bit for bit, scores within max(1e-4, 8 x the float32 law's own error);
    V = 9 expands every token, tokens = 1 uses the frame pass at width 1, V = 1500 takes the frame pass's path for long rows; lengths
    include 0 and 1."""
    bs = pkg("beam_search")
    B = 6
    lm = _lm(V, order, bos)
    lp = torch.from_numpy(np.stack([R.make_log_probs(400 + T + b, T, V) for b in range(B)]))
    lens = torch.tensor([T, 0, T // 2, 1, T - 1, T])
    hi, hs, hg = bs.prefix_beam_search(lp, W, 0, lengths=lens, nbest=W, return_scores=True, lm=lm, lm_weight=alpha, token_bonus=beta, tokens=K)
    di, ds, dg = bs.prefix_beam_search(lp.cuda(), W, 0, lengths=lens.cuda(), nbest=W, return_scores=True, lm=lm, lm_weight=alpha,
                                       token_bonus=beta, tokens=K)
    refs = LR.references([lp[b, :int(lens[b])].numpy() for b in (0, 2, 4, 5)], W, 0, LR.lm_dict(lm), alpha, beta, K)
    e32 = 0.0                                                                # as in beam_ref.check_agreement
    for r64, r32 in refs:
        s64 = {tuple(i): s for i, s, _ in r64}
        e32 = max([e32] + [abs(s - s64[tuple(i)]) for i, s, _ in r32 if tuple(i) in s64 and np.isfinite(s64[tuple(i)])])
    tol = max(R.SCORE_FLOOR, R.SCORE_FACTOR * e32)
    for b in range(B):
        fin = [k for k, s in enumerate(hs[b]) if np.isfinite(s)]               # entries without any alignment tie at -inf
        assert [di[b][k] for k in fin] == [hi[b][k] for k in fin], (b, di[b], hi[b])
        assert len(di[b]) == len(hi[b])
        assert np.array_equal(_bits([dg[b][k] for k in fin]), _bits([hg[b][k] for k in fin]))
        assert all(abs(ds[b][k] - hs[b][k]) <= tol for k in fin), (b, ds[b], hs[b], tol)
    assert di[1] == [[]] and ds[1] == [0.0] and dg[1] == [0.0]
    assert bs.prefix_beam_search(lp.cuda(), W, 0, lengths=lens, lm=lm, lm_weight=alpha, token_bonus=beta, tokens=K) == [h[0] for h in hi]


# ---- (e) determinism and padding ----
@pytest.mark.parametrize("W,nbest,K", [(5, 5, 6), (16, 7, 40), (64, 64, 65)])
def test_runs_are_bit_identical_and_outputs_are_padded(library, W, nbest, K):
    B, T, V = 5, 120, 300
    lm = _lm(V, 3)
    lp = _strided(np.stack([R.make_log_probs(77 + b, T, V) for b in range(B)]))
    lens = torch.tensor([120, 3, 0, 64, 119], device="cuda")
    a, b = _raw(lp, lens, W, nbest, lm, K, 0.5, 0.25), _raw(lp, lens, W, nbest, lm, K, 0.5, 0.25)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32))
    out, cnt, sc, gl = a
    assert not torch.isnan(sc).any() and not torch.isnan(gl).any()
    for i in range(B):
        for k in range(nbest):
            n = int(cnt[i, k])
            assert -1 <= n <= int(lens[i])
            if n < 0:                                                        # fewer than nbest hypotheses exist (length 0: only the empty one)
                assert sc[i, k] == float("-inf") and gl[i, k] == 0.0 and bool((out[i, k] == -1).all())
                continue
            assert bool((out[i, k, n:] == -1).all()) and bool(((out[i, k, :n] >= 1) & (out[i, k, :n] < V)).all())
        valid = [k for k in range(nbest) if int(cnt[i, k]) >= 0]
        assert valid == list(range(len(valid))) and len(valid) >= 1
        s = sc[i, :len(valid)].tolist()
        assert all(x >= y for x, y in zip(s, s[1:])), s
        assert len({tuple(out[i, k, :int(cnt[i, k])].tolist()) for k in valid}) == len(valid)            # hypotheses are distinct prefixes
    assert int(cnt[2, 0]) == 0 and float(sc[2, 0]) == 0.0 and float(gl[2, 0]) == 0.0 and bool((cnt[2, 1:] == -1).all())


# ---- (f) evaluate() ----
def test_evaluate_uses_the_language_model_only_when_asked(tmp_path):
    """evaluate() with eval_beam_width = 8 and no eval_lm decodes with the plain beam; with eval_lm it decodes both speakers with
    prefix_beam_search(lm=...) on the log-probs of that run, at the trainer's weights; the loss does not depend on the decoder."""
    from test_dataset_gpu import _Tok, _make_corpus
    from test_step_gpu import build as build_trainer
    ds = pkg("dataset.multi_speaker_dataset"); cf = pkg("dataset.collate_fn").collate_fn; init = pkg("utils.init"); bs = pkg("beam_search")
    _, sents = _make_corpus(tmp_path)
    pairs = [(sents[0], sents[2]), (sents[1], sents[3]), (sents[2], sents[1]), (sents[3], sents[0])]
    loader = torch.utils.data.DataLoader(ds.FixedSentencePairDataset(pairs, _Tok()), batch_size=2, shuffle=False, collate_fn=cf, num_workers=0)
    t = build_trainer(init.W2V2_TINY, "fp32")
    assert t.eval_lm is None
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
        calls.append(kw.get("lm"))
        return search(*a, **kw)
    t.forward_losses = recording
    tr.prefix_beam_search = counting
    try:
        t.eval_beam_width = 8
        loss0, _ = t.evaluate(loader)
        assert calls == [None] * 4                                           # two batches x two speakers, no language model
        want_plain = tuple([bs.fast_decode(i, tok) for lp in seen for i in bs.prefix_beam_search(lp[s], 8, tok.blank_id)] for s in (0, 1))
        assert t.last_decoded == want_plain
        del seen[:], calls[:]
        t.eval_lm, t.eval_lm_weight, t.eval_token_bonus = lm, 0.8, 1.0
        loss1, _ = t.evaluate(loader)
        assert calls == [lm] * 4
    finally:
        tr.prefix_beam_search = search
    assert loss1 == loss0 and len(seen) == 2
    want = tuple([bs.fast_decode(i, tok) for lp in seen
                  for i in bs.prefix_beam_search(lp[s], 8, tok.blank_id, lm=lm, lm_weight=0.8, token_bonus=1.0)] for s in (0, 1))
    assert t.last_decoded == want and len(want[0]) == len(want[1]) == 4
