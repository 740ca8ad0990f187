"""GPU: CTC prefix beam search on the device (csrc/ctc_beam.hip, beam_search.prefix_beam_search) in both libraries, against the float64
reference law of tests/beam_ref.py under the agreement rule stated there, against brute force, against the package's host path, for
determinism and output padding, and as the opt-in decoder of MultimodalTrainer.evaluate()."""
import itertools

import numpy as np
import pytest
import torch

from conftest import pkg
import beam_ref as R

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


_CASES = {}


def _case(B, T, V, W):
    """Inputs, ragged lengths and both references of one shape, computed once for both libraries."""
    key = (B, T, V, W)
    if key not in _CASES:
        lp = np.stack([R.make_log_probs(9000 + 1000 * W + T + b, T, V) for b in range(B)])
        rng = np.random.default_rng(T * 131 + W)
        lens = [T if b % 3 == 0 else int(rng.integers(T // 3, T)) for b in range(B)]
        refs = R.references([lp[b, :lens[b]] for b in range(B)], W, 0, workers=16)
        _CASES[key] = (lp, lens, refs)
    return _CASES[key]


@pytest.mark.parametrize("B,T,V,W", [(8, 199, 800, 1), (8, 199, 800, 5), (8, 199, 800, 16), (8, 199, 800, 64), (3, 749, 800, 5)])
def test_device_against_the_reference_law(library, B, T, V, W):
    """The agreement rule with nbest = W on strided input with ragged lengths.  Measured on an MI355X (DESIGN "CTC prefix beam search")."""
    lp, lens, refs = _case(B, T, V, W)
    ids, scores = pkg("beam_search").prefix_beam_search(_strided(lp), W, 0, lengths=torch.tensor(lens, device="cuda"), nbest=W,
                                                        return_scores=True)
    if W == 1:                                                               # nbest = 1 returns one hypothesis per utterance, not a list of them
        ids, scores = [[i] for i in ids], [[s] for s in scores]
    R.check_agreement(list(zip(ids, scores)), refs, f"device {library} B={B} T={T} V={V} W={W}")


def test_brute_force_on_the_device(library):
    labellings = [l for n in range(5) for l in itertools.product((1, 2), repeat=n)]
    lp = np.stack([R.make_log_probs(1000 + seed, 4, 3) for seed in range(20)])
    ids, scores = pkg("beam_search").prefix_beam_search(torch.from_numpy(lp).cuda(), 31, 0, nbest=31, return_scores=True)
    for seed in range(20):
        ll = [R.exact_loglik(lp[seed], l, 0) for l in labellings]
        best = int(np.argmax(ll))
        assert ids[seed][0] == list(labellings[best]), (seed, ids[seed][0], labellings[best])
        assert abs(scores[seed][0] - ll[best]) <= 1e-5, (seed, scores[seed][0], ll[best])


@pytest.mark.parametrize("T,V,W,blank", [(60, 40, 5, 0), (40, 12, 8, 3), (25, 9, 16, 0), (199, 800, 16, 3), (30, 1500, 4, 7)])
def test_host_and_device_paths_give_equal_ids(library, T, V, W, blank):
    """Same law, same order, same tie rule on both paths; V = 9 at W = 16 expands every token, V = 1500 takes the frame pass's path for rows
    that do not fit in registers; lengths include 0."""
    bs = pkg("beam_search")
    B = 6
    lp = torch.from_numpy(np.stack([R.make_log_probs(400 + T + b, T, V, blank) for b in range(B)]))
    lens = torch.tensor([T, 0, T // 2, 1, T - 1, T])
    hi, hs = bs.prefix_beam_search(lp, W, blank, lengths=lens, nbest=W, return_scores=True)
    di, ds = bs.prefix_beam_search(lp.cuda(), W, blank, lengths=lens.cuda(), nbest=W, return_scores=True)
    for b in range(B):
        fin = [k for k, s in enumerate(hs[b]) if np.isfinite(s)]               # entries without any alignment tie at -inf
        assert [di[b][k] for k in fin] == [hi[b][k] for k in fin], (b, di[b], hi[b])
        assert len(di[b]) == len(hi[b])
    assert di[1] == [[]] and ds[1] == [0.0]
    assert bs.prefix_beam_search(lp.cuda(), W, blank, lengths=lens) == [h[0] for h in hi]


def test_minus_infinity_column_on_the_device(library):
    lp = R.make_log_probs(5, 25, 9)
    lp[:, 4] = -np.inf
    lp[3, 0] = -np.inf
    for W in (3, 8, 16):
        ids, scores = pkg("beam_search").prefix_beam_search(torch.from_numpy(lp).cuda(), W, 0, nbest=W, return_scores=True)
        assert not any(np.isnan(s) for s in scores[0])
        assert np.isfinite(scores[0][0]) and 4 not in ids[0][0]


def _raw(lp, lens, W, nbest, blank=0):
    L = pkg("_lib"); ops = pkg("ops")
    B, T, V = lp.shape
    need = L.ll(0)
    L.check(L.lib().av_ctc_beam_workspace_bytes(B, T, V, W, L.C.byref(need)))
    ws = torch.empty(((need.value + 7) // 8,), dtype=torch.int64, device="cuda")
    out = torch.full((B, nbest, T), 12345, dtype=torch.int32, device="cuda")
    cnt = torch.full((B, nbest), 12345, dtype=torch.int32, device="cuda")
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device="cuda")
    L.check(L.lib().av_ctc_beam_search(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(lens), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                       ops.ptr(ws), need.value, B, T, V, blank, W, nbest, ops.stream()), "av_ctc_beam_search")
    torch.cuda.synchronize()
    return out.cpu(), cnt.cpu(), sc.cpu()


@pytest.mark.parametrize("W,nbest", [(5, 5), (16, 7), (64, 64)])
def test_runs_are_bit_identical_and_outputs_are_padded(library, W, nbest):
    B, T, V = 5, 120, 300
    lp = _strided(np.stack([R.make_log_probs(77 + b, T, V) for b in range(B)]))
    lens = torch.tensor([120, 3, 0, 64, 119], device="cuda")
    a, b = _raw(lp, lens, W, nbest), _raw(lp, lens, W, nbest)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32))
    out, cnt, sc = a
    assert not torch.isnan(sc).any()
    for i in range(B):
        for k in range(nbest):
            n = int(cnt[i, k])
            assert -1 <= n <= int(lens[i])
            if n < 0:                                                        # fewer than nbest hypotheses exist (length 0: only the empty one)
                assert sc[i, k] == float("-inf") and bool((out[i, k] == -1).all())
                continue
            assert bool((out[i, k, n:] == -1).all()) and bool(((out[i, k, :n] >= 1) & (out[i, k, :n] < V)).all())
        valid = [k for k in range(nbest) if int(cnt[i, k]) >= 0]
        assert valid == list(range(len(valid))) and len(valid) >= 1
        s = sc[i, :len(valid)].tolist()
        assert all(x >= y for x, y in zip(s, s[1:])), s
        assert len({tuple(out[i, k, :int(cnt[i, k])].tolist()) for k in valid}) == len(valid)            # hypotheses are distinct prefixes
    assert int(cnt[2, 0]) == 0 and float(sc[2, 0]) == 0.0 and bool((cnt[2, 1:] == -1).all())


def test_evaluate_decodes_with_the_beam_only_when_asked(tmp_path):
    """evaluate() with eval_beam_width = 0 is the greedy path (equal to a second default run); with 8 it decodes both speakers with
    prefix_beam_search on the log-probs of that run; the loss does not depend on the decoder."""
    from test_dataset_gpu import _Tok, _make_corpus
    from test_step_gpu import build as build_trainer
    ds = pkg("dataset.multi_speaker_dataset"); cf = pkg("dataset.collate_fn").collate_fn; init = pkg("utils.init"); bs = pkg("beam_search")
    _, sents = _make_corpus(tmp_path)
    pairs = [(sents[0], sents[2]), (sents[1], sents[3]), (sents[2], sents[1]), (sents[3], sents[0])]
    loader = torch.utils.data.DataLoader(ds.FixedSentencePairDataset(pairs, _Tok()), batch_size=2, shuffle=False, collate_fn=cf, num_workers=0)
    t = build_trainer(init.W2V2_TINY, "fp32")
    assert t.eval_beam_width == 0
    seen = []
    inner = t.forward_losses

    def recording(batch):
        out = inner(batch)
        seen.append((out["log_probs1"].detach().clone(), out["log_probs2"].detach().clone()))
        return out
    t.forward_losses = recording
    loss0, _ = t.evaluate(loader)
    greedy = t.last_decoded
    want_greedy = tuple([bs.fast_decode(i, t.tokenizer) for lp in seen for i in bs.greedy_batch(lp[s], t.tokenizer.blank_id)] for s in (0, 1))
    assert greedy == want_greedy
    loss0b, _ = t.evaluate(loader)
    assert t.last_decoded == greedy and loss0b == loss0
    del seen[:]
    t.eval_beam_width = 8
    loss8, _ = t.evaluate(loader)
    assert loss8 == loss0
    assert len(seen) == 2
    want = tuple([bs.fast_decode(i, t.tokenizer) for lp in seen for i in bs.prefix_beam_search(lp[s], 8, t.tokenizer.blank_id)] for s in (0, 1))
    assert t.last_decoded == want
    assert len(want[0]) == len(want[1]) == 4
