"""CPU: the host path of confidence.py (float32 numpy) against the float64 restatement of tests/confidence_ref.py, its fixed points and edge
cases, the aggregations, word confidences, host_meta.inference_masks against the oracle's mixing law, the greedy path as the Viterbi path
of its own labelling, every rejected argument, the new option rows, and the three new symbols of the C-ABI in both libraries."""
import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import cpu_trainer as _trainer
import confidence_ref as R

# Every operation of the float32 law (the exponent, exp, the pairwise sums of V <= 2051 terms, log, the divisions) is rounded to 2^-24 relative,
# and what they are applied to is O(1) after the normalisation: a term exp(a d) with a rounded exponent is off by |a d| exp(a d) 2^-24
# <= 0.37 x 2^-24, the sums carry log2(V) = 11 roundings, and the final quotient (x - u) / (1 - u) does not amplify (|x| <= max(u, 1)).
# 32 such roundings bound the lot; the worst measured value (printed below) is the yardstick of tests/test_confidence_gpu.py.
F32_BOUND = 32 * 2.0 ** -24


def _C():
    return pkg("confidence")


def test_float32_host_law_against_float64():
    C = _C()
    worst = {}
    for V in R.VS:
        for scale in R.SCALES:
            lp = R.make_logits(1, 3, 8, V, scale)
            for method, alpha in R.settings():
                got = C.frame_confidence(torch.from_numpy(lp), None, method, alpha)
                assert got.dtype == torch.float32 and got.shape == (3, 8)
                err = float(np.abs(got.numpy().astype(np.float64) - R.frame_conf(lp, [8] * 3, method, alpha)).max())
                worst[(method, alpha)] = max(worst.get((method, alpha), 0.0), err)
                assert err <= F32_BOUND, (V, scale, method, alpha, err)
    print("[confidence host] worst |float32 - float64| per setting: " + ", ".join(f"{m} {a}: {e:.2e}" for (m, a), e in worst.items()))
    print(f"[confidence host] worst overall {max(worst.values()):.2e} (bound {F32_BOUND:.2e})")


@pytest.mark.parametrize("V", [5, 800])
def test_fixed_points(V):
    """A one-hot row gives exactly 1.  A uniform row gives exactly 0 for max_prob, entropy and the default tsallis exponent; for the other
    exponents V / V^a and V^(1 - a) are two float32 roundings of one number, so the law leaves at most their difference (<= 2^-22)."""
    C = _C()
    hot = np.full((1, 3, V), -np.inf, np.float32)
    hot[0, 0, 0] = hot[0, 1, V - 1] = 0.0
    hot[0, 2, 2] = -3.5                                              # not normalised: the law renormalises
    flat = np.full((1, 2, V), np.log(np.float32(1.0 / V)), np.float32)
    flat[0, 1] = 7.25
    for method, alpha in R.settings():
        assert C.frame_confidence(torch.from_numpy(hot), None, method, alpha).tolist() == [[1.0, 1.0, 1.0]], (method, alpha)
        u = C.frame_confidence(torch.from_numpy(flat), None, method, alpha)
        if method != "tsallis" or alpha == 0.33:
            assert u.tolist() == [[0.0, 0.0]], (method, alpha, u)
        else:
            assert float(u.min()) >= 0.0 and float(u.max()) <= 2.0 ** -22, (method, alpha, u)


def test_edge_rows_lengths_and_layout():
    C = _C()
    V, T = 9, 6
    lp = R.make_logits(3, 4, T, V, 3.0)
    lp[0, 1, 3:] = -np.inf                                           # -inf entries add 0 to every sum: the row is its finite part
    lp[0, 2, :] = -np.inf                                            # no finite maximum
    lp[0, 3, 4] = np.nan
    lp[0, 4, 0] = np.inf
    il = torch.tensor([T, 3, 0, 99])
    for method, alpha in R.settings():
        got = C.frame_confidence(torch.from_numpy(lp), il, method, alpha).numpy()
        want = R.frame_conf(lp, [T, 3, 0, T], method, alpha)
        assert np.abs(got - want).max() <= F32_BOUND, (method, alpha)
        assert got[0, 2] == 0 and got[0, 3] == 0 and got[0, 4] == 0 and not np.isnan(got).any()
        assert (got[1, 3:] == 0).all() and (got[2] == 0).all() and (got[3] > 0).all()          # t >= T_b, T_b = 0, T_b clamped to T
        tm = C.frame_confidence(torch.from_numpy(lp).transpose(0, 1), il, method, alpha, batch_first=False)
        assert torch.equal(tm, torch.from_numpy(got))
        assert torch.equal(C.frame_confidence(torch.from_numpy(lp).double(), il, method, alpha), torch.from_numpy(got))     # computed in float32


def test_a_sharper_row_never_scores_lower():
    """log_softmax(k x) for growing k majorises the flatter rows before it: every measure is Schur-convex, so the confidence cannot fall
    (the float32 law: by more than its own rounding)."""
    C = _C()
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 12, 67))
    ks = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
    rows = []
    for k in ks:
        y = k * x
        y = y - y.max(-1, keepdims=True)
        rows.append((y - np.log(np.exp(y).sum(-1, keepdims=True))).astype(np.float32))
    for method, alpha in R.settings():
        c32 = [C.frame_confidence(torch.from_numpy(r), None, method, alpha).numpy()[0] for r in rows]
        c64 = [R.frame_conf(r, [12], method, alpha)[0] for r in rows]
        for a, b, a64, b64 in zip(c32, c32[1:], c64, c64[1:]):
            assert (b64 >= a64).all() and (b >= a - F32_BOUND).all(), (method, alpha)
        assert (c32[-1] > c32[0] + 0.2).all()


def test_aggregations():
    C = _C()
    rng = np.random.default_rng(11)
    B, T = 3, 10
    conf = rng.random((B, T)).astype(np.float32)
    spans = torch.tensor([[[0, 3], [3, 4], [4, 10], [-1, -1], [8, 14], [5, 5], [7, 2]]] * B, dtype=torch.int32)
    il = torch.tensor([T, 9, 0])
    for agg in R.AGGREGATIONS:
        got = C.span_confidence(torch.from_numpy(conf), spans, il, agg)
        assert got.dtype == torch.float32 and got.shape == (B, 7)
        want = R.span_conf(conf.astype(np.float64), spans.numpy(), il.tolist(), agg)
        assert np.abs(got.numpy() - want).max() <= 10 * 2.0 ** -24, agg               # at most 10 terms below 1
        assert got[:, 3].tolist() == [0, 0, 0] and got[:, 5].tolist() == [0, 0, 0] and got[:, 6].tolist() == [0, 0, 0] and bool((got[2] == 0).all())
        assert float(got[1, 4]) == float(conf[1, 8])                                  # [8, 14) clipped to [8, 9)
        # one in-order float32 loop per span, written out here
        acc = conf[0, 4]
        for t in range(5, 10):
            acc = np.float32(acc + conf[0, t]) if agg == "mean" else (min(acc, conf[0, t]) if agg == "min" else np.float32(acc * conf[0, t]))
        assert float(got[0, 2]) == float(np.float32(acc / np.float32(6)) if agg == "mean" else acc)
        assert C.span_confidence(torch.from_numpy(conf), spans[:, :0], il, agg).shape == (B, 0)      # L = 0
        assert torch.equal(C.span_confidence(torch.from_numpy(conf), spans.long(), il.tolist(), agg), got)
        utt = C.utterance_confidence(got, torch.tensor([3, 0, 7]), agg)
        assert utt.shape == (B,) and float(utt[1]) == 0.0
        assert float(utt[0]) == float(C.host_span_law(got[0].numpy(), 0, 3, 3, agg))
        assert C.utterance_confidence(got[:, :0], torch.tensor([0, 0, 0]), agg).tolist() == [0, 0, 0]


def test_word_segments_with_and_without_token_conf():
    A = pkg("align")
    tok = pkg("utils.tokenizer").SyntheticTokenizer(800)
    sp, a, b, c = tok.token_to_id["▁"], 5, 6, 7
    ids = [sp, a, b, sp, sp, c, sp]
    spans = [[0, 1], [1, 3], [3, 4], [5, 6], [6, 7], [8, 10], [10, 11], [-1, -1]]
    scores = [-0.1, -0.25, -0.5, -0.1, -0.1, -1.0, -0.1, 0.0]
    conf = [0.9, 0.5, 0.25, 0.9, 0.9, 0.75, 0.9, 0.0]
    old = A.word_segments(tok, ids, torch.tensor(spans, dtype=torch.int32), torch.tensor(scores), frame_rate=25.0)
    assert [sorted(w) for w in old] == [["end", "score", "start", "word"]] * 2
    want = {"min": [0.25, 0.75], "mean": [0.375, 0.75], "prod": [0.125, 0.75]}
    for agg in R.AGGREGATIONS:
        new = A.word_segments(tok, ids, torch.tensor(spans, dtype=torch.int32), torch.tensor(scores), 25.0, token_conf=torch.tensor(conf),
                              aggregation=agg)
        assert [w["confidence"] for w in new] == want[agg]
        assert [{k: v for k, v in w.items() if k != "confidence"} for w in new] == old              # the old keys are unchanged
    assert A.word_segments(tok, ids, [[-1, -1]] * 8, [0.0] * 8, token_conf=conf) == []
    with pytest.raises(ValueError, match="aggregation"):
        A.word_segments(tok, ids, spans, scores, token_conf=conf, aggregation="max")
    with pytest.raises(ValueError, match="token_conf"):
        A.word_segments(tok, ids, spans, scores, token_conf=conf[:3])


@pytest.mark.parametrize("n1,n2", [(5, 5), (3, 7), (7, 3), (0, 4)])
def test_inference_masks_are_the_oracle_mix_masks_plus_pad(n1, n2):
    from oracle import pipeline_oracle as PO
    hm = pkg("model.host_meta")
    width = 9
    _, m1, m2 = PO.mix_pair(np.ones(n1, np.float32), np.ones(n2, np.float32))
    pad = lambda m: np.concatenate([m, np.full(width - len(m), 3, np.int64)])       # noqa: E731  the collate's pad code
    got1, got2 = hm.inference_masks([max(n1, n2)], [n1], [n2], width)
    assert got1.dtype == torch.int64 and got1.shape == (1, width)
    assert got1[0].tolist() == pad(m1).tolist() and got2[0].tolist() == pad(m2).tolist()
    # from a batch: lip lengths in frames of 640 samples, clamped to the audio; everything optional
    b = {"audio": torch.zeros(2, 2000), "audio_lengths": torch.tensor([2000, 1500]), "lip1_lengths": torch.tensor([2, 3]),
         "lip2_lengths": torch.tensor([3, 1])}
    g1, g2 = hm.batch_inference_masks(b)
    w1, w2 = hm.inference_masks([2000, 1500], [1280, 1500], [1920, 640], 2000)
    assert torch.equal(g1, w1) and torch.equal(g2, w2) and g1[1, 1499] == 2 and g1[1, 1500] == 3 and g2[1, 640] == 0
    f1, f2 = hm.batch_inference_masks({"audio": torch.zeros(2, 50)})
    assert bool((f1 == 1).all()) and bool((f2 == 1).all())


def test_greedy_path_is_the_viterbi_path():
    """40 seeds of T = 23, V = 7: the runs of the host greedy law are forced_align's spans for the greedy ids, exactly; ids and lengths are
    greedy_batch's, the token confidences are the span law over the runs."""
    C = _C(); A = pkg("align"); bs = pkg("beam_search")
    mismatches = 0
    for seed in range(40):
        lp = torch.log_softmax(2 * torch.randn(1, 23, 7, generator=torch.Generator().manual_seed(seed)), -1)
        g = C.greedy_timed(lp, 0)
        n = int(g.lengths[0])
        assert g.ids.dtype == torch.int32 and g.spans.shape == (1, 23, 2) and g.token_conf.shape == (1, 23) and g.frame_conf.shape == (1, 23)
        assert g.ids[0, :n].tolist() == bs.greedy_batch(lp, 0)[0] and bool((g.ids[0, n:] == -1).all()) and bool((g.spans[0, n:] == -1).all())
        al = A.forced_align(lp, g.ids[:, :max(n, 1)].long().clamp_min(0), None, g.lengths, blank=0)
        mismatches += not torch.equal(al.spans[0, :n], g.spans[0, :n])
        assert torch.equal(g.frame_conf, C.frame_confidence(lp))
        assert torch.equal(g.token_conf, C.span_confidence(g.frame_conf, g.spans))
    assert mismatches == 0
    # lengths, another blank, an all-blank utterance
    lp = torch.log_softmax(2 * torch.randn(3, 23, 7, generator=torch.Generator().manual_seed(99)), -1)
    lp[2, :, 3] = 5.0
    g = C.greedy_timed(lp, 3, torch.tensor([23, 9, 23]), "entropy", 0.33, "mean")
    assert g.ids[1, :int(g.lengths[1])].tolist() == bs.greedy_batch(lp[1:2, :9], 3)[0] and int(g.spans[1].max()) <= 9
    assert int(g.lengths[2]) == 0 and bool((g.ids[2] == -1).all()) and bool((g.token_conf[2] == 0).all())
    assert bool((g.frame_conf[1, 9:] == 0).all())


def test_rejected_arguments():
    C = _C(); ops = pkg("ops")
    lp = torch.log_softmax(torch.randn(2, 5, 8), -1)
    for bad in (float("nan"), float("inf"), 0.0, -0.5, 1.0, 1.01, 0.99):
        with pytest.raises(ValueError, match="entropy" if abs(bad - 1) < 0.02 else "alpha"):
            C.frame_confidence(lp, None, "tsallis", bad)
        with pytest.raises(ValueError):
            C.greedy_timed(lp, 0, None, "tsallis", bad)
    assert C.frame_confidence(lp, None, "entropy", 1.0).shape == (2, 5)                  # alpha is the tsallis exponent only
    with pytest.raises(ValueError, match="method"):
        C.frame_confidence(lp, None, "gibbs")
    with pytest.raises(ValueError, match="V >= 2"):
        C.frame_confidence(lp[:, :, :1])
    with pytest.raises(ValueError, match="4096"):
        C.frame_confidence(torch.zeros(1, 4097, 2))
    with pytest.raises(ValueError, match=r"\[B, T, V\]"):
        C.frame_confidence(lp[0])
    with pytest.raises(TypeError, match="floating"):
        C.frame_confidence(lp.long())
    with pytest.raises(ValueError, match="one length per batch item"):
        C.frame_confidence(lp, torch.tensor([5, 5, 5]))
    with pytest.raises(TypeError, match="integer"):
        C.frame_confidence(lp, torch.tensor([5.0, 5.0]))
    cf = C.frame_confidence(lp)
    with pytest.raises(ValueError, match="aggregation"):
        C.span_confidence(cf, torch.zeros(2, 1, 2, dtype=torch.int32), None, "max")
    with pytest.raises(ValueError, match="spans"):
        C.span_confidence(cf, torch.zeros(3, 1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="spans"):
        C.span_confidence(cf, torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(TypeError, match="integer"):
        C.span_confidence(cf, torch.zeros(2, 1, 2))
    with pytest.raises(TypeError, match="frame_conf"):
        C.span_confidence(cf[0], torch.zeros(2, 1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="blank"):
        C.greedy_timed(lp, 8)
    with pytest.raises(ValueError, match="aggregation"):
        C.greedy_timed(lp, 0, aggregation="median")
    with pytest.raises(ValueError, match="aggregation"):
        C.utterance_confidence(cf, torch.tensor([5, 5]), "max")
    # the device wrappers validate before the C call and have no CPU fallback
    for call in (lambda: ops.ctc_frame_conf(lp), lambda: ops.ctc_greedy_timed(lp, 0),
                 lambda: ops.ctc_span_conf(cf, torch.zeros(2, 1, 2, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="method"):
        ops.ctc_frame_conf(lp, method="gibbs")
    with pytest.raises(ValueError, match="entropy"):
        ops.ctc_greedy_timed(lp, 0, alpha=1.0)
    with pytest.raises(ValueError, match="aggregation"):
        ops.ctc_span_conf(cf, torch.zeros(2, 1, 2, dtype=torch.int32), aggregation="max")


def test_option_rows(monkeypatch):
    for var in ("AVAMD_CONF_METHOD", "AVAMD_CONF_ALPHA", "AVAMD_CONF_AGG"):
        monkeypatch.delenv(var, raising=False)
    t = _trainer()
    assert (t.conf_method, t.conf_alpha, t.conf_aggregation) == ("tsallis", 0.33, "min")
    monkeypatch.setenv("AVAMD_CONF_METHOD", "entropy"); monkeypatch.setenv("AVAMD_CONF_ALPHA", "0.5"); monkeypatch.setenv("AVAMD_CONF_AGG", "mean")
    t = _trainer()
    assert (t.conf_method, t.conf_alpha, t.conf_aggregation) == ("entropy", 0.5, "mean")
    t = _trainer(conf_method="tsallis", conf_alpha=2, conf_aggregation="prod")                # an argument wins over the variable
    assert (t.conf_method, t.conf_alpha, t.conf_aggregation) == ("tsallis", 2.0, "prod") and isinstance(t.conf_alpha, float)
    for kw in (dict(conf_method="gibbs"), dict(conf_aggregation="max"), dict(conf_method="tsallis", conf_alpha=1.0),
               dict(conf_method="tsallis", conf_alpha=0.0), dict(conf_method="tsallis", conf_alpha=float("nan"))):
        with pytest.raises(ValueError):
            _trainer(**kw)
    monkeypatch.setenv("AVAMD_CONF_METHOD", "tsallis"); monkeypatch.setenv("AVAMD_CONF_ALPHA", "1.0")
    with pytest.raises(ValueError, match="entropy"):
        _trainer()
    monkeypatch.setenv("AVAMD_CONF_ALPHA", "0.33"); monkeypatch.setenv("AVAMD_CONF_AGG", "median")
    with pytest.raises(ValueError, match="aggregation"):
        _trainer()


def test_trainer_transcribe_has_no_cpu_fallback_and_checks_nbest():
    synth = pkg("dataset.synthetic")
    t = _trainer()
    mods = (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1)
    modes = [m.training for m in mods]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.transcribe(synth.make_batch(2, 1.0, seed=1))
    with pytest.raises(ValueError, match="nbest"):
        t.transcribe(synth.make_batch(2, 1.0, seed=1), nbest=2)                              # the greedy decode has one hypothesis
    assert [m.training for m in mods] == modes


def _libs():
    L = pkg("_lib"); P = pkg("precision")
    old = P.get_precision()
    out = []
    try:
        for mode, suffix in (("fp32", "libavhip.so"), ("fp16", "libavhip_f16.so")):
            P.set_precision(mode)
            lib = L.lib()
            assert lib._name.endswith(suffix)
            out.append(lib)
    finally:
        P.set_precision(old)
    return out


def test_abi_symbols_bound_and_argument_errors_are_statuses():
    L = pkg("_lib")
    assert [len(L.SIGNATURES[n]) for n in ("av_ctc_frame_conf", "av_ctc_span_conf", "av_ctc_greedy_timed")] == [11, 9, 17]
    assert L.CONF_METHODS == {"max_prob": 0, "entropy": 1, "tsallis": 2} and L.CONF_AGGREGATIONS == {"mean": 0, "min": 1, "prod": 2}
    P = 4096                                     # any non-null address: argument checks come before a launch, nothing is dereferenced
    for lib in _libs():
        for n in ("av_ctc_frame_conf", "av_ctc_span_conf", "av_ctc_greedy_timed"):
            assert list(getattr(lib, n).argtypes) == list(L.SIGNATURES[n])
        err = lib.av_last_error
        # (log_probs, stride_b, stride_t, lengths, B, T, V, method, alpha, conf, stream)
        f = lib.av_ctc_frame_conf
        assert f(None, 80, 8, None, 2, 10, 8, 2, 0.33, P, None) != 0 and b"null" in err()
        assert f(P, 80, 8, None, 2, 10, 8, 2, 0.33, None, None) != 0 and b"null" in err()
        assert f(P, 10, 1, None, 2, 10, 1, 2, 0.33, P, None) != 0 and b"bad shape" in err()               # V < 2
        assert f(P, 80, 8, None, 2, 0, 8, 2, 0.33, P, None) != 0 and b"bad shape" in err()                # T < 1
        assert f(P, 4097 * 8, 8, None, 2, 4097, 8, 2, 0.33, P, None) != 0 and b"bad shape" in err()       # T > 4096
        assert f(P, 80, 8, None, 2, 10, 8, 3, 0.33, P, None) != 0 and b"unknown method" in err()
        assert f(P, 80, 8, None, 2, 10, 8, -1, 0.33, P, None) != 0 and b"unknown method" in err()
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            assert f(P, 80, 8, None, 2, 10, 8, 2, bad, P, None) != 0 and b"finite and > 0" in err()
        for bad in (1.0, 1.0 + 1.0 / 128, 1.0 - 1.0 / 128):
            assert f(P, 80, 8, None, 2, 10, 8, 2, bad, P, None) != 0 and b"entropy" in err()
        assert f(P, 80, 4, None, 2, 10, 8, 2, 0.33, P, None) != 0 and b"strides" in err()                 # time stride < row
        assert f(P, 8, 8, None, 2, 10, 8, 2, 0.33, P, None) != 0 and b"strides" in err()                  # neither [B][T][V] nor [T][B][V]
        assert f(P, 80, 8, None, 0, 10, 8, 2, 0.33, P, None) == 0                                         # B = 0: nothing to do
        # (conf, spans, lengths, B, T, L, aggregation, token_conf, stream)
        s = lib.av_ctc_span_conf
        assert s(None, P, None, 2, 10, 3, 1, P, None) != 0 and b"null" in err()
        assert s(P, None, None, 2, 10, 3, 1, P, None) != 0 and b"null" in err()
        assert s(P, P, None, 2, 10, 3, 1, None, None) != 0 and b"null" in err()
        assert s(P, P, None, 2, 10, 3, 3, P, None) != 0 and b"unknown aggregation" in err()
        assert s(P, P, None, 2, 4097, 3, 1, P, None) != 0 and b"bad shape" in err()
        assert s(P, P, None, 2, 10, -1, 1, P, None) != 0 and b"bad shape" in err()
        assert s(P, P, None, 2, 10, 0, 1, P, None) == 0                                                   # L = 0: no launch
        # (log_probs, stride_b, stride_t, lengths, B, T, V, blank, method, alpha, aggregation, ids, len, spans, token_conf, frame_conf, stream)
        g = lib.av_ctc_greedy_timed
        for k in (0, 11, 12, 13, 14, 15):
            a = [P, 80, 8, None, 2, 10, 8, 0, 2, 0.33, 1, P, P, P, P, P, None]
            a[k] = None
            assert g(*a) != 0 and b"null" in err()
        assert g(P, 80, 8, None, 2, 10, 8, 8, 2, 0.33, 1, P, P, P, P, P, None) != 0 and b"blank" in err()
        assert g(P, 80, 8, None, 2, 10, 8, -1, 2, 0.33, 1, P, P, P, P, P, None) != 0 and b"blank" in err()
        assert g(P, 80, 8, None, 2, 10, 8, 0, 5, 0.33, 1, P, P, P, P, P, None) != 0 and b"unknown method" in err()
        assert g(P, 80, 8, None, 2, 10, 8, 0, 2, 1.0, 1, P, P, P, P, P, None) != 0 and b"entropy" in err()
        assert g(P, 80, 8, None, 2, 10, 8, 0, 2, 0.33, 9, P, P, P, P, P, None) != 0 and b"unknown aggregation" in err()
        assert g(P, 80, 8, None, 2, 4097, 8, 0, 2, 0.33, 1, P, P, P, P, P, None) != 0 and b"bad shape" in err()
        assert g(P, 10, 1, None, 2, 10, 1, 0, 2, 0.33, 1, P, P, P, P, P, None) != 0 and b"bad shape" in err()
        assert g(P, 80, 4, None, 2, 10, 8, 0, 2, 0.33, 1, P, P, P, P, P, None) != 0 and b"strides" in err()
