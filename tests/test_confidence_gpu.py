"""GPU: the kernels of csrc/ctc_confidence.hip in both libraries.  The frame pass against the float64 law of tests/confidence_ref.py within
4 x the error the float32 host law makes on the same inputs (floor 2^-22), on every load path, layout and length; the span pass bit for bit
against the host law on the device's own frame confidences; greedy_timed against greedy_batch, the separate passes and forced_align; and
MultimodalTrainer.transcribe on labeled and unlabeled batches."""
import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import gpu_trainer
import confidence_ref as R

pytestmark = pytest.mark.gpu

B, T = 3, 8
FLOOR = 2.0 ** -22


@pytest.fixture(params=["fp32", "fp16"])
def library(request):
    """libavhip.so and libavhip_f16.so (the confidences are float32 in both)."""
    P = pkg("precision")
    old = P.get_precision()
    P.set_precision(request.param)
    yield request.param
    P.set_precision(old)


_CASES = {}
_RATIO = {"worst": 0.0}


def _case(V, scale):
    """The inputs of tests/test_confidence_cpu.py for (V, scale), and per setting the float64 reference and the float32 host law's error
    against it: computed once for both libraries."""
    key = (V, scale)
    if key not in _CASES:
        C = pkg("confidence")
        lp = R.make_logits(1, B, T, V, scale)
        per = {}
        for method, alpha in R.settings():
            want = R.frame_conf(lp, [T] * B, method, alpha)
            host = C.frame_confidence(torch.from_numpy(lp), None, method, alpha).numpy().astype(np.float64)
            per[(method, alpha)] = (want, float(np.abs(host - want).max()))
        _CASES[key] = (lp, per)
    return _CASES[key]


def _check(got, want, yard, what):
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape, what
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    bound = max(4 * yard, FLOOR)
    _RATIO["worst"] = max(_RATIO["worst"], err / bound)
    print(f"[confidence gpu] {what}: |device - float64| {err:.2e}, host float32 {yard:.2e}, bound {bound:.2e}, ratio {err / bound:.3f} "
          f"(worst so far {_RATIO['worst']:.3f})")
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("V", R.VS)
def test_frame_pass_against_float64(library, V, scale):
    C = pkg("confidence")
    lp, per = _case(V, scale)
    x = torch.from_numpy(lp).cuda()
    stacked = torch.cat([x, x.flip(0)], 0)                              # lp12[:B]: a view of a stacked tensor
    tm = x.transpose(0, 1).contiguous()                                 # [T, B, V]
    flat = torch.empty(B * T * V + 1, dtype=torch.float32, device="cuda")
    off = flat[1:].view(B, T, V)                                        # a row base that is not 16-byte aligned
    off.copy_(x)
    assert off.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    il = torch.tensor([0, 1, T])
    keep = (np.arange(T)[None, :] < il.numpy()[:, None])
    for (method, alpha), (want, yard) in per.items():
        tag = f"{library} V={V} scale={scale} {method} {alpha}"
        _check(C.frame_confidence(stacked[:B], None, method, alpha), want, yard, tag)
        _check(C.frame_confidence(tm, None, method, alpha, batch_first=False), want, yard, tag + " [T][B][V]")
        _check(C.frame_confidence(off, None, method, alpha), want, yard, tag + " unaligned")
        got = C.frame_confidence(x, il.cuda(), method, alpha)
        _check(got, want * keep, yard, tag + " lengths 0, 1, T")
        assert bool((got.cpu()[~torch.from_numpy(keep)] == 0).all())
        assert torch.equal(C.frame_confidence(x, il, method, alpha), got)                       # host lengths: copied


def test_frame_pass_edge_rows(library):
    """-inf entries, a row without a finite maximum, a NaN, a +inf, one-hot and uniform rows, under the bound of the frame test; V = 2052:
    the 16-byte loads of a row that is read twice."""
    C = pkg("confidence")
    for V in (9, 800, 2052):
        lp = R.make_logits(3, 2, 8, V, 3.0)
        lp[0, 1, 3:] = -np.inf
        lp[0, 2, :] = -np.inf
        lp[0, 3, 4] = np.nan
        lp[0, 4, 0] = np.inf
        lp[0, 5, :] = -np.inf
        lp[0, 5, V - 1] = 0.0
        lp[0, 6, :] = np.log(np.float32(1.0 / V))
        for method, alpha in R.settings():
            dev = C.frame_confidence(torch.from_numpy(lp).cuda(), None, method, alpha)
            want = R.frame_conf(lp, [8, 8], method, alpha)
            host = C.frame_confidence(torch.from_numpy(lp), None, method, alpha).numpy().astype(np.float64)
            _check(dev, want, float(np.abs(host - want).max()), f"{library} edge rows V={V} {method} {alpha}")
            got = dev.cpu().numpy()
            assert not np.isnan(got).any() and got[0, 2] == 0 and got[0, 3] == 0 and got[0, 4] == 0 and got[0, 5] == 1.0


@pytest.mark.parametrize("agg", R.AGGREGATIONS)
def test_span_pass_equals_the_host_law_on_the_device_confidences(library, agg):
    C = pkg("confidence")
    Bs, Ts, V = 4, 40, 67
    lp = torch.from_numpy(R.make_logits(7, Bs, Ts, V, 3.0)).cuda()
    il = torch.tensor([Ts, 17, 0, 1])
    conf = C.frame_confidence(lp, il)
    rng = np.random.default_rng(3)
    lo = rng.integers(0, Ts, size=(Bs, 300))
    spans = np.stack([lo, lo + rng.integers(0, 12, size=(Bs, 300))], -1).astype(np.int32)        # some empty, some past T_b and past T
    spans[:, :5] = -1
    spans[:, 5] = (0, Ts)
    spans[:, 6] = (-3, 4)
    sp = torch.from_numpy(spans)
    want = C.span_confidence(conf.cpu(), sp, il, agg)
    got = C.span_confidence(conf, sp.cuda(), il.cuda(), agg)
    assert got.is_cuda and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(C.span_confidence(conf, sp, il, agg), got)                               # host spans and lengths: copied
    assert bool((got[:, :5] == 0).all()) and bool((got[2] == 0).all())
    assert C.span_confidence(conf, sp[:, :0].cuda(), il, agg).shape == (Bs, 0)                   # L = 0
    n = torch.tensor([300, 4, 0, 7])
    utt = C.utterance_confidence(got, n.cuda(), agg)
    assert torch.equal(utt.cpu().view(torch.int32), C.utterance_confidence(got.cpu(), n, agg).view(torch.int32))


def _greedy_checks(C, lp, blank, il, method, alpha, agg):
    bs = pkg("beam_search")
    g = C.greedy_timed(lp, blank, il, method, alpha, agg)
    assert all(x.is_cuda for x in g)
    Bn, Tn, _ = lp.shape
    want_ids = bs.greedy_batch(lp.contiguous(), blank, il)
    n = g.lengths.cpu().tolist()
    assert n == [len(w) for w in want_ids]
    ids = g.ids.cpu()
    for b in range(Bn):
        assert ids[b, :n[b]].tolist() == want_ids[b] and bool((ids[b, n[b]:] == -1).all()) and bool((g.spans[b, n[b]:] == -1).all())
    assert torch.equal(g.frame_conf.view(torch.int32), C.frame_confidence(lp, il, method, alpha).view(torch.int32))
    assert torch.equal(g.token_conf.view(torch.int32), C.span_confidence(g.frame_conf, g.spans, il, agg).view(torch.int32))
    again = C.greedy_timed(lp, blank, il, method, alpha, agg)
    for p, q in zip(g, again):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    return g


def test_greedy_timed_spans_are_forced_align_spans(library):
    """The 40 seeds of tests/test_confidence_cpu.py, four per call: no allowance."""
    C = pkg("confidence"); A = pkg("align")
    for s0 in range(0, 40, 4):
        lp = torch.cat([torch.log_softmax(2 * torch.randn(1, 23, 7, generator=torch.Generator().manual_seed(s)), -1) for s in range(s0, s0 + 4)])
        x = lp.cuda()
        g = _greedy_checks(C, x, 0, None, "tsallis", 0.33, "min")
        al = A.forced_align(x, g.ids.clamp_min(0), None, g.lengths, blank=0)
        assert torch.equal(al.spans, g.spans), s0
        host = C.greedy_timed(lp, 0)
        assert torch.equal(host.ids, g.ids.cpu()) and torch.equal(host.spans, g.spans.cpu()) and torch.equal(host.lengths, g.lengths.cpu())


@pytest.mark.parametrize("V", [67, 800, 2051])
def test_greedy_timed_equals_the_separate_passes(library, V):
    C = pkg("confidence")
    Bg, Tg = 4, 40
    lp = torch.from_numpy(R.make_logits(11, Bg, Tg, V, 3.0)).clone()
    lp[:, :, 3] += 6.0                                                  # the blank wins about half of the frames
    lp[2, :, 3] = 50.0                                                  # an all-blank utterance
    lp[0, 5:9, 10] = 40.0                                               # a run of four equal frames between two blanks
    lp[0, 4, 3] = lp[0, 9, 3] = 60.0
    x = lp.cuda()
    il = torch.tensor([Tg, 17, Tg, 0]).cuda()
    for (method, alpha), agg in zip(R.settings(), ("min", "mean", "prod", "min", "mean")):
        g = _greedy_checks(C, x, 3, il, method, alpha, agg)
        assert int(g.lengths[2]) == 0 and int(g.lengths[3]) == 0 and bool((g.token_conf[2:] == 0).all())
        sp = g.spans[0, :int(g.lengths[0])].cpu().tolist()
        assert [5, 9] in sp
        _greedy_checks(C, x, 3, None, method, alpha, agg)
    stacked = torch.cat([x, x], 0)
    a, b = C.greedy_timed(stacked[:Bg], 3, il), C.greedy_timed(x.transpose(0, 1).contiguous(), 3, il, batch_first=False)
    for p, q in zip(a, b):
        assert torch.equal(p, q)


def test_trainer_transcribe():
    """transcribe() on a batch without ``text*`` and ``mask*``; with the dataset's masks its texts are evaluate()'s at beam width 0 and 4,
    its word times are word_segments(forced_align(hypothesis)); module modes are restored and the next training step is untouched."""
    init = pkg("utils.init"); synth = pkg("dataset.synthetic"); A = pkg("align"); bs = pkg("beam_search")
    batch = synth.make_batch(3, 1.0, seed=5, ragged=True)
    t = gpu_trainer(init.W2V2_TINY, "fp32")
    mods = [sm for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1) for sm in m.modules()]
    blank = t.tokenizer.blank_id
    for W in (0, 4):
        t.eval_beam_width = W
        t.evaluate([batch])
        want_text = t.last_decoded
        t.decoder1.train(); t.fusion_module.train()
        modes = [m.training for m in mods]
        assert any(modes) and not all(modes)
        seen = []
        inner = t.forward_log_probs

        def recording(b):
            assert not any(m.training for m in mods)
            seen.append(inner(b))
            return seen[-1]
        t.forward_log_probs = recording
        res = t.transcribe(batch, nbest=1 if W == 0 else 3)
        t.forward_log_probs = inner
        assert len(seen) == 1 and [m.training for m in mods] == modes
        words = 0
        for k, spk in enumerate(("1", "2")):
            assert [r["text"] for r in res[k]] == want_text[k], (W, spk)
            lp = seen[0]["log_probs" + spk].float()
            ids = [r["ids"] for r in res[k]]
            tg = torch.zeros((len(ids), max(1, max(len(i) for i in ids))), dtype=torch.long)
            for i, seq in enumerate(ids):
                tg[i, :len(seq)] = torch.tensor(seq, dtype=torch.long)
            al = A.forced_align(lp, tg, None, torch.tensor([len(i) for i in ids]), blank=blank)
            for i, r in enumerate(res[k]):
                assert sorted(r) == sorted(["text", "ids", "confidence", "words"] + (["nbest"] if W else []))
                assert r["text"] == bs.fast_decode(r["ids"], t.tokenizer) and 0.0 <= r["confidence"] <= 1.0
                seg = A.word_segments(t.tokenizer, r["ids"], al.spans[i].cpu(), al.token_scores[i].cpu(), 25.0)
                assert [(w["word"], w["start"], w["end"]) for w in r["words"]] == [(w["word"], w["start"], w["end"]) for w in seg]
                for w, s in zip(r["words"], seg):
                    assert abs(w["score"] - s["score"]) <= 1e-5 * max(1.0, abs(s["score"])) and 0.0 <= w["confidence"] <= 1.0
                    assert sorted(w) == ["confidence", "end", "score", "start", "word"]
                words += len(r["words"])
                if W:
                    assert 1 <= len(r["nbest"]) <= 3 and r["nbest"][0][0] == r["text"]
                    assert all(a[1] >= b[1] for a, b in zip(r["nbest"], r["nbest"][1:]))
        print(f"[trainer.transcribe] beam {W}: {words} words; speaker 1: {[(r['text'], round(r['confidence'], 3)) for r in res[0]]}")
        # no transcript, no masks: the masks come from the lengths the batch carries
        bare = {k: v for k, v in batch.items() if not k.startswith(("text", "mask"))}
        res_b = t.transcribe(bare)
        assert [len(x) for x in res_b] == [3, 3] and all(isinstance(r["text"], str) and isinstance(r["words"], list) for x in res_b for r in x)
        assert [m.training for m in mods] == modes
        only = {k: batch[k] for k in ("audio", "lip1", "lip2")}
        assert [len(x) for x in t.transcribe(only)] == [3, 3]
    # a following training step is the step of a trainer that never transcribed
    t.eval_beam_width = 0
    fresh = gpu_trainer(init.W2V2_TINY, "fp32")
    losses = []
    for tr in (t, fresh):
        for m in (tr.visual_encoder, tr.audio_encoder, tr.fusion_module, tr.decoder1):
            m.train()
        torch.manual_seed(0)
        losses.append(float(tr.train_step(batch)["total"].detach()))
    assert losses[0] == losses[1], losses
