"""GPU: the kernels of csrc/ctc_longform.hip in both libraries against the host laws of longform.py (centre stitch, cut points and segments
exactly; the average stitch against the float64 law of tests/longform_ref.py within 4 x the error of the float32 host law on the same inputs),
on strided and offset views, and MultimodalTrainer.transcribe_long on the tiny trainer against the host pipeline and against transcribe()."""
import math

import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import gpu_trainer
import longform_ref as R

pytestmark = pytest.mark.gpu

W = 12
STRIDES = (0, 2, 4)                     # 4: three and four sources per frame
FRAMES = (1, 12, 13, 29, 61)
SEGMENT, RADIUS = 30, 5                 # N = 20


@pytest.fixture(params=["fp32", "fp16"])
def library(request):
    """libavhip.so and libavhip_f16.so (the long-form kernels are float32 in both)."""
    P = pkg("precision")
    old = P.get_precision()
    P.set_precision(request.param)
    yield request.param
    P.set_precision(old)


_CASES = {}
_RATIO = {"worst": 0.0}


def _case(V, S, F):
    """Window log-probs for (V, S, F) with an S axis of 2, the host laws' results and the float64 average: computed once for both libraries."""
    key = (V, S, F)
    if key not in _CASES:
        LF = pkg("longform")
        p = LF.plan_windows(F, W, S)
        win = R.make_windows(1000 * V + 10 * F + S, 2, p.count, p.width, V)
        if V > 4 and p.count > 1:
            win[0, 0, p.width - 1, 3] = -np.inf                # a -inf source beside finite ones, and a class that is -inf in every source
            win[:, :, :, 4] = -np.inf
        x = torch.from_numpy(win)
        centre, average = LF.stitch(x, p), LF.stitch(x, p, "average")
        want = R.stitch(win, F, W, S, "average")
        ok = np.isfinite(want)
        yard = float(np.abs(average.numpy().astype(np.float64)[ok] - want[ok]).max())
        _CASES[key] = (p, win, centre, average, want, ok, yard)
    return _CASES[key]


@pytest.mark.parametrize("V", [2, 37, 800])
def test_kernels_against_the_host_laws(library, V):
    LF = pkg("longform")
    blank = V - 1
    for S in STRIDES:
        for F in FRAMES:
            p, win, centre, average, want, ok, yard = _case(V, S, F)
            x = torch.from_numpy(win).cuda()
            got = LF.stitch(x, p)
            assert got.is_cuda and got.dtype == torch.float32
            assert torch.equal(got.cpu().view(torch.int32), centre.view(torch.int32)), (V, S, F)           # bit for bit
            avg = LF.stitch(x, p, "average")
            a = avg.cpu().numpy()
            assert np.array_equal(np.isnan(a), np.isnan(want)) and np.array_equal(a == -np.inf, want == -np.inf), (V, S, F)
            err = float(np.abs(a.astype(np.float64)[ok] - want[ok]).max())
            ratio = err / yard if yard > 0 else (0.0 if err == 0 else math.inf)
            _RATIO["worst"] = max(_RATIO["worst"], ratio)
            print(f"[longform gpu] {library} V={V} S={S} F={F} coverage {p.coverage}: |device - float64| {err:.3e}, host float32 {yard:.3e}, "
                  f"ratio {ratio:.3f} (worst so far {_RATIO['worst']:.3f})")
            assert err <= 4 * yard, (V, S, F, err, yard)
            row, _ = p.sources("average")
            single = torch.from_numpy((row >= 0).sum(1) == 1)
            assert torch.equal(avg.cpu()[:, single].view(torch.int32), average[:, single].view(torch.int32))   # single-source frames: copies
            # cut points and segments: on the device's own stitched tensor, against the host laws on its copy
            for lp in (got, avg):
                h = lp.cpu()
                cuts = LF.cut_points(lp, blank, SEGMENT, RADIUS)
                assert cuts.is_cuda and cuts.dtype == torch.int32
                assert torch.equal(cuts.cpu(), LF.cut_points(h, blank, SEGMENT, RADIUS)), (V, S, F)
                seg, ln = LF.split_segments(lp, cuts, SEGMENT)
                hs, hl = LF.split_segments(h, cuts.cpu(), SEGMENT)
                assert seg.is_cuda and ln.is_cuda and ln.dtype == torch.int64
                assert tuple(seg.shape) == (2 * (LF.boundaries(F, SEGMENT, RADIUS) + 1), SEGMENT, V)
                assert torch.equal(seg.cpu().view(torch.int32), hs.view(torch.int32)) and torch.equal(ln.cpu(), hl), (V, S, F)


def test_cut_points_ties_and_nan_on_the_device(library):
    LF = pkg("longform")
    F, V, blank = 150, 37, 2
    lp = torch.log_softmax(2 * torch.randn(2, F, V, generator=torch.Generator().manual_seed(9)), -1)
    lp[0, 15:26, blank] = -0.25                                            # a tie over a whole zone: its first frame
    lp[1, 17, blank] = float("nan")
    lp[1, 18, blank] = lp[1, 21, blank] = 0.0                              # a tie of two: the first
    lp[0, 35:46, blank] = float("nan")                                     # a zone of NaN: its first frame
    lp[1, 35:46, blank] = float("-inf")
    cuts = LF.cut_points(lp.cuda(), blank, SEGMENT, RADIUS)
    assert torch.equal(cuts.cpu(), LF.cut_points(lp, blank, SEGMENT, RADIUS))
    assert cuts[:, 1].tolist() == [15, 18] and cuts[:, 2].tolist() == [35, 35]
    for s in range(2):
        assert cuts[s].tolist() == R.cut_points(lp[s, :, blank].numpy(), SEGMENT, RADIUS)


@pytest.mark.parametrize("V", [37, 800])
def test_strided_and_offset_views(library, V):
    """Rows that are not 16-byte aligned, a row stride larger than V, a speaker stride larger than the block: the same results."""
    LF = pkg("longform")
    S, F = 4, 61
    p, win, centre, average, _, _, _ = _case(V, S, F)
    x = torch.from_numpy(win).cuda()
    flat = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")
    off = flat[1:].view(x.shape)                                           # every row base off by 4 bytes
    off.copy_(x)
    wide = torch.zeros((3, p.count, p.width, V + 3), dtype=torch.float32, device="cuda")
    wide[:2, :, :, :V] = x
    views = {"offset": off, "wide rows": wide[:2, :, :, :V], "wide speakers": torch.cat([x, x], 1)[:, :p.count]}
    assert off.data_ptr() % 16 == 4 and not views["wide rows"].is_contiguous()
    for what, v in views.items():
        ref_avg = LF.stitch(x, p, "average")
        assert torch.equal(LF.stitch(v, p).cpu().view(torch.int32), centre.view(torch.int32)), what
        assert torch.equal(LF.stitch(v, p, "average").view(torch.int32), ref_avg.view(torch.int32)), what
    lp = LF.stitch(x, p)
    big = torch.zeros((3, F + 2, V + 1), dtype=torch.float32, device="cuda")
    big[:2, 1:F + 1, :V] = lp
    view = big[:2, 1:F + 1, :V]
    blank = 5
    cuts = LF.cut_points(lp, blank, SEGMENT, RADIUS)
    assert torch.equal(LF.cut_points(view, blank, SEGMENT, RADIUS), cuts)
    seg, ln = LF.split_segments(lp, cuts, SEGMENT)
    seg2, ln2 = LF.split_segments(view, cuts, SEGMENT)
    assert torch.equal(seg.view(torch.int32), seg2.view(torch.int32)) and torch.equal(ln, ln2)
    assert torch.equal(LF.split_segments(lp, cuts.cpu(), SEGMENT)[0].view(torch.int32), seg.view(torch.int32))       # host cuts: copied


def _recording(frames, seed):
    """Synthetic clips of one second, concatenated and cut to ``frames`` lip frames."""
    synth = pkg("dataset.synthetic")
    clips = [synth.make_batch(1, 1.0, seed=seed + i) for i in range(-(-frames // 25))]
    return {"audio": torch.cat([c["audio"][0] for c in clips])[:640 * frames],
            "lip1": torch.cat([c["lip1"][0] for c in clips])[:frames], "lip2": torch.cat([c["lip2"][0] for c in clips])[:frames]}


def _host_pipeline(t, LF, windows, plan, beam):
    """The recorded window log-probs [2, nw, W, V] on the host through longform's host laws and the host decoders -> per speaker (ids, spans)."""
    C = pkg("confidence"); A = pkg("align"); bs = pkg("beam_search")
    blank = t.tokenizer.blank_id
    lp = LF.stitch(windows, plan, t.long_policy)
    cuts = LF.cut_points(lp, blank, t.long_segment, t.long_radius)
    seg, ln = LF.split_segments(lp, cuts, t.long_segment)
    ns = cuts.shape[1] - 1
    if beam == 0:
        g = C.greedy_timed(seg, blank, ln)
        ids = [g.ids[i, :int(g.lengths[i])].tolist() for i in range(2 * ns)]
        spans = g.spans
    else:
        ids = bs.prefix_beam_search(seg, beam, blank, lengths=ln)
        tg = torch.zeros((2 * ns, max(1, max(len(i) for i in ids))), dtype=torch.long)
        for i, q in enumerate(ids):
            tg[i, :len(q)] = torch.tensor(q, dtype=torch.long)
        spans = A.forced_align(seg, tg, ln, torch.tensor([len(i) for i in ids]), blank=blank).spans
    out = []
    for s in range(2):
        all_ids, all_spans = [], []
        for j in range(ns):
            i = s * ns + j
            all_ids += ids[i]
            all_spans += (spans[i, :len(ids[i])] + int(cuts[s, j])).tolist()
        out.append((all_ids, all_spans, cuts[s].tolist()))
    return out


def test_trainer_transcribe_long():
    """F = 65 in windows of 25 (5 discarded per side, 3 per forward call), segments of 30: the result is the host pipeline's on the recorded
    window log-probs at beam 0 and 4; module modes are restored and the next training step is untouched."""
    init = pkg("utils.init"); synth = pkg("dataset.synthetic"); LF = pkg("longform"); A = pkg("align"); bs = pkg("beam_search")
    F = 65
    kw = dict(long_window=25, long_stride=5, long_batch=3, long_segment=30, long_radius=5)
    t = gpu_trainer(init.W2V2_TINY, "fp32", **kw)
    rec = _recording(F, 11)
    plan = LF.plan_windows(F, 25, 5)
    assert plan.count == 4
    mods = [sm for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1) for sm in m.modules()]
    for beam in (0, 4):
        t.eval_beam_width = beam
        t.decoder1.train(); t.fusion_module.train()
        modes = [m.training for m in mods]
        assert any(modes)
        seen = []
        inner = t.forward_log_probs

        def recording(b):
            assert not any(m.training for m in mods)
            assert tuple(b["lip1"].shape[1:]) == (25, 1, 96, 96) and b["audio"].shape[1] == 640 * 25
            seen.append(inner(b))
            return seen[-1]
        t.forward_log_probs = recording
        res = t.transcribe_long(rec if beam == 0 else {k: v.cuda() for k, v in rec.items()}, nbest=1 if beam == 0 else 2)
        t.forward_log_probs = inner
        assert len(seen) == -(-plan.count // 3) and [m.training for m in mods] == modes
        windows = torch.stack([torch.cat([o["log_probs" + spk].float().cpu() for o in seen]) for spk in ("1", "2")])
        assert tuple(windows.shape[:3]) == (2, plan.count, 25)
        want = _host_pipeline(t, LF, windows, plan, beam)
        words = 0
        for s in range(2):
            r, (ids, spans, cuts) = res[s], want[s]
            assert sorted(r) == ["confidence", "ids", "segments", "text", "words"]
            assert r["ids"] == ids and r["text"] == bs.fast_decode(ids, t.tokenizer), (beam, s)
            seg = A.word_segments(t.tokenizer, ids, torch.tensor(spans, dtype=torch.int32).reshape(-1, 2), torch.zeros(len(ids)), 25.0)
            assert [(w["word"], w["start"], w["end"]) for w in r["words"]] == [(w["word"], w["start"], w["end"]) for w in seg], (beam, s)
            times = [x for w in r["words"] for x in (w["start"], w["end"])]
            assert times == sorted(times) and all(0.0 <= x <= F / 25.0 for x in times)
            assert all(0.0 <= w["confidence"] <= 1.0 for w in r["words"]) and 0.0 <= r["confidence"] <= 1.0
            assert [(p["start"], p["end"]) for p in r["segments"]] == [(a / 25.0, b / 25.0) for a, b in zip(cuts, cuts[1:])]
            assert len(r["segments"]) == 3 and "".join(p["text"] for p in r["segments"]).replace(" ", "") == r["text"].replace(" ", "")
            for p in r["segments"]:
                assert sorted(p) == sorted(["start", "end", "text", "confidence"] + (["nbest"] if beam else []))
                if beam:
                    assert 1 <= len(p["nbest"]) <= 2 and p["nbest"][0][0] == p["text"]
            words += len(r["words"])
        print(f"[trainer.transcribe_long] beam {beam}: {words} words, cuts {want[0][2]} / {want[1][2]}; speaker 1: {res[0]['text']!r} "
              f"{res[0]['confidence']:.3f}")
    # a following training step is the step of a trainer that never transcribed
    t.eval_beam_width = 0
    batch = synth.make_batch(3, 1.0, seed=5, ragged=True)
    fresh = gpu_trainer(init.W2V2_TINY, "fp32")
    losses = []
    for tr in (t, fresh):
        for m in (tr.visual_encoder, tr.audio_encoder, tr.fusion_module, tr.decoder1):
            m.train()
        torch.manual_seed(0)
        losses.append(float(tr.train_step(batch)["total"].detach()))
    assert losses[0] == losses[1], losses


def test_short_recording_is_transcribe():
    """F = 20 <= long_window and <= long_segment: field by field what transcribe() gives for that clip, at beam 0 and 4."""
    init = pkg("utils.init")
    t = gpu_trainer(init.W2V2_TINY, "fp32", long_window=25, long_stride=5, long_batch=3, long_segment=30, long_radius=5)
    rec = _recording(20, 3)
    batch = {k: v[None] for k, v in rec.items()}
    for beam in (0, 4):
        t.eval_beam_width = beam
        nb = 1 if beam == 0 else 3
        want = t.transcribe(batch, nbest=nb)
        got = t.transcribe_long(rec, nbest=nb)
        again = t.transcribe_long(batch, nbest=nb)                          # the [1, ...] forms
        for s in range(2):
            w, g = want[s][0], got[s]
            for key in ("text", "ids", "confidence", "words"):
                assert g[key] == w[key], (beam, s, key, g[key], w[key])
            assert len(g["segments"]) == 1 and (g["segments"][0]["start"], g["segments"][0]["end"]) == (0.0, 20 / 25.0)
            assert g["segments"][0]["text"] == w["text"] and g["segments"][0]["confidence"] == w["confidence"]
            if beam:
                assert g["segments"][0]["nbest"] == w["nbest"]
            assert again[s] == g
        print(f"[trainer.transcribe_long] F=20 beam {beam}: {got[0]['text']!r} == transcribe()")
