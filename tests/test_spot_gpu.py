"""GPU: CTC keyword spotting on the kernels of csrc/ctc_spot.hip against the package's host law (spot.keyword_spot on host tensors, float32
numpy; tests/test_spot_cpu.py holds that law to the float64 reference).  The law is exact, so every case asks for equality: torch.equal on
hits and counts and on the BITS of the scores, in both libraries.  Then MultimodalTrainer.spot / spot_long on the tiny synthetic model."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import gpu_trainer
import spot_ref as R

pytestmark = pytest.mark.gpu

NEG = float("-inf")


@pytest.fixture(params=["fp32", "fp16"])
def library(request):
    """libavhip.so and libavhip_f16.so (the spotting kernels are float32 in both)."""
    P = pkg("precision")
    old = P.get_precision()
    P.set_precision(request.param)
    yield request.param
    P.set_precision(old)


_HOST = {}


def _host(key, lp, keywords, **kw):
    """The host law's result, computed once per case and shared by both libraries."""
    if key not in _HOST:
        _HOST[key] = pkg("spot").keyword_spot(lp, keywords, **kw)
    return _HOST[key]


def _same(dev, host, what):
    assert dev.hits.is_cuda and dev.hits.dtype == torch.int32 and dev.scores.dtype == torch.float32 and dev.counts.dtype == torch.int32
    assert torch.equal(dev.counts.cpu(), host.counts), (what, dev.counts.cpu(), host.counts)
    assert torch.equal(dev.hits.cpu(), host.hits), what
    assert torch.equal(dev.scores.cpu().view(torch.int32), host.scores.view(torch.int32)), what


def _sequence(rng, labels, L):
    """L ids with no two neighbours equal: it fits into L frames."""
    y = []
    for _ in range(L):
        c = int(rng.choice(labels))
        while y and c == y[-1]:
            c = int(rng.choice(labels))
        y.append(c)
    return y


def _small_case(T, V):
    """B 3 utterances; K 5 keywords of 1, 2, 31 and 32 ids (63 states: every lane of the wavefront; 1 id: one lane) and one with a repeated
    label, in a table wider than L_max; a few -inf entries and one row that is -inf throughout."""
    rng = np.random.default_rng(1000 * V + T)
    blank = int(rng.integers(0, V))
    labels = [v for v in range(V) if v != blank]
    lp = np.stack([R.make_log_probs(10000 * V + 10 * T + b, T, V, 3.0) for b in range(3)])
    lp[rng.random(lp.shape) < 0.02] = -np.inf
    if T >= 16:
        lp[1, T // 2, :] = -np.inf
    kws = [_sequence(rng, labels, L) for L in (1, 2, 31, 32)] + [[labels[0], labels[0], labels[1]]]
    ids = torch.zeros((5, 40), dtype=torch.int32)
    for k, y in enumerate(kws):
        ids[k, :len(y)] = torch.tensor(y, dtype=torch.int32)
    return torch.from_numpy(lp), blank, kws, ids, torch.tensor([len(y) for y in kws])


@pytest.mark.parametrize("V", [5, 800])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 33])
def test_small_shapes_against_the_host_law(library, T, V):
    """T around the 16-frame chunk, V 5 (4-byte loads) and 800 (16-byte loads), K 5 and K 1, max_hits 8 and 1, no lengths / ragged lengths
    on the host (0 and above T among them) / on the device, the table's leading dimension above L_max."""
    S = pkg("spot")
    lp, blank, kws, ids, lens = _small_case(T, V)
    x = lp.cuda()
    table = ids.cuda()[:, :32]                                         # int32 on the device: taken as it is, 40 ids apart
    assert table.stride(0) == 40
    ragged = torch.tensor([T + 7, 0, max(1, T - 3)])
    for name, il, N in (("none", None, 8), ("host", ragged, 8), ("device", ragged, 1)):
        want = _host((T, V, name), lp, kws, input_lengths=il, blank=blank, max_hits=N)
        il_d = il.cuda() if name == "device" else il
        _same(S.keyword_spot(x, kws, input_lengths=il_d, blank=blank, max_hits=N), want, (T, V, name, "lists"))
        _same(S.keyword_spot(x, (table, lens.cuda()), input_lengths=il_d, blank=blank, max_hits=N), want, (T, V, name, "device table"))
    one = _host((T, V, "one"), lp, kws[2:3], blank=blank, max_hits=8)
    _same(S.keyword_spot(x, kws[2:3], blank=blank, max_hits=8), one, (T, V, "K 1"))
    if T >= 32:
        assert int(_HOST[(T, V, "none")].counts[:, 2:4].sum()) > 0                # the 61- and 63-state lattices reach their last state


@pytest.mark.parametrize("V", [5, 800])
def test_views_and_an_invalid_row_among_valid_ones(library, V):
    """A [T, B, V] block, its [B, T, V] view, and sliced views with a padded row stride (V 800 + 4: still 16-byte loads; + 3: not) are taken
    as they are; a keyword row that holds the blank, one with an id outside [0, V) and one of length 0 give count 0 beside valid rows."""
    S = pkg("spot")
    T = 33
    lp, blank, kws, ids, lens = _small_case(T, V)
    il = torch.tensor([T, 20, 31])
    bad = torch.zeros((8, 32), dtype=torch.int64)
    bad[:5] = ids[:, :32]
    bad[5, :2] = torch.tensor([kws[0][0], blank]); bad[6, :2] = torch.tensor([kws[0][0], V]); bad[7, 0] = kws[0][0]
    bad_len = torch.cat([lens, torch.tensor([2, 2, 0])])
    want = _host((V, "invalid"), lp, (bad, bad_len), input_lengths=il, blank=blank, max_hits=4)
    assert want.counts[:, 5:].sum() == 0 and torch.equal(want.hits[:, :5], _host((V, "valid"), lp, kws, input_lengths=il, blank=blank).hits)
    x = lp.cuda()
    table = (bad.cuda(), bad_len.cuda())
    _same(S.keyword_spot(x, table, input_lengths=il, blank=blank), want, (V, "invalid row"))
    tbv = x.transpose(0, 1).contiguous()
    _same(S.keyword_spot(tbv, table, input_lengths=il, blank=blank, batch_first=False), want, (V, "[T, B, V]"))
    _same(S.keyword_spot(tbv.transpose(0, 1), table, input_lengths=il, blank=blank), want, (V, "[B, T, V] view of [T, B, V]"))
    for pad in (3, 4):
        wide = torch.full((3, T + 2, V + pad), float("nan"), device="cuda")
        wide[:, 1:T + 1, :V] = x
        view = wide[:, 1:T + 1, :V]
        assert view.stride(1) == V + pad and not view.is_contiguous()
        _same(S.keyword_spot(view, table, input_lengths=il, blank=blank), want, (V, "padded rows", pad))


_LONG = {}


def _long_case():
    """B 2, T 5000, V 32, K 3: argmax paths of filler runs (labels outside the keywords) with the keywords planted at known frames - one
    starts on frame 0, one lies across frame 4096, one ends on the last frame (utterance 0) or on the last frame of a shorter length
    (utterance 1)."""
    if not _LONG:
        T, V, blank = 5000, 32, 0
        kws = [[3, 5, 5, 7], [9], [4, 6]]
        others = [v for v in range(V) if v not in (3, 5, 7, 9, 4, 6)]
        shapes = {0: [3, 3, 5, 0, 5, 5, 7, 7, 7], 1: [9, 9], 2: [4, 0, 0, 6]}            # frames of one occurrence of each keyword
        lens = [T, 4500]
        lps, planted = [], []
        for b in range(2):
            rng = np.random.default_rng(50 + b)
            path = np.repeat(rng.choice(others, size=T), rng.integers(1, 4, size=T))[:T]
            at = {0: [0, 4090, lens[b] - 9, 1000 + b], 1: [20, 4200, 2500], 2: [30, lens[b] - 17, 3000]}
            want = {k: [] for k in at}
            for k, starts in at.items():
                for s in starts:
                    path[s:s + len(shapes[k])] = shapes[k]
                    want[k].append((s, s + len(shapes[k])))
            x = rng.random((T, V))
            x[np.arange(T), path] += 12.0
            x = x - x.max(axis=1, keepdims=True)
            lp = (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)
            assert lp.argmax(axis=1).tolist() == path.tolist()
            lps.append(lp)
            planted.append(want)
        _LONG.update(lp=torch.from_numpy(np.stack(lps)), kws=kws, lens=torch.tensor(lens), planted=planted, blank=blank)
    return _LONG


def test_a_walk_of_5000_frames_and_planted_occurrences(library):
    """Past the aligner's 4096 frames and far past one chunk.  With min_score 0.0 the device reports exactly the planted intervals with
    score +0.0; without a threshold it equals the host law on everything else it finds; two runs give the same bits."""
    S = pkg("spot")
    c = _long_case()
    x, il = c["lp"].cuda(), c["lens"].cuda()
    exact = S.keyword_spot(x, c["kws"], input_lengths=il, blank=c["blank"], max_hits=8, min_score=0.0)
    _same(exact, _host("long exact", c["lp"], c["kws"], input_lengths=c["lens"], blank=c["blank"], max_hits=8, min_score=0.0), "T 5000, planted")
    for b in range(2):
        for k, want in c["planted"][b].items():
            n = int(exact.counts[b, k])
            assert sorted(map(tuple, exact.hits[b, k, :n].tolist())) == sorted(want), (b, k)
            assert bool((exact.scores[b, k, :n].view(torch.int32) == 0).all())
    every = S.keyword_spot(x, c["kws"], input_lengths=il, blank=c["blank"], max_hits=8)
    _same(every, _host("long all", c["lp"], c["kws"], input_lengths=c["lens"], blank=c["blank"], max_hits=8), "T 5000, no threshold")
    again = S.keyword_spot(x, c["kws"], input_lengths=il, blank=c["blank"], max_hits=8)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(every, again))


def test_small_planted_occurrences_on_the_device(library):
    S = pkg("spot")
    for keyword in ([3, 5, 5, 7], [5, 5], [3]):
        lp, path, spans = R.planted(7 + len(keyword), keyword, 3, 10, 0, [0, 1, 2, 4, 6, 8, 9])
        s = S.keyword_spot(torch.from_numpy(lp)[None].cuda(), [keyword], blank=0, max_hits=8, min_score=0.0)
        assert s.hits[0, 0, :int(s.counts[0, 0])].tolist() == [list(x) for x in spans[::-1]]
        assert bool((s.scores[0, 0, :3].view(torch.int32) == 0).all()) and bool((s.scores[0, 0, 3:] == NEG).all())


def test_a_workspace_one_byte_short_is_an_error_not_a_launch(library):
    L = pkg("_lib"); ops = pkg("ops")
    B, T, V, K = 2, 20, 8, 3
    lp = torch.from_numpy(np.stack([R.make_log_probs(b, T, V) for b in range(B)])).cuda()
    kw = torch.tensor([[1, 2], [3, 0], [4, 5]], dtype=torch.int32, device="cuda")
    kl = torch.tensor([2, 1, 2], dtype=torch.int32, device="cuda")
    hits = torch.full((B, K, 4, 2), 7, dtype=torch.int32, device="cuda")
    scores = torch.full((B, K, 4), 7.0, device="cuda")
    counts = torch.full((B, K), 7, dtype=torch.int32, device="cuda")
    need = L.ll(0)
    L.check(L.lib().av_ctc_spot_workspace_bytes(B, T, K, ctypes.byref(need)))
    assert need.value == 4 * B * T * (1 + 2 * K)
    ws = torch.empty((need.value // 4,), dtype=torch.int32, device="cuda")

    def call(nbytes):
        return L.lib().av_ctc_spot(ops.ptr(lp), T * V, V, None, ops.ptr(kw), 2, ops.ptr(kl), B, T, V, K, 2, 0, 4, NEG, ops.ptr(hits),
                                   ops.ptr(scores), ops.ptr(counts), ops.ptr(ws), nbytes, ops.stream())
    assert call(need.value - 1) != 0 and b"too small" in L.lib().av_last_error()
    torch.cuda.synchronize()
    assert bool((hits == 7).all()) and bool((scores == 7.0).all()) and bool((counts == 7).all())
    assert call(need.value) == 0
    want = pkg("spot").keyword_spot(lp.cpu(), (kw.cpu(), kl.cpu()), blank=0, max_hits=4)
    _same(pkg("spot").Spots(hits, scores, counts), want, "raw call")


# ---- the trainer ----
LONG_KW = dict(long_window=25, long_stride=5, long_batch=2, long_segment=30, long_radius=5)
_TRAINER = {}


def _trainer():
    if not _TRAINER:
        _TRAINER["t"] = gpu_trainer(pkg("utils.init").W2V2_TINY, "fp32", **LONG_KW)
    pkg("precision").set_precision("fp32")
    _TRAINER["t"].eval_beam_width = 0
    return _TRAINER["t"]


def _recorded(t, fn):
    """Run ``fn`` with forward_log_probs recorded -> (its result, the outputs of every call, whether a module was in training mode inside)."""
    mods = [sm for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1) for sm in m.modules()]
    seen, training, inner = [], [], t.forward_log_probs

    def recording(b):
        training.append(any(m.training for m in mods))
        seen.append(inner(b))
        return seen[-1]
    t.forward_log_probs = recording
    try:
        res = fn()
    finally:
        t.forward_log_probs = inner
    return res, seen, any(training)


def _recording(frames, seed):
    """Synthetic clips of one second, concatenated and cut to ``frames`` lip frames."""
    synth = pkg("dataset.synthetic")
    clips = [synth.make_batch(1, 1.0, seed=seed + i) for i in range(-(-frames // 25))]
    return {"audio": torch.cat([c["audio"][0] for c in clips])[:640 * frames],
            "lip1": torch.cat([c["lip1"][0] for c in clips])[:frames], "lip2": torch.cat([c["lip2"][0] for c in clips])[:frames]}


def test_trainer_spot_is_keyword_spot_on_its_log_probs_and_agrees_with_the_greedy_transcript():
    """spot() on a batch without text or masks equals hit_segments(keyword_spot(...)) on the log-probs of its own forward_log_probs call; a
    keyword cut from an utterance's greedy transcript is reported for that utterance with score 0.0 at the frames of the greedy spans
    (the spans behind transcribe()'s word times); module modes are restored."""
    S = pkg("spot"); C = pkg("confidence"); B = pkg("bias")
    t = _trainer()
    batch = {k: v for k, v in pkg("dataset.synthetic").make_batch(3, 1.0, seed=21).items() if k in ("audio", "lip1", "lip2")}
    blank, pieces = t.tokenizer.blank_id, t.tokenizer.id_to_token
    out = _recorded(t, lambda: t.spot(batch, [[5]]))[1][0]             # the log-probs spot() sees: eval mode
    # keywords from the greedy transcripts: per utterance and speaker the first (up to) three tokens and the next (up to) two
    cut = {}
    for spk in ("1", "2"):
        g = C.greedy_timed(out["log_probs" + spk].float(), blank)
        ids, n, spans = g.ids.cpu(), g.lengths.cpu(), g.spans.cpu()
        for b in range(ids.shape[0]):
            for j0, j1 in ((0, 3), (3, 5)):
                j1 = min(j1, int(n[b]))
                if j0 < j1:
                    cut[(spk, b, j0)] = (tuple(ids[b, j0:j1].tolist()), int(spans[b, j0, 0]), int(spans[b, j1 - 1, 1]))
    assert cut, "the tiny model's greedy transcripts are empty"
    bias = B.ContextBias.from_phrases([y for y, _, _ in cut.values()], vocab_size=t.tokenizer.vocab_size, blank=blank)
    names = ["".join(pieces[i] for i in p).replace("▁", " ") for p in bias.phrases]
    mods = [sm for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1) for sm in m.modules()]
    t.decoder1.train(); t.fusion_module.train()
    modes = [m.training for m in mods]
    (h1, h2), seen, trained = _recorded(t, lambda: t.spot(batch, bias, max_hits=8, min_score=0.0))
    assert len(seen) == 1 and not trained and [m.training for m in mods] == modes and any(modes)
    for spk, got in (("1", h1), ("2", h2)):
        lp = seen[0]["log_probs" + spk].float()
        assert torch.equal(lp, out["log_probs" + spk].float())
        want = S.hit_segments(S.keyword_spot(lp, bias, blank=blank, max_hits=8, min_score=0.0), names)
        assert got == want and len(got) == 3
        assert got == S.hit_segments(S.keyword_spot(lp.cpu(), bias.phrases, blank=blank, max_hits=8, min_score=0.0), names)
    for (spk, b, _), (y, first, end) in cut.items():
        name = names[bias.phrases.index(y)]
        rows = [h for h in (h1 if spk == "1" else h2)[b] if h["keyword"] == name]
        assert {"keyword": name, "start": first / 25.0, "end": end / 25.0, "score": 0.0, "per_frame": 0.0} in rows, (spk, b, y, rows)
    # strings go through the tokenizer; None reads the options
    text = pieces[5] + pieces[6]
    a = t.spot(batch, [text])
    assert a == t.spot(batch, B.ContextBias.from_phrases([text], t.tokenizer), max_hits=4, min_score=NEG)
    assert all(h["keyword"] == text and 0.0 <= h["start"] < h["end"] <= 1.0 and h["score"] <= 0.0 for u in a[0] + a[1] for h in u)
    assert all(1 <= len(u) <= 4 for u in a[0] + a[1])
    print(f"[trainer.spot] {len(cut)} keywords cut from greedy transcripts, all found at their spans with score 0.0")


def test_spot_long_is_keyword_spot_on_the_stitched_windows():
    """F = 55 in windows of 25 (5 discarded per side): three windows, two forward calls.  The result equals keyword_spot on longform.stitch
    of the recorded windows, so times count from the start of the recording; module modes are restored."""
    S = pkg("spot"); LF = pkg("longform"); B = pkg("bias")
    t = _trainer()
    F = 55
    rec = _recording(F, 11)
    plan = LF.plan_windows(F, 25, 5)
    assert plan.count == 3
    pieces = t.tokenizer.id_to_token
    bias = B.ContextBias.from_phrases([pieces[5], pieces[7] + pieces[8], pieces[9] + pieces[9]], t.tokenizer)
    names = [pieces[5], pieces[7] + pieces[8], pieces[9] + pieces[9]]
    res, seen, trained = _recorded(t, lambda: t.spot_long(rec, bias, max_hits=8))
    assert len(seen) == 2 and not trained
    windows = torch.stack([torch.cat([o["log_probs" + spk].float() for o in seen]) for spk in ("1", "2")])
    stitched = LF.stitch(windows, plan, t.long_policy)
    assert tuple(stitched.shape[:2]) == (2, F)
    want = S.hit_segments(S.keyword_spot(stitched, bias, blank=t.tokenizer.blank_id, max_hits=8), names)
    assert list(res) == want and all(len(u) > 0 for u in res)
    assert want == S.hit_segments(S.keyword_spot(stitched.cpu(), bias, blank=t.tokenizer.blank_id, max_hits=8), names)
    assert all(0.0 <= h["start"] < h["end"] <= F / 25.0 for u in res for h in u)
    assert res == t.spot_long({k: v[None].cuda() for k, v in rec.items()}, bias, max_hits=8)          # the [1, ...] forms, on the device
    print(f"[trainer.spot_long] F={F}: {[len(u) for u in res]} hits, latest end {max(h['end'] for u in res for h in u):.2f} s")


def test_spot_long_on_a_recording_of_one_window_is_spot():
    t = _trainer()
    rec = _recording(20, 3)
    batch = {k: v[None] for k, v in rec.items()}
    pieces = t.tokenizer.id_to_token
    kws = [pieces[5], pieces[6] + pieces[7]]
    want = t.spot(batch, kws, max_hits=8)
    got = t.spot_long(rec, kws, max_hits=8)
    assert len(want[0]) == 1 and (want[0][0], want[1][0]) == got and all(len(u) > 0 for u in got)
