"""GPU: CTC segmentation on the device (csrc/ctc_segment.hip, segmentation.ctc_segment) in both libraries: bit for bit against the package's
host path (the float32 law, which tests/test_segment_cpu.py ties to tests/segment_ref.py) on strided input with ragged, tight and infeasible
items, on the [T][B][V] view, with every combination of free ends, at every ownership width of the kernel (1, 4 and 16 states per thread)
and past both limits of forced_align; against forced_align on the device with fixed ends; infeasible items; all-tie inputs; the path's
structure from the outputs alone; determinism and output padding; and MultimodalTrainer.align_long."""
import numpy as np
import pytest
import torch

from conftest import pkg
from trainer_util import gpu_trainer
import align_ref as AR
import segment_ref as R

pytestmark = pytest.mark.gpu

PAD = 24                    # the device input is a [B, T, V] view of a [B, T, V + PAD] block whose padding holds NaN: strided, and never read
FIELDS = ("states", "spans", "token_scores", "score", "frame_scores", "utt_spans", "utt_means", "utt_scores")


@pytest.fixture(params=["fp32", "fp16"])
def library(request):
    """libavhip.so and libavhip_f16.so (the segmentation is float32 in both)."""
    P = pkg("precision")
    old = P.get_precision()
    P.set_precision(request.param)
    yield request.param
    P.set_precision(old)


def _strided(lp, time_major=False):
    """[B, T, V] numpy -> strided device view with NaN padding; ``time_major``: the [T, B, V] view of a [T, B, V + PAD] block."""
    x = torch.from_numpy(lp)
    if time_major:
        x = x.transpose(0, 1)
    block = torch.full(tuple(x.shape[:2]) + (lp.shape[2] + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    block[:, :, :lp.shape[2]] = x.cuda()
    view = block[:, :, :lp.shape[2]]
    assert view.stride(1) == lp.shape[2] + PAD and not view.is_contiguous()
    return view


def _assert_same_bits(got, want, what):
    for name, g, w in zip(FIELDS, got, want):
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bits = (lambda x: x.view(torch.int32)) if g.dtype == torch.float32 else (lambda x: x)
        if not torch.equal(bits(g), bits(w)):
            bad = torch.nonzero(bits(g) != bits(w))
            raise AssertionError((what, name, int(bad.shape[0]), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


_HOST = {}


def _host(key, make):
    """The inputs of a case and the host path's result, computed once for both libraries and left unchanged."""
    if key not in _HOST:
        lp, tg, il, tl, ut, kw = make()
        want = pkg("segmentation").ctc_segment(torch.from_numpy(lp), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl),
                                               utterances=torch.from_numpy(ut), **kw)
        _HOST[key] = (lp, tg, il, tl, ut, kw, want)
    return _HOST[key]


def _check_both_layouts(library, case):
    S = pkg("segmentation")
    lp, tg, il, tl, ut, kw, want = case
    t = lambda x: torch.from_numpy(x)                                         # noqa: E731
    got = S.ctc_segment(_strided(lp), t(tg).cuda(), t(il).cuda(), t(tl).cuda(), utterances=t(ut).cuda(), **kw)
    assert all(x.is_cuda for x in got)
    _assert_same_bits(got, want, f"{library} [B][T][V] {kw}")
    got_t = S.ctc_segment(_strided(lp, time_major=True), t(tg), t(il), t(tl), utterances=t(ut), batch_first=False, **kw)      # host tensors: copied
    _assert_same_bits(got_t, want, f"{library} [T][B][V] {kw}")
    return got


def _kw(blank, free, w):
    return dict(blank=blank, free_start=bool(free & 1), free_end=bool(free & 2), score_window=w)


MATRIX = [(37, 5, 12, b, f, 4) for b in (0, 3) for f in (0, 1, 2, 3)] + [(100, 800, 30, 0, 0, 30), (100, 800, 30, 3, 3, 30),
                                                                        (300, 800, 130, 3, 0, 30), (300, 800, 130, 0, 3, 7)]


@pytest.mark.parametrize("T,V,Lmax,blank,free,w", MATRIX)
def test_device_equals_the_host_law_bit_for_bit(library, T, V, Lmax, blank, free, w):
    """The items of segment_ref.matrix (full, 0 frames, 1 frame with 1 label, all labels equal, exactly tight, one frame short) with its
    utterance ranges (a gap, an empty range, a range past L_b).  Lmax 130: S = 261, the ownership crosses a wavefront."""
    case = _host((T, V, Lmax, blank, free, w), lambda: R.matrix(T, V, Lmax, blank)[:5] + (_kw(blank, free, w),))
    want = case[-1]
    assert np.isfinite(want.score.numpy()).tolist() == [True, True, True, True, True, False]
    assert int((want.utt_spans[..., 0] >= 0).sum()) >= 6
    _check_both_layouts(library, case)


def _long_case(T, V, L, lens, free, seed):
    def make():
        rng = np.random.default_rng(seed)
        B = len(lens)
        lp = np.stack([R.make_log_probs(seed + b, T, V, 0) for b in range(B)])
        tg = np.zeros((B, L), np.int64)
        for b in range(B):
            tg[b] = R.labels(rng, list(range(1, V)), L, 0 if V < 20 else L // 40)
        il = np.array([x[0] for x in lens], np.int64)
        tl = np.array([x[1] for x in lens], np.int64)
        q = L // 4
        ut = np.tile(np.array([[0, q], [q, 2 * q], [2 * q + 3, 3 * q], [3 * q, L], [5, 5], [L - 1, L + 1]], np.int32), (B, 1, 1))
        return lp, tg, il, tl, ut, _kw(0, free, 30)
    return make


@pytest.mark.parametrize("free", [0, 3])
def test_past_both_limits_of_forced_align(library, free):
    """T 4500 (a multiple of neither 16 nor 256), L 1500 (S = 3001: four states per thread), B 2 with the second item ragged: the path
    crosses many back-trace windows."""
    case = _host(("long", free), _long_case(4500, 40, 1500, [(4500, 1500), (3777, 1234)], free, 8100))
    want = case[-1]
    assert bool(torch.isfinite(want.score).all()) and int((want.states[1, 3777:] != -1).sum()) == 0
    assert int((want.utt_spans[0, :4, 0] >= 0).sum()) == 4 and want.utt_spans[1, 3].tolist() == [-1, -1]     # [3 q, L) ends past L_b = 1234
    _check_both_layouts(library, case)


def test_one_item_at_the_largest_transcript(library):
    """Lmax 8191 (S = 16383: sixteen states per thread of 1024), T 8400, V 8, labels with no equal neighbours (random labels at this shape
    have about 1150 repeats and are infeasible), both ends free."""
    S = pkg("segmentation")
    case = _host("largest", _long_case(8400, 8, 8191, [(8400, 8191)], 3, 9300))
    lp, tg, il, tl, ut, kw, want = case
    assert bool(torch.isfinite(want.score).all()) and int((want.spans[0, :, 0] >= 0).sum()) == 8191
    t = lambda x: torch.from_numpy(x)                                         # noqa: E731
    got = S.ctc_segment(_strided(lp), t(tg).cuda(), t(il).cuda(), t(tl).cuda(), utterances=t(ut).cuda(), **kw)
    _assert_same_bits(got, want, library)


def test_fixed_ends_equal_forced_align_on_the_device(library):
    S = pkg("segmentation"); A = pkg("align")
    for blank in (0, 3):
        lp, tg, il, tl, ut, _ = R.matrix(100, 800, 30, blank)
        x, tgd, ild, tld = _strided(lp), torch.from_numpy(tg).cuda(), torch.from_numpy(il).cuda(), torch.from_numpy(tl).cuda()
        got = S.ctc_segment(x, tgd, ild, tld, blank=blank)
        want = A.forced_align(x, tgd, ild, tld, blank=blank)
        for name, g, w in zip(FIELDS, got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.view(torch.int32), w.view(torch.int32)), (blank, name)


@pytest.mark.parametrize("free", [0, 3])
def test_infeasible_items(library, free):
    """test_align_gpu.test_infeasible_items' batch - a label >= V, a label equal to the blank, a -inf column every path must cross, a frame
    without any finite emission - with utterance ranges on every item: score -inf, states and every span -1, every score 0, no NaN."""
    S = pkg("segmentation")
    T, V, blank = 40, 12, 3
    lp = np.stack([AR.make_log_probs(300 + b, T, V, blank) for b in range(6)])
    lp[3, :, 7] = -np.inf                                                     # item 3 must emit 7
    lp[4, :, 9] = -np.inf                                                     # item 4 never emits 9: stays feasible
    lp[5, 10, :] = -np.inf                                                    # a frame without any finite emission
    tg = torch.tensor([[1, 2, 4, 5, 1, 1], [1, V, 2, 0, 0, 0], [1, blank, 2, 0, 0, 0], [1, 7, 2, 0, 0, 0], [1, 2, 2, 4, 0, 0], [5, 6, 0, 0, 0, 0]])
    tl = torch.tensor([6, 3, 3, 3, 4, 2])
    il = torch.tensor([T, T, T, T, 7, T])
    ut = torch.tensor([[[0, 2], [1, 3]]] * 6, dtype=torch.int32)
    kw = _kw(blank, free, 4)
    want = S.ctc_segment(torch.from_numpy(lp), tg, il, tl, utterances=ut, **kw)
    got = S.ctc_segment(_strided(lp), tg.cuda(), il.cuda(), tl.cuda(), utterances=ut.cuda(), **kw)
    _assert_same_bits(got, want, library)
    got = [x.cpu() for x in got]
    assert not any(torch.isnan(x).any() for x in got if x.dtype == torch.float32)
    # with free ends item 5 may end before (or start after) its dead frame
    assert torch.isfinite(got[3]).tolist() == [True, False, False, False, True, free != 0]
    for b in (1, 2, 3) + (() if free else (5,)):
        assert float(got[3][b]) == float("-inf") and all(bool((got[k][b] == -1).all()) for k in (0, 1, 5))
        assert all(bool((got[k][b] == 0).all()) for k in (2, 4, 6, 7))
    assert bool((got[5][0] >= 0).all()) and bool((got[5][4] >= 0).all())


def test_uniform_log_probs_on_the_device(library):
    """Every path ties: the device takes the one the tie rule dictates, as the host law does - with free ends too, where every emission is
    0.0 and the path is the shortest one from frame 0."""
    S = pkg("segmentation")
    T, V, L = 64, 30, 20
    lp = torch.full((2, T, V), float(np.log(np.float32(1.0 / V))), dtype=torch.float32)
    tg = torch.stack([torch.arange(1, L + 1), torch.tensor([1, 1, 2, 2, 3] * 4)])
    ut = torch.tensor([[[0, 10], [10, 20]]] * 2, dtype=torch.int32)
    for free in (0, 1, 2, 3):
        kw = _kw(0, free, 5)
        want = S.ctc_segment(lp, tg, utterances=ut, **kw)
        got = S.ctc_segment(lp.cuda(), tg.cuda(), utterances=ut.cuda(), **kw)
        _assert_same_bits(got, want, f"{library} free={free}")
    fixed = S.ctc_segment(lp, tg)
    assert fixed.states[0, :L].tolist() == list(range(1, 2 * L, 2)) and bool((fixed.states[0, L:] == 2 * L - 1).all())     # no blank at all
    assert want.score.tolist() == [0.0, 0.0] and want.states[0].tolist() == list(range(1, 2 * L, 2)) + [-1] * (T - L)


def test_structure_of_the_path_from_the_outputs_alone(library):
    """Both ends free at (100, 800, 30): the path is one run of frames, starts in state 0 or 1, ends in S-1 or S-2, moves by 0, 1 or 2 and
    skips only onto a differing label; spans tile the odd frames; frame scores are <= 0 on the path and 0 off it; token scores and the
    utterance means are sums of them; and the score is their sum to T_b 2^-23 relative (one float32 rounding per frame)."""
    S = pkg("segmentation")
    T, V, Lmax, blank = 100, 800, 30, 3
    lp, tg, il, tl, ut, items = R.matrix(T, V, Lmax, blank)
    got = S.ctc_segment(_strided(lp), torch.from_numpy(tg).cuda(), torch.from_numpy(il).cuda(), torch.from_numpy(tl).cuda(), blank=blank,
                        utterances=torch.from_numpy(ut).cuda(), free_start=True, free_end=True, score_window=4)
    states, spans, tok, score, fsc, usp, um, us = (x.cpu() for x in got)
    checked = 0
    for b, (Tb, lab) in enumerate(items):
        if not np.isfinite(float(score[b])) or Tb == 0:
            continue
        checked += 1
        Sn = 2 * len(lab) + 1
        ext = [blank if s % 2 == 0 else lab[s // 2] for s in range(Sn)]
        on = [t for t in range(T) if int(states[b, t]) >= 0]
        assert on == list(range(on[0], on[-1] + 1)) and on[-1] < Tb
        st = states[b, on[0]:on[-1] + 1].tolist()
        assert st[0] in (0, 1) and st[-1] in (Sn - 1, Sn - 2) and all(0 <= s < Sn for s in st)
        for a, c in zip(st, st[1:]):
            assert c - a in (0, 1, 2)
            assert c - a < 2 or ext[c] != ext[a], (b, a, c)
        odd = [t for t in on if int(states[b, t]) % 2 == 1]
        tiled = [t for j in range(len(lab)) for t in range(int(spans[b, j, 0]), int(spans[b, j, 1]))]
        assert tiled == odd and bool((spans[b, len(lab):] == -1).all()) and bool((tok[b, len(lab):] == 0).all())
        f = fsc[b].double()
        assert bool((fsc[b] <= 0).all()) and bool((fsc[b, :on[0]] == 0).all()) and bool((fsc[b, on[-1] + 1:] == 0).all())
        m = torch.from_numpy(lp[b]).max(dim=1).values
        want_f = torch.from_numpy(lp[b][on, [ext[int(states[b, t])] for t in on]]) - m[on[0]:on[-1] + 1]
        assert torch.equal(fsc[b, on[0]:on[-1] + 1], want_f)
        total = float(f.sum())
        assert abs(float(score[b]) - total) <= Tb * 2.0 ** -23 * abs(total)
        for j in range(len(lab)):
            part = float(f[int(spans[b, j, 0]):int(spans[b, j, 1])].sum())
            assert abs(float(tok[b, j]) - part) <= Tb * 2.0 ** -23 * abs(part)
        for u in range(usp.shape[1]):
            a, z = usp[b, u].tolist()
            if a >= 0:
                b0, e0 = ut[b, u].tolist()
                assert (a, z) == (int(spans[b, b0, 0]), int(spans[b, e0 - 1, 1]))
                mean = float(f[a:z].sum()) / (z - a)
                assert abs(float(um[b, u]) - mean) <= (z - a + 1) * 2.0 ** -23 * abs(mean)
                low = min(float(f[k:min(k + 4, z)].sum()) / (min(k + 4, z) - k) for k in range(a, z, 4))
                assert abs(float(us[b, u]) - low) <= 6 * 2.0 ** -23 * abs(low)
    assert checked == 4


def _raw(lp, tg, il, tl, ut, blank, free, w):
    L = pkg("_lib"); ops = pkg("ops")
    B, T, V = lp.shape
    Lmax, U = tg.shape[1], ut.shape[1]
    need = L.ll(0)
    L.check(L.lib().av_ctc_segment_workspace_bytes(B, T, 2 * Lmax + 1, L.C.byref(need)))
    ws = torch.empty(((need.value + 3) // 4,), dtype=torch.int32, device="cuda")
    ints = lambda *shape: torch.full(shape, 12345, dtype=torch.int32, device="cuda")                     # noqa: E731
    nans = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")            # noqa: E731
    out = (ints(B, T), ints(B, Lmax, 2), nans(B, Lmax), nans(B), nans(B, T), ints(B, U, 2), nans(B, U), nans(B, U))
    L.check(L.lib().av_ctc_segment(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(tg), tg.stride(0), ops.ptr(il), ops.ptr(tl), ops.ptr(ut),
                                   B, T, V, 2 * Lmax + 1, U, blank, free, w, *(ops.ptr(x) for x in out), ops.ptr(ws), need.value,
                                   ops.stream()), "av_ctc_segment")
    torch.cuda.synchronize()
    return tuple(x.cpu() for x in out)


@pytest.mark.parametrize("T,V,Lmax,blank,free,w", [(100, 800, 30, 0, 0, 30), (300, 800, 130, 0, 3, 7)])
def test_runs_are_bit_identical_and_outputs_are_padded(library, T, V, Lmax, blank, free, w):
    lp, tg, il, tl, ut, kw, want = _host((T, V, Lmax, blank, free, w), lambda: R.matrix(T, V, Lmax, blank)[:5] + (_kw(blank, free, w),))
    args = (_strided(lp), torch.from_numpy(tg).cuda(), torch.from_numpy(il).cuda(), torch.from_numpy(tl).cuda(), torch.from_numpy(ut).cuda())
    a, b = _raw(*args, blank, free, w), _raw(*args, blank, free, w)
    for p, q in zip(a, b):
        assert p.dtype == q.dtype and torch.equal(p.view(torch.int32), q.view(torch.int32))
    _assert_same_bits(a, want, library)
    assert not any((x == 12345).any() for x in a if x.dtype == torch.int32) and not any(torch.isnan(x).any() for x in a if x.dtype == torch.float32)
    states, spans, tok, score, fsc, usp, um, us = a
    for i in range(lp.shape[0]):
        ok = bool(torch.isfinite(score[i]))
        on = states[i] >= 0
        assert bool((fsc[i][~on] == 0).all()) and (ok or not bool(on.any())) and not bool(on[int(il[i]):].any())
        n = int(tl[i]) if ok else 0
        assert bool((spans[i, n:] == -1).all()) and bool((tok[i, n:] == 0).all()) and bool((spans[i, :n] >= 0).all())
        none = usp[i, :, 0] < 0
        assert bool((usp[i][none] == -1).all()) and bool((um[i][none] == 0).all()) and bool((us[i][none] == 0).all())
        assert ok or (float(score[i]) == float("-inf") and bool(none.all()))


def test_a_clip_forced_align_refuses_is_aligned(library):
    S = pkg("segmentation"); A = pkg("align")
    T, V, L = 4097, 16, 50
    lp = torch.from_numpy(R.make_log_probs(4242, T, V, 0))[None]
    tg = torch.from_numpy(np.array([R.labels(np.random.default_rng(5), list(range(1, V)), L, 3)]))
    with pytest.raises(ValueError, match="4096"):
        A.forced_align(lp.cuda(), tg.cuda())
    want = S.ctc_segment(lp, tg)
    got = S.ctc_segment(lp.cuda(), tg.cuda())
    _assert_same_bits(got, want, library)
    assert bool(torch.isfinite(want.score[0])) and bool((want.states[0] >= 0).all()) and bool((want.spans[0] >= 0).all())
    # ... and a workspace above the caller's limit is refused by name, before anything runs
    with pytest.raises(ValueError, match=r"T = 4097 frames against L = 50 labels"):
        S.ctc_segment(lp.cuda(), tg.cuda(), max_workspace_bytes=1000)


# ---- the trainer ----
def _recording(frames, seed):
    """Synthetic clips of one second, concatenated and cut to ``frames`` lip frames."""
    synth = pkg("dataset.synthetic")
    clips = [synth.make_batch(1, 1.0, seed=seed + i) for i in range(-(-frames // 25))]
    return {"audio": torch.cat([c["audio"][0] for c in clips])[:640 * frames],
            "lip1": torch.cat([c["lip1"][0] for c in clips])[:frames], "lip2": torch.cat([c["lip2"][0] for c in clips])[:frames]}


def test_trainer_align_long(tmp_path):
    """F = 260 in windows of 100 (12 discarded per side): align_long equals ctc_segment + word_segments + utterance_segments on the output
    of its one _stitched_windows call; times lie inside the recording; module modes are restored; evaluate() is untouched; a string is a
    one-element list."""
    from test_dataset_gpu import _Tok, _make_corpus
    ds = pkg("dataset.multi_speaker_dataset"); cf = pkg("dataset.collate_fn").collate_fn; init = pkg("utils.init")
    S = pkg("segmentation"); A = pkg("align")
    _, sents = _make_corpus(tmp_path)
    loader = torch.utils.data.DataLoader(ds.FixedSentencePairDataset([(sents[0], sents[2]), (sents[1], sents[3])], _Tok()), batch_size=2,
                                         shuffle=False, collate_fn=cf, num_workers=0)
    t = gpu_trainer(init.W2V2_TINY, "fp32", segment_window=10)
    before = t.evaluate(loader), t.last_decoded
    F, rate = 260, 25.0
    rec = _recording(F, 31)
    pc = t.tokenizer.id_to_token
    word = lambda *ids: "".join(pc[i] for i in ids)                           # noqa: E731
    tr1 = [word(5, 6, 7) + " " + word(8, 9), word(10, 11), word(12, 12, 13) + " " + word(14)]
    tr2 = [word(20, 21), word(22, 23, 24) + " " + word(25, 26), word(27)]
    mods = [sm for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1) for sm in m.modules()]
    t.decoder1.train(); t.fusion_module.train()
    modes = [m.training for m in mods]
    assert any(modes) and not all(modes)
    seen, inner = [], t._stitched_windows

    def recording(*a, **k):
        seen.append(inner(*a, **k))
        return seen[-1]
    t._stitched_windows = recording
    try:
        res = t.align_long(rec, tr1, tr2, frame_rate=rate, free_start=True, free_end=True)
        fixed = t.align_long(rec, tr1, tr2, frame_rate=rate)
    finally:
        t._stitched_windows = inner
    assert len(seen) == 2 and tuple(seen[0].shape[:2]) == (2, F) and [m.training for m in mods] == modes
    blank, space = t.tokenizer.blank_id, t.tokenizer.token_to_id["▁"]
    ids, ranges = [], []
    for utts in (tr1, tr2):
        row, rng = [], []
        for k, text in enumerate(utts):
            row += [space] if k else []
            rng.append((len(row), len(row) + len(text)))
            row += t.tokenizer.encode(text)
        ids.append(row); ranges.append(rng)
    Lmax = max(len(r) for r in ids)
    tg = torch.tensor([r + [blank] * (Lmax - len(r)) for r in ids])
    for out, stitched, free in ((res, seen[0], True), (fixed, seen[1], False)):
        seg = S.ctc_segment(stitched, tg, None, torch.tensor([len(r) for r in ids]), blank=blank, utterances=torch.tensor(ranges, dtype=torch.int32),
                            free_start=free, free_end=free, score_window=10)
        utts = S.utterance_segments(seg, [tr1, tr2], rate)
        for i in range(2):
            assert bool(torch.isfinite(seg.score[i]))
            want = {"score": float(seg.score[i]), "words": A.word_segments(t.tokenizer, ids[i], seg.spans[i], seg.token_scores[i], rate),
                    "utterances": utts[i]}
            assert out[i] == want, (free, i, out[i], want)
            assert [w["word"] for w in out[i]["words"]] == " ".join((tr1, tr2)[i]).split()
            assert [u["text"] for u in out[i]["utterances"]] == (tr1, tr2)[i]
            for x in out[i]["words"] + out[i]["utterances"]:
                assert 0.0 <= x["start"] < x["end"] <= F / rate
            assert not free or all(u["score"] <= u["mean"] + 1e-6 and u["mean"] <= 0.0 for u in out[i]["utterances"])
    one = t.align_long(rec, "".join(pc[i] for i in (5, 6, 7)), [word(20, 21)])
    assert one == t.align_long(rec, [word(5, 6, 7)], [word(20, 21)]) and len(one[0]["utterances"]) == 1
    cannot = t.align_long(_recording(30, 7), word(*range(5, 45)), word(20))    # 40 labels in 30 frames
    assert cannot[0] == {"score": float("-inf"), "words": [], "utterances": []} and cannot[1]["words"]
    print(f"[trainer.align_long] F={F}: free ends {res[0]['score']:.2f} / {res[1]['score']:.2f}, fixed {fixed[0]['score']:.2f} / {fixed[1]['score']:.2f}; "
          f"{res[0]['utterances']}")
    t.decoder1.eval(); t.fusion_module.eval()
    assert (t.evaluate(loader), t.last_decoded) == before
