"""GPU: CTC forced alignment on the device (csrc/ctc_align.hip, align.forced_align) in both libraries: bit for bit against the package's
host path (the float32 law, which tests/test_align_cpu.py ties to tests/align_ref.py) on strided input with ragged, tight and infeasible
items, on the [T][B][V] view, on all-tie inputs; infeasible items against ops.ctc_loss; the path's structure from the outputs alone;
determinism and output padding; and MultimodalTrainer.align."""
import numpy as np
import pytest
import torch

from conftest import pkg
import align_ref as R

pytestmark = pytest.mark.gpu

PAD = 24                    # the device input is a [B, T, V] view of a [B, T, V + PAD] block whose padding holds NaN: strided, and never read


@pytest.fixture(params=["fp32", "fp16"])
def library(request):
    """libavhip.so and libavhip_f16.so (the alignment is float32 in both)."""
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


def _labels(rng, pool, L, reps):
    """L labels from ``pool`` with exactly ``reps`` equal neighbours."""
    same = set(rng.choice(L - 1, size=reps, replace=False).tolist()) if reps else set()
    out = [int(pool[int(rng.integers(len(pool)))])]
    for i in range(1, L):
        out.append(out[-1] if (i - 1) in same else int(rng.choice([c for c in pool if c != out[-1]])))
    assert R.repeats(out) == reps
    return out


_CASES = {}


def _case(T, V, Lmax, blank, variant):
    """Inputs of one shape and the host path's result, computed once for both libraries.  Items (T_b, labels):
    variant "a" (B = 6): T with Lmax labels | 0 frames, no labels | 1 frame, 1 label | T-1 with all labels equal |
                         T/2 exactly tight (T_b = L_b + repeats: a single path) | T/2 one frame short (infeasible)
    variant "b" (B = 3): T with Lmax labels | T/2 exactly tight | T-1 with all labels equal, L_b = Lmax
    variant "c" (B = 3): 0 frames with Lmax labels (infeasible) | 1 frame, 1 label | T/2 one frame short (infeasible)"""
    key = (T, V, Lmax, blank, variant)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(T * 1009 + V * 7 + blank)
    pool = [c for c in range(V) if c != blank][:5]
    h = T // 2
    full = (T, _labels(rng, pool, Lmax, min(Lmax // 5, T - Lmax)))
    tight_L = min(Lmax, (h + 1) // 2 + h // 6)                               # L_b + repeats = T/2 needs (T/2 + 1) / 2 <= L_b
    assert h - tight_L + 1 <= tight_L - 1
    tight = (h, _labels(rng, pool, tight_L, h - tight_L))
    short = (h, _labels(rng, pool, tight_L, h - tight_L + 1))
    one = (1, [pool[1]])
    items = {"a": [full, (0, []), one, (T - 1, [pool[2]] * min(Lmax, T // 2)), tight, short],
             "b": [full, tight, (T - 1, [pool[2]] * Lmax)],
             "c": [(0, _labels(rng, pool, Lmax, 0)), one, short]}[variant]
    B = len(items)
    lp = np.stack([R.make_log_probs(61000 + T + 17 * b + blank, T, V, blank) for b in range(B)])
    tg = torch.full((B, Lmax), blank, dtype=torch.long)                       # padding = the blank: never read as a label
    for b, (_, lab) in enumerate(items):
        tg[b, :len(lab)] = torch.tensor(lab, dtype=torch.long)
    il = torch.tensor([x[0] for x in items])
    tl = torch.tensor([len(x[1]) for x in items])
    want = pkg("align").forced_align(torch.from_numpy(lp), tg, il, tl, blank=blank)
    _CASES[key] = (lp, tg, il, tl, items, want)
    return _CASES[key]


def _assert_same_bits(got, want, what):
    for name, g, w in zip(("states", "spans", "token_scores", "score"), got, want):
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bits = (lambda x: x.view(torch.int32)) if g.dtype == torch.float32 else (lambda x: x)
        assert torch.equal(bits(g), bits(w)), (what, name, g, w)


SHAPES = [(37, 5, 12, 0, "a"), (37, 5, 12, 3, "a"), (100, 800, 30, 0, "a"), (100, 800, 30, 3, "a"),
          (300, 800, 130, 3, "b"), (300, 800, 130, 0, "c")]          # Lmax 130: S = 261 > 256, the state loop takes a second trip


@pytest.mark.parametrize("T,V,Lmax,blank,variant", SHAPES)
def test_device_equals_the_host_law_bit_for_bit(library, T, V, Lmax, blank, variant):
    A = pkg("align")
    lp, tg, il, tl, items, want = _case(T, V, Lmax, blank, variant)
    # the host result is what the case was built for: tight items have a single path, short ones none
    for b, (Tb, lab) in enumerate(items):
        need = len(lab) + R.repeats(lab)
        assert bool(torch.isfinite(want.score[b])) == (Tb >= need and (Tb > 0 or not lab)), (b, Tb, need)
        if Tb == need and Tb > 0:
            assert R.collapse(R.emitted(want.states[b, :Tb].tolist(), lab, blank), blank) == lab
            assert int((want.states[b, :Tb] % 2 == 1).sum()) == len(lab) and want.spans[b, :len(lab), 0].tolist() == \
                [t for t in range(Tb) if int(want.states[b, t]) % 2 == 1]
    if T == 37:                                                               # and it is the float32 law of tests/align_ref.py
        for b, (Tb, lab) in enumerate(items):
            st, sp, tk, sc = R.law(lp[b, :Tb], lab, blank)
            assert want.states[b, :Tb].tolist() == (st or [-1] * Tb) and np.float32(sc).view(np.int32) == want.score[b].numpy().view(np.int32)
    got = A.forced_align(_strided(lp), tg.cuda(), il.cuda(), tl.cuda(), blank=blank)
    assert all(x.is_cuda for x in got)
    _assert_same_bits(got, want, f"{library} [B][T][V]")
    got_t = A.forced_align(_strided(lp, time_major=True), tg, il, tl, blank=blank, batch_first=False)      # host targets / lengths: copied
    _assert_same_bits(got_t, want, f"{library} [T][B][V]")
    ids = A.token_path(got, tg.cuda(), blank)
    assert ids.is_cuda and ids.dtype == torch.int64
    for b, (Tb, lab) in enumerate(items):
        row = ids[b].tolist()
        if bool(torch.isfinite(want.score[b])):
            assert R.collapse(row[:Tb], blank) == lab and all(i == -1 for i in row[Tb:])
        else:
            assert all(i == -1 for i in row)


def test_infeasible_items(library):
    """A label >= V, a label equal to the blank, a -inf column every path must cross: score -inf, states and spans -1, token scores 0, no
    NaN.  For targets without the blank, feasible <=> the CTC loss of the same inputs is finite."""
    A = pkg("align"); ops = pkg("ops")
    T, V, Lmax, blank = 40, 12, 6, 3
    lp = np.stack([R.make_log_probs(300 + b, T, V, blank) for b in range(6)])
    lp[3, :, 7] = -np.inf                                                     # item 3 must emit 7
    lp[4, :, 9] = -np.inf                                                     # item 4 never emits 9: stays feasible
    lp[5, 10, :] = -np.inf                                                    # a frame without any finite emission
    tg = torch.tensor([[1, 2, 4, 5, 1, 1], [1, V, 2, 0, 0, 0], [1, blank, 2, 0, 0, 0], [1, 7, 2, 0, 0, 0], [1, 2, 2, 4, 0, 0], [5, 6, 0, 0, 0, 0]])
    tl = torch.tensor([6, 3, 3, 3, 4, 2])
    il = torch.tensor([T, T, T, T, 7, T])
    want = A.forced_align(torch.from_numpy(lp), tg, il, tl, blank=blank)
    x = _strided(lp)
    got = A.forced_align(x, tg.cuda(), il.cuda(), tl.cuda(), blank=blank)
    _assert_same_bits(got, want, library)
    states, spans, tok, score = (t.cpu() for t in got)
    assert not torch.isnan(score).any() and not torch.isnan(tok).any()
    assert torch.isfinite(score).tolist() == [True, False, False, False, True, False]
    for b in (1, 2, 3, 5):
        assert float(score[b]) == float("-inf") and bool((states[b] == -1).all()) and bool((spans[b] == -1).all()) and bool((tok[b] == 0).all())
    # the loss sees the same lattice for targets without the blank (it clamps nothing differently; a label >= V is infeasible there too)
    keep = [0, 1, 3, 4, 5]
    nll = ops.ctc_loss(x[keep], tg[keep].cuda(), il[keep].cuda(), tl[keep].cuda(), blank=blank, reduction="none", zero_infinity=False,
                       batch_first=True).cpu()
    assert torch.isfinite(nll).tolist() == torch.isfinite(score[keep]).tolist()
    # ... and on the ragged / tight / short items of the matrix
    lp2, tg2, il2, tl2, _, want2 = _case(100, 800, 30, 3, "a")
    nll2 = ops.ctc_loss(_strided(lp2), tg2.cuda(), il2.cuda(), tl2.cuda(), blank=3, reduction="none", zero_infinity=False, batch_first=True).cpu()
    assert torch.isfinite(nll2).tolist() == torch.isfinite(want2.score).tolist()


def test_uniform_log_probs_on_the_device(library):
    """Every path ties: the device takes the one the tie rule dictates, as the host law does."""
    A = pkg("align")
    T, V, L = 64, 30, 20
    lp = torch.full((2, T, V), float(np.log(np.float32(1.0 / V))), dtype=torch.float32)
    tg = torch.stack([torch.arange(1, L + 1), torch.tensor([1, 1, 2, 2, 3] * 4)])
    want = A.forced_align(lp, tg, blank=0)
    got = A.forced_align(lp.cuda(), tg.cuda(), blank=0)
    _assert_same_bits(got, want, library)
    assert want.states[0, :L].tolist() == list(range(1, 2 * L, 2)) and bool((want.states[0, L:] == 2 * L - 1).all())     # no blank at all


def test_structure_of_the_path_from_the_outputs_alone(library):
    A = pkg("align")
    T, V, Lmax, blank = 100, 800, 30, 3
    lp, tg, il, tl, items, _ = _case(T, V, Lmax, blank, "a")
    got = A.forced_align(_strided(lp), tg.cuda(), il.cuda(), tl.cuda(), blank=blank)
    ids = A.token_path(got, tg.cuda(), blank).cpu()
    states, spans, tok, score = (t.cpu() for t in got)
    checked = 0
    for b, (Tb, lab) in enumerate(items):
        if not np.isfinite(float(score[b])) or Tb == 0:
            continue
        checked += 1
        S = 2 * len(lab) + 1
        ext = [blank if s % 2 == 0 else lab[s // 2] for s in range(S)]
        st = states[b, :Tb].tolist()
        assert st[0] in (0, 1) and st[-1] in (S - 1, S - 2) and all(0 <= s < S for s in st)
        for a, c in zip(st, st[1:]):
            assert c - a in (0, 1, 2)
            assert c - a < 2 or ext[c] != ext[a], (b, a, c)                   # a skip only onto a label that differs from the one two back
        odd = [t for t in range(Tb) if st[t] % 2 == 1]
        tiled = [t for j in range(len(lab)) for t in range(int(spans[b, j, 0]), int(spans[b, j, 1]))]
        assert tiled == odd and all(int(spans[b, j, 0]) < int(spans[b, j, 1]) for j in range(len(lab)))
        assert all(st[t] == 2 * j + 1 for j in range(len(lab)) for t in range(int(spans[b, j, 0]), int(spans[b, j, 1])))
        assert bool((spans[b, len(lab):] == -1).all()) and bool((tok[b, len(lab):] == 0).all())
        assert R.collapse(ids[b, :Tb].tolist(), blank) == lab
        # the score is the sum of the path's emissions: token scores plus the blank frames, to float32 rounding of T terms
        total = R.path_score64(lp[b], st, lab, blank)
        assert abs(float(score[b]) - total) <= Tb * 2.0 ** -23 * abs(total)
    assert checked == 4


def _raw(lp, tg, il, tl, blank):
    L = pkg("_lib"); ops = pkg("ops")
    B, T, V = lp.shape
    Lmax = tg.shape[1]
    need = L.ll(0)
    L.check(L.lib().av_ctc_align_workspace_bytes(B, T, 2 * Lmax + 1, L.C.byref(need)))
    ws = torch.empty(((need.value + 3) // 4,), dtype=torch.int32, device="cuda")
    states = torch.full((B, T), 12345, dtype=torch.int32, device="cuda")
    spans = torch.full((B, Lmax, 2), 12345, dtype=torch.int32, device="cuda")
    tok = torch.full((B, Lmax), float("nan"), dtype=torch.float32, device="cuda")
    score = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    L.check(L.lib().av_ctc_align(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(tg), tg.stride(0), ops.ptr(il), ops.ptr(tl), B, T, V,
                                 2 * Lmax + 1, blank, ops.ptr(states), ops.ptr(spans), ops.ptr(tok), ops.ptr(score), ops.ptr(ws), need.value,
                                 ops.stream()), "av_ctc_align")
    torch.cuda.synchronize()
    return states.cpu(), spans.cpu(), tok.cpu(), score.cpu()


@pytest.mark.parametrize("T,V,Lmax,blank,variant", [(100, 800, 30, 0, "a"), (300, 800, 130, 0, "c")])
def test_runs_are_bit_identical_and_outputs_are_padded(library, T, V, Lmax, blank, variant):
    lp, tg, il, tl, items, want = _case(T, V, Lmax, blank, variant)
    x, tgd, ild, tld = _strided(lp), tg.cuda(), il.cuda(), tl.cuda()
    a, b = _raw(x, tgd, ild, tld, blank), _raw(x, tgd, ild, tld, blank)
    for p, q in zip(a, b):
        assert p.dtype == q.dtype and torch.equal(p.view(torch.int32), q.view(torch.int32))
    _assert_same_bits(a, want, library)
    states, spans, tok, score = a
    assert not (states == 12345).any() and not (spans == 12345).any() and not torch.isnan(tok).any() and not torch.isnan(score).any()
    for i, (Tb, lab) in enumerate(items):
        ok = bool(torch.isfinite(score[i]))
        assert bool((states[i, Tb if ok else 0:] == -1).all()) and bool((states[i, :Tb if ok else 0] >= 0).all())
        n = len(lab) if ok else 0
        assert bool((spans[i, n:] == -1).all()) and bool((tok[i, n:] == 0).all()) and bool((spans[i, :n] >= 0).all())
        assert ok or float(score[i]) == float("-inf")


def test_trainer_align(tmp_path):
    """align() returns word_segments(forced_align(...)) of the log-probs of its one forward_losses call, restores every module's mode and
    leaves evaluate() as it was."""
    from test_dataset_gpu import _Tok, _make_corpus
    from test_step_gpu import build as build_trainer
    ds = pkg("dataset.multi_speaker_dataset"); cf = pkg("dataset.collate_fn").collate_fn; init = pkg("utils.init"); A = pkg("align")
    _, sents = _make_corpus(tmp_path)
    pairs = [(sents[0], sents[2]), (sents[1], sents[3])]
    loader = torch.utils.data.DataLoader(ds.FixedSentencePairDataset(pairs, _Tok()), batch_size=2, shuffle=False, collate_fn=cf, num_workers=0)
    batch = next(iter(loader))
    t = build_trainer(init.W2V2_TINY, "fp32")
    before = t.evaluate(loader), t.last_decoded
    mods = [sm for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1) for sm in m.modules()]
    t.decoder1.train(); t.fusion_module.train()
    modes = [m.training for m in mods]
    assert any(modes) and not all(modes)
    seen = []
    inner = t.forward_losses

    def recording(b):
        assert not any(m.training for m in mods)                              # eval mode, as in evaluate()
        out = inner(b)
        seen.append(out)
        return out
    t.forward_losses = recording
    lam = t.lambda_
    seg1, seg2 = t.align(batch, frame_rate=25.0)
    t.forward_losses = inner
    assert len(seen) == 1 and [m.training for m in mods] == modes and t.lambda_ == lam
    blank = t.tokenizer.blank_id
    feasible = 0
    for spk, segs in (("1", seg1), ("2", seg2)):
        txt, tl = batch["text" + spk], batch["text" + spk + "_lengths"]
        al = A.forced_align(seen[0]["log_probs" + spk], txt, seen[0]["input_lengths" + spk], tl, blank=blank)
        want = [A.word_segments(t.tokenizer, txt[i, :int(tl[i])], al.spans[i], al.token_scores[i], 25.0) for i in range(txt.shape[0])]
        assert segs == want and len(segs) == 2
        for i, w in enumerate(segs):
            assert bool(w) == bool(torch.isfinite(al.score[i])), (spk, i)
            feasible += bool(w)
            for x in w:
                assert 0.0 <= x["start"] < x["end"] <= int(seen[0]["input_lengths" + spk][i]) / 25.0 and x["score"] <= 0.0 and x["word"]
    print(f"[trainer.align] {feasible} of 4 transcripts aligned: {seg1} {seg2}")
    assert t.align(batch, frame_rate=50.0)[0] == [[dict(x, start=x["start"] / 2, end=x["end"] / 2) for x in w] for w in seg1]
    t.decoder1.eval(); t.fusion_module.eval()
    assert (t.evaluate(loader), t.last_decoded) == before
