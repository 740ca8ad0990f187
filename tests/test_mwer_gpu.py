"""GPU: the n-best form of the CTC loss (av_ctc_nbest_fwd / _bwd, ops.ctc_nbest_nll), beam_search.nbest_on_device, mwer.mwer_loss and the
trainer's MWER term.

  nll        bit for bit ops.ctc_loss(reduction="none", zero_infinity=False) of the same item (the same lattice kernel), +inf at out items
  gradient   sum c[b, n] nll[b, n] with weights of both signs against float64 torch (tests/mwer_ref.py: ctc_loss on log-probs expanded N
             times); gate = the project's own: ours <= 4 x e_ref, e_ref = the max-abs gradient error of torch's float32 CPU ctc_loss on the
             same expanded inputs against float64; exact zeros past T_b and for utterances whose items are all out
  mwer_loss  posterior, errors, loss and gradient against mwer_ref fed the hypotheses the device call found
  trainer    weight 0 = today's step; weight 0.5 adds exactly 0.5 (mwer1 + mwer2) / 2 and the two gradients meet at the log-probs"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mwer_ref
from conftest import pkg

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------------------------------------------
# case sets: log_probs [B, T, V], ids [B, N, Lh] (padding = the valid id 1, which must never be read), lens [B, N], T_b [B], max_len
# ---------------------------------------------------------------------------------------------------------------------------------
def _block(rows, Lh):
    """rows[b][n] = (id list, length or None for len(list)) -> ids int32 [B, N, Lh], lens int64 [B, N]."""
    B, N = len(rows), len(rows[0])
    ids = torch.ones((B, N, Lh), dtype=torch.int32)
    lens = torch.zeros((B, N), dtype=torch.long)
    for b, r in enumerate(rows):
        for n, (lab, ln) in enumerate(r):
            ids[b, n, :len(lab)] = torch.tensor(lab, dtype=torch.int32)
            lens[b, n] = len(lab) if ln is None else ln
    return ids, lens


def set_edges(V):
    """B = 4, N = 5, T = 17 (neither a multiple of the 16-frame chunk nor of the rows per workgroup), T_b = 17, 14, 1, 0, Lh = 10,
    max_len = 8.  Lengths 0, -1 and > max_len; [2 x 7, 1] needs 8 + 6 = 14 frames = T_b (just feasible), [2 x 8] needs 15 (infeasible by a
    repeat); ids shared between hypotheses and repeated within one; an id >= V and an id < 0."""
    g = torch.Generator().manual_seed(100 + V)
    lp = F.log_softmax(torch.randn(4, 17, V, generator=g) * 1.5, -1)
    rows = [
        [([1, 2, 3], None), ([1, 2, 3, 3], None), ([], None), ([4, 4], -1), ([1, 2, 3, 4, 5, 6, 1, 2, 3], None)],
        [([2] * 7 + [1], None), ([2] * 8, None), ([1, V + 3, 2], None), ([4, 5, 6, 1], None), ([4, 5, 6], None)],
        [([3], None), ([], None), ([3, 4], None), ([3], -1), ([5], None)],
        [([], None), ([1], None), ([2], -7), ([1, 2, 3, 4, 5, 6, 1, 2, 3, 4], None), ([-1], None)],
    ]
    ids, lens = _block(rows, 10)
    return dict(lp=lp, ids=ids, lens=lens, il=torch.tensor([17, 14, 1, 0]), max_len=8, blank=0,
                out=torch.tensor([[0, 0, 0, 1, 1], [0, 1, 1, 0, 0], [0, 0, 1, 1, 0], [0, 1, 1, 1, 1]], dtype=torch.bool))


def set_n1():
    """N = 1 (the existing entry point's shape), B = 3; utterance 1's only hypothesis is absent: all out with T_b > 0."""
    g = torch.Generator().manual_seed(201)
    lp = F.log_softmax(torch.randn(3, 17, 8, generator=g) * 1.5, -1)
    ids, lens = _block([[([5, 5, 6], None)], [([1, 2], -1)], [([7, 1, 7], None)]], 4)
    return dict(lp=lp, ids=ids, lens=lens, il=torch.tensor([17, 12, 9]), max_len=None, blank=3,
                out=torch.tensor([[0], [1], [0]], dtype=torch.bool))


def set_long():
    """B = 1, N = 2, T = 300, Lh = 140: S = 281 > 256 states, so the lattice's states loop over the threads."""
    g = torch.Generator().manual_seed(202)
    lp = F.log_softmax(torch.randn(1, 300, 8, generator=g) * 1.5, -1)
    ids = torch.randint(1, 8, (1, 2, 140), generator=g).to(torch.int32)
    return dict(lp=lp, ids=ids, lens=torch.tensor([[140, 121]]), il=torch.tensor([300]), max_len=None, blank=0,
                out=torch.zeros((1, 2), dtype=torch.bool))


SETS = {"edges7": lambda: set_edges(7), "edges8": lambda: set_edges(8), "n1": set_n1, "long": set_long}
CASES = [("edges7", "btv"), ("edges8", "btv"), ("edges8", "tbv_view"), ("n1", "btv"), ("long", "btv"), ("long", "tbv_view")]


def _ours(c, layout="btv", upstream=None):
    """-> (nll [B, N], grad [B, T, V] or None) of ops.ctc_nbest_nll; ``upstream`` [B, N] = the gradient handed to nll.backward."""
    ops = pkg("ops")
    x = c["lp"].detach().cuda().clone().requires_grad_(upstream is not None)
    arg, bf = (x, True) if layout == "btv" else (x.transpose(0, 1), False)     # the [T, B, V] VIEW of [B, T, V] storage
    nll = ops.ctc_nbest_nll(arg, c["ids"].cuda(), c["lens"].cuda(), c["il"].cuda(), blank=c["blank"], batch_first=bf, max_len=c["max_len"])
    if upstream is None:
        return nll.detach(), None
    nll.backward(upstream.cuda())
    return nll.detach(), x.grad.detach()


@pytest.mark.parametrize("name,layout", CASES)
def test_nll_is_the_existing_law_bit_for_bit(name, layout):
    ops = pkg("ops")
    c = SETS[name]()
    nll, _ = _ours(c, layout)
    B, N = c["lens"].shape
    assert nll.shape == (B, N) and nll.dtype == torch.float32
    Lh = c["ids"].shape[2]
    max_len = Lh if c["max_len"] is None else c["max_len"]
    lens, ids, V = c["lens"], c["ids"].long(), c["lp"].shape[2]
    inside = torch.arange(Lh)[None, None, :] < lens[..., None]
    in_range = (lens >= 0) & (lens <= max_len) & ~(inside & ((ids < 0) | (ids >= V))).any(-1)
    # every present, in-range hypothesis as an item of the existing entry point (its own targets row, its utterance's log-probs)
    b_of = torch.arange(B).repeat_interleave(N)
    keep = in_range.reshape(-1)
    lp_items = c["lp"][b_of[keep]].cuda()
    tg = ids.reshape(B * N, Lh)[keep].clamp(0, V - 1).cuda()
    want = ops.ctc_loss(lp_items, tg, c["il"].repeat_interleave(N)[keep].cuda(), lens.reshape(-1)[keep].cuda(), blank=c["blank"],
                        reduction="none", zero_infinity=False, batch_first=True)
    got = nll.reshape(-1)[keep.cuda()]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (got, want)
    assert bool((nll[~in_range.cuda()] == INF).all())
    assert torch.equal(torch.isinf(nll).cpu(), c["out"]), nll
    assert bool((nll[~c["out"].cuda()] >= 0).all())


def _weights(c, seed=5, poison=False):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(c["lens"].shape, generator=g) * 2 - 1                        # both signs
    if poison:                                                                  # what an out item's upstream gradient may hold
        bad = torch.tensor([INF, NAN, -INF]).repeat(w.numel())[:w.numel()].reshape(w.shape)
        w = torch.where(c["out"], bad, w)
    return w


def _reference_grad(c, w, dtype):
    x = c["lp"].detach().clone().to(dtype).requires_grad_()
    nll, out = mwer_ref.nbest_nll(x, c["ids"], c["lens"], c["il"], c["blank"], max_len=c["max_len"], dtype=dtype)
    assert torch.equal(out, c["out"])
    (torch.where(out, torch.zeros_like(nll), nll) * torch.where(out, torch.zeros_like(w), w).to(dtype)).sum().backward()
    return nll.detach(), x.grad


@pytest.mark.parametrize("name,layout", CASES)
def test_gradient_vs_float64_torch(name, layout):
    c = SETS[name]()
    w = _weights(c)
    n64, g64 = _reference_grad(c, w, torch.float64)
    n32, g32 = _reference_grad(c, w, torch.float32)
    e_ref = float((g32.double() - g64).abs().max())
    nll, grad = _ours(c, layout, upstream=w)
    assert grad.shape == g64.shape and bool(torch.isfinite(grad).all())
    ours = float((grad.double().cpu() - g64).abs().max())
    print(f"\nn-best CTC set {name} [{layout}]: max|nll| {float(n64[~c['out']].abs().max()):.1f}  gradient e_ref {e_ref:.3e}  "
          f"ours {ours:.3e} ({ours / max(e_ref, 1e-300):.2f} x)")
    B, T, V = c["lp"].shape
    g_cpu = grad.cpu()
    for b in range(B):
        Tb = int(c["il"][b])
        if Tb < T:
            assert float(g_cpu[b, Tb:].abs().max()) == 0.0, b
        if bool(c["out"][b].all()):
            assert float(g_cpu[b].abs().max()) == 0.0, b
        elif Tb > 0:
            assert float(g_cpu[b].abs().max()) > 0.0, b
    assert ours <= 4 * e_ref, (ours, e_ref)
    # an inf / NaN upstream gradient at an out item is never read into any sum
    _, poisoned = _ours(c, layout, upstream=_weights(c, poison=True))
    assert bool(torch.isfinite(poisoned).all()) and torch.equal(poisoned, grad)


def test_deterministic_bit_for_bit():
    c = set_edges(8)
    w = _weights(c)
    n1, g1 = _ours(c, upstream=w)
    n2, g2 = _ours(c, upstream=w)
    assert torch.equal(n1.view(torch.int32), n2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))


def test_values_only_call_allocates_no_workspace_and_accepts_host_lengths_and_int64_ids():
    ops = pkg("ops")
    c = set_edges(8)
    want, _ = _ours(c)
    got = ops.ctc_nbest_nll(c["lp"].cuda(), c["ids"].long().cuda(), c["lens"].to(torch.int32), c["il"], blank=0, max_len=8)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and got.grad_fn is None


# ---------------------------------------------------------------------------------------------------------------------------------
def _beam_case():
    g = torch.Generator().manual_seed(31)
    return F.log_softmax(torch.randn(3, 20, 9, generator=g) * 2.0, -1), torch.tensor([20, 13, 0])


@pytest.mark.parametrize("fused", [False, True])
def test_nbest_on_device_equals_prefix_beam_search(fused):
    bs = pkg("beam_search")
    import lm_ref as LR
    lp, ln = _beam_case()
    kw = {}
    if fused:
        kw = dict(lm=pkg("lm").NGramLM.from_corpus(LR.make_corpus(11, 300, 9), 9, 0, order=2), lm_weight=0.4, token_bonus=0.1)
    res = bs.prefix_beam_search(lp.cuda(), 6, 0, lengths=ln, nbest=4, return_scores=True, **kw)
    dev = bs.nbest_on_device(lp.cuda(), 6, 0, lengths=ln, nbest=4, **kw)
    assert len(dev) == (4 if fused else 3) and all(t.is_cuda for t in dev)
    ids, lens, sc = dev[0].cpu(), dev[1].cpu(), dev[2].cpu()
    assert ids.shape == (3, 4, 20) and ids.dtype == torch.int32 and lens.shape == (3, 4) and lens.dtype == torch.int32 and sc.dtype == torch.float32
    for b in range(3):
        k = [n for n in range(4) if int(lens[b, n]) >= 0]
        assert k == list(range(len(res[0][b])))
        for n in k:
            assert ids[b, n, :int(lens[b, n])].tolist() == res[0][b][n]
            assert np.float32(res[1][b][n]).view(np.int32) == sc[b, n].numpy().view(np.int32)
            if fused:
                assert np.float32(res[2][b][n]).view(np.int32) == dev[3].cpu()[b, n].numpy().view(np.int32)
    assert lens[2].tolist() == [0, -1, -1, -1]                                   # no frame: the empty hypothesis alone, the rest absent


# ---------------------------------------------------------------------------------------------------------------------------------
_TOK = []


def _tok():
    if not _TOK:
        import error_ref
        _TOK.append(error_ref.tokenizer())
    return _TOK[0]


def _mwer_case(level):
    """B = 3, T = 24, V = 800 through tokenizer800.vocab: log-probs peaked (not one-hot) on a frame path near each reference, so the beam
    holds competing hypotheses with different error counts; utterance 2 has T_b = 0 (one empty hypothesis)."""
    tok = _tok()
    V, blank, pid = tok.vocab_size, tok.blank_id, tok.token_to_id
    g = torch.Generator().manual_seed(41)
    sents = [[pid["▁우리나라"], pid["▁사회"], pid["▁문제"]], [pid["▁사회"], pid["▁문제"], pid["▁그"], pid["▁우리나라"]], [pid["▁그"]]]
    T = 24
    x = torch.randn(3, T, V, generator=g)
    for b, s in enumerate(sents):
        for k, tkn in enumerate(s):
            x[b, 1 + 4 * k:3 + 4 * k, tkn] += 5.5
            x[b, 1 + 4 * k, sents[(b + 1) % 3][0]] += 5.0                        # a rival for the same frames
        x[b, :, blank] += 4.0
    refs = torch.zeros((3, 4), dtype=torch.long)
    for b, s in enumerate(sents):
        refs[b, :len(s)] = torch.tensor(s)
    table = pkg("error_rate").PieceTable.from_tokenizer(tok) if level != "token" else None
    return dict(lp=F.log_softmax(x, -1), refs=refs, rl=torch.tensor([3, 4, 1]), il=torch.tensor([24, 19, 0]), blank=blank, table=table)


@pytest.mark.parametrize("level", ["word", "token"])
def test_mwer_loss_on_the_device_vs_float64_reference(level):
    mw = pkg("mwer"); er = pkg("error_rate")
    c = _mwer_case(level)
    x = c["lp"].cuda().requires_grad_()
    loss, det = mw.mwer_loss(x, c["refs"].cuda(), c["rl"].cuda(), c["il"].cuda(), c["blank"], nbest=4, beam_width=8, table=c["table"], level=level,
                             return_details=True)
    loss.backward()
    assert all(det[k].is_cuda for k in ("ids", "lens", "nll", "posterior", "errors"))
    ids, lens = det["ids"].cpu(), det["lens"].cpu()
    assert int((lens[0] >= 0).sum()) == 4 and lens[2].tolist() == [0, -1, -1, -1]
    counts = er.error_counts(c["refs"], ids, c["rl"], lens, table=c["table"], ref_skip=c["blank"], hyp_skip=c["blank"])[:, :, er.LEVELS.index(level)]
    errors, counted = counts[..., :3].sum(-1), counts[..., 3] >= 0
    assert torch.equal(det["errors"].cpu()[counted], errors[counted]) and len(set(errors[0].tolist())) > 1

    def ref(dtype):
        y = c["lp"].detach().clone().to(dtype).requires_grad_()
        val, d = mwer_ref.mwer(y, ids, lens, c["il"], c["blank"], errors, counted, dtype=dtype)
        val.backward()
        return val.detach(), y.grad, d
    v64, g64, d64 = ref(torch.float64)
    v32, g32, d32 = ref(torch.float32)
    e_ref = float((g32.double() - g64).abs().max())
    ours = float((x.grad.double().cpu() - g64).abs().max())
    # float32 rounding of the float64 value: nll is a sum of T terms (|nll| eps T / 2 absolute) and enters the posterior through exp, the
    # risk is a sum of N products with errors up to Emax
    fin = torch.isfinite(d64["nll"])
    tol = 8 * EPS32 * 24 * float(d64["nll"][fin].abs().max()) * max(float(errors[counted].max()), 1.0)
    d_loss = abs(float(loss.detach()) - float(v64))
    d_post = float((det["posterior"].double().cpu() - d64["posterior"]).abs().max())
    print(f"\nmwer {level}: loss {float(v64):.6f} |d| {d_loss:.2e} (relative {d_loss / abs(float(v64)):.2e}; torch fp32 {abs(float(v32) - float(v64)):.2e}) "
          f"posterior |d| {d_post:.2e} (tol {tol:.2e})  gradient e_ref {e_ref:.3e} ours {ours:.3e} ({ours / max(e_ref, 1e-300):.2f} x)")
    assert abs(float(v64)) > 1e-3                                                # a case with something to minimise
    assert torch.equal(torch.isfinite(det["nll"]).cpu(), fin)
    assert d_loss < tol * max(1.0, abs(float(v64))) and d_post < tol
    assert float(x.grad[2].abs().max()) == 0.0 and bool(torch.isfinite(x.grad).all())
    assert ours <= 4 * e_ref, (ours, e_ref)


def test_mwer_loss_forward_and_backward_do_not_synchronise():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch has no torch.cuda.set_sync_debug_mode")
    mw = pkg("mwer")
    c = _mwer_case("word")
    x = c["lp"].cuda().requires_grad_()
    args = (c["refs"].cuda(), c["rl"].cuda(), c["il"].cuda(), c["blank"])
    mw.mwer_loss(x, *args, table=c["table"], level="word").backward()           # library load, piece table upload, allocator warm-up
    first = x.grad.clone()
    x.grad = None
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = mw.mwer_loss(x, *args, table=c["table"], level="word")
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert bool(torch.isfinite(loss)) and torch.equal(x.grad, first)


# ---------------------------------------------------------------------------------------------------------------------------------
# trainer, tiny fixture, fp32
# ---------------------------------------------------------------------------------------------------------------------------------
PARENT_KEYS = {"visual_feat1", "visual_feat2", "audio_last", "audio_mid", "fused1", "fused2", "input_lengths1", "input_lengths2", "log_probs1",
               "log_probs2", "loss1", "loss2", "contrast1", "contrast2", "total"}


def _tiny(**attrs):
    from test_step_gpu import build
    t = build(pkg("utils.init").W2V2_TINY, "fp32")
    for k, v in attrs.items():
        setattr(t, k, v)
    t.visual_encoder.train(); t.audio_encoder.train(); t.fusion_module.train(); t.decoder1.train()
    return t


def _batch(unequal_lips=False):
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny.npz"))
    batch = pkg("dataset.synthetic").make_batch(int(fx["batch"]), float(fx["seconds"]), seed=int(fx["seed_batch"]), ragged=bool(fx["ragged"]))
    if unequal_lips:                                                            # the collate pads lip1 and lip2 separately: one frame more for speaker 2
        batch["lip2"] = F.pad(batch["lip2"], (0, 0, 0, 0, 0, 0, 0, 1))
    return batch, fx


def _refs_near_the_beam(t, batch):
    """The fixture's transcripts are random ids an untrained head never emits: every hypothesis is then equally wrong, the risk is 0 and
    its gradient vanishes identically.  Give each utterance its second-best hypothesis as the transcript: that one has no errors, the
    others of the list at least one."""
    bs = pkg("beam_search")
    with torch.no_grad():
        out = t.forward_losses(dict(batch))
    batch = dict(batch)
    for spk in ("1", "2"):
        ids, lens, _ = bs.nbest_on_device(out["log_probs" + spk].float(), t.mwer_beam, t.tokenizer.blank_id, out["input_lengths" + spk], t.mwer_nbest)
        ids, lens = ids.cpu(), lens.cpu()
        rows = [ids[b, 1, :max(0, int(lens[b, 1]))].tolist() or [7] for b in range(ids.shape[0])]
        txt = torch.zeros((len(rows), max(len(r) for r in rows)), dtype=torch.long)
        for b, r in enumerate(rows):
            txt[b, :len(r)] = torch.tensor(r)
        batch["text" + spk], batch["text" + spk + "_lengths"] = txt, torch.tensor([len(r) for r in rows])
    return batch


def _grad_at_lp1(t, batch, pick):
    """forward_losses, backward of ``pick(out)`` -> (out, the gradient at speaker 1's log-probs as the CTC head returned them).  In the
    stacked branch out["log_probs1"] is a slice taken beside the losses' path, so the head's own output (retain_grad) is what is read."""
    t.projection_layer = None
    seen = []

    def keep(mod, args, o):
        o.retain_grad()
        seen.append(o)
    hook = t.decoder1.register_forward_hook(keep)
    try:
        out = t.forward_losses(dict(batch))
    finally:
        hook.remove()
    pick(out).backward()
    B = out["log_probs1"].shape[0]
    assert torch.equal(seen[0][:B].detach(), out["log_probs1"].detach())
    return out, seen[0].grad[:B].detach().clone()


@pytest.mark.parametrize("unequal_lips", [False, True])
def test_trainer_term_adds_exactly_and_gradients_meet_at_the_log_probs(unequal_lips):
    batch, fx = _batch(unequal_lips)
    t = _tiny(mwer_weight=0.0, mwer_level="token")
    assert t.mwer_weight == 0
    off, _ = _grad_at_lp1(t, batch, lambda o: o["total"])
    assert set(off.keys()) == PARENT_KEYS and t._mwer_table is None
    if not unequal_lips:                                                         # the committed fixture of the parent's step
        assert abs(float(off["total"].detach()) - float(fx["train_total"])) < 5e-3
    batch = _refs_near_the_beam(t, batch)
    off, g_ctc = _grad_at_lp1(t, batch, lambda o: o["total"])
    assert set(off.keys()) == PARENT_KEYS
    t.mwer_weight = 0.5
    on, g_both = _grad_at_lp1(t, batch, lambda o: o["total"])
    assert t._pair_step is (not unequal_lips)
    assert set(on.keys()) == PARENT_KEYS | {"mwer1", "mwer2"}
    # weight 0 is the step without the term, bit for bit, and the term is added exactly as stated
    for k in ("loss1", "loss2", "contrast1", "contrast2"):
        assert torch.equal(on[k].detach(), off[k].detach()), k
    want = off["total"].detach() + 0.5 * (on["mwer1"].detach() + on["mwer2"].detach()) / 2
    assert torch.equal(on["total"].detach(), want), (on["total"], want)
    assert bool(torch.isfinite(on["mwer1"])) and bool(torch.isfinite(on["mwer2"]))
    _, g_mwer = _grad_at_lp1(t, batch, lambda o: 0.5 * (o["mwer1"] + o["mwer2"]) / 2)
    assert float(g_mwer.abs().max()) > 0
    d = float((g_both - (g_ctc + g_mwer)).abs().max())
    lim = 4 * EPS32 * float(g_both.abs().max())                                 # one float32 add of the two terms, in either order
    print(f"\ntrainer (unequal lips {unequal_lips}): mwer1 {float(on['mwer1'].detach()):.5f} mwer2 {float(on['mwer2'].detach()):.5f}  max|g_ctc| {float(g_ctc.abs().max()):.3e} "
          f"max|g_mwer| {float(g_mwer.abs().max()):.3e}  |g_both - (g_ctc + g_mwer)| {d:.3e} (limit {lim:.3e})")
    assert d <= lim


def test_trainer_train_step_with_the_term_and_no_synchronisation_with_native_ctc():
    batch, _ = _batch()
    t = _tiny(mwer_weight=0.5, native_ctc=True)
    out = t.train_step(dict(batch))                                             # also the warm-up: library, piece table, allocator
    assert "mwer1" in out and bool(torch.isfinite(out["total"])) and t._mwer_table is not None
    for mod in (t.audio_encoder, t.fusion_module, t.decoder1):
        for n, p in mod.named_parameters():
            assert bool(torch.isfinite(p).all()), n
    with torch.no_grad():                                                       # evaluate()'s loss stays the CTC loss: no term without gradients
        assert "mwer1" not in t.forward_losses(dict(batch))
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch has no torch.cuda.set_sync_debug_mode")
    t.optimizer.zero_grad(set_to_none=True)
    host = {k: v for k, v in batch.items()}
    host.update(t.host_metadata(batch, int(out["audio_last"].shape[1])))        # class counts from the host copy: nothing to read back
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        o = t.forward_losses(host)
        o["total"].backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert bool(torch.isfinite(o["total"])) and "mwer1" in o
