"""GPU: word / character / token error counts on the device (csrc/error_counts.hip, error_rate.error_counts) in both libraries: exactly
equal to the package's host path (which tests/test_error_rate_cpu.py ties to tests/error_ref.py) at the column-chunk edges of the 64-lane
row, at the 4096 limit, through tokenizer800.vocab with n-best lists and absent hypotheses, beyond the text limit, on strided views whose
padding holds ids that would change the counts; every output element written; determinism; a side stream; and evaluate()'s report."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
import error_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7
EDGES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200]


def E():
    return pkg("error_rate")


@pytest.fixture(params=["fp32", "fp16"])
def library(request):
    """libavhip.so and libavhip_f16.so (the counts are integers in both)."""
    P = pkg("precision")
    old = P.get_precision()
    P.set_precision(request.param)
    yield request.param
    P.set_precision(old)


_CACHE = {}


def _once(key, make):
    """Inputs and the host path's result of one case, computed once for both libraries."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _raw(ref, rl, hyp, hl, table=None, ref_skip=-1, hyp_skip=-1, pad=5, fill=19, stream=None):
    """av_error_counts itself on strided views: ``ref`` int [B, Lr] and ``hyp`` int [B, N, Lh] (host) are placed in wider device blocks
    filled with the valid id ``fill`` (``▁것`` in tokenizer800: reading it would change every level), positions at or past a length hold
    ``fill`` too, and the output is pre-filled with SENTINEL."""
    L = pkg("_lib"); ops = pkg("ops")
    ref, hyp = torch.as_tensor(ref, dtype=torch.int32), torch.as_tensor(hyp, dtype=torch.int32)
    rl, hl = torch.as_tensor(rl, dtype=torch.long), torch.as_tensor(hl, dtype=torch.long)
    B, Lr = ref.shape
    _, N, Lh = hyp.shape
    ref, hyp = ref.clone(), hyp.clone()
    ref[torch.arange(Lr)[None, :] >= rl.clamp(0, Lr)[:, None]] = fill
    hyp[torch.arange(Lh)[None, None, :] >= hl.clamp(0, Lh)[:, :, None]] = fill
    rblock = torch.full((B, Lr + pad), fill, dtype=torch.int32, device="cuda")
    hblock = torch.full((B, N + 1, Lh + pad), fill, dtype=torch.int32, device="cuda")
    rblock[:, :Lr] = ref.cuda(); hblock[:, :N, :Lh] = hyp.cuda()
    rv, hv = rblock[:, :Lr], hblock[:, :N, :Lh]
    assert rv.stride(0) == Lr + pad and hv.stride(1) == Lh + pad and hv.stride(0) == (N + 1) * (Lh + pad)
    rl_d, hl_d = rl.cuda(), hl.cuda()
    out = torch.full((B, N, 3, 4), SENTINEL, dtype=torch.int32, device="cuda")
    if table is None:
        off = chars = None; V = mp = 0
    else:
        (off, chars), V, mp = table.on("cuda"), table.vocab_size, table.max_piece
    need = L.ll(0)
    L.check(L.lib().av_error_counts_workspace_bytes(B, N, Lr, Lh, mp, ctypes.byref(need)), "workspace")
    ws = torch.full((need.value // 4 + 4,), 0x55555555, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib().av_error_counts(ops.ptr(rv), rv.stride(0), ops.ptr(rl_d), ops.ptr(hv), hv.stride(0), hv.stride(1), ops.ptr(hl_d), B, N, Lr, Lh,
                                    ref_skip, hyp_skip, ops.ptr(off), ops.ptr(chars), V, mp, ops.ptr(out), ops.ptr(ws), need.value,
                                    ops.stream() if stream is None else stream), "av_error_counts")
    return out


def _host(ref, rl, hyp, hl, table=None, ref_skip=-1, hyp_skip=-1):
    return E().error_counts(torch.as_tensor(ref), torch.as_tensor(hyp), rl, hl, table=table, ref_skip=ref_skip, hyp_skip=hyp_skip)


def _same(got, want, what):
    got = got.cpu()
    assert got.dtype == torch.int32 and got.shape == want.shape, (what, got.dtype, got.shape)
    assert not bool((got == SENTINEL).any()), (what, "an output element was not written")
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (what, bad[:5].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


def _edges():
    """Token level, no table: ten references of the EDGES lengths, each against ten hypotheses of the EDGES lengths (four symbols, so
    matches matter); hypotheses are noisy copies of the reference where they overlap."""
    rng = np.random.default_rng(64)
    n = len(EDGES)
    ref = rng.integers(0, 4, size=(n, 200))
    hyp = np.repeat(ref[:, None, :], n, axis=1)
    noise = rng.random(hyp.shape) < 0.2
    hyp[noise] = rng.integers(0, 4, size=int(noise.sum()))
    hyp[:, ::2] = np.roll(hyp[:, ::2], 1, axis=2)                              # every other one shifted: insertions and deletions
    rl = torch.tensor(EDGES)
    hl = torch.tensor(EDGES)[None, :].repeat(n, 1)
    return ref, rl, hyp, hl, _host(ref, rl, hyp, hl)


def test_token_level_at_the_chunk_edges(library):
    ref, rl, hyp, hl, want = _once("edges", _edges)
    assert bool((want[:, :, 0, 3] == torch.tensor(EDGES)[:, None]).all()) and bool((want[:, :, 1:] == -1).all())
    _same(_raw(ref, rl, hyp, hl), want, "edges")
    # and through the wrapper, with a skip id on each side
    want_s = _once("edges skip", lambda: _host(ref, rl, hyp, hl, ref_skip=1, hyp_skip=2))
    got = E().error_counts(torch.as_tensor(ref).cuda(), torch.as_tensor(hyp).cuda(), rl, hl.cuda(), ref_skip=1, hyp_skip=2)
    assert got.is_cuda
    _same(got, want_s, "edges skip")
    _same(_raw(ref, rl, hyp, hl, ref_skip=1, hyp_skip=2), want_s, "edges skip raw")


def _limit():
    rng = np.random.default_rng(4096)
    ref = rng.integers(0, 6, size=(2, 4096))
    hyp = ref.copy()[:, None, :]
    noise = rng.random(hyp.shape) < 0.3
    hyp[noise] = rng.integers(0, 6, size=int(noise.sum()))
    hyp = np.roll(hyp, 3, axis=2)
    rl, hl = torch.tensor([4096, 4096]), torch.tensor([[4096], [0]])
    return ref, rl, hyp, hl, _host(ref, rl, hyp, hl)


def test_token_level_at_the_length_limit(library):
    ref, rl, hyp, hl, want = _once("limit", _limit)
    assert want[1, 0, 0].tolist() == [0, 4096, 0, 4096] and want[0, 0, 0, 3] == 4096 and int(want[0, 0, 0, :3].sum()) > 1000
    _same(_raw(ref, rl, hyp, hl, pad=3), want, "4096")


def _pad(rows, width=None, fill=0):
    width = max([len(r) for r in rows] + [1]) if width is None else width
    out = np.full((len(rows), width), fill, dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, [len(r) for r in rows]


def _vocab(N):
    tok = R.tokenizer()
    table = E().PieceTable.from_tokenizer(tok)
    cases = R.vocab_cases(tok)
    B = len(cases)
    ref, rl = _pad([c[1] for c in cases])
    hyps = [c[2] for c in cases]
    flat, hl = [], []
    for b in range(B):
        for n in range(N):
            h = hyps[(b + 3 * n) % B]                                          # entry 0: the case's own hypothesis
            absent = N > 1 and ((n == 1 and b % 3 == 0) or (n == N - 1 and b % 2 == 0))       # in the middle and at the end of a list
            flat.append(h)
            hl.append(-1 if absent else len(h))
    hyp, _ = _pad(flat)
    hyp = hyp.reshape(B, N, -1)
    hl = torch.tensor(hl).reshape(B, N)
    rl = torch.tensor(rl)
    want = _host(ref, rl, hyp, hl, table, -1, tok.blank_id)
    return tok, table, ref, rl, hyp, hl, want


@pytest.mark.parametrize("N", [1, 4])
def test_through_the_vocabulary(library, N):
    tok, table, ref, rl, hyp, hl, want = _once(("vocab", N), lambda: _vocab(N))
    if N == 1:                                                                 # the host path itself is tied to the strings on the CPU; once more here
        for b, (name, r, h) in enumerate(R.vocab_cases(tok)):
            assert want[b, 0].tolist() == [list(x) for x in R.id_counts(tok, r, h)], name
    else:
        assert bool((want[hl < 0] == -1).all()) and bool((want[hl >= 0][:, 0] >= 0).all()) and int((hl < 0).sum()) >= 8
    _same(_raw(ref, rl, hyp, hl, table, -1, tok.blank_id), want, ("vocab", N))
    got = E().error_counts(torch.as_tensor(ref).cuda(), torch.as_tensor(hyp, dtype=torch.int32).cuda(), rl.cuda(), hl, table=table,
                           hyp_skip=tok.blank_id)
    _same(got, want, ("vocab wrapper", N))
    assert E().rates(got) == E().rates(want)


def _overflow():
    tok = R.tokenizer()
    table = E().PieceTable.from_tokenizer(tok)
    long7 = tok.token_to_id["▁우리나라에서"]
    cases = R.vocab_cases(tok)
    rows_r = [cases[0][1], [long7] * 600, cases[2][1], [long7] * 585]          # 4200 > 4096 code points | 4095: the last that fits
    rows_h = [[cases[0][2], [long7] * 600], [[long7] * 599 + [5], cases[1][2]], [cases[2][2], cases[3][2]], [[long7] * 584, [long7] * 586]]
    ref, rl = _pad(rows_r)
    hyp, hl = _pad([h for row in rows_h for h in row])
    hyp, hl = hyp.reshape(4, 2, -1), torch.tensor(hl).reshape(4, 2)
    rl = torch.tensor(rl)
    return tok, table, ref, rl, hyp, hl, _host(ref, rl, hyp, hl, table, -1, tok.blank_id)


def test_texts_beyond_the_limit(library):
    tok, table, ref, rl, hyp, hl, want = _once("overflow", _overflow)
    over = torch.tensor([[False, True], [True, True], [False, False], [False, True]])        # 586 x 7 = 4102 is beyond it too
    assert bool((want[:, :, 1:][over] == -1).all()) and bool((want[:, :, 1:][~over] >= 0).all()) and bool((want[:, :, 0] >= 0).all())
    assert want[1, 0, 0].tolist() == [1, 0, 0, 600] and want[3, 0, 2].tolist() == [0, 1, 0, 585] and want[3, 0, 1, 3] == 4094
    _same(_raw(ref, rl, hyp, hl, table, -1, tok.blank_id), want, "overflow")


def test_single_pair_runs_twice_and_on_a_side_stream(library):
    tok, table, ref, rl, hyp, hl, want = _once(("vocab", 4), lambda: _vocab(4))
    one = _raw(ref[4:5], rl[4:5], hyp[4:5, :1], hl[4:5, :1], table, -1, tok.blank_id)
    _same(one, want[4:5, :1], "B = 1, N = 1")
    a = _raw(ref, rl, hyp, hl, table, -1, tok.blank_id)
    b = _raw(ref, rl, hyp, hl, table, -1, tok.blank_id)
    assert torch.equal(a, b)
    # two calls back to back on a side stream, nothing synchronises between them
    e_ref, e_rl, e_hyp, e_hl, e_want = _once("edges", _edges)
    side = torch.cuda.Stream()
    rd, hd, rld, hld = torch.as_tensor(ref).cuda(), torch.as_tensor(hyp).cuda(), rl.cuda(), hl.cuda()
    erd, ehd, erld, ehld = torch.as_tensor(e_ref).cuda(), torch.as_tensor(e_hyp).cuda(), e_rl.cuda(), e_hl.cuda()
    table.on("cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = E().error_counts(rd, hd, rld, hld, table=table, hyp_skip=tok.blank_id)
        y = E().error_counts(erd, ehd, erld, ehld)
    side.synchronize()
    _same(x, want, "side stream, first")
    _same(y, e_want, "side stream, second")


def test_evaluate_reports_only_when_asked(tmp_path):
    """eval_report off: evaluate() as before and last_report None.  On (greedy and beam 8): loss, WER and last_decoded equal the off run's,
    and the report's word and character counts are the reference's on the texts evaluate() compared."""
    from test_dataset_gpu import _Tok, _make_corpus
    from test_step_gpu import build as build_trainer
    ds = pkg("dataset.multi_speaker_dataset"); cf = pkg("dataset.collate_fn").collate_fn; init = pkg("utils.init")
    _, sents = _make_corpus(tmp_path)
    pairs = [(sents[0], sents[2]), (sents[1], sents[3]), (sents[2], sents[1]), (sents[3], sents[0])]
    loader = torch.utils.data.DataLoader(ds.FixedSentencePairDataset(pairs, _Tok()), batch_size=2, shuffle=False, collate_fn=cf, num_workers=0)
    t = build_trainer(init.W2V2_TINY, "fp32")
    assert t.eval_report is False and t.last_report is None
    for width in (0, 8):
        t.eval_beam_width = width
        t.eval_report = False
        off = t.evaluate(loader)
        decoded = t.last_decoded
        assert t.last_report is None
        assert t.evaluate(loader) == off and t.last_decoded == decoded and t.last_report is None
        t.eval_report = True
        on = t.evaluate(loader)
        assert on == off and t.last_decoded == decoded                         # the WER from the device counts is the host function's float
        rep = t.last_report
        assert sorted(rep) == ["speaker1", "speaker2"]
        for s, name in enumerate(("speaker1", "speaker2")):
            refs = [t.tokenizer.decode(batch["text%d" % (s + 1)][i][:int(batch["text%d_lengths" % (s + 1)][i])].tolist())
                    for batch in loader for i in range(batch["text1"].shape[0])]
            hyps = decoded[s]
            assert len(refs) == len(hyps) == 4
            for level, split in (("word", str.split), ("char", list)):
                want = np.array([R.counts(split(r), split(h)) for r, h in zip(refs, hyps)]).sum(0).tolist()
                got = rep[name][level]
                assert [got["S"], got["D"], got["I"], got["R"]] == want, (width, name, level, got, want)
                assert got["rate"] == sum(want[:3]) / max(1, want[3])
            assert rep[name]["token"]["R"] > 0
    t.eval_report = False
    t.evaluate(loader)
    assert t.last_report is None
