"""CPU: the host law of error_rate.py against tests/error_ref.py (exhaustive enumeration of every alignment on tiny pairs, the tuple
recurrence on longer ones, a fixed case list), through tests/golden/tokenizer800.vocab against trainer.word_error_rate and the reference
on the decoded strings, the piece table's white-space check, the input forms of error_counts / rates, and the C-ABI's argument errors."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
import error_ref as R


def E():
    return pkg("error_rate")


def _token(r, h):
    """(S, D, I, R) of the package's host path at token level, no table."""
    out = E().error_counts([list(r)], [list(h)])
    assert out.dtype == torch.int32 and tuple(out.shape) == (1, 1, 3, 4)
    assert bool((out[0, 0, 1:] == -1).all())                                  # no table: no character or word level
    return tuple(out[0, 0, 0].tolist())


def test_host_law_equals_exhaustive_enumeration_on_tiny_pairs():
    rng = np.random.default_rng(3)
    for _ in range(3000):
        r = rng.integers(0, 3, size=rng.integers(0, 7)).tolist()
        h = rng.integers(0, 3, size=rng.integers(0, 7)).tolist()
        want = R.enumerate_counts(r, h)
        assert R.counts(r, h) == want, (r, h)
        assert _token(r, h) == want, (r, h)


def test_host_law_equals_the_tuple_recurrence_on_longer_pairs():
    rng = np.random.default_rng(4)
    for k in range(60):
        sym = int(rng.integers(2, 12))
        r = rng.integers(0, sym, size=rng.integers(0, 91)).tolist()
        h = rng.integers(0, sym, size=rng.integers(0, 91)).tolist()
        assert _token(r, h) == R.counts(r, h), (k, r, h)


@pytest.mark.parametrize("r,h,want", [
    ("", "", (0, 0, 0, 0)),
    ("", "abc", (0, 0, 3, 0)),
    ("abc", "", (0, 3, 0, 3)),
    ("abca", "abca", (0, 0, 0, 4)),
    ("ab", "ba", (0, 1, 1, 2)),                                               # one deletion and one insertion, not two substitutions
    ("abc", "xyz", (3, 0, 0, 3)),
    ("aaaa", "aa", (0, 2, 0, 4)),
    ("aa", "aaaaa", (0, 0, 3, 2)),
    ("abab", "baba", (0, 1, 1, 4)),
])
def test_fixed_cases(r, h, want):
    r, h = [ord(c) for c in r], [ord(c) for c in h]
    assert R.enumerate_counts(r, h) == want
    assert R.counts(r, h) == want
    assert _token(r, h) == want


def test_through_the_vocabulary_equals_the_string_metrics():
    tok = R.tokenizer()
    wer = pkg("model.trainer").word_error_rate
    table = E().PieceTable.from_tokenizer(tok)
    assert E().PieceTable.from_tokenizer(tok) is table                        # cached on the tokenizer
    assert table.vocab_size == 800 and table.max_piece == 7
    cases = R.vocab_cases(tok)
    got = E().error_counts([c[1] for c in cases], [c[2] for c in cases], table=table, hyp_skip=tok.blank_id)
    assert tuple(got.shape) == (len(cases), 1, 3, 4)
    for (name, r, h), g in zip(cases, got[:, 0].tolist()):
        want = R.id_counts(tok, r, h)
        assert [tuple(x) for x in g] == want, (name, g, want)
        S, D, I, Rw = g[2]
        assert (S + D + I) / max(1, Rw) == wer([R.ref_text(tok, r)], [R.hyp_text(tok, h)]), name
    by_name = {c[0]: tuple(map(tuple, g)) for c, g in zip(cases, got[:, 0].tolist())}
    tk, ch, wd = by_name["same words, other pieces"]
    assert sum(wd[:3]) == 0 and sum(ch[:3]) == 0 and sum(tk[:3]) > 0 and wd[3] == 3
    assert by_name["blank in the reference"][1][3] == len("사회<blank> 문제")   # decode keeps the literal piece
    assert by_name["reference strips to nothing"][2] == (0, 0, 3, 0) and by_name["both strip to nothing"][1] == (0, 0, 0, 0)
    # the whole set at once: the rate of the summed word counts is word_error_rate over the set
    rt = E().rates(got)
    refs, hyps = [R.ref_text(tok, c[1]) for c in cases], [R.hyp_text(tok, c[2]) for c in cases]
    assert rt["word"]["rate"] == wer(refs, hyps) and rt["word"]["R"] == sum(len(x.split()) for x in refs)
    assert rt["char"]["R"] == sum(len(x) for x in refs) and "oracle" not in rt
    assert E().rates(got[:, 0].sum(0)) == rt                                  # an accumulated total gives the same


def test_input_forms_lengths_absent_entries_and_oracle():
    tok = R.tokenizer()
    table = E().PieceTable.from_tokenizer(tok)
    cases = R.vocab_cases(tok)[:6]
    refs, hyps = [c[1] for c in cases], [c[2] for c in cases]
    base = E().error_counts(refs, hyps, table=table, hyp_skip=tok.blank_id)
    # padded tensors of another integer dtype with explicit lengths; the padding holds valid ids that must not be read
    Lr, Lh = max(map(len, refs)) + 3, max(map(len, hyps)) + 2
    rt = torch.full((len(cases), Lr), 19, dtype=torch.int64); ht = torch.full((len(cases), Lh), 33, dtype=torch.int16)
    for i, (r, h) in enumerate(zip(refs, hyps)):
        rt[i, :len(r)] = torch.tensor(r).clamp(-2 ** 15, 2 ** 15 - 1); ht[i, :len(h)] = torch.tensor(h).clamp(-2 ** 15, 2 ** 15 - 1)
    got = E().error_counts(rt, ht, [len(r) for r in refs], torch.tensor([len(h) for h in hyps]), table=table, hyp_skip=tok.blank_id)
    assert torch.equal(got, base)
    # ragged n-best lists: missing entries are absent (-1 everywhere); the oracle picks the fewest word errors, lowest index on ties
    nbest = [[hyps[0], refs[0]], [refs[1]], [hyps[2], hyps[2], refs[2]], [hyps[3]], [hyps[4]], [hyps[5]]]
    nb = E().error_counts(refs, nbest, table=table, hyp_skip=tok.blank_id)
    assert tuple(nb.shape) == (6, 3, 3, 4)
    assert torch.equal(nb[:, 0], E().error_counts(refs, [n[0] for n in nbest], table=table, hyp_skip=tok.blank_id)[:, 0])
    assert bool((nb[1, 1:] == -1).all()) and bool((nb[0, 2] == -1).all()) and bool((nb[2] != -1).all())
    rates = E().rates(nb)
    pick = []
    for i, n in enumerate(nbest):
        errs = [sum(R.id_counts(tok, refs[i], h)[2][:3]) for h in n]
        pick.append(errs.index(min(errs)))
    want_err = sum(sum(R.id_counts(tok, refs[i], nbest[i][k])[2][:3]) for i, k in enumerate(pick))
    assert rates["oracle"]["word"]["errors"] == want_err and rates["oracle"]["word"]["R"] == rates["word"]["R"]
    assert rates["oracle"]["word"]["errors"] <= rates["word"]["errors"]
    # a negative length given explicitly is an absent hypothesis; lengths beyond the width are clamped
    one = E().error_counts(rt, ht, [len(r) for r in refs], [-1] + [10 ** 6] * 5, table=table, hyp_skip=tok.blank_id)
    assert bool((one[0] == -1).all()) and bool((one[1:, 0, 0, 3] >= 0).all())


def test_texts_beyond_the_limit_lose_character_and_word_levels_only():
    tok = R.tokenizer()
    table = E().PieceTable.from_tokenizer(tok)
    long7 = tok.token_to_id["▁우리나라에서"]
    refs = [[long7] * 600, [long7] * 3]                                       # 4200 > 4096 code points | 21
    hyps = [[long7] * 599 + [5], [long7] * 2]
    got = E().error_counts(refs, hyps, table=table, hyp_skip=tok.blank_id)
    assert got[0, 0].tolist() == [[1, 0, 0, 600], [-1] * 4, [-1] * 4]
    assert got[1, 0].tolist() == [list(x) for x in R.id_counts(tok, refs[1], hyps[1])]
    with pytest.raises(ValueError):
        E().error_counts([[1] * 4097], [[1]])


def test_piece_table_refuses_other_white_space():
    Tok = pkg("utils.tokenizer").SyntheticTokenizer
    good = Tok(50)
    E().PieceTable.from_tokenizer(good)
    bad = Tok(50)
    bad.id_to_token[20] = "가　나"
    with pytest.raises(ValueError, match="3000"):
        E().PieceTable.from_tokenizer(bad)
    spaced = Tok(50)
    spaced.id_to_token[20] = "가 각"                                          # U+0020 itself is the space of the law
    t = E().PieceTable.from_tokenizer(spaced)
    assert E().error_counts([[20]], [[5, 4, 6]], table=t)[0, 0, 2].tolist() == [0, 0, 0, 2]


def test_abi_argument_errors_are_reported_without_a_device():
    L = pkg("_lib")
    lib = L.lib()
    n = L.ll(0)
    P = 4096                                                                  # stands for a (16-byte aligned) device pointer: nothing is launched

    def call(**kw):
        a = dict(ref_ids=P, ref_ld=8, ref_lens=P, hyp_ids=P, ld_b=16, ld_n=8, hyp_lens=P, B=2, N=2, Lr=8, Lh=8, rs=-1, hs=3, off=P, chars=P,
                 V=800, mp=7, out=P, ws=P, wsb=1 << 20)
        a.update(kw)
        return lib.av_error_counts(a["ref_ids"], a["ref_ld"], a["ref_lens"], a["hyp_ids"], a["ld_b"], a["ld_n"], a["hyp_lens"], a["B"], a["N"],
                                   a["Lr"], a["Lh"], a["rs"], a["hs"], a["off"], a["chars"], a["V"], a["mp"], a["out"], a["ws"], a["wsb"], None)
    for kw, word in [(dict(B=0), b"bad shape"), (dict(N=0), b"bad shape"), (dict(Lr=4097, ref_ld=4097), b"bad shape"), (dict(Lh=-1), b"bad shape"),
                     (dict(V=0), b"piece table"), (dict(mp=0), b"piece table"), (dict(out=None), b"null"), (dict(ws=None), b"null"),
                     (dict(ref_lens=None), b"null"), (dict(hyp_lens=None), b"null"), (dict(ref_ids=None), b"null"), (dict(chars=None), b"null"),
                     (dict(wsb=64), b"too small"), (dict(ws=P + 4), b"aligned"), (dict(ref_ld=7), b"leading"), (dict(ld_n=7), b"leading"),
                     (dict(ld_b=15), b"leading")]:
        assert call(**kw) != 0, kw
        assert word in lib.av_last_error(), (kw, lib.av_last_error())
    assert lib.av_error_counts_workspace_bytes(1, 1, 1, 1, 1, None) != 0 and b"null" in lib.av_last_error()
    for bad in [(0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 4097, 1, 1), (1, 1, 1, -1, 1), (1, 1, 1, 1, -1), (2 ** 31 - 1, 2 ** 31 - 1, 1, 1, 1)]:
        assert lib.av_error_counts_workspace_bytes(*bad, ctypes.byref(n)) != 0 and b"av_error_counts_workspace_bytes" in lib.av_last_error()

    def size(*a):
        assert lib.av_error_counts_workspace_bytes(*a, ctypes.byref(n)) == 0, lib.av_last_error()
        return n.value
    base = (3, 2, 40, 50, 7)
    assert size(*base) > 0 and size(1, 1, 0, 0, 0) > 0
    for k, hi in enumerate([9, 8, 4096, 4096, 64]):
        steps = [size(*(base[:k] + (v,) + base[k + 1:])) for v in range(base[k], hi + 1, max(1, (hi - base[k]) // 7))]
        assert all(x <= y for x, y in zip(steps, steps[1:])), (k, steps)
    assert size(3, 2, 40, 50, 7) > size(3, 2, 40, 50, 0)                      # the table's text and words take room
