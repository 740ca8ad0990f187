"""Word, character and token error counts: edit distance with operation counts between one reference and N hypotheses per utterance,
computed from token ids through the tokenizer's piece table - on the kernels of csrc/error_counts.hip for GPU tensors (the result stays on
the device, nothing synchronises), in numpy for host tensors and lists.  Both follow ONE law, in integers, and agree exactly:

  text of a sequence of ids (``Tokenizer.decode`` / ``beam_search.fast_decode``, then ``.split()`` as ``trainer.word_error_rate`` does):
    with a piece table, ids outside [0, V) are dropped; ids equal to the sequence's skip id are dropped (-1: none; ``evaluate()`` skips
    nothing in a reference and the blank in a hypothesis - the difference between ``decode`` and ``fast_decode``); the code points of the
    remaining pieces are concatenated, U+2581 read as U+0020, and leading and trailing U+0020 stripped
    token level      the kept ids
    character level  the code points of the stripped text, inner spaces included and not collapsed
    word level       maximal runs of non-space code points; words are equal when their code points are equal
    without a table the ids are the symbols as given (only the skip id is dropped) and the character and word levels are -1
  counts of a pair (reference r, hypothesis h): among all alignments of r to h (match, substitution, deletion of a reference symbol,
    insertion of a hypothesis symbol) the lexicographically smallest (cost = S + D + I, S, D): minimum edits, then fewest substitutions,
    then fewest deletions.  That is a property of the pair, not of an algorithm.  Per level (S, D, I, R = len(r)); hits are R - S - D and
    the hypothesis holds R - D + I symbols; the error rate over a set is sum(S + D + I) / max(1, sum R), at word level exactly
    ``word_error_rate``.  The distance always equals jiwer's; the S / D / I split need not (jiwer's depends on its back-trace).
  limits: at most 4096 ids per sequence; a sequence whose expanded text (before the strip) exceeds 4096 code points has character and
    word levels -1 (all four fields) in every pair it takes part in, its token level is still computed; a hypothesis length < 0 means
    absent (the beam kernel's ``out_len``): all three levels -1; lengths are clamped to [0, L]."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

MAX_LEN = 4096
LEVELS = ("token", "char", "word")
_INS, _DEL, _SUB = 1 << 32, (1 << 32) | 1, (1 << 32) | (1 << 16)
_SPACE, _META_SPACE = 0x20, 0x2581


def word_error_rate(refs, hyps) -> float:
    """jiwer.wer stand-in (jiwer is not installed): total word-level edit distance / total reference words."""
    errs = words = 0
    for r, h in zip(refs, hyps):
        r, h = r.split(), h.split()
        prev = list(range(len(h) + 1))
        for i in range(1, len(r) + 1):
            cur = [i] + [0] * len(h)
            for j in range(1, len(h) + 1):
                cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (r[i - 1] != h[j - 1]))
            prev = cur
        errs += prev[-1]
        words += len(r)
    return errs / max(1, words)


class PieceTable:
    """The tokenizer's pieces as code points: ``offsets`` int32 [V + 1], ``chars`` int32 [offsets[V]] (piece i = chars[offsets[i] :
    offsets[i + 1]]), ``max_piece`` the longest piece; ``on(device)`` is the cached device copy."""

    def __init__(self, pieces):
        pieces = list(pieces)
        for i, p in enumerate(pieces):
            for ch in p:
                if ch != " " and ch.isspace():
                    raise ValueError(f"PieceTable: piece {i} ({p!r}) holds the white-space character U+{ord(ch):04X}: str.strip() / "
                                     "str.split() would treat it as a space, the error counts only U+0020 and U+2581")
        self.pieces = tuple(pieces)
        self.vocab_size = len(pieces)
        if self.vocab_size < 1:
            raise ValueError("PieceTable: no pieces")
        lens = np.array([len(p) for p in pieces], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        self.chars = np.array([ord(ch) for p in pieces for ch in p], dtype=np.int32)
        self.max_piece = max(1, int(lens.max()))
        self._dev = {}

    @classmethod
    def from_tokenizer(cls, tok) -> "PieceTable":
        """Built once per tokenizer and kept on it (rebuilt if its pieces have changed since)."""
        cached = tok.__dict__.get("_piece_table")
        if cached is None or len(cached.pieces) != len(tok.id_to_token) or cached.pieces != tuple(tok.id_to_token):
            cached = cls(tok.id_to_token)
            tok.__dict__["_piece_table"] = cached
        return cached

    def on(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._dev.get(device)
        if t is None:
            chars = self.chars if self.chars.size else np.zeros(1, np.int32)
            t = (torch.from_numpy(self.offsets).to(device), torch.from_numpy(chars).to(device))
            self._dev[device] = t
        return t


# ---------------------------------------------------------------------------------------------------------------------------------------
# the law on the host
def _pair(r: np.ndarray, h: np.ndarray):
    """(S, D, I, R) of two int64 symbol rows: the recurrence over the packed key cost << 32 | S << 16 | D with plain integer min (adding
    a step's key is monotone in that order); the insertion chain along a row is a prefix-min of a[k] - k INS."""
    nr, nh = len(r), len(h)
    j = np.arange(nh + 1, dtype=np.int64) * _INS
    row = j.copy()
    for i in range(nr):
        a = row + _DEL
        if nh:
            np.minimum(a[1:], row[:-1] + np.where(h == r[i], 0, _SUB), out=a[1:])
        row = np.minimum.accumulate(a - j) + j
    key = int(row[nh])
    cost, S, D = key >> 32, (key >> 16) & 0xFFFF, key & 0xFFFF
    return S, D, cost - S - D, nr


def _expand(ids, skip: int, table: Optional[PieceTable]):
    """ids of one sequence -> (kept ids int64, stripped text int64 or None, words: list of code-point tuples or None)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    keep = np.ones(ids.shape, bool) if skip < 0 else ids != skip
    if table is None:
        return ids[keep], None, None
    keep &= (ids >= 0) & (ids < table.vocab_size)
    kept = ids[keep]
    if int((table.offsets[kept + 1] - table.offsets[kept]).sum()) > MAX_LEN:
        return kept, None, None
    text = np.concatenate([table.chars[table.offsets[i]:table.offsets[i + 1]] for i in kept.tolist()] + [np.zeros(0, np.int32)]).astype(np.int64)
    text[text == _META_SPACE] = _SPACE
    solid = np.flatnonzero(text != _SPACE)
    text = text[solid[0]:solid[-1] + 1] if solid.size else text[:0]
    words, run = [], []
    for c in text.tolist():
        if c == _SPACE:
            if run:
                words.append(tuple(run)); run = []
        else:
            run.append(c)
    if run:
        words.append(tuple(run))
    return kept, text, words


def _host_counts(ref, ref_len, hyp, hyp_len, table, ref_skip, hyp_skip) -> np.ndarray:
    """ref int [B, Lr], ref_len [B], hyp int [B, N, Lh], hyp_len [B, N] (numpy) -> int32 [B, N, 3, 4]."""
    B, N = hyp_len.shape
    out = np.full((B, N, 3, 4), -1, np.int32)
    for b in range(B):
        rk, rt, rw = _expand(ref[b, :min(max(int(ref_len[b]), 0), ref.shape[1])], ref_skip, table)
        for n in range(N):
            if hyp_len[b, n] < 0:
                continue
            hk, ht, hw = _expand(hyp[b, n, :min(int(hyp_len[b, n]), hyp.shape[2])], hyp_skip, table)
            out[b, n, 0] = _pair(rk, hk)
            if rt is None or ht is None:
                continue
            out[b, n, 1] = _pair(rt, ht)
            sym = {}
            rs = np.array([sym.setdefault(w, len(sym)) for w in rw], dtype=np.int64)
            hs = np.array([sym.setdefault(w, len(sym)) for w in hw], dtype=np.int64)
            out[b, n, 2] = _pair(rs, hs)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
def _is_int_tensor(t) -> bool:
    return isinstance(t, torch.Tensor) and not t.dtype.is_floating_point and not t.dtype.is_complex and t.dtype != torch.bool


def _pad_rows(rows, width=None):
    """list of id lists -> (int32 [len(rows), width] padded with 0, lengths)."""
    lens = [len(r) for r in rows]
    width = max(lens + [0]) if width is None else width
    out = torch.zeros((len(rows), width), dtype=torch.int32)
    for i, r in enumerate(rows):
        if lens[i]:
            out[i, :lens[i]] = torch.as_tensor(r, dtype=torch.int32)
    return out, lens


def _normalise(refs, hyps, ref_lengths, hyp_lengths):
    """-> refs [B, Lr], ref lengths [B], hyps [B, N, Lh], hyp lengths [B, N] as integer tensors on whatever device each arrived on."""
    if isinstance(refs, torch.Tensor):
        if not _is_int_tensor(refs) or refs.dim() != 2:
            raise ValueError(f"error_counts: refs must be an integer tensor [B, Lr] or a list of id lists, got {refs.dtype} {tuple(refs.shape)}")
        rl = None
    else:
        refs, rl = _pad_rows([list(r) for r in refs])
        rl = torch.tensor(rl, dtype=torch.long)
    B = refs.shape[0]
    if isinstance(hyps, torch.Tensor):
        if not _is_int_tensor(hyps) or hyps.dim() not in (2, 3):
            raise ValueError(f"error_counts: hyps must be an integer tensor [B, Lh] or [B, N, Lh] or lists, got {hyps.dtype} {tuple(hyps.shape)}")
        if hyps.dim() == 2:
            hyps = hyps.unsqueeze(1)
        hl = None
    else:
        items = [list(h) for h in hyps]
        if any(len(h) and isinstance(h[0], (list, tuple, np.ndarray, torch.Tensor)) for h in items):       # n-best lists, possibly ragged
            N = max(len(h) for h in items)
            flat, absent = [], []
            for h in items:
                for n in range(N):
                    flat.append(list(h[n]) if n < len(h) else [])
                    absent.append(n >= len(h))
        else:
            N, flat, absent = 1, items, [False] * len(items)
        hyps, hl = _pad_rows(flat)
        hyps = hyps.reshape(len(items), N, -1)
        hl = torch.tensor([-1 if a else n for n, a in zip(hl, absent)], dtype=torch.long).reshape(len(items), N)
    if hyps.shape[0] != B:
        raise ValueError(f"error_counts: {hyps.shape[0]} hypothesis rows for {B} references")
    N = hyps.shape[1]

    def lengths(given, own, shape, default, name):
        if given is None:
            return own if own is not None else torch.full(shape, default, dtype=torch.long)
        t = given if isinstance(given, torch.Tensor) else torch.as_tensor(given)
        if not _is_int_tensor(t) or t.numel() != int(np.prod(shape)):
            raise ValueError(f"error_counts: {name} must hold {shape} integer lengths, got {t.dtype} {tuple(t.shape)}")
        return t.reshape(shape)
    rl = lengths(ref_lengths, rl, (B,), refs.shape[1], "ref_lengths")
    hl = lengths(hyp_lengths, hl, (B, N), hyps.shape[2], "hyp_lengths")
    if refs.shape[1] > MAX_LEN or hyps.shape[2] > MAX_LEN:
        raise ValueError(f"error_counts: at most {MAX_LEN} ids per sequence, got Lr={refs.shape[1]} Lh={hyps.shape[2]}")
    return refs, rl, hyps, hl


def _ids_on(t: torch.Tensor, dev) -> torch.Tensor:
    """int32 on the device with contiguous rows; an int32 device view with unit inner stride is taken as it is."""
    t = t.to(device=dev, dtype=torch.int32, non_blocking=True)
    if t.shape[-1] and (t.stride(-1) != 1 or any(s < 0 for s in t.stride())):
        t = t.contiguous()
    return t


def _device_counts(refs, rl, hyps, hl, table, ref_skip, hyp_skip, dev) -> torch.Tensor:
    from . import _lib as L
    from . import ops
    B, Lr = refs.shape
    _, N, Lh = hyps.shape
    out = torch.empty((B, N, 3, 4), dtype=torch.int32, device=dev)
    if B == 0:
        return out
    refs, hyps = _ids_on(refs, dev), _ids_on(hyps, dev)
    ref_ld = refs.stride(0) if B > 1 else max(Lr, 1)
    ld_n = hyps.stride(1) if N > 1 else max(Lh, 1)
    ld_b = hyps.stride(0) if B > 1 else (N - 1) * ld_n + max(Lh, 1)
    if ref_ld < Lr:
        refs, ref_ld = refs.contiguous(), max(Lr, 1)
    if ld_n < Lh or ld_b < (N - 1) * ld_n + Lh:
        hyps = hyps.contiguous()
        ld_n, ld_b = max(Lh, 1), N * max(Lh, 1)
    rl = rl.to(device=dev, dtype=torch.long, non_blocking=True).contiguous()
    hl = hl.to(device=dev, dtype=torch.long, non_blocking=True).contiguous()
    if table is None:
        off = chars = None
        V = max_piece = 0
    else:
        off, chars = table.on(dev)
        V, max_piece = table.vocab_size, table.max_piece
    need = L.ll(0)
    L.check(L.lib().av_error_counts_workspace_bytes(B, N, Lr, Lh, max_piece, C.byref(need)), "av_error_counts_workspace_bytes")
    ws = torch.empty((max(4, (need.value + 3) // 4),), dtype=torch.int32, device=dev)
    L.check(L.lib().av_error_counts(ops.ptr(refs) if Lr else None, ref_ld, ops.ptr(rl), ops.ptr(hyps) if Lh else None, ld_b, ld_n,
                                    ops.ptr(hl), B, N, Lr, Lh, int(ref_skip), int(hyp_skip), ops.ptr(off), ops.ptr(chars), V, max_piece,
                                    ops.ptr(out), ops.ptr(ws), ws.numel() * 4, ops.stream()), "av_error_counts")
    return out


def error_counts(refs, hyps, ref_lengths=None, hyp_lengths=None, table: Optional[PieceTable] = None, ref_skip: int = -1,
                 hyp_skip: int = -1) -> torch.Tensor:
    """int32 [B, N, 3, 4]: level (token, character, word) x (S, D, I, R) of each reference against each of its hypotheses; the law is in
    the module docstring.  S / D / I are the lexicographically smallest (cost, S, D) alignment's: the distance S + D + I equals jiwer's,
    the split need not (jiwer's depends on its back-trace).

    ``refs``: integer tensor [B, Lr] (any integer dtype) or a list of id lists; ``hyps``: integer tensor [B, Lh] or [B, N, Lh] (the beam
    kernel's ``out_ids`` with ``hyp_lengths`` = its ``out_len`` as they are), a list of id lists, or a list of n-best lists - a shorter
    n-best list is filled with absent entries.  Lengths default to the full width (lists: their own lengths); a hypothesis length < 0
    means absent.  ``table``: a ``PieceTable``; None = token level only, ids compared as given.

    If either ``refs`` or ``hyps`` is a GPU tensor the kernels of csrc/error_counts.hip run on that device and the result stays there:
    no host transfer, no synchronisation.  Host tensors and lists go through the same law in numpy."""
    refs, rl, hyps, hl = _normalise(refs, hyps, ref_lengths, hyp_lengths)
    dev = next((t.device for t in (refs, hyps) if t.is_cuda), None)
    if dev is not None:
        return _device_counts(refs, rl, hyps, hl, table, ref_skip, hyp_skip, dev)
    out = _host_counts(refs.numpy(), rl.cpu().numpy(), hyps.numpy(), hl.cpu().numpy(), table, int(ref_skip), int(hyp_skip))
    return torch.from_numpy(out)


def _level_rates(sdir) -> dict:
    S, D, I, R = (int(x) for x in sdir)
    return {"S": S, "D": D, "I": I, "R": R, "hits": R - S - D, "errors": S + D + I, "rate": (S + D + I) / max(1, R)}


def rates(counts) -> dict:
    """Sums and rates per level of whatever is summed over: the [B, N, 3, 4] output of ``error_counts`` (hypothesis 0 of every utterance;
    pairs of -1 are left out) or an accumulated total [3, 4].  -> {"token" | "char" | "word": {S, D, I, R, hits, errors, rate}} with
    rate = (S + D + I) / max(1, R); with N > 1 also "oracle": the same per level over, for each utterance, the hypothesis with the fewest
    word errors (token errors where the word level is -1), lowest index on ties, absent hypotheses left out."""
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    c = c.astype(np.int64)
    if c.shape == (3, 4):
        return {name: _level_rates(c[k]) for k, name in enumerate(LEVELS)}
    if c.ndim == 3:
        c = c[:, None]
    if c.ndim != 4 or c.shape[2:] != (3, 4):
        raise ValueError(f"rates: counts must be [B, N, 3, 4], [B, 3, 4] or [3, 4], got {c.shape}")

    def total(sel):                                                            # sel [B, 3, 4]
        ok = sel[:, :, 3:4] >= 0
        return (sel * ok).sum(0)
    res = {name: _level_rates(v) for name, v in zip(LEVELS, total(c[:, 0]))}
    if c.shape[1] > 1:
        err = c[:, :, :, :3].sum(3)                                            # [B, N, 3]
        key = np.where(c[:, :, 2, 3] >= 0, err[:, :, 2], err[:, :, 0])
        key = np.where(c[:, :, 0, 3] >= 0, key, np.iinfo(np.int64).max)       # absent
        best = key.argmin(1)                                                   # first minimum
        res["oracle"] = {name: _level_rates(v) for name, v in zip(LEVELS, total(c[np.arange(c.shape[0]), best]))}
    return res
