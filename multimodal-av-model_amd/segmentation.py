"""CTC segmentation: lay a known transcript over a recording of any length, and say how well each utterance of it fits.

``ctc_segment`` is ``align.forced_align`` without its limits (T <= 4096, about 400 labels) and with what a long recording needs: ends that
may float (the recording may start before and go on after the transcript), a score per frame, and a confidence per utterance - the
min-of-window-means of CTC segmentation (Kuerzinger et al. 2020).  GPU tensors run the kernel of csrc/ctc_segment.hip, host tensors the same
law in float32 numpy.  Both follow ONE law and agree bit for bit - every operation is a float32 max, compare, add, subtract or one division,
in a fixed order.

The law, for item b (T_b = input_lengths[b] clamped to [0, T], L_b = target_lengths[b] clamped to [0, Lmax]):
  lattice    as forced_align: extended label row l' of S = 2 L_b + 1 states (blank, l1, blank, ..., lL, blank); the skip s-2 -> s exists
             where l'_s != l'_{s-2}; ties go to the smaller move.
  emissions  free = 0 (fixed ends): e[t][s] = lp[t][l'_s].  free != 0: spot.py's costs - m[t] = max_v lp[t][v] (a NaN never wins),
             e[t][s] = lp[t][l'_s] - m[t], one subtraction, <= 0; every e of a frame whose m[t] is not finite is -inf.  A score is then a
             log-likelihood ratio against the best unconstrained path over the same frames: 0.0 exactly on an argmax path.
  walk       d[0][0] = e[0][0], d[0][1] = e[0][1], the rest -inf, every move of frame 0 is 0.  At t >= 1 state s sets best = d[t-1][s]
             (move 0), takes d[t-1][s-1] only if strictly greater (move 1), then d[t-1][s-2] only if the skip exists and it is strictly
             greater than the better of those two (move 2); with a free start (bit 0 of ``free``) states 0 and 1 then take a fresh start
             (best = 0, move 3) only if 0 > best strictly.  d[t][s] = best + e[t][s]: one add.
  end        c[t] = the better of d[t][S-1] and d[t][S-2]: S-1 only if strictly greater (S = 1: state 0).  Fixed end: the path ends at
             frame T_b - 1.  Free end (bit 1): at the first t < T_b with the greatest c[t] - a later t replaces an earlier one only if its
             c[t] is strictly greater.  The score is c at the end frame.
  back-trace from the end frame and state: state[t] = s, then stop if move[t][s] is 3 or t is 0, else s -= move[t][s], t -= 1.  Frames
             before the start and after the end have state -1.
  outputs    the four of ``Alignment`` (states, spans, token_scores, score) and frame_scores[t] = e[t][state[t]], 0 off the path.  A token
             score is the sum of frame_scores over the token's span: 0.0, then one add per frame in frame order.  With free = 0 states,
             spans, token scores and score are bit for bit forced_align's.
  utterances utterance u is the token range [b, e) of ``utterances[b][u]``; it is valid if 0 <= b < e <= L_b.  Its frames are [f, g) =
             first frame of token b to end frame of token e-1, blank frames in between included.  utt_means = (the sum of frame_scores
             over [f, g): 0.0, then one add per frame in frame order) / (float)(g - f).  utt_scores = the minimum over the consecutive
             windows [f + k w, min(f + (k+1) w, g)), w = ``score_window``, of (the window's sum, likewise) / (float)(its frame count): the
             first window's mean, replaced by a later one only if that is strictly less.  An invalid utterance gives -1, -1 and 0, 0.
An item is infeasible (score -inf, states and every span -1, every score 0) if a label is outside [0, V) or equal to the blank, or if the
score is -inf (too few frames, -inf emissions on every path, T_b = 0 with L_b > 0).  T_b = 0 with L_b = 0 is feasible with score 0 and an
empty path."""
from __future__ import annotations

from typing import List, NamedTuple

import numpy as np
import torch

MAX_LABELS = 8191                    # Lmax of the kernel: S_max = 16383 states, 16 per thread of a 1024-thread workgroup
DEFAULT_WORKSPACE_BYTES = 4 << 30


class Segmentation(NamedTuple):
    states: torch.Tensor            # int32 [B, T]: extended-state index per frame; -1 off the path and for infeasible items
    spans: torch.Tensor             # int32 [B, Lmax, 2]: first frame, end frame (exclusive) of target position j; -1, -1 where there is none
    token_scores: torch.Tensor      # float32 [B, Lmax]: sum of frame_scores over the span, in frame order; 0 where the span is -1
    score: torch.Tensor             # float32 [B]: score of the path; -inf if infeasible
    frame_scores: torch.Tensor      # float32 [B, T]: e[t][state[t]]; 0 off the path
    utt_spans: torch.Tensor         # int32 [B, U, 2]: first frame, end frame (exclusive) of utterance u; -1, -1 where there is none
    utt_means: torch.Tensor         # float32 [B, U]: mean frame score of the utterance
    utt_scores: torch.Tensor        # float32 [B, U]: the least mean frame score of its windows of score_window frames


def _seq_sum(x: np.ndarray):
    """0.0, then one float32 add per element in order (cumsum is strictly sequential)."""
    return np.cumsum(np.concatenate((np.zeros(1, np.float32), x)), dtype=np.float32)[-1]


def _host_segment(lp: np.ndarray, target, Tb: int, Lb: int, Lmax: int, blank: int, free: int, utts: np.ndarray, w: int):
    """One item in float32 ([T, V]; the law the device follows) -> the eight outputs of one item; T_b and L_b already clamped.  One Python
    step per frame, every state in one array operation."""
    T, V = lp.shape
    Z = np.float32
    NEG = Z(-np.inf)
    U = utts.shape[0]
    states = np.full(T, -1, np.int32)
    spans = np.full((Lmax, 2), -1, np.int32)
    tok = np.zeros(Lmax, np.float32)
    fs = np.zeros(T, np.float32)
    usp = np.full((U, 2), -1, np.int32)
    umean = np.zeros(U, np.float32)
    uscore = np.zeros(U, np.float32)
    out = lambda score: (states, spans, tok, score, fs, usp, umean, uscore)     # noqa: E731
    labels = np.asarray(target[:Lb], dtype=np.int64)
    if ((labels < 0) | (labels >= V) | (labels == blank)).any():
        return out(NEG)
    if Tb == 0:
        return out(Z(0.0) if Lb == 0 else NEG)
    S = 2 * Lb + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = labels
    skip = np.zeros(S, bool)
    skip[2:] = ext[2:] != ext[:-2]
    if free:
        m = np.where(np.isnan(lp[:Tb]), NEG, lp[:Tb]).max(axis=1)
        fin = np.isfinite(m)

    def em(t, cols):
        x = lp[t, cols]
        if free:
            x = x - m[t] if fin[t] else np.full(np.shape(x), NEG, np.float32)
        return x

    def end_of(d):
        if S == 1:
            return d[0], 0
        return (d[S - 1], S - 1) if d[S - 1] > d[S - 2] else (d[S - 2], S - 2)

    d = np.full(S, NEG, np.float32)
    moves = np.zeros((Tb, S), np.int8)
    a2, a3 = np.empty_like(d), np.empty_like(d)
    with np.errstate(invalid="ignore"):
        d[:2] = em(0, ext[:2])
        best_c, best_s = end_of(d)
        best_t = 0
        for t in range(1, Tb):
            a2[0] = NEG; a2[1:] = d[:-1]
            a3[:2] = NEG; a3[2:] = d[:-2]
            a3[~skip] = NEG
            m1 = a2 > d
            best = np.where(m1, a2, d)
            m2 = a3 > best
            best = np.where(m2, a3, best)
            mv = np.where(m2, 2, m1.astype(np.int8)).astype(np.int8)
            if free & 1:
                fresh = Z(0.0) > best[:2]
                best[:2][fresh] = Z(0.0)
                mv[:2][fresh] = 3
            moves[t] = mv
            d = best + em(t, ext)
            c, s = end_of(d)
            if (c > best_c) if free & 2 else (t == Tb - 1):
                best_c, best_s, best_t = c, s, t
    score = Z(best_c)
    if score == NEG:
        return out(NEG)
    t, s = best_t, best_s
    while True:
        states[t] = s
        mv = int(moves[t, s])
        if mv == 3 or t == 0:
            break
        s -= mv
        t -= 1
    a, z = t, best_t + 1                                                       # the path's frames [a, z)
    p = states[a:z]
    tt = np.arange(a, z)
    with np.errstate(invalid="ignore"):
        x = lp[tt, ext[p]]
        fs[a:z] = np.where(fin[tt], x - m[tt], NEG) if free else x
    odd = (p & 1) == 1
    change = p[1:] != p[:-1]
    first = odd & np.concatenate(([True], change))
    last = odd & np.concatenate((change, [True]))
    spans[p[first] >> 1, 0] = tt[first]
    spans[p[last] >> 1, 1] = tt[last] + 1
    spans[(spans < 0).any(axis=1)] = -1                                        # (a path with NaN scores may leave a label state out)
    for j in np.flatnonzero(spans[:, 0] >= 0):
        tok[j] = _seq_sum(fs[spans[j, 0]:spans[j, 1]])
    for u in range(U):
        b0, e0 = int(utts[u, 0]), int(utts[u, 1])
        if not 0 <= b0 < e0 <= Lb:
            continue
        f, g = int(spans[b0, 0]), int(spans[e0 - 1, 1])
        if f < 0 or g <= f:
            continue
        usp[u] = (f, g)
        umean[u] = _seq_sum(fs[f:g]) / Z(g - f)
        low = None
        for k in range(f, g, w):
            n = min(k + w, g) - k
            mean = Z(_seq_sum(fs[k:k + n]) / Z(n))
            if low is None or mean < low:
                low = mean
        uscore[u] = low
    return out(score)


def _utterance_table(utterances, B: int):
    """-> int32 [B, U, 2] tensor (on the device it came from) of token ranges; None is U = 0."""
    if utterances is None:
        return torch.zeros((B, 0, 2), dtype=torch.int32)
    ut = utterances if isinstance(utterances, torch.Tensor) else torch.as_tensor(np.asarray(utterances, dtype=np.int64).reshape(B, -1, 2))
    if ut.dim() != 3 or ut.shape[0] != B or ut.shape[2] != 2 or ut.dtype.is_floating_point or ut.dtype == torch.bool:
        raise ValueError(f"ctc_segment: utterances must be an integer tensor [B={B}, U, 2] of token ranges, got {ut.dtype} {tuple(ut.shape)}")
    return ut.to(torch.int32)


def ctc_segment(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths=None, target_lengths=None, blank: int = 0, utterances=None,
                free_start: bool = False, free_end: bool = False, score_window: int = 30, batch_first: bool = True,
                max_workspace_bytes: int = DEFAULT_WORKSPACE_BYTES) -> Segmentation:
    """``log_probs`` [B, T, V] (``batch_first=False``: [T, B, V]), any T; ``targets`` integer [B, Lmax <= 8191] padded; lengths [B]
    (default: T and Lmax); ``utterances`` integer [B, U, 2] token ranges [begin, end) into the target ((-1, -1) or an empty range: none;
    ranges may leave gaps; None: U = 0) -> ``Segmentation`` of tensors on the input's device.

    GPU tensor: the kernel of csrc/ctc_segment.hip; strided views with contiguous rows are taken as they are, lengths, targets and
    utterances may live on the device (nothing is read back) or on the host (copied without blocking): no host transfer, no
    synchronisation.  Its move workspace holds 2 bits per frame and state; a call that needs more than ``max_workspace_bytes`` raises.
    Host tensor: the same law in float32 numpy, bit for bit."""
    from .align import _lengths
    if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3:
        raise ValueError("ctc_segment: log_probs must be a [B, T, V] tensor (or [T, B, V] with batch_first=False)")
    if targets.dim() != 2 or targets.dtype.is_floating_point or targets.dtype == torch.bool:
        raise ValueError(f"ctc_segment: targets must be an integer tensor [B, Lmax], got {targets.dtype} {tuple(targets.shape)}")
    blank, w = int(blank), int(score_window)
    free = (1 if free_start else 0) | (2 if free_end else 0)
    if batch_first:
        B, T, V = log_probs.shape
    else:
        T, B, V = log_probs.shape
    Lmax = targets.shape[1]
    if targets.shape[0] != B:
        raise ValueError(f"ctc_segment: targets has {targets.shape[0]} rows for a batch of {B}")
    if not 0 <= blank < V or T < 1 or w < 1:
        raise ValueError(f"ctc_segment: need 0 <= blank < V, T >= 1 and score_window >= 1, got T={T} V={V} blank={blank} score_window={w}")
    ut = _utterance_table(utterances, B)
    dev = log_probs.device
    il = _lengths(input_lengths, "input_lengths", B, T, dev)
    tl = _lengths(target_lengths, "target_lengths", B, Lmax, dev)
    if log_probs.is_cuda:
        from . import ops
        lp = log_probs.detach()
        if lp.dtype != torch.float32:
            lp = lp.float()
        return Segmentation(*ops.ctc_segment(lp, targets, il, tl, ut, blank=blank, free=free, score_window=w, batch_first=batch_first,
                                             max_workspace_bytes=max_workspace_bytes))
    lp_h = log_probs.detach().to(torch.float32)
    lp_h = (lp_h if batch_first else lp_h.transpose(0, 1)).numpy()
    tg_h = targets.detach().to(torch.long).numpy()
    ut_h = ut.detach().cpu().numpy()
    U = ut_h.shape[1]
    res = (np.empty((B, T), np.int32), np.empty((B, Lmax, 2), np.int32), np.empty((B, Lmax), np.float32), np.empty((B,), np.float32),
           np.empty((B, T), np.float32), np.empty((B, U, 2), np.int32), np.empty((B, U), np.float32), np.empty((B, U), np.float32))
    for b in range(B):
        Tb, Lb = min(max(int(il[b]), 0), T), min(max(int(tl[b]), 0), Lmax)
        for dst, src in zip(res, _host_segment(lp_h[b], tg_h[b], Tb, Lb, Lmax, blank, free, ut_h[b], w)):
            dst[b] = src
    return Segmentation(*(torch.from_numpy(x) for x in res))


def utterance_segments(seg: Segmentation, texts, frame_rate: float = 25.0) -> List[List[dict]]:
    """Host helper: per item the list of its aligned utterances in order, each a dict with ``text`` (``texts[b][u]``), ``start`` = first
    frame / frame_rate, ``end`` = end frame / frame_rate (seconds), ``score`` (utt_scores: the least window mean) and ``mean`` (utt_means).
    An utterance without a span (-1, -1) is left out; ``texts[b]`` may be shorter than U."""
    usp, um, us = (np.asarray(x.detach().cpu()) for x in (seg.utt_spans, seg.utt_means, seg.utt_scores))
    if len(texts) != usp.shape[0]:
        raise ValueError(f"utterance_segments: {len(texts)} lists of texts for {usp.shape[0]} items")
    out = []
    for b, names in enumerate(texts):
        if len(names) > usp.shape[1]:
            raise ValueError(f"utterance_segments: item {b} has {len(names)} texts for {usp.shape[1]} utterances")
        out.append([{"text": names[u], "start": int(usp[b, u, 0]) / frame_rate, "end": int(usp[b, u, 1]) / frame_rate,
                     "score": float(us[b, u]), "mean": float(um[b, u])} for u in range(len(names)) if usp[b, u, 0] >= 0])
    return out
