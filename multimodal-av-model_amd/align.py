"""CTC forced alignment: given the transcript, WHEN was it said.

``forced_align`` returns the best frame path (Viterbi) of each target through the CTC lattice of the log-probs the trainer hands to its
loss (model/trainer.py:116-117, 229-242 of the reference), the frames each target position occupies and their scores: on the kernel of
csrc/ctc_align.hip for GPU tensors, in float32 numpy for host tensors.  Both follow ONE law and agree bit for bit:

  extended label row l' of S = 2 L + 1 states (blank, l1, blank, ..., lL, blank); the skip s-2 -> s exists where l'_s != l'_{s-2}
  d[0][0] = lp[0][blank], d[0][1] = lp[0][l1], the rest -inf
  d[t][s] = max(d[t-1][s], d[t-1][s-1], skip ? d[t-1][s-2] : -inf) + lp[t][l'_s]      (float32: one max, one add per cell)
  ties go to the smaller move: s-1 only if strictly greater than s, s-2 only if strictly greater than the better of those two
  final state S-1 if d[T_b-1][S-1] > d[T_b-1][S-2] strictly, else S-2 (S = 1: state 0)

An utterance is infeasible (score -inf, states and spans -1, token scores 0) if a label is outside [0, V) or equal to the blank, or if the
final score is -inf (T_b < L_b + repeats, -inf emissions on every path, T_b = 0 with L_b > 0).  The CTC head runs at the lip-frame rate, so
a span of frames is directly a piece of video: ``word_segments`` turns spans into word times."""
from __future__ import annotations

from typing import List, NamedTuple

import numpy as np
import torch


class Alignment(NamedTuple):
    states: torch.Tensor            # int32 [B, T]: extended-state index per frame; -1 for t >= T_b and for infeasible items
    spans: torch.Tensor             # int32 [B, Lmax, 2]: first frame, end frame (exclusive) of target position j; -1, -1 where there is none
    token_scores: torch.Tensor      # float32 [B, Lmax]: sum of lp[t][l_j] over the span, in frame order; 0 where the span is -1
    score: torch.Tensor             # float32 [B]: log-probability of the path; -inf if infeasible


def _host_align(lp: np.ndarray, target, Tb: int, Lb: int, Lmax: int, blank: int):
    """One utterance in the dtype of ``lp`` ([T, V]; float32 = the law the device follows) -> (states [T], spans [Lmax, 2],
    token scores [Lmax], score); T_b and L_b already clamped."""
    T, V = lp.shape
    Z = lp.dtype.type
    NEG = Z(-np.inf)
    states = np.full(T, -1, np.int32)
    spans = np.full((Lmax, 2), -1, np.int32)
    tok = np.zeros(Lmax, lp.dtype)
    labels = np.asarray(target[:Lb], dtype=np.int64)
    if ((labels < 0) | (labels >= V) | (labels == blank)).any():
        return states, spans, tok, NEG
    if Tb == 0:
        return states, spans, tok, (Z(0.0) if Lb == 0 else NEG)
    S = 2 * Lb + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = labels
    skip = np.zeros(S, bool)
    skip[2:] = ext[2:] != ext[:-2]
    em = lp[:Tb][:, ext]                                                      # [T_b, S] gathered emissions
    d = np.full(S, NEG, lp.dtype)
    d[:2] = em[0, :2]
    moves = np.zeros((Tb, S), np.int8)
    a2, a3 = np.empty_like(d), np.empty_like(d)
    for t in range(1, Tb):
        a2[0] = NEG; a2[1:] = d[:-1]
        a3[:2] = NEG; a3[2:] = d[:-2]
        a3[~skip] = NEG
        m1 = a2 > d
        best = np.where(m1, a2, d)
        m2 = a3 > best
        best = np.where(m2, a3, best)
        moves[t] = np.where(m2, 2, m1.astype(np.int8))
        d = best + em[t]
    s = (S - 1 if d[S - 1] > d[S - 2] else S - 2) if S > 1 else 0
    score = d[s]
    if score == NEG:
        return states, spans, tok, NEG
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        s -= int(moves[t, s])
    path = states[:Tb]
    for j in range(Lb):
        fr = np.flatnonzero(path == 2 * j + 1)
        if fr.size:                                                            # always, on a feasible path: contiguous and non-empty
            spans[j] = (fr[0], fr[-1] + 1)
            tok[j] = np.cumsum(em[fr[0]:fr[-1] + 1, 2 * j + 1], dtype=lp.dtype)[-1]       # cumsum: strictly in frame order
    return states, spans, tok, score


def _lengths(t, name: str, B: int, default: int, device) -> torch.Tensor:
    if t is None:
        return torch.full((B,), default, dtype=torch.long, device=device)
    from .ops import _ctc_lengths
    return _ctc_lengths("forced_align", name, t, B, device)


def forced_align(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths=None, target_lengths=None, blank: int = 0,
                 batch_first: bool = True) -> Alignment:
    """``log_probs`` [B, T, V] (``batch_first=False``: [T, B, V]), ``targets`` integer [B, Lmax] padded, lengths [B] (default: T and
    Lmax) -> ``Alignment`` of tensors on the input's device.

    GPU tensor: the kernel of csrc/ctc_align.hip; strided views with contiguous rows are taken as they are, lengths and targets may live
    on the device (nothing is read back) or on the host (copied without blocking): no host transfer, no synchronisation.  Host tensor:
    the same law in float32 numpy, bit for bit."""
    if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3:
        raise ValueError("forced_align: log_probs must be a [B, T, V] tensor (or [T, B, V] with batch_first=False)")
    if targets.dim() != 2 or targets.dtype.is_floating_point or targets.dtype == torch.bool:
        raise ValueError(f"forced_align: targets must be an integer tensor [B, Lmax], got {targets.dtype} {tuple(targets.shape)}")
    blank = int(blank)
    if batch_first:
        B, T, V = log_probs.shape
    else:
        T, B, V = log_probs.shape
    Lmax = targets.shape[1]
    if targets.shape[0] != B:
        raise ValueError(f"forced_align: targets has {targets.shape[0]} rows for a batch of {B}")
    if not 0 <= blank < V or not 1 <= T <= 4096:
        raise ValueError(f"forced_align: need 0 <= blank < V and 1 <= T <= 4096, got T={T} V={V} blank={blank}")
    dev = log_probs.device
    il = _lengths(input_lengths, "input_lengths", B, T, dev)
    tl = _lengths(target_lengths, "target_lengths", B, Lmax, dev)
    if log_probs.is_cuda:
        from . import ops
        lp = log_probs.detach()
        if lp.dtype != torch.float32:
            lp = lp.float()
        return Alignment(*ops.ctc_align(lp, targets, il, tl, blank=blank, batch_first=batch_first))
    lp_h = log_probs.detach().to(torch.float32)
    lp_h = (lp_h if batch_first else lp_h.transpose(0, 1)).numpy()
    tg_h = targets.detach().to(torch.long).numpy()
    states = np.empty((B, T), np.int32)
    spans = np.empty((B, Lmax, 2), np.int32)
    tok = np.empty((B, Lmax), np.float32)
    score = np.empty((B,), np.float32)
    for b in range(B):
        Tb, Lb = min(max(int(il[b]), 0), T), min(max(int(tl[b]), 0), Lmax)
        states[b], spans[b], tok[b], score[b] = _host_align(lp_h[b], tg_h[b], Tb, Lb, Lmax, blank)
    return Alignment(torch.from_numpy(states), torch.from_numpy(spans), torch.from_numpy(tok), torch.from_numpy(score))


def token_path(alignment: Alignment, targets: torch.Tensor, blank: int) -> torch.Tensor:
    """int64 [B, T]: the id emitted at each frame of the path (``blank`` on even states, the target's label on odd ones, -1 where the state
    is -1), on the device of the alignment."""
    st = alignment.states.long()
    tg = targets.to(device=st.device, dtype=torch.long)
    if tg.shape[1] == 0:
        lab = torch.full_like(st, int(blank))
    else:
        lab = tg.gather(1, (st.clamp_min(0) >> 1).clamp_max(tg.shape[1] - 1))
    ids = torch.where((st & 1) == 1, lab, torch.full_like(st, int(blank)))
    return torch.where(st < 0, torch.full_like(st, -1), ids)


def word_segments(tokenizer, target_ids, spans, token_scores, frame_rate: float = 25.0, token_conf=None, aggregation: str = "min") -> List[dict]:
    """Word times of ONE utterance (host).  ``target_ids``: its L label ids; ``spans`` [>= L, 2] and ``token_scores`` [>= L] as returned by
    ``forced_align`` for it.  Words are the maximal runs of tokens between '▁' pieces (utils/tokenizer.py); each is a dict with ``word``,
    ``start`` = first token's first frame / frame_rate, ``end`` = last token's end frame / frame_rate (seconds), ``score`` = mean token
    score per frame of the word.  An infeasible utterance (a span of -1) gives [].  With ``token_conf`` [>= L] (confidence.py) every word
    also has ``confidence``: the ``aggregation`` ("mean", "min", "prod"; confidence.py's span law in float32) of its tokens' confidences."""
    ids = [int(i) for i in (target_ids.tolist() if hasattr(target_ids, "tolist") else target_ids)]
    sp = np.asarray(spans.cpu() if isinstance(spans, torch.Tensor) else spans).reshape(-1, 2)[:len(ids)]
    sc = np.asarray(token_scores.cpu() if isinstance(token_scores, torch.Tensor) else token_scores, dtype=np.float64).reshape(-1)[:len(ids)]
    if len(sp) < len(ids) or len(sc) < len(ids) or (sp < 0).any():
        return []
    if token_conf is not None:
        from .confidence import check_aggregation, host_span_law
        check_aggregation("word_segments", aggregation)
        tc = np.asarray(token_conf.cpu() if isinstance(token_conf, torch.Tensor) else token_conf, dtype=np.float32).reshape(-1)[:len(ids)]
        if len(tc) < len(ids):
            raise ValueError(f"word_segments: token_conf holds {len(tc)} values for {len(ids)} tokens")
    space = tokenizer.token_to_id.get("▁")
    words, run = [], []

    def close():
        if run:
            frames = sum(int(sp[j, 1] - sp[j, 0]) for j in run)
            words.append({"word": "".join(tokenizer.id_to_token[ids[j]] if 0 <= ids[j] < tokenizer.vocab_size else "" for j in run),
                          "start": int(sp[run[0], 0]) / frame_rate, "end": int(sp[run[-1], 1]) / frame_rate,
                          "score": float(sum(sc[j] for j in run) / max(frames, 1))})
            if token_conf is not None:
                words[-1]["confidence"] = float(host_span_law(tc[run], 0, len(run), len(run), aggregation))
            del run[:]
    for j, i in enumerate(ids):
        if i == space:
            close()
        else:
            run.append(j)
    close()
    return words
