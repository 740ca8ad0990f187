"""CTC keyword spotting: was this phrase said, where, and how sure.

``keyword_spot`` searches the CTC log-probs of a batch (forward_log_probs for clips, longform.stitch for recordings of any length) for K
keywords given as token ids: on the kernels of csrc/ctc_spot.hip for GPU tensors, in float32 numpy for host tensors.  Both follow ONE law
and agree bit for bit - every operation is a float32 max, compare, subtraction or addition in a fixed order.

The law, for utterance b (T_b = input_lengths[b] clamped to [0, T], T without lengths) and keyword y_1..y_L (1 <= L <= 32, no id the blank,
every id in [0, V)):
  costs    m[t] = max_v lp[t][v] (a NaN never wins) ; c[t][v] = lp[t][v] - m[t], one subtraction, c <= 0 ; if m[t] is not finite every cost
           of frame t is -inf.  A path's score is the sum of c along it in frame order: the log-likelihood ratio of the path against the
           best unconstrained path over the same frames, 0.0 exactly when the path is an argmax path.
  lattice  S = 2 L - 1 states y_1, blank, y_2, ..., blank, y_L: no leading or trailing blank, a hit starts on the first frame of y_1 and
           ends on the last frame of y_L.  The skip s-2 -> s exists for even s >= 2 where y differs from the label two states back.
  walk     each cell carries (d, start); before frame 0 d = -inf and start = -1 everywhere.  At frame t state s sets best = d[t-1][s],
           takes d[t-1][s-1] only if strictly greater, then the skip predecessor d[t-1][s-2] only if the skip exists and it is strictly
           greater than the better of those two; state 0 alone then takes a fresh start (0, start = t) only if 0 > best strictly (ties
           keep the earlier start).  d[t][s] = best + c[t][label_s], start carried from the chosen predecessor.
           e[t] = d[t][S-1], es[t] = start[t][S-1].
  hits     a candidate is a frame t < T_b with e[t] > -inf and e[t] >= min_score.  Up to N times (1 <= N <= 8): the candidate with the
           greatest e[t] (ties: the greater t) is reported as (es[t], t + 1, e[t]) and every candidate whose interval [es[u], u + 1)
           overlaps the reported one is dropped.  Hits come out in the order found: scores descend.
An invalid keyword (length < 1 after clamping to [0, Lmax], an id outside [0, V) or equal to the blank) and T_b = 0 give no hits.
The CTC head runs at the lip-frame rate, so an interval of frames is directly a piece of video: ``hit_segments`` turns hits into times."""
from __future__ import annotations

from typing import List, NamedTuple

import numpy as np
import torch

from .bias import MAX_PHRASE, ContextBias

MAX_HITS = 8


class Spots(NamedTuple):
    hits: torch.Tensor              # int32 [B, K, N, 2]: first frame, end frame (exclusive) of hit r of keyword k; -1, -1 past the count
    scores: torch.Tensor            # float32 [B, K, N]: descending; -inf past the count
    counts: torch.Tensor            # int32 [B, K]


def _host_end_series(lp: np.ndarray, keywords, Tb: int, blank: int):
    """The walk of one utterance for K VALID keywords (sequences of ids) at once, in the dtype of ``lp`` ([T, V]; float32 = the law the
    device follows) -> (e [K, T_b], es int32 [K, T_b]).  One Python step per frame, every keyword and state in one array operation."""
    Z = lp.dtype.type
    NEG = Z(-np.inf)
    K = len(keywords)
    e = np.full((K, Tb), NEG, lp.dtype)
    es = np.full((K, Tb), -1, np.int32)
    if K == 0 or Tb == 0:
        return e, es
    Smax = max(2 * len(y) - 1 for y in keywords)
    lab = np.full((K, Smax), blank, np.int64)
    skip = np.zeros((K, Smax), bool)
    last = np.empty(K, np.int64)
    for k, y in enumerate(keywords):
        y = np.asarray(y, np.int64)
        lab[k, 0:2 * len(y) - 1:2] = y
        skip[k, 2:2 * len(y) - 1:2] = y[1:] != y[:-1]
        last[k] = 2 * len(y) - 2
    rows = np.arange(K)
    m = np.where(np.isnan(lp[:Tb]), NEG, lp[:Tb]).max(axis=1)
    finite = np.isfinite(m)
    d = np.full((K, Smax), NEG, lp.dtype)
    st = np.full((K, Smax), -1, np.int32)
    p1, p2 = np.empty_like(d), np.empty_like(d)
    s1, s2 = np.empty_like(st), np.empty_like(st)
    with np.errstate(invalid="ignore"):
        for t in range(Tb):
            c = lp[t][lab] - m[t] if finite[t] else np.full((K, Smax), NEG, lp.dtype)
            p1[:, 0] = NEG; p1[:, 1:] = d[:, :-1]
            s1[:, 0] = -1; s1[:, 1:] = st[:, :-1]
            p2[:, :2] = NEG; p2[:, 2:] = d[:, :-2]
            s2[:, :2] = -1; s2[:, 2:] = st[:, :-2]
            take = p1 > d
            best, bs = np.where(take, p1, d), np.where(take, s1, st)
            take = skip & (p2 > best)
            best, bs = np.where(take, p2, best), np.where(take, s2, bs)
            fresh = Z(0.0) > best[:, 0]
            best[fresh, 0] = Z(0.0)
            bs[fresh, 0] = t
            d, st = best + c, bs
            e[:, t], es[:, t] = d[rows, last], st[rows, last]
    return e, es


def _host_select(e: np.ndarray, es: np.ndarray, N: int, min_score):
    """The hits of one (utterance, keyword) from its end series -> list of (first frame, end frame, score)."""
    out = []
    cand = (e > -np.inf) & (e >= min_score)
    u = np.arange(len(e))
    for _ in range(N):
        idx = np.flatnonzero(cand)
        if not idx.size:
            break
        t = int(idx[e[idx] == e[idx].max()][-1])
        a, b = int(es[t]), t + 1
        out.append((a, b, e[t]))
        cand &= ~((es < b) & (a < u + 1))
    return out


def _check_phrases(phrases, V: int, blank: int):
    out = []
    for ph in phrases:
        try:
            ids = tuple(int(i) for i in ph)
        except (TypeError, ValueError):
            raise ValueError(f"keyword_spot: keyword {ph!r} is not a sequence of token ids") from None
        if not ids:
            raise ValueError(f"keyword_spot: keyword {ph!r} is empty")
        if len(ids) > MAX_PHRASE:
            raise ValueError(f"keyword_spot: keyword {ph!r} has {len(ids)} ids, more than {MAX_PHRASE}")
        if any(not 0 <= i < V for i in ids):
            raise ValueError(f"keyword_spot: keyword {ph!r} holds an id outside [0, {V})")
        if blank in ids:
            raise ValueError(f"keyword_spot: keyword {ph!r} holds the blank {blank}")
        out.append(ids)
    return out


def _keyword_table(keywords, V: int, blank: int):
    """-> (ids [K, Lmax] integer tensor or int32 numpy array, lengths [K] likewise).  A ContextBias and a sequence of id sequences are
    checked here (ValueError naming the phrase); a tensor is taken as it is - its invalid rows give count 0, as in the law."""
    if isinstance(keywords, ContextBias):
        keywords = keywords.phrases
    elif isinstance(keywords, torch.Tensor):
        keywords = (keywords, None)
    if isinstance(keywords, (tuple, list)) and len(keywords) == 2 and isinstance(keywords[0], torch.Tensor) and keywords[0].dim() == 2:
        ids, lens = keywords
        if ids.dtype.is_floating_point or ids.dtype == torch.bool or not 1 <= ids.shape[1] <= MAX_PHRASE:
            raise ValueError(f"keyword_spot: a keyword tensor must be integer [K, 1 <= Lmax <= {MAX_PHRASE}], got {ids.dtype} {tuple(ids.shape)}")
        if lens is None:
            lens = torch.full((ids.shape[0],), ids.shape[1], dtype=torch.int32, device=ids.device)
        elif not isinstance(lens, torch.Tensor):
            lens = torch.as_tensor(lens, dtype=torch.int32)
        if lens.dim() != 1 or lens.numel() != ids.shape[0] or lens.dtype.is_floating_point or lens.dtype == torch.bool:
            raise ValueError(f"keyword_spot: keyword lengths must be {ids.shape[0]} integers, got {lens.dtype} {tuple(lens.shape)}")
        return ids, lens
    phrases = _check_phrases(keywords, V, blank)
    Lmax = max([len(p) for p in phrases], default=1)
    ids = np.zeros((len(phrases), Lmax), np.int32)
    for k, p in enumerate(phrases):
        ids[k, :len(p)] = p
    return ids, np.asarray([len(p) for p in phrases], np.int32)


def keyword_spot(log_probs: torch.Tensor, keywords, input_lengths=None, blank: int = 0, max_hits: int = 4, min_score: float = float("-inf"),
                 batch_first: bool = True) -> Spots:
    """``log_probs`` [B, T, V] (``batch_first=False``: [T, B, V]), any T -> ``Spots`` of tensors on the input's device.  ``keywords``: a
    ``bias.ContextBias`` (its ``.phrases``, in order: one phrase list serves biasing and spotting), a sequence of id sequences (checked
    like ``ContextBias.from_phrases``: ValueError naming the phrase), or an integer tensor [K, Lmax <= 32] - alone, or as ``(ids,
    lengths)`` - which may already live on the device; its invalid rows give count 0.

    GPU tensor: the kernels of csrc/ctc_spot.hip; strided views with contiguous rows are taken as they are, lengths may live on the device
    (nothing is read back) or on the host (copied without blocking): no host transfer, no synchronisation.  Host tensor: the same law in
    float32 numpy, bit for bit."""
    if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3:
        raise ValueError("keyword_spot: log_probs must be a [B, T, V] tensor (or [T, B, V] with batch_first=False)")
    blank, N, min_score = int(blank), int(max_hits), float(min_score)
    if batch_first:
        B, T, V = log_probs.shape
    else:
        T, B, V = log_probs.shape
    if not 0 <= blank < V or T < 1:
        raise ValueError(f"keyword_spot: need 0 <= blank < V and T >= 1, got T={T} V={V} blank={blank}")
    if not 1 <= N <= MAX_HITS or min_score != min_score:
        raise ValueError(f"keyword_spot: need 1 <= max_hits <= {MAX_HITS} and a min_score that is not NaN, got {N}, {min_score}")
    ids, lens = _keyword_table(keywords, V, blank)
    K = ids.shape[0]
    if log_probs.is_cuda:
        from . import ops
        lp = log_probs.detach()
        if lp.dtype != torch.float32:
            lp = lp.float()
        if isinstance(ids, np.ndarray):
            if K == 0:
                ids, lens = torch.zeros((0, 1), dtype=torch.int32), torch.zeros((0,), dtype=torch.int32)
            else:
                ids, lens = ops.h2d_async(ids, lp.device), ops.h2d_async(lens, lp.device)
        return Spots(*ops.ctc_spot(lp, ids, lens, input_lengths, blank=blank, max_hits=N, min_score=min_score, batch_first=batch_first))
    lp_h = log_probs.detach().to(torch.float32)
    lp_h = (lp_h if batch_first else lp_h.transpose(0, 1)).numpy()
    ids_h = ids if isinstance(ids, np.ndarray) else ids.detach().cpu().numpy()
    lens_h = lens if isinstance(lens, np.ndarray) else lens.detach().cpu().numpy()
    Lmax = ids_h.shape[1]
    if input_lengths is None:
        il = [T] * B
    else:
        il = torch.as_tensor(input_lengths).reshape(-1).tolist()
        if len(il) != B:
            raise ValueError(f"keyword_spot: input_lengths must hold one length per batch item ({B}), got {len(il)}")
    valid, kws = [], []
    for k in range(K):
        y = ids_h[k, :min(max(int(lens_h[k]), 0), Lmax)].astype(np.int64)
        if y.size >= 1 and not ((y < 0) | (y >= V) | (y == blank)).any():
            valid.append(k); kws.append(y)
    hits = np.full((B, K, N, 2), -1, np.int32)
    scores = np.full((B, K, N), -np.inf, np.float32)
    counts = np.zeros((B, K), np.int32)
    ms = np.float32(min_score)
    for b in range(B):
        Tb = min(max(int(il[b]), 0), T)
        e, es = _host_end_series(lp_h[b], kws, Tb, blank)
        for j, k in enumerate(valid):
            found = _host_select(e[j], es[j], N, ms)
            counts[b, k] = len(found)
            for r, (a, z, s) in enumerate(found):
                hits[b, k, r] = (a, z)
                scores[b, k, r] = s
    return Spots(torch.from_numpy(hits), torch.from_numpy(scores), torch.from_numpy(counts))


def hit_segments(spots: Spots, names, frame_rate: float = 25.0) -> List[List[dict]]:
    """Host helper: per utterance the list of its hits, keyword by keyword in the order found, each a dict with ``keyword`` (``names[k]``),
    ``start`` = first frame / frame_rate, ``end`` = end frame / frame_rate (seconds), ``score`` and ``per_frame`` = score / (end frame -
    first frame) - a reporting convenience computed here, not part of the law."""
    hits, scores, counts = (np.asarray(x.detach().cpu()) for x in spots)
    B, K = counts.shape
    if len(names) != K:
        raise ValueError(f"hit_segments: {len(names)} names for {K} keywords")
    out = []
    for b in range(B):
        rows = []
        for k in range(K):
            for r in range(int(counts[b, k])):
                a, z, s = int(hits[b, k, r, 0]), int(hits[b, k, r, 1]), float(scores[b, k, r])
                rows.append({"keyword": names[k], "start": a / frame_rate, "end": z / frame_rate, "score": s, "per_frame": s / max(z - a, 1)})
        out.append(rows)
    return out
