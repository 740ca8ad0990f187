"""CTC confidences: how sure the model is of each frame, token, word and utterance of a hypothesis.

The frame measure is the entropy-based confidence of Laptev & Ginsburg 2022 ("Fast Entropy-Based Methods of Word-Level Confidence Estimation
for End-to-End ASR"; the NeMo method): the normalised Gibbs or Tsallis entropy of the frame's distribution, or its normalised maximum
probability; a token's confidence aggregates its frames, a word's its tokens, an utterance's its tokens.  GPU tensors run on the kernels of
csrc/ctc_confidence.hip, host tensors on the same laws in float32 numpy.

Frame law for one row x[0..V) (it renormalises, so the row need not sum to 1), every operation in float32:
  m = max x ; d = x - m ; e = exp(d) ; s = sum e
  max_prob   c = (V / s - 1) / (V - 1)
  entropy    c = 1 + (sum_{e > 0} e d / s - ln s) / ln V
  tsallis a  c = (sum exp(a d) / exp(a ln s) - u) / (1 - u),  u = exp((1 - a) ln V)       a finite, > 0, |a - 1| >= 1/64
  result     c >= 0 ? min(c, 1) : 0;  a NaN entry and a row without a finite maximum give 0, a -inf entry adds 0 to every sum
A one-hot row gives exactly 1, a uniform row 0 (to the rounding of V^(1 - a) for tsallis).  Frames t >= T_b get 0.

Span law for frames [f, e) of an utterance, clipped to [0, T_b); 0 for a span of -1 and for one that is empty after clipping:
  mean   the float32 sum in frame order, then one division by the count
  min    the minimum
  prod   the float32 product in frame order
Given the same frame confidences the device and the host agree bit for bit.

Whether these confidences predict that a word is correct has not been measured here: there is no trained checkpoint and no data."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from ._lib import CONF_AGGREGATIONS, CONF_METHODS


class GreedyTimed(NamedTuple):
    ids: torch.Tensor               # int32 [B, T]: the greedy ids (first maximal index, repeats collapsed, blanks dropped), -1 padded
    lengths: torch.Tensor           # int32 [B]: number of ids
    spans: torch.Tensor             # int32 [B, T, 2]: first frame, end frame (exclusive) of the run of equal argmax frames behind id j; -1 padded
    token_conf: torch.Tensor        # float32 [B, T]: the aggregation of frame_conf over that run; 0 padded
    frame_conf: torch.Tensor        # float32 [B, T]: 0 for t >= T_b


def check_method(who: str, method: str, alpha: float) -> float:
    if method not in CONF_METHODS:
        raise ValueError(f"{who}: method must be one of {sorted(CONF_METHODS)}, got {method!r}")
    alpha = float(alpha)
    if method == "tsallis":
        if not 0.0 < alpha < float("inf"):                                # NaN fails both comparisons
            raise ValueError(f"{who}: the tsallis alpha must be finite and > 0, got {alpha}")
        if abs(alpha - 1.0) < 1.0 / 64.0:
            raise ValueError(f"{who}: tsallis alpha {alpha} is within 1/64 of 1, where the law loses its digits: use method='entropy', its "
                             "alpha -> 1 limit")
    return alpha


def check_aggregation(who: str, aggregation: str) -> str:
    if aggregation not in CONF_AGGREGATIONS:
        raise ValueError(f"{who}: aggregation must be one of {sorted(CONF_AGGREGATIONS)}, got {aggregation!r}")
    return aggregation


def host_frame_law(x: np.ndarray, method: str, alpha: float) -> np.ndarray:
    """The frame law on rows [..., V] in the dtype of ``x`` (float32: the law the device follows; tests/confidence_ref.py hands it float64)."""
    Z = x.dtype.type
    V = x.shape[-1]
    with np.errstate(all="ignore"):
        m = x.max(axis=-1, keepdims=True)
        d = x - m
        e = np.exp(d)
        s = e.sum(axis=-1)
        fV, one = Z(V), Z(1)
        if method == "max_prob":
            c = (fV / s - one) / (fV - one)
        elif method == "entropy":
            r = np.where(e > 0, e * d, Z(0)).sum(axis=-1)
            c = one + (r / s - np.log(s)) / np.log(fV)
        else:
            a = Z(alpha)
            r = np.exp(a * d).sum(axis=-1)
            u = np.exp((one - a) * np.log(fV))
            c = (r / np.exp(a * np.log(s)) - u) / (one - u)
        c = np.where(c >= 0, np.minimum(c, one), Z(0))
        return np.where(np.isfinite(m[..., 0]), c, Z(0)).astype(x.dtype)


def host_span_law(conf: np.ndarray, f: int, e: int, Tb: int, aggregation: str):
    """The span law on one utterance's confidences [T] for the span [f, e), in the dtype of ``conf``: one in-order loop."""
    Z = conf.dtype.type
    f, e = max(int(f), 0), min(int(e), int(Tb))
    if f >= e:
        return Z(0)
    acc = conf[f]
    for t in range(f + 1, e):
        acc = acc + conf[t] if aggregation == "mean" else (min(acc, conf[t]) if aggregation == "min" else acc * conf[t])
    return Z(acc / Z(e - f)) if aggregation == "mean" else Z(acc)


def _rows(who: str, log_probs, batch_first: bool):
    if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3:
        raise ValueError(f"{who}: log_probs must be a [B, T, V] tensor (or [T, B, V] with batch_first=False)")
    if not log_probs.dtype.is_floating_point:
        raise TypeError(f"{who}: log_probs must be a floating-point tensor, got {log_probs.dtype}")
    B, T, V = log_probs.shape if batch_first else (log_probs.shape[1], log_probs.shape[0], log_probs.shape[2])
    if V < 2 or not 1 <= T <= 4096:
        raise ValueError(f"{who}: need V >= 2 and 1 <= T <= 4096, got T={T} V={V}")
    return B, T, V


def _host_lengths(who: str, t, B: int, T: int):
    if t is None:
        return [T] * B
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, dtype=torch.long)
    if t.dim() != 1 or t.numel() != B:
        raise ValueError(f"{who}: lengths must hold one length per batch item ({B}), got shape {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError(f"{who}: lengths must be an integer tensor, got {t.dtype}")
    return [min(max(int(v), 0), T) for v in t.tolist()]


def _host_rows(log_probs, batch_first: bool) -> np.ndarray:
    lp = log_probs.detach().to(torch.float32)
    return (lp if batch_first else lp.transpose(0, 1)).contiguous().numpy()


def _f32(lp: torch.Tensor) -> torch.Tensor:
    lp = lp.detach()
    return lp if lp.dtype == torch.float32 else lp.float()


def frame_confidence(log_probs: torch.Tensor, input_lengths=None, method: str = "tsallis", alpha: float = 0.33,
                     batch_first: bool = True) -> torch.Tensor:
    """``log_probs`` [B, T, V] (``batch_first=False``: [T, B, V]), ``input_lengths`` [B] on either side (default T) -> float32 [B, T] on
    the input's device: the frame law above, 0 for t >= T_b.  GPU tensor: av_ctc_frame_conf, strided views with contiguous rows are taken
    as they are, nothing is read back.  Host tensor: the same law in float32 numpy."""
    alpha = check_method("frame_confidence", method, alpha)
    B, T, V = _rows("frame_confidence", log_probs, batch_first)
    if log_probs.is_cuda:
        from . import ops
        return ops.ctc_frame_conf(_f32(log_probs), input_lengths, method, alpha, batch_first)
    ln = _host_lengths("frame_confidence", input_lengths, B, T)
    conf = host_frame_law(_host_rows(log_probs, batch_first), method, alpha)
    conf[np.arange(T)[None, :] >= np.asarray(ln, np.int64)[:, None]] = 0
    return torch.from_numpy(conf)


def span_confidence(frame_conf: torch.Tensor, spans: torch.Tensor, input_lengths=None, aggregation: str = "min") -> torch.Tensor:
    """``frame_conf`` float32 [B, T], ``spans`` integer [B, L, 2] (first frame, end exclusive, as ``forced_align`` returns them),
    ``input_lengths`` [B] (default T); spans and lengths on either side -> float32 [B, L] on the device of ``frame_conf``: the span law."""
    check_aggregation("span_confidence", aggregation)
    if not isinstance(frame_conf, torch.Tensor) or frame_conf.dim() != 2 or not frame_conf.dtype.is_floating_point:
        raise TypeError("span_confidence: frame_conf must be a floating-point [B, T] tensor")
    B, T = frame_conf.shape
    if not isinstance(spans, torch.Tensor) or spans.dim() != 3 or spans.shape[0] != B or spans.shape[2] != 2:
        raise ValueError(f"span_confidence: spans must be [B={B}, L, 2], got "
                         f"{tuple(spans.shape) if isinstance(spans, torch.Tensor) else type(spans).__name__}")
    if spans.dtype.is_floating_point or spans.dtype == torch.bool:
        raise TypeError(f"span_confidence: spans must be an integer tensor, got {spans.dtype}")
    if not 1 <= T <= 4096:
        raise ValueError(f"span_confidence: need 1 <= T <= 4096, got T={T}")
    if frame_conf.is_cuda:
        from . import ops
        return ops.ctc_span_conf(_f32(frame_conf), spans, input_lengths, aggregation)
    ln = _host_lengths("span_confidence", input_lengths, B, T)
    cf = frame_conf.detach().to(torch.float32).contiguous().numpy()
    sp = spans.detach().cpu().numpy()
    out = np.zeros((B, sp.shape[1]), np.float32)
    for b in range(B):
        for j in range(sp.shape[1]):
            out[b, j] = host_span_law(cf[b], sp[b, j, 0], sp[b, j, 1], ln[b], aggregation)
    return torch.from_numpy(out)


def utterance_confidence(token_conf: torch.Tensor, lengths, aggregation: str = "min") -> torch.Tensor:
    """``token_conf`` float32 [B, L], ``lengths`` [B] (tokens per utterance) -> float32 [B]: the span law over the tokens [0, L_b) (the
    same kernel); an utterance without tokens gives 0."""
    check_aggregation("utterance_confidence", aggregation)
    if not isinstance(token_conf, torch.Tensor) or token_conf.dim() != 2:
        raise TypeError("utterance_confidence: token_conf must be a [B, L] tensor")
    B, Lt = token_conf.shape
    if Lt == 0:
        return torch.zeros((B,), dtype=torch.float32, device=token_conf.device)
    whole = torch.zeros((B, 1, 2), dtype=torch.int32, device=token_conf.device)
    whole[:, :, 1] = Lt
    return span_confidence(token_conf, whole, lengths, aggregation)[:, 0]


def _host_greedy(ids_t, blank: int):
    """Per-frame argmax of one utterance [T_b] -> (ids, spans): repeats collapsed, blanks dropped, and the run behind each id."""
    ids, spans, prev = [], [], None
    for t, i in enumerate(ids_t):
        if i != prev:
            if spans and spans[-1][1] < 0:
                spans[-1][1] = t
            if i != blank:
                ids.append(i)
                spans.append([t, -1])
            prev = i
    if spans and spans[-1][1] < 0:
        spans[-1][1] = len(ids_t)
    return ids, spans


def greedy_timed(log_probs: torch.Tensor, blank: int, input_lengths=None, method: str = "tsallis", alpha: float = 0.33,
                 aggregation: str = "min", batch_first: bool = True) -> GreedyTimed:
    """Greedy CTC decoding that keeps what it has computed: the ids of ``beam_search.greedy_batch``, the frames behind each (the argmax path
    is the Viterbi path of its own labelling, so these are ``forced_align``'s spans for these ids), each token's confidence and the frame
    confidences, from ONE read of ``log_probs`` (av_ctc_greedy_timed); host tensors: the same laws in float32 numpy.  Everything stays on
    the input's device."""
    alpha = check_method("greedy_timed", method, alpha)
    check_aggregation("greedy_timed", aggregation)
    B, T, V = _rows("greedy_timed", log_probs, batch_first)
    blank = int(blank)
    if not 0 <= blank < V:
        raise ValueError(f"greedy_timed: blank {blank} outside [0, {V})")
    if log_probs.is_cuda:
        from . import ops
        return GreedyTimed(*ops.ctc_greedy_timed(_f32(log_probs), blank, input_lengths, method, alpha, aggregation, batch_first))
    ln = _host_lengths("greedy_timed", input_lengths, B, T)
    lp = _host_rows(log_probs, batch_first)
    conf = frame_confidence(torch.from_numpy(lp), torch.tensor(ln), method, alpha).numpy()
    arg = torch.argmax(torch.from_numpy(lp), dim=-1).tolist()
    ids = np.full((B, T), -1, np.int32)
    cnt = np.zeros((B,), np.int32)
    spans = np.full((B, T, 2), -1, np.int32)
    tok = np.zeros((B, T), np.float32)
    for b in range(B):
        i, sp = _host_greedy(arg[b][:ln[b]], blank)
        cnt[b] = len(i)
        ids[b, :len(i)] = i
        for j, (f, e) in enumerate(sp):
            spans[b, j] = (f, e)
            tok[b, j] = host_span_law(conf[b], f, e, ln[b], aggregation)
    return GreedyTimed(*(torch.from_numpy(a) for a in (ids, cnt, spans, tok, conf)))
