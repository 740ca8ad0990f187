"""Minimum word error rate (MWER) training: the expected number of word errors of an n-best list under the model's own posterior over that
list, as a loss on the log-probs of the CTC head.  On the device it is a composition of the pieces the evaluation side already has - the
n-best prefix beam search (csrc/ctc_beam.hip), the error counts (csrc/error_counts.hip) and the n-best form of the CTC loss
(csrc/ctc_loss.hip: av_ctc_nbest_fwd / _bwd) - on [B, N] tensors that never leave the device: nothing synchronises.

The law, for log_probs [B, T, V], references ``refs`` [B, Lr] with ``ref_lengths`` and frame counts ``input_lengths``:

  1. hypotheses   (ids [B, N, Lh], lens [B, N]) = ``hyps`` if given, else nbest_on_device(log_probs.detach(), beam_width, blank,
                  input_lengths, nbest): the search is not differentiated.  lens < 0 = absent.
  2. errors       E[b, n] = S + D + I of error_counts(refs, ids, ref_lengths, lens, table=table, ref_skip=blank, hyp_skip=blank) at
                  ``level`` ("word" / "char": through the PieceTable; "token": the ids).  A count of -1 makes the hypothesis out.
  3. posterior    nll[b, n] = the exact CTC negative log-likelihood of hypothesis n (ops.ctc_nbest_nll; +inf = out: absent, longer than
                  the id block, an id outside [0, V), or no path);  P^[b, :] = softmax of -nll over the hypotheses that are not out - the
                  exact posterior renormalised over the list, not the search's score (which is only the mass the search kept).
  4. risk         risk[b] = sum_n P^[b, n] (E[b, n] - E~[b]),  E~[b] = the mean of E over the hypotheses that are not out: the usual
                  baseline, which leaves the gradient unchanged (sum_n dP^ = 0).  An utterance with no hypothesis left has risk 0 and a
                  zero gradient (no NaN from a softmax over nothing).
  5. reduction    "mean" over the batch, "sum" or "none".
  6. details      ``return_details``: (loss, {"ids", "lens", "nll", "posterior", "errors"}), tensors on the device of ``log_probs``.

Steps 2 - 5 are ordinary torch operations on [B, N] tensors; autograd differentiates them down to the gradient at nll, which
av_ctc_nbest_bwd turns into ONE [B, T, V] gradient.  Host tensors run the same law with the host beam search, the host error counts and
torch's ``ctc_loss`` on log-probs expanded N times."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .beam_search import nbest_on_device, prefix_beam_search
from .error_rate import LEVELS, error_counts


def _host_hyps(log_probs, beam_width, blank, input_lengths, nbest):
    B, T, _ = log_probs.shape
    found = prefix_beam_search(log_probs.detach(), beam_width, blank, lengths=input_lengths, nbest=nbest)
    if nbest == 1:
        found = [[h] for h in found]
    ids = torch.zeros((B, nbest, T), dtype=torch.int32)
    lens = torch.full((B, nbest), -1, dtype=torch.int32)
    for b, hs in enumerate(found):
        for n, h in enumerate(hs):
            lens[b, n] = len(h)
            if h:
                ids[b, n, :len(h)] = torch.as_tensor(h, dtype=torch.int32)
    return ids, lens


def _host_nbest_nll(log_probs, ids, lens, input_lengths, blank):
    """ops.ctc_nbest_nll's law on the host: torch's ctc_loss on log-probs expanded N times, out items +inf and without a gradient."""
    B, T, V = log_probs.shape
    N, Lh = ids.shape[1], ids.shape[2]
    ids, lens = ids.long(), lens.long()
    inside = torch.arange(Lh)[None, None, :] < lens[..., None]
    out = (lens < 0) | (lens > Lh) | (inside & ((ids < 0) | (ids >= V))).any(-1)
    tg = torch.where(inside & ~out[..., None], ids, torch.zeros_like(ids)).reshape(B * N, Lh)
    tl = torch.where(out, torch.zeros_like(lens), lens).reshape(B * N)
    il = torch.as_tensor(input_lengths).long().clamp(0, T).repeat_interleave(N)
    lp = log_probs.repeat_interleave(N, 0).transpose(0, 1)
    if Lh == 0:
        tg = torch.zeros((B * N, 1), dtype=torch.long)
    with torch.no_grad():                                  # which items have no path: an infinite loss would leave NaN in torch's gradient
        out = out | torch.isinf(F.ctc_loss(lp, tg, il, tl, blank=blank, reduction="none", zero_infinity=False)).reshape(B, N)
    nll = F.ctc_loss(lp, tg, il, tl, blank=blank, reduction="none", zero_infinity=True).reshape(B, N)
    return torch.where(out, torch.full_like(nll, float("inf")), nll)


def risk_from_nll(nll: torch.Tensor, errors: torch.Tensor, counted: torch.Tensor):
    """Steps 3 and 4 of the law on [B, N] tensors: -> (risk [B], posterior [B, N], live [B, N]).  ``counted`` is False where the error
    count is -1.  Every intermediate is finite, so no NaN can appear in the values or in the gradient at ``nll``."""
    live = counted & torch.isfinite(nll)
    z = torch.where(live, -nll, torch.zeros_like(nll))
    m = torch.where(live, z, torch.full_like(z, float("-inf"))).amax(1, keepdim=True).detach()
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(z - m) * live
    den = e.sum(1, keepdim=True)
    post = e / torch.where(den > 0, den, torch.ones_like(den))
    E = torch.where(live, errors.to(nll.dtype), torch.zeros_like(nll))
    mean = E.sum(1, keepdim=True) / live.sum(1, keepdim=True).clamp_min(1).to(nll.dtype)
    risk = (post * (E - mean) * live).sum(1)
    return risk, post, live


def mwer_loss(log_probs, refs, ref_lengths, input_lengths, blank, *, nbest=4, beam_width=8, table=None, level="word", hyps=None,
              reduction="mean", return_details=False):
    """The MWER loss of the module docstring.  ``log_probs`` float [B, T, V] (GPU: float32, the kernels have no CPU fallback and host
    tensors run the host law), ``refs`` integer [B, Lr], ``ref_lengths`` [B], ``input_lengths`` [B]; ``table``: the tokenizer's
    ``error_rate.PieceTable`` (needed for ``level`` "word" and "char"); ``hyps`` = (ids integer [B, N, Lh], lens [B, N]) replaces the
    search and is used verbatim.  For GPU inputs the forward and the backward hold no synchronising call."""
    if level not in LEVELS:
        raise ValueError(f"mwer_loss: level must be one of {LEVELS}, got {level!r}")
    if level != "token" and table is None:
        raise ValueError(f"mwer_loss: level {level!r} needs table= (error_rate.PieceTable of the tokenizer)")
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"mwer_loss: reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
    if not isinstance(log_probs, torch.Tensor) or log_probs.dim() != 3:
        raise ValueError("mwer_loss: log_probs must be a tensor [B, T, V]")
    nbest, beam_width, blank = int(nbest), int(beam_width), int(blank)
    dev = log_probs.device
    if hyps is None:
        if dev.type == "cuda":
            ids, lens = nbest_on_device(log_probs.detach(), beam_width, blank, input_lengths, nbest)[:2]
        else:
            ids, lens = _host_hyps(log_probs, beam_width, blank, input_lengths, nbest)
    else:
        ids, lens = hyps
        ids, lens = ids.to(dev, non_blocking=True), torch.as_tensor(lens).to(dev, non_blocking=True)
        if ids.dim() != 3 or ids.shape[0] != log_probs.shape[0] or lens.shape != ids.shape[:2]:
            raise ValueError(f"mwer_loss: hyps must be (ids [B, N, Lh], lens [B, N]), got {tuple(ids.shape)} and {tuple(lens.shape)}")
    refs = refs.to(dev, non_blocking=True)
    counts = error_counts(refs, ids, ref_lengths, lens, table=table, ref_skip=blank, hyp_skip=blank)[:, :, LEVELS.index(level)]
    errors, counted = counts[..., :3].sum(-1), counts[..., 3] >= 0
    if dev.type == "cuda":
        from . import ops
        nll = ops.ctc_nbest_nll(log_probs, ids, lens, input_lengths, blank=blank, batch_first=True)
    else:
        nll = _host_nbest_nll(log_probs, ids, lens, input_lengths, blank)
    risk, post, _ = risk_from_nll(nll, errors, counted)
    loss = risk if reduction == "none" else (risk.sum() if reduction == "sum" else risk.mean())
    if not return_details:
        return loss
    return loss, {"ids": ids, "lens": lens, "nll": nll.detach(), "posterior": post.detach(), "errors": errors}
