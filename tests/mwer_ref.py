"""The float64 reference of the MWER law (mwer.py) in plain torch, never through the package's kernels or its mwer module:
torch.nn.functional.ctc_loss(reduction="none") on log-probs expanded N times with repeat_interleave, out-masking, softmax over the
hypotheses that are left, and the risk with the mean-error baseline.  The error counts are handed in (the tests take them from
tests/error_ref.py or from the package's host path, which test_error_rate_cpu.py ties to it).

Out items: torch's ctc_loss with zero_infinity=False decides which items have no path (its value is +inf); its gradient at such an item is
NaN even under a zero upstream gradient, so the differentiated call is the same function with zero_infinity=True, whose values are equal at
every other item.  An absent hypothesis (length < 0), one longer than the lattice (length > max_len) and one with an id outside [0, V)
never reach torch: they are replaced by the empty label row and masked."""
import torch
import torch.nn.functional as F

INF = float("inf")


def nbest_nll(log_probs, ids, lens, input_lengths, blank, max_len=None, dtype=torch.float64):
    """log_probs [B, T, V] (a leaf or any tensor; upcast to ``dtype``), ids int [B, N, Lh], lens [B, N], input_lengths [B] ->
    (nll [B, N] with +inf at out items, differentiable with respect to ``log_probs``; out bool [B, N])."""
    B, T, V = log_probs.shape
    N, Lh = ids.shape[1], ids.shape[2]
    max_len = Lh if max_len is None else max_len
    ids, lens = ids.long().cpu(), torch.as_tensor(lens).long().cpu().reshape(B, N)
    inside = torch.arange(Lh)[None, None, :] < lens[..., None]
    out = (lens < 0) | (lens > max_len) | (inside & ((ids < 0) | (ids >= V))).any(-1)
    tg = torch.where(inside & ~out[..., None], ids, torch.zeros_like(ids)).reshape(B * N, Lh)
    if Lh == 0:
        tg = torch.zeros((B * N, 1), dtype=torch.long)
    tl = torch.where(out, torch.zeros_like(lens), lens).reshape(B * N)
    il = torch.as_tensor(input_lengths).long().cpu().clamp(0, T).repeat_interleave(N)
    lp = log_probs.to(dtype).repeat_interleave(N, 0).transpose(0, 1)
    with torch.no_grad():
        out = out | torch.isinf(F.ctc_loss(lp, tg, il, tl, blank=blank, reduction="none", zero_infinity=False)).reshape(B, N)
    nll = F.ctc_loss(lp, tg, il, tl, blank=blank, reduction="none", zero_infinity=True).reshape(B, N)
    return torch.where(out, torch.full_like(nll, INF), nll), out


def risk(nll, errors, counted):
    """nll [B, N] (+inf = out), errors int [B, N], counted bool [B, N] (False where the count is -1) -> (risk [B], posterior [B, N])."""
    live = counted & torch.isfinite(nll)
    rows, posts = [], []
    for b in range(nll.shape[0]):
        k = torch.nonzero(live[b]).reshape(-1)
        post = torch.zeros_like(nll[b])
        if k.numel() == 0:
            rows.append(nll.new_zeros(()))
        else:
            p = torch.softmax(-nll[b, k], 0)
            e = errors[b, k].to(nll.dtype)
            rows.append((p * (e - e.mean())).sum())
            post = post.index_put((k,), p)
        posts.append(post)
    return torch.stack(rows), torch.stack(posts)


def mwer(log_probs, ids, lens, input_lengths, blank, errors, counted, reduction="mean", dtype=torch.float64):
    """The whole law for given hypotheses and error counts -> (loss, details) with the float64 graph back to ``log_probs``."""
    nll, _ = nbest_nll(log_probs, ids, lens, input_lengths, blank, dtype=dtype)
    r, post = risk(nll, errors.cpu(), counted.cpu())
    loss = r if reduction == "none" else (r.sum() if reduction == "sum" else r.mean())
    return loss, {"nll": nll.detach(), "posterior": post.detach(), "risk": r.detach()}
