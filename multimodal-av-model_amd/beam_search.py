"""Decoding helpers with the reference's names (beam_search.py:2-48).

``simple_beam_search`` there scores raw frame paths additively without prefix merging, so its best beam is
always the per-frame argmax path: it equals greedy CTC decoding (pinned in tests/golden).  This
version computes exactly that with one argmax over the whole [T,V] matrix and one host transfer instead of
T*beam_width ``.item()`` calls.

``prefix_beam_search`` is what the name promises: CTC prefix beam search without a language model (blank-ending and non-blank-ending
mass per prefix, equal prefixes merged), n-best, on the device kernels of csrc/ctc_beam.hip for GPU tensors and in numpy for host tensors.
With ``lm=`` (an lm.NGramLM over token ids) it is the same search with n-gram shallow fusion: the same kernel's other instantiation, and the
same function in numpy."""
from __future__ import annotations

import functools

import numpy as np
import torch


def simple_beam_search(log_probs: torch.Tensor, beam_width=5, blank=0):
    ids = torch.argmax(log_probs, dim=-1).tolist()
    out, prev = [], None
    for i in ids:
        if i != prev and i != blank:
            out.append(i)
        prev = i
    return out


def greedy_batch(log_probs: torch.Tensor, blank: int, lengths: torch.Tensor = None):
    """[B,T,V] -> list of B id lists.  On the GPU: argmax + collapse in one HIP kernel (decode.hip), only the collapsed ids and
    their counts travel to the host."""
    if log_probs.is_cuda and log_probs.dim() == 3 and log_probs.shape[1] <= 4096:
        from . import _lib as L
        from . import ops
        lp = log_probs.detach().float().contiguous()
        B, T, V = lp.shape
        out = torch.empty((B, T), dtype=torch.int32, device=lp.device)
        cnt = torch.empty((B,), dtype=torch.int32, device=lp.device)
        ln = None if lengths is None else lengths.to(device=lp.device, dtype=torch.long).contiguous()
        L.check(L.lib().av_ctc_greedy(ops.ptr(lp), ops.ptr(ln), ops.ptr(out), ops.ptr(cnt), B, T, V, int(blank), ops.stream()), "av_ctc_greedy")
        out_h, cnt_h = out.cpu(), cnt.cpu().tolist()
        return [out_h[i, :cnt_h[i]].tolist() for i in range(B)]
    ids = torch.argmax(log_probs, dim=-1).cpu().tolist()
    res = []
    for row in ids:
        out, prev = [], None
        for i in row:
            if i != prev and i != blank:
                out.append(i)
            prev = i
        res.append(out)
    return res


def _host_prefix_beam(lp: np.ndarray, W: int, blank: int, lm=None, alpha=0.0, beta=0.0, tokens=None):
    """One utterance, float32 [T, V] -> (id lists, scores, g or None) of the surviving entries in descending score order.  The law and the
    order of csrc/ctc_beam.hip: per frame only the K best non-blank tokens (value descending, token ascending) are expanded, plus every
    extension that lands on a live prefix (compared by content), which is merged into that prefix's stay; candidate slot * (K + 1) + r
    (r = 0: stay, r >= 1: token of rank r - 1) is ranked by score, equal scores by candidate id.  Without ``lm`` K = min(W + 1, V - 1) and
    the score is p_b (+) p_nb.  With ``lm`` K = min(tokens, V - 1), an entry also carries g = sum over its tokens of
    (alpha s(token | tokens before) + beta), every operation rounded to float32 on its own, and the score is (p_b (+) p_nb) + g.  There is
    no g arithmetic at all without ``lm``: adding a zero would turn a score of -0.0 into +0.0."""
    T, V = lp.shape
    K = min(W + 1 if lm is None else tokens, V - 1)
    NEG = np.float32(-np.inf)
    cols = np.delete(np.arange(V), blank)
    order = np.argsort(-lp[:, cols], axis=1, kind="stable")[:, :K]           # stable: equal values keep the smaller token first
    top_t = cols[order]                                                       # [T, K]
    top_v = np.take_along_axis(lp, top_t, axis=1)
    prefixes = [()]
    pb, pnb = np.zeros(1, np.float32), np.full(1, NEG, np.float32)
    last = np.full(1, -1)
    if lm is not None:
        alpha, beta = np.float32(alpha), np.float32(beta)
        ctx, g, s = [lm.start_ctx], np.zeros(1, np.float32), functools.lru_cache(None)(lm.score_ctx)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            row, n = lp[t], len(prefixes)
            tot = np.logaddexp(pb, pnb)
            cand_pb = np.full((n, K + 1), NEG, np.float32)
            cand_pnb = np.empty((n, K + 1), np.float32)
            cand_pb[:, 0] = tot + row[blank]
            cand_pnb[:, 0] = np.where(last >= 0, pnb + row[np.maximum(last, 0)], NEG)
            cand_pnb[:, 1:] = np.where(top_t[t][None, :] == last[:, None], pb[:, None], tot[:, None]) + top_v[t][None, :]
            dead = np.zeros((n, K + 1), bool)
            dead[:, 1:] = np.isnan(top_v[t])[None, :]
            if n > 1:
                slot = {p: i for i, p in enumerate(prefixes)}
                rank = {int(c): r for r, c in enumerate(top_t[t])}
                for j, p in enumerate(prefixes):
                    i = slot.get(p[:-1]) if p else None
                    if i is None:
                        continue
                    c = p[-1]                                                  # prefixes[i] + c is prefixes[j]: merge, and drop the duplicate
                    cand_pnb[j, 0] = np.logaddexp(cand_pnb[j, 0], (pb[i] if last[i] == c else tot[i]) + row[c])
                    if c in rank:
                        dead[i, 1 + rank[c]] = True
            score = np.logaddexp(cand_pb, cand_pnb)
            if lm is not None:
                cand_g = np.empty((n, K + 1), np.float32)
                cand_g[:, 0] = g
                for i in range(n):
                    for k in range(K):
                        cand_g[i, 1 + k] = g[i] + (alpha * s(ctx[i], int(top_t[t, k])) + beta)
                score = score + cand_g
            ids = np.flatnonzero(~dead.ravel())
            ids = ids[np.argsort(-score.ravel()[ids], kind="stable")[:W]]
            src, r = np.divmod(ids, K + 1)
            prefixes = [prefixes[i] if k == 0 else prefixes[i] + (int(top_t[t, k - 1]),) for i, k in zip(src.tolist(), r.tolist())]
            if lm is not None:
                ctx = [ctx[i] if k == 0 else lm.push(ctx[i], int(top_t[t, k - 1])) for i, k in zip(src.tolist(), r.tolist())]
                g = cand_g.ravel()[ids]
            pb, pnb = cand_pb.ravel()[ids], cand_pnb.ravel()[ids]
            last = np.where(r == 0, last[src], top_t[t][np.maximum(r - 1, 0)])
        final = np.logaddexp(pb, pnb)
        if lm is not None:
            final = final + g
    return [list(p) for p in prefixes], [float(x) for x in final], (None if lm is None else [float(x) for x in g])


def _device_prefix_beam(log_probs, lengths, W, blank, nbest, lm, lm_weight, token_bonus, tokens):
    """[B, T, V] on the GPU -> per utterance the lists of ids, of scores and (with ``lm``, else None) of g of its hypotheses.  The kernels of
    csrc/ctc_beam.hip and ONE transfer: an int32 block [B][nbest][T + 2 (+ 1)] of ids, then the length, then the bits of the score (and of g)."""
    from . import _lib as L
    from . import ops
    B, T, V = log_probs.shape
    lp = log_probs.detach()
    if lp.dtype != torch.float32 or lp.stride(2) != 1 or lp.stride(1) < V or lp.stride(0) < T * lp.stride(1):
        lp = lp.float().contiguous()
    ln = None if lengths is None else lengths.to(device=lp.device, dtype=torch.long).contiguous()
    nbytes = L.ll(0)
    if lm is None:
        L.check(L.lib().av_ctc_beam_workspace_bytes(B, T, V, W, L.C.byref(nbytes)), "av_ctc_beam_workspace_bytes")
    else:
        L.check(L.lib().av_ctc_beam_lm_workspace_bytes(B, T, V, W, tokens, L.C.byref(nbytes)), "av_ctc_beam_lm_workspace_bytes")
    ws = torch.empty((max(1, (nbytes.value + 7) // 8),), dtype=torch.int64, device=lp.device)
    out = torch.empty((B, nbest, T), dtype=torch.int32, device=lp.device)
    cnt = torch.empty((B, nbest), dtype=torch.int32, device=lp.device)
    sc = torch.empty((B, nbest), dtype=torch.float32, device=lp.device)
    cols = [out, cnt[..., None], sc.view(torch.int32)[..., None]]
    if lm is None:
        L.check(L.lib().av_ctc_beam_search(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(ln), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                           ops.ptr(ws), ws.numel() * 8, B, T, V, blank, W, nbest, ops.stream()), "av_ctc_beam_search")
    else:
        d = lm.to_device(lp.device)
        gl = torch.empty((B, nbest), dtype=torch.float32, device=lp.device)
        L.check(L.lib().av_ctc_beam_search_lm(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(ln), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                              ops.ptr(gl), ops.ptr(ws), ws.numel() * 8, B, T, V, blank, W, nbest, tokens,
                                              ops.ptr(d.unigrams), ops.ptr(d.table), d.slots, d.order, d.vocab_size, d.bos, d.probe_bound,
                                              lm_weight, token_bonus, ops.stream()), "av_ctc_beam_search_lm")
        cols.append(gl.view(torch.int32)[..., None])
    packed = torch.cat(cols, dim=2).cpu()
    cnt_h = packed[..., T].tolist()

    def floats(col):
        x = packed[..., col].contiguous().view(torch.float32).tolist()
        return [[x[b][k] for k in range(nbest) if cnt_h[b][k] >= 0] for b in range(B)]
    ids = [[packed[b, k, :cnt_h[b][k]].tolist() for k in range(nbest) if cnt_h[b][k] >= 0] for b in range(B)]
    return ids, floats(T + 1), (None if lm is None else floats(T + 2))


def prefix_beam_search(log_probs: torch.Tensor, beam_width=5, blank=0, lengths=None, nbest=1, return_scores=False, lm=None, lm_weight=0.5,
                       token_bonus=0.0, tokens=None):
    """CTC prefix beam search.  [B,T,V] (or [T,V] = one utterance) -> list of B id lists; ``nbest`` > 1: list of
    B lists of up to ``nbest`` id lists in descending score order (fewer where fewer hypotheses exist); ``return_scores``: (ids, scores)
    with the scores in the same nesting.  ``lengths`` [B]: frames to consume per item (0 gives the empty hypothesis with score 0).

    GPU tensor: the two kernels of csrc/ctc_beam.hip (strided views with contiguous rows are taken as they are) and ONE transfer of ids,
    lengths and scores.  Host tensor: the same law in float32 numpy.  Ties: equal scores are ordered by candidate id (ctc_beam.hip).

    ``lm`` = an lm.NGramLM over this vocabulary: shallow fusion (the search kernel's other instantiation, av_ctc_beam_search_lm; host
    tensors: the same law in numpy).  Hypotheses are ranked by acoustic score + g, g = sum over the tokens of
    (lm_weight * s(token | tokens before) + token_bonus); the returned score is that sum and ``return_scores`` gives (ids, scores, g).  A
    frame extends an entry by its ``tokens`` best non-blank acoustic tokens (1 <= tokens <= 65, default beam_width + 1) and by every token
    that leads to a live prefix.  Without ``lm`` the three arguments must keep their defaults."""
    W, nbest, blank = int(beam_width), int(nbest), int(blank)
    if log_probs.dim() == 2:
        log_probs = log_probs[None]
    if log_probs.dim() != 3:
        raise ValueError(f"prefix_beam_search: log_probs must be [B, T, V] or [T, V], got shape {tuple(log_probs.shape)}")
    B, T, V = log_probs.shape
    if not 1 <= W <= 64 or not 1 <= nbest <= W:
        raise ValueError(f"prefix_beam_search: need 1 <= nbest <= beam_width <= 64, got beam_width={W} nbest={nbest}")
    if V < 2 or not 0 <= blank < V or not 1 <= T <= 4096:
        raise ValueError(f"prefix_beam_search: need V >= 2, 0 <= blank < V and 1 <= T <= 4096, got T={T} V={V} blank={blank}")
    if lengths is not None and (not isinstance(lengths, torch.Tensor) or lengths.numel() != B):
        lengths = torch.as_tensor(lengths, dtype=torch.long).reshape(B)
    if lm is None:
        if tokens is not None or lm_weight != 0.5 or token_bonus != 0.0:
            raise ValueError("prefix_beam_search: lm_weight, token_bonus and tokens need lm=")
    else:
        tokens = W + 1 if tokens is None else int(tokens)
        lm_weight, token_bonus = float(lm_weight), float(token_bonus)
        if not 1 <= tokens <= 65:
            raise ValueError(f"prefix_beam_search: tokens {tokens} outside [1, 65]")
        if lm.vocab_size != V or lm.blank != blank:
            raise ValueError(f"prefix_beam_search: the language model is over {lm.vocab_size} ids with blank {lm.blank}, the log-probs over "
                             f"{V} with blank {blank}")
        if not (np.isfinite(np.float32(lm_weight)) and np.isfinite(np.float32(token_bonus))):
            raise ValueError(f"prefix_beam_search: lm_weight {lm_weight} and token_bonus {token_bonus} must be finite")
    if log_probs.is_cuda:
        ids, scores, lms = _device_prefix_beam(log_probs, lengths, W, blank, nbest, lm, lm_weight, token_bonus, tokens)
    else:
        lp_h = log_probs.detach().to(torch.float32).numpy()
        ln_h = [T] * B if lengths is None else [min(max(int(x), 0), T) for x in lengths.tolist()]
        found = [_host_prefix_beam(np.ascontiguousarray(lp_h[b, :ln_h[b]]), W, blank, lm, lm_weight, token_bonus, tokens) for b in range(B)]
        ids, scores = [i[:nbest] for i, _, _ in found], [s[:nbest] for _, s, _ in found]
        lms = None if lm is None else [g[:nbest] for _, _, g in found]
    if nbest == 1:
        ids, scores = [i[0] for i in ids], [s[0] for s in scores]
        lms = None if lms is None else [g[0] for g in lms]
    if not return_scores:
        return ids
    return (ids, scores) if lm is None else (ids, scores, lms)


def fast_decode(ids, tokenizer):
    return "".join(tokenizer.id_to_token[i] for i in ids if i != tokenizer.blank_id and 0 <= i < tokenizer.vocab_size
                   ).replace("▁", " ").strip()
