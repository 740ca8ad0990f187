"""Decoding helpers with the reference's names (beam_search.py:2-48).

``simple_beam_search`` there scores raw frame paths additively without prefix merging, so its best beam is
always the per-frame argmax path: it equals greedy CTC decoding (pinned in tests/golden).  This
version computes exactly that with one argmax over the whole [T,V] matrix and one host transfer instead of
T*beam_width ``.item()`` calls.

``prefix_beam_search`` is what the name promises: CTC prefix beam search without a language model (blank-ending and non-blank-ending
mass per prefix, equal prefixes merged), n-best, on the device kernels of csrc/ctc_beam.hip for GPU tensors and in numpy for host tensors.
With ``lm=`` (an lm.NGramLM over token ids) it is the same search with n-gram shallow fusion: the same kernel's other instantiation, and the
same function in numpy.  With ``bias=`` (a bias.ContextBias: phrases that are likely in this recording) it is the same search with contextual
phrase biasing, with or without ``lm``: the kernel's third instantiation, and again the same function in numpy."""
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


def _host_prefix_beam(lp: np.ndarray, W: int, blank: int, lm=None, alpha=0.0, beta=0.0, tokens=None, bias=None, w=0.0):
    """One utterance, float32 [T, V] -> (id lists, scores, g or None, k or None) of the surviving entries in descending score order.  The law and the
    order of csrc/ctc_beam.hip: per frame only the K best non-blank tokens (value descending, token ascending) are expanded, plus every
    extension that lands on a live prefix (compared by content), which is merged into that prefix's stay; candidate slot * (K + 1) + r
    (r = 0: stay, r >= 1: token of rank r - 1) is ranked by score, equal scores by candidate id.  Without ``lm`` K = min(W + 1, V - 1) and
    the score is p_b (+) p_nb.  With ``lm`` K = min(tokens, V - 1), an entry also carries g = sum over its tokens of
    (alpha s(token | tokens before) + beta), every operation rounded to float32 on its own, and the score is (p_b (+) p_nb) + g.  There is
    no g arithmetic at all without ``lm``: adding a zero would turn a score of -0.0 into +0.0.  With ``bias`` (with or without ``lm``;
    K = min(tokens, V - 1)) g above is g_lm, +0 throughout without ``lm``; an entry also carries the phrase automaton's state (node, k),
    it is ranked by (p_b (+) p_nb) + (g_lm + w * float32(k + |tail|)), and after the last frame the entries are ranked again (stable) by
    (p_b (+) p_nb) + (g_lm + w * float32(k)), which is the returned score (bias.py: the law)."""
    T, V = lp.shape
    fused = lm is not None or bias is not None
    K = min(tokens if fused else W + 1, V - 1)
    NEG = np.float32(-np.inf)
    cols = np.delete(np.arange(V), blank)
    order = np.argsort(-lp[:, cols], axis=1, kind="stable")[:, :K]           # stable: equal values keep the smaller token first
    top_t = cols[order]                                                       # [T, K]
    top_v = np.take_along_axis(lp, top_t, axis=1)
    prefixes = [()]
    pb, pnb = np.zeros(1, np.float32), np.full(1, NEG, np.float32)
    last = np.full(1, -1)
    if fused:
        g = np.zeros(1, np.float32)
    if lm is not None:
        alpha, beta = np.float32(alpha), np.float32(beta)
        ctx, s = [lm.start_ctx], functools.lru_cache(None)(lm.score_ctx)
    if bias is not None:
        w, state, depth = np.float32(w), [(0, 0)], bias.depth
        step = functools.lru_cache(None)(bias.step)
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
            if fused:
                cand_g = np.empty((n, K + 1), np.float32)
                cand_g[:, 0] = g
                for i in range(n):
                    for k in range(K):
                        cand_g[i, 1 + k] = g[i] if lm is None else g[i] + (alpha * s(ctx[i], int(top_t[t, k])) + beta)
                if bias is None:
                    score = score + cand_g
                else:
                    m = np.empty((n, K + 1), np.float32)
                    for i, (node, kb) in enumerate(state):
                        m[i, 0] = kb + depth[node]
                        for k in range(K):
                            nd, kk = step(node, kb, int(top_t[t, k]))
                            m[i, 1 + k] = kk + depth[nd]
                    score = score + (cand_g + w * m)
            ids = np.flatnonzero(~dead.ravel())
            ids = ids[np.argsort(-score.ravel()[ids], kind="stable")[:W]]
            src, r = np.divmod(ids, K + 1)
            prefixes = [prefixes[i] if k == 0 else prefixes[i] + (int(top_t[t, k - 1]),) for i, k in zip(src.tolist(), r.tolist())]
            if lm is not None:
                ctx = [ctx[i] if k == 0 else lm.push(ctx[i], int(top_t[t, k - 1])) for i, k in zip(src.tolist(), r.tolist())]
            if bias is not None:
                state = [state[i] if k == 0 else step(*state[i], int(top_t[t, k - 1])) for i, k in zip(src.tolist(), r.tolist())]
            if fused:
                g = cand_g.ravel()[ids]
            pb, pnb = cand_pb.ravel()[ids], cand_pnb.ravel()[ids]
            last = np.where(r == 0, last[src], top_t[t][np.maximum(r - 1, 0)])
        final = np.logaddexp(pb, pnb)
        if bias is not None:
            kb = np.array([k for _, k in state], np.int64)
            final = final + (g + w * kb.astype(np.float32))
            order = np.argsort(-final, kind="stable")
            prefixes, final, g, kb = [prefixes[i] for i in order], final[order], g[order], kb[order]
        elif lm is not None:
            final = final + g
    return ([list(p) for p in prefixes], [float(x) for x in final], (None if not fused else [float(x) for x in g]),
            (None if bias is None else [int(x) for x in kb]))


def _device_beam_launch(log_probs, lengths, W, blank, nbest, lm, lm_weight, token_bonus, tokens, bias=None, bias_weight=0.0):
    """[B, T, V] on the GPU -> the device tensors the kernels of csrc/ctc_beam.hip wrote, and no transfer: ids int32 [B, nbest, T], lengths
    int32 [B, nbest] (< 0: absent), scores fp32 [B, nbest], g fp32 [B, nbest] (with ``lm`` or ``bias``, else None) and the banked phrase
    counts int32 [B, nbest] (with ``bias``, else None)."""
    from . import _lib as L
    from . import ops
    B, T, V = log_probs.shape
    lp = log_probs.detach()
    if lp.dtype != torch.float32 or lp.stride(2) != 1 or lp.stride(1) < V or lp.stride(0) < T * lp.stride(1):
        lp = lp.float().contiguous()
    ln = None if lengths is None else lengths.to(device=lp.device, dtype=torch.long, non_blocking=True).contiguous()
    nbytes = L.ll(0)
    if lm is None and bias is None:
        L.check(L.lib().av_ctc_beam_workspace_bytes(B, T, V, W, L.C.byref(nbytes)), "av_ctc_beam_workspace_bytes")
    else:
        L.check(L.lib().av_ctc_beam_lm_workspace_bytes(B, T, V, W, tokens, L.C.byref(nbytes)), "av_ctc_beam_lm_workspace_bytes")
    ws = torch.empty((max(1, (nbytes.value + 7) // 8),), dtype=torch.int64, device=lp.device)
    out = torch.empty((B, nbest, T), dtype=torch.int32, device=lp.device)
    cnt = torch.empty((B, nbest), dtype=torch.int32, device=lp.device)
    sc = torch.empty((B, nbest), dtype=torch.float32, device=lp.device)
    gl = kb = None
    if bias is not None:
        d, db = (None if lm is None else lm.to_device(lp.device)), bias.to_device(lp.device)
        gl = torch.empty((B, nbest), dtype=torch.float32, device=lp.device)
        kb = torch.empty((B, nbest), dtype=torch.int32, device=lp.device)
        lm_args = (None, None, 0, 0, 0, -1, 0, 0.0, 0.0) if d is None else (ops.ptr(d.unigrams), ops.ptr(d.table), d.slots, d.order,
                                                                            d.vocab_size, d.bos, d.probe_bound, lm_weight, token_bonus)
        L.check(L.lib().av_ctc_beam_search_bias(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(ln), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                                ops.ptr(gl), ops.ptr(kb), ops.ptr(ws), ws.numel() * 8, B, T, V, blank, W, nbest, tokens,
                                                *lm_args, ops.ptr(db.nodes), ops.ptr(db.edges), db.node_count, db.slots, db.probe_bound,
                                                bias_weight, ops.stream()), "av_ctc_beam_search_bias")
    elif lm is None:
        L.check(L.lib().av_ctc_beam_search(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(ln), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                           ops.ptr(ws), ws.numel() * 8, B, T, V, blank, W, nbest, ops.stream()), "av_ctc_beam_search")
    else:
        d = lm.to_device(lp.device)
        gl = torch.empty((B, nbest), dtype=torch.float32, device=lp.device)
        L.check(L.lib().av_ctc_beam_search_lm(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(ln), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                              ops.ptr(gl), ops.ptr(ws), ws.numel() * 8, B, T, V, blank, W, nbest, tokens,
                                              ops.ptr(d.unigrams), ops.ptr(d.table), d.slots, d.order, d.vocab_size, d.bos, d.probe_bound,
                                              lm_weight, token_bonus, ops.stream()), "av_ctc_beam_search_lm")
    return out, cnt, sc, gl, kb


def _device_prefix_beam(log_probs, lengths, W, blank, nbest, lm, lm_weight, token_bonus, tokens, bias=None, bias_weight=0.0):
    """[B, T, V] on the GPU -> per utterance the lists of ids, of scores, (with ``lm`` or ``bias``, else None) of g and (with ``bias``, else
    None) of the banked phrase counts of its hypotheses.  The launches of ``_device_beam_launch`` and ONE transfer: an int32 block
    [B][nbest][T + 2 (+ 1) (+ 1)] of ids, then the length, then the bits of the score (and of g, and the count)."""
    B, T, V = log_probs.shape
    out, cnt, sc, gl, kb = _device_beam_launch(log_probs, lengths, W, blank, nbest, lm, lm_weight, token_bonus, tokens, bias, bias_weight)
    cols = [out, cnt[..., None], sc.view(torch.int32)[..., None]]
    if gl is not None:
        cols.append(gl.view(torch.int32)[..., None])
    if kb is not None:
        cols.append(kb[..., None])
    packed = torch.cat(cols, dim=2).cpu()
    cnt_h = packed[..., T].tolist()

    def floats(col):
        x = packed[..., col].contiguous().view(torch.float32).tolist()
        return [[x[b][k] for k in range(nbest) if cnt_h[b][k] >= 0] for b in range(B)]
    ids = [[packed[b, k, :cnt_h[b][k]].tolist() for k in range(nbest) if cnt_h[b][k] >= 0] for b in range(B)]
    counts = None if bias is None else [[packed[b, k, T + 3].item() for k in range(nbest) if cnt_h[b][k] >= 0] for b in range(B)]
    return ids, floats(T + 1), (None if lm is None and bias is None else floats(T + 2)), counts


def _beam_args(log_probs, beam_width, blank, lengths, nbest, lm, lm_weight, token_bonus, tokens, bias, bias_weight):
    """The validation ``prefix_beam_search`` and ``nbest_on_device`` share -> the normalised arguments."""
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
    if bias is None and bias_weight != 1.0:
        raise ValueError("prefix_beam_search: bias_weight needs bias=")
    if lm is None and (lm_weight != 0.5 or token_bonus != 0.0 or (tokens is not None and bias is None)):
        raise ValueError("prefix_beam_search: lm_weight, token_bonus and tokens need lm=")
    if lm is not None or bias is not None:
        tokens = W + 1 if tokens is None else int(tokens)
        if not 1 <= tokens <= 65:
            raise ValueError(f"prefix_beam_search: tokens {tokens} outside [1, 65]")
    if bias is not None:
        bias_weight = float(bias_weight)
        if bias.vocab_size != V or bias.blank != blank:
            raise ValueError(f"prefix_beam_search: the phrases are over {bias.vocab_size} ids with blank {bias.blank}, the log-probs over "
                             f"{V} with blank {blank}")
        if not abs(bias_weight) <= float(np.finfo(np.float32).max):          # NaN, an infinity, or one once it is a float32
            raise ValueError(f"prefix_beam_search: bias_weight {bias_weight} must be finite")
    if lm is not None:
        lm_weight, token_bonus = float(lm_weight), float(token_bonus)
        if lm.vocab_size != V or lm.blank != blank:
            raise ValueError(f"prefix_beam_search: the language model is over {lm.vocab_size} ids with blank {lm.blank}, the log-probs over "
                             f"{V} with blank {blank}")
        if not (np.isfinite(np.float32(lm_weight)) and np.isfinite(np.float32(token_bonus))):
            raise ValueError(f"prefix_beam_search: lm_weight {lm_weight} and token_bonus {token_bonus} must be finite")
    return log_probs, lengths, W, blank, nbest, lm_weight, token_bonus, tokens, bias_weight


def nbest_on_device(log_probs: torch.Tensor, beam_width=5, blank=0, lengths=None, nbest=1, lm=None, lm_weight=0.5, token_bonus=0.0, tokens=None,
                    bias=None, bias_weight=1.0):
    """``prefix_beam_search`` on a GPU tensor without its transfer: the same arguments and validation, the same kernels, and the result
    stays on the device - nothing is copied to the host and nothing synchronises.  -> (ids int32 [B, nbest, T], lens int32 [B, nbest],
    scores fp32 [B, nbest]), with ``lm`` also g fp32 [B, nbest], with ``bias`` g (zeros without ``lm``) and the phrase counts int32
    [B, nbest].  Row n of an utterance is its n-th best hypothesis; lens < 0 marks an absent one (fewer than ``nbest`` exist), ids at or
    past a length are unspecified.  This is the block ``error_rate.error_counts`` and ``ops.ctc_nbest_nll`` take as it is."""
    if not isinstance(log_probs, torch.Tensor) or not log_probs.is_cuda:
        raise RuntimeError("nbest_on_device: log_probs must be on the GPU; there is no CPU fallback (prefix_beam_search decodes host tensors)")
    log_probs, lengths, W, blank, nbest, lm_weight, token_bonus, tokens, bias_weight = _beam_args(
        log_probs, beam_width, blank, lengths, nbest, lm, lm_weight, token_bonus, tokens, bias, bias_weight)
    out, cnt, sc, gl, kb = _device_beam_launch(log_probs, lengths, W, blank, nbest, lm, lm_weight, token_bonus, tokens, bias, bias_weight)
    if bias is not None:
        return out, cnt, sc, gl, kb
    return (out, cnt, sc) if lm is None else (out, cnt, sc, gl)


def prefix_beam_search(log_probs: torch.Tensor, beam_width=5, blank=0, lengths=None, nbest=1, return_scores=False, lm=None, lm_weight=0.5,
                       token_bonus=0.0, tokens=None, bias=None, bias_weight=1.0):
    """CTC prefix beam search.  [B,T,V] (or [T,V] = one utterance) -> list of B id lists; ``nbest`` > 1: list of
    B lists of up to ``nbest`` id lists in descending score order (fewer where fewer hypotheses exist); ``return_scores``: (ids, scores)
    with the scores in the same nesting.  ``lengths`` [B]: frames to consume per item (0 gives the empty hypothesis with score 0).

    GPU tensor: the two kernels of csrc/ctc_beam.hip (strided views with contiguous rows are taken as they are) and ONE transfer of ids,
    lengths and scores.  Host tensor: the same law in float32 numpy.  Ties: equal scores are ordered by candidate id (ctc_beam.hip).

    ``lm`` = an lm.NGramLM over this vocabulary: shallow fusion (the search kernel's other instantiation, av_ctc_beam_search_lm; host
    tensors: the same law in numpy).  Hypotheses are ranked by acoustic score + g, g = sum over the tokens of
    (lm_weight * s(token | tokens before) + token_bonus); the returned score is that sum and ``return_scores`` gives (ids, scores, g).  A
    frame extends an entry by its ``tokens`` best non-blank acoustic tokens (1 <= tokens <= 65, default beam_width + 1) and by every token
    that leads to a live prefix.  Without ``lm`` lm_weight and token_bonus must keep their defaults, and so must ``tokens`` unless ``bias`` is given.

    ``bias`` = a bias.ContextBias over this vocabulary: contextual phrase biasing, with or without ``lm`` (the kernel's third
    instantiation, av_ctc_beam_search_bias; host tensors: the same law in numpy).  During the search a hypothesis is also credited
    ``bias_weight`` (float32 nats, finite, may be negative) for every token of a completed phrase and of a running partial match; after the
    last frame the credit of a partial match is taken back and the hypotheses are ranked again (the law: bias.py).  The returned score is
    acoustic score + g + bias_weight * count and ``return_scores`` gives (ids, scores, g, counts): g as above (zeros without ``lm``),
    counts = the tokens of completed phrases per hypothesis.  Biasing re-ranks among the ``tokens`` acoustically best tokens of a frame
    (and the live extensions); it does not inject tokens: raise ``tokens`` (<= 65) to let weaker phrase continuations in.  Without
    ``bias``, bias_weight must keep its default."""
    log_probs, lengths, W, blank, nbest, lm_weight, token_bonus, tokens, bias_weight = _beam_args(
        log_probs, beam_width, blank, lengths, nbest, lm, lm_weight, token_bonus, tokens, bias, bias_weight)
    B, T, V = log_probs.shape
    if log_probs.is_cuda:
        ids, scores, lms, counts = _device_prefix_beam(log_probs, lengths, W, blank, nbest, lm, lm_weight, token_bonus, tokens, bias, bias_weight)
    else:
        lp_h = log_probs.detach().to(torch.float32).numpy()
        ln_h = [T] * B if lengths is None else [min(max(int(x), 0), T) for x in lengths.tolist()]
        found = [_host_prefix_beam(np.ascontiguousarray(lp_h[b, :ln_h[b]]), W, blank, lm, lm_weight, token_bonus, tokens, bias, bias_weight)
                 for b in range(B)]
        ids, scores = [f[0][:nbest] for f in found], [f[1][:nbest] for f in found]
        lms = None if lm is None and bias is None else [f[2][:nbest] for f in found]
        counts = None if bias is None else [f[3][:nbest] for f in found]
    if nbest == 1:
        ids, scores = [i[0] for i in ids], [s[0] for s in scores]
        lms = None if lms is None else [g[0] for g in lms]
        counts = None if counts is None else [k[0] for k in counts]
    if not return_scores:
        return ids
    if bias is not None:
        return ids, scores, lms, counts
    return (ids, scores) if lm is None else (ids, scores, lms)


def fast_decode(ids, tokenizer):
    return "".join(tokenizer.id_to_token[i] for i in ids if i != tokenizer.blank_id and 0 <= i < tokenizer.vocab_size
                   ).replace("▁", " ").strip()
