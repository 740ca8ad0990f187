"""The measuring stick of the attention tests (test_attention_matrix_gpu.py, test_attention_ref_cpu.py): one statement of masked,
dropped-out attention and its gradients, written twice in plain PyTorch - no autograd, no call into the library.

Layout: q, do, o, dq are [B, Tq, H, D]; k, v, dk, dv are [B, Tk, H, D] (the library's views); lse is [B, H, Tq]; ``mult`` is the dropout
multiplier [B, H, Tq, Tk] (0 for a dropped probability, 1 / keep fraction for a survivor; None = ones).  ``klen`` [B] is clamped to
[1, Tk] - the one rule every kernel follows - and keys >= klen get a score of -inf.

    S = scale q k^T      P = softmax(S)      lse = logsumexp(S)      o = (P o mult) v
    dV = (P o mult)^T do      dP = (do v^T) o mult      dS = scale P o (dP - rowsum(dP o P))      dQ = dS k      dK = dS^T q
"""
import torch

EPS32 = 2.0 ** -23
FACTOR = 4.0                                           # ours <= FACTOR x the error of the same-precision emulation (as test_ctc_native_gpu.py)
SCALE_TOL = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}      # half an ulp of the output type as a relative factor
SCALE_MIN_NUMEL = 4096
OUTS = ("o", "dq", "dk", "dv")

# The shapes of the GPU matrix (test_attention_matrix_gpu.py says which dispatcher branch each list is for); test_attention_ref_cpu.py
# runs the emulation over the same list.
WHOLE_TK = [1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 199, 224, 225, 255, 256]      # D = 64: every NKP = ceil(Tk / 32) at both edges
WHOLE_CROSS = [(70, 130), (130, 70), (17, 256), (256, 17), (1, 199), (199, 1)]
CHUNKED = [(257, 257), (384, 384), (385, 385), (749, 749), (130, 600), (600, 130), (300, 257)]         # D = 64, chunks of 128 keys
CHUNKED_KLEN = [129, 256, 100]                         # one key into the second chunk, a chunk edge, inside the first chunk (item 0: whole)
TILED = [(D, T, T) for D in (16, 32, 128) for T in (25, 64, 65, 100)] + [(128, 375, 375), (128, 70, 130)]
MISALIGNED_T = [49, 199, 300]                          # D = 64 through the alignment fallback


def klens(Tk, B):
    """[Tk, a value in the middle of a 16-key tile, a multiple of 16] (+ Tk for further items), inside [1, Tk]."""
    c = lambda x: min(max(1, x), Tk)
    return ([Tk, c(Tk // 2 // 16 * 16 + 7), c(max(16, 3 * Tk // 4 // 16 * 16))] + [Tk] * B)[:B]


def batch_heads(Tmin, D, B=3):
    """B, H such that every output tensor has at least 4096 elements (so the scale check applies to all of them)."""
    if Tmin == 1:
        return 4, SCALE_MIN_NUMEL // (4 * D)
    for H in (2, 4, 8, 16):
        if B * H * Tmin * D >= SCALE_MIN_NUMEL:
            return B, H
    raise AssertionError((Tmin, D, B))


def matrix_shapes():
    """(B, H, Tq, Tk, D, klen) of every 16-bit attention case of the GPU matrix."""
    out = []
    for Tq, Tk in [(T, T) for T in WHOLE_TK] + WHOLE_CROSS:
        B, H = batch_heads(min(Tq, Tk), 64)
        out.append((B, H, Tq, Tk, 64, klens(Tk, B)))
    out += [(4, 2, Tq, Tk, 64, [Tk] + CHUNKED_KLEN) for Tq, Tk in CHUNKED]
    for D, Tq, Tk in TILED:
        B, H = batch_heads(min(Tq, Tk), D)
        out.append((B, H, Tq, Tk, D, klens(Tk, B)))
    out += [(3, 2, T, T, 64, klens(T, 3)) for T in MISALIGNED_T]
    return out


def _statement(q, k, v, do, klen, scale, mult, wt, rnd, delta_from_o=False):
    """The statement above in working type ``wt``; ``rnd`` is applied where a 16-bit kernel has to round.  ``delta_from_o``: the row sum
    rowsum(dP o P) is taken as rowsum(do o o) from the ROUNDED o (the same number exactly: sum_k mult P (do . v_k) = do . o)."""
    q, k, v, do = (t.to(wt).permute(0, 2, 1, 3) for t in (q, k, v, do))          # [B, H, T, D]
    Tk = k.shape[2]
    S = (q @ k.transpose(2, 3)) * scale
    if klen is not None:
        kl = klen.to(S.device).long().clamp(1, Tk)
        dead = torch.arange(Tk, device=S.device)[None, :] >= kl[:, None]
        S = S.masked_fill(dead[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(S, -1)
    P = torch.softmax(S, -1)
    M = torch.ones_like(P) if mult is None else mult.to(wt)
    Pm = rnd(P * M)
    o = rnd(Pm @ v)
    dv = rnd(Pm.transpose(2, 3) @ do)
    dP = (do @ v.transpose(2, 3)) * M
    delta = (do * o).sum(-1, keepdim=True) if delta_from_o else (dP * P).sum(-1, keepdim=True)
    dS = rnd(scale * P * (dP - delta))
    dq = rnd(dS @ k)
    dk = rnd(dS.transpose(2, 3) @ q)
    smax = S[torch.isfinite(S)].abs().max()
    back = lambda t: t.permute(0, 2, 1, 3).contiguous()
    return dict(o=back(o), lse=lse, dq=back(dq), dk=back(dk), dv=back(dv), smax=float(smax))


def ref64(q, k, v, do, klen, scale, mult=None):
    """Everything in float64, nothing rounded."""
    return _statement(q, k, v, do, klen, scale, mult, torch.float64, lambda t: t)


def emul(lp, q, k, v, do, klen, scale, mult=None):
    """The same statement in float32 with the 16-bit operand type ``lp`` applied where a kernel must round: P o mult, o, dS, dQ, dK, dV
    are each rounded to ``lp`` and back (products of 16-bit operands are exact in float32, sums are float32: an MFMA's arithmetic).
    Its distance to ref64 is e_ref, the error a correct kernel of this precision is expected to have.

    One rounding point beyond that list, added because the kernels have it: a backward that does not keep the T x T probabilities reads
    the row sum of dS as delta = rowsum(do o o) from the forward's 16-bit o, so the rounding of o enters dS un-attenuated where the
    softmax is peaked.  Measured on the device with p = 0.1 and one valid key (P = 1, o = round(mult v)): dk off by 0.12 (bfloat16) /
    0.016 (float16) in every kernel family, 6 .. 9 x the e_ref of an emulation that sums dP o P instead; with it the ratio is about 1."""
    return _statement(q, k, v, do, klen, scale, mult, torch.float32, lambda t: t.to(lp).to(torch.float32), delta_from_o=True)


def max_err(a, b):
    return float((a.double() - b.double()).abs().max())


def scale_dev(ours, ref):
    """|s - 1| of the least-squares factor s = <ours, ref> / <ref, ref>: what a max-error gate cannot see."""
    a, b = ours.double().flatten(), ref.double().flatten()
    return abs(float((a * b).sum() / (b * b).sum()) - 1.0)


def zero_bound(q, k, v, do, scale):
    """Bound of the rounding residue of an output whose exact value is identically zero (one valid key: softmax = 1, dS = 0): the terms
    that cancel have size A = scale D max|do| max|v| max(max|q|, max|k|); the float32 residue is allowed 64 eps32 A.  Without dropout
    o = v exactly and the residue is float32 summation order only (e_ref is of that size too, so 4 x e_ref is no gate); with dropout
    o = round(mult v) and the residue has 16-bit size, in the emulation as in a kernel: the gate is max(4 e_ref, 64 eps32 A)."""
    mx = lambda t: float(t.double().abs().max())
    return 64.0 * EPS32 * scale * q.shape[-1] * mx(do) * mx(v) * max(mx(q), mx(k))


def lse_gate(e_ref_lse, smax):
    return max(FACTOR * e_ref_lse, 64.0 * EPS32 * max(1.0, smax))


def judge(lp, ours, r64, em, zero_tol):
    """Apply the rule to one case.  ``ours`` / ``r64`` / ``em``: dicts with o, dq, dk, dv (+ lse where ours has one).  Returns
    (rows, failures): rows = (name, err, e_ref, ratio, scale deviation or None) for printing, failures = list of messages."""
    rows, bad = [], []
    for n in OUTS:
        if n not in ours:
            continue
        x = ours[n]
        if not bool(torch.isfinite(x.float()).all()):
            bad.append(f"{n}: non-finite values")
            continue
        err, e_ref = max_err(x, r64[n]), max_err(em[n], r64[n])
        if float(r64[n].abs().max()) == 0.0:                                     # the exact-zero corner
            rows.append((n, err, e_ref, err / max(FACTOR * e_ref, zero_tol) * FACTOR, None))
            if err > max(FACTOR * e_ref, zero_tol):
                bad.append(f"{n}: exact value is zero, residue {err:.3e} > max(4 x e_ref {e_ref:.3e}, {zero_tol:.3e})")
            continue
        ratio = err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))
        sd = scale_dev(x, r64[n]) if x.numel() >= SCALE_MIN_NUMEL else None
        rows.append((n, err, e_ref, ratio, sd))
        if not err <= FACTOR * e_ref:
            bad.append(f"{n}: err {err:.3e} > {FACTOR:g} x e_ref {e_ref:.3e} (ratio {ratio:.2f})")
        if sd is not None and not sd <= SCALE_TOL[lp]:
            bad.append(f"{n}: scale factor off by {sd:.3e} > {SCALE_TOL[lp]:.3e}")
    if ours.get("lse") is not None:
        x = ours["lse"]
        err, e_ref = max_err(x, r64["lse"]), max_err(em["lse"], r64["lse"])
        gate = lse_gate(e_ref, r64["smax"])
        rows.append(("lse", err, e_ref, err / gate, None))
        if not (bool(torch.isfinite(x).all()) and err <= gate):
            bad.append(f"lse: err {err:.3e} > gate {gate:.3e}")
    return rows, bad


def fmt(rows):
    out = []
    for n, err, e_ref, ratio, sd in rows:
        s = f"{n} {err:.2e}/{e_ref:.2e}={ratio:.2f}"
        if sd is not None:
            s += f" |s-1|={sd:.1e}"
        out.append(s)
    return "  ".join(out)
