"""The references of the attention tests are the measuring stick, so they are tested themselves (no GPU, no library): ref64 against
torch's own scaled_dot_product_attention and float64 autograd of the plain formula; the 16-bit emulation has a positive error, passes
the scale check at every shape of the GPU matrix that has a 4096-element output, and an injected defect (one valid key masked out)
or a 1.1 % scale error on the survivors is caught by the rule the GPU tests apply (attention_ref.judge)."""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_ref as R


def _inputs(B, H, Tq, Tk, D, lp, seed, klen=None, p=0.0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(lp)
    q, k, v, do = rn(B, Tq, H, D), rn(B, Tk, H, D), rn(B, Tk, H, D), rn(B, Tq, H, D)
    mult = None
    if p > 0:
        mult = (torch.rand(B, H, Tq, Tk, generator=g) >= p).double() / (1.0 - p)
    kl = None if klen is None else torch.tensor(klen, dtype=torch.int32)
    return q, k, v, do, kl, D ** -0.5, mult


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("Tq,Tk", [(49, 49), (70, 130), (199, 199)])
def test_ref64_equals_sdpa_and_float64_autograd(Tq, Tk, drop):
    B, H, D = 3, 2, 64
    klen = [Tk, Tk // 2 + 3, 0]                                            # 0: clamped to one key
    q, k, v, do, kl, scale, mult = _inputs(B, H, Tq, Tk, D, torch.float64, 5 + Tq, klen, 0.1 if drop else 0.0)
    r = R.ref64(q, k, v, do, kl, scale, mult)
    qa, ka, va = (t.permute(0, 2, 1, 3).detach().clone().requires_grad_(True) for t in (q, k, v))
    keep = torch.arange(Tk)[None, :] < kl.long().clamp(1, Tk)[:, None]                     # [B, Tk], True = attend
    if not drop:
        sd = F.scaled_dot_product_attention(qa, ka, va, attn_mask=keep[:, None, None, :], scale=scale)
        assert R.max_err(sd.detach().permute(0, 2, 1, 3), r["o"]) <= 1e-12
    s = (qa @ ka.transpose(2, 3)) * scale
    s = s.masked_fill(~keep[:, None, None, :], float("-inf"))
    P = torch.softmax(s, -1)
    o = (P * mult if drop else P) @ va
    o.backward(do.permute(0, 2, 1, 3))
    assert R.max_err(o.detach().permute(0, 2, 1, 3), r["o"]) <= 1e-12
    assert R.max_err(torch.logsumexp(s.detach(), -1), r["lse"]) <= 1e-12
    for n, gr in (("dq", qa.grad), ("dk", ka.grad), ("dv", va.grad)):
        assert R.max_err(gr.permute(0, 2, 1, 3), r[n]) <= 1e-12, n
    for b in range(B):                                                    # gradients of masked keys are exactly zero
        c = int(kl.long().clamp(1, Tk)[b])
        assert float(r["dk"][b, c:].abs().max() if c < Tk else 0.0) == 0.0 and float(r["dv"][b, c:].abs().max() if c < Tk else 0.0) == 0.0


@pytest.mark.parametrize("lp", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,Tq,Tk,D,klen", R.matrix_shapes() + [(1, 4, 112, 112, 128, None), (3, 4, 17, 17, 128, None)])      # + fusion core
def test_emulation_has_a_positive_error_and_passes_the_scale_check(lp, B, H, Tq, Tk, D, klen):
    """Every shape of the GPU matrix: rounding alone cannot fail the scale check, and e_ref is a positive yardstick."""
    for p in (0.0, 0.1):
        q, k, v, do, kl, scale, mult = _inputs(B, H, Tq, Tk, D, lp, 11 * Tq + Tk, klen, p)
        r = R.ref64(q, k, v, do, kl, scale, mult)
        e = R.emul(lp, q, k, v, do, kl, scale, mult)
        for n in R.OUTS:
            if float(r[n].abs().max()) == 0.0:                            # one valid key: dq, dk identically zero, the emulation keeps a residue
                assert p > 0 or float(e[n].abs().max()) <= R.zero_bound(q, k, v, do, scale)
                continue
            if Tk == 1 and p == 0.0 and (n == "o" or (n == "dv" and Tq == 1)):       # softmax = 1, no multiplier: o = v, and dv = do at Tq = 1, exactly
                assert R.max_err(e[n], r[n]) == 0.0
                continue
            assert R.max_err(e[n], r[n]) > 0.0, n
            assert e[n].numel() >= R.SCALE_MIN_NUMEL
            assert R.scale_dev(e[n], r[n]) <= R.SCALE_TOL[lp], (n, R.scale_dev(e[n], r[n]))
        # the emulation judged by its own rule passes (ratio 1 by construction)
        rows, bad = R.judge(lp, {n: e[n] for n in R.OUTS + ("lse",)}, r, e, R.zero_bound(q, k, v, do, scale))
        assert not bad, bad


@pytest.mark.parametrize("lp", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,Tq,Tk,D,p", [(2, 4, 199, 199, 64, 0.0), (2, 4, 49, 49, 64, 0.1), (2, 2, 70, 130, 64, 0.1), (3, 4, 17, 17, 128, 0.0)])
def test_injected_defects_are_caught(lp, B, H, Tq, Tk, D, p):
    klen = [Tk - 5] * B
    q, k, v, do, kl, scale, mult = _inputs(B, H, Tq, Tk, D, lp, 3 * Tq + Tk, klen, p)
    r = R.ref64(q, k, v, do, kl, scale, mult)
    e = R.emul(lp, q, k, v, do, kl, scale, mult)
    zt = R.zero_bound(q, k, v, do, scale)
    # (a) one valid key masked out: beyond 4 x e_ref on every output
    wrong = R.emul(lp, q, k, v, do, kl - 1, scale, mult)
    rows, bad = R.judge(lp, {n: wrong[n] for n in R.OUTS}, r, e, zt)
    assert all(row[3] > R.FACTOR for row in rows), R.fmt(rows)
    assert len(bad) >= len(R.OUTS)
    # (b) survivors scaled by 1.011: o and dv carry the factor, the scale check sees it whether or not the max-error gate does
    m2 = (torch.ones(B, H, Tq, Tk, dtype=torch.float64) if mult is None else mult) * 1.011
    wrong = R.emul(lp, q, k, v, do, kl, scale, m2)
    for n in ("o", "dv"):
        assert R.scale_dev(wrong[n], r[n]) > R.SCALE_TOL[lp], n
    rows, bad = R.judge(lp, {n: wrong[n] for n in R.OUTS}, r, e, zt)
    assert any(b.startswith("o: scale") for b in bad) and any(b.startswith("dv: scale") for b in bad), bad


def test_zero_corner_and_lse_gate_forms():
    q, k, v, do, kl, scale, _ = _inputs(4, 16, 199, 1, 64, torch.bfloat16, 9)
    r = R.ref64(q, k, v, do, None, scale)
    e = R.emul(torch.bfloat16, q, k, v, do, None, scale)
    zt = R.zero_bound(q, k, v, do, scale)
    assert float(r["dq"].abs().max()) == 0.0 and float(r["dk"].abs().max()) == 0.0 and float(e["dq"].abs().max()) <= zt / 16
    assert 0.0 < zt < 1e-1
    ours = {n: e[n].clone() for n in R.OUTS}
    ours["dq"] = ours["dq"] + 0.5 * zt                                    # a residue inside the bound passes, one beyond it does not
    assert not R.judge(torch.bfloat16, ours, r, e, zt)[1]
    ours["dq"] = ours["dq"] + zt
    assert any(b.startswith("dq") for b in R.judge(torch.bfloat16, ours, r, e, zt)[1])
    assert R.lse_gate(0.0, 0.5) == 64.0 * R.EPS32 and math.isclose(R.lse_gate(1e-3, 8.0), 4e-3)
