"""The measuring stick of test_rowops_matrix_gpu.py, checked on the CPU: every reference of rowops_ref.py against torch's own double-precision
operator where one exists, the restated float32 interpolation laws against F.interpolate, and the shape lists against the dispatch conditions
(restated in rowops_ref.py) so that a later change to a list cannot silently drop a branch."""
import pytest
import torch
import torch.nn.functional as F

import rowops_ref as R
from attention_ref import EPS32

F32, F64 = torch.float32, torch.float64
TOL = dict(rtol=1e-12, atol=1e-12)


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# references against torch's double-precision operators
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 65), (7, 256), (3, 2047)])
def test_layernorm_and_backward(rows, cols):
    g = _g(cols)
    x = torch.randn(rows, cols, generator=g, dtype=F64).requires_grad_()
    gamma = (1 + 0.1 * torch.randn(cols, generator=g, dtype=F64)).requires_grad_()
    beta = (0.1 * torch.randn(cols, generator=g, dtype=F64)).requires_grad_()
    dy, dres = torch.randn(rows, cols, generator=g, dtype=F64), torch.randn(rows, cols, generator=g, dtype=F64)
    want = F.layer_norm(x, (cols,), gamma, beta, float(torch.tensor(R.LN_EPS, dtype=F32)))
    y, mean, rstd = R.layernorm(x.detach(), gamma.detach(), beta.detach())
    torch.testing.assert_close(y, want.detach(), **TOL)
    torch.testing.assert_close(R.layernorm(x.detach(), gamma.detach(), beta.detach(), act=True)[0], F.gelu(want.detach()), **TOL)
    torch.testing.assert_close(mean, x.detach().mean(1), **TOL)
    want.backward(dy)
    dx, dg, db, dg_abs, db_abs = R.layernorm_bwd(x.detach(), dy, gamma.detach(), mean, rstd, dres)
    torch.testing.assert_close(dx, x.grad + dres, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(dg, gamma.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(db, beta.grad, rtol=1e-10, atol=1e-10)
    assert bool((dg_abs >= dg.abs() - 1e-12).all()) and bool((db_abs >= db.abs() - 1e-12).all())
    # the emulation: float32 arithmetic, 16-bit rounding of y - finite and close
    for lp in R.LIBS.values():
        em = R.layernorm(x.detach().float(), gamma.detach().float(), beta.detach().float(), True, F32, R.rounder(lp))[0]
        assert float((em.double() - F.gelu(want.detach())).abs().max()) < 2.0 ** -7 * max(1.0, float(want.detach().abs().max()))


def test_layernorm_offset_rows_have_exact_sums():
    """Rows of 1000 + k / 64: every partial sum of up to 256 of them fits 24 bits, so the float32 mean is exact in any order of summation."""
    for cols in R.LN_OFFSET_COLS:
        x = R.offset_row(cols)
        assert float(x.double().sum()) == float(x.sum()) and float(x.double().abs().sum()) < 2 ** 24 / 64
        assert float((x.double() - 1000).abs().max()) <= 1.0 and float(x.std()) > 0.3


@pytest.mark.parametrize("rows,cols", [(1, 1), (4, 65), (3, 800)])
def test_log_softmax_and_backward(rows, cols):
    g = _g(cols)
    x = (3 * torch.randn(rows, cols, generator=g, dtype=F64)).requires_grad_()
    dy = torch.randn(rows, cols, generator=g, dtype=F64)
    want = torch.log_softmax(x, -1)
    y = R.log_softmax(x.detach())
    torch.testing.assert_close(y, want.detach(), **TOL)
    want.backward(dy)
    ld = (cols + 63) // 64 * 64
    dx = R.log_softmax_bwd(y, dy, ld)
    torch.testing.assert_close(dx[:, :cols], x.grad, **TOL)
    assert dx.shape == (rows, ld) and float(dx[:, cols:].abs().sum()) == 0.0
    wide = torch.tensor([[1e4, -1e4, 0.0, 9999.0]], dtype=F64)
    torch.testing.assert_close(R.log_softmax(wide), torch.log_softmax(wide, -1), **TOL)
    assert bool(torch.isfinite(R.log_softmax(wide.float(), F32)).all())


@pytest.mark.parametrize("C,k,stride,L_out,with_bias", [(32, 10, 5, 7, True), (96, 3, 2, 5, False), (512, 16, 1, 3, True)])
def test_conv0_ln_gelu(C, k, stride, L_out, with_bias):
    g = _g(C + k)
    T_in = (L_out - 1) * stride + k
    wav, w = torch.randn(2, T_in, generator=g, dtype=F64), torch.randn(C, k, generator=g, dtype=F64)
    bias = torch.randn(C, generator=g, dtype=F64) if with_bias else None
    gamma, beta = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    conv = F.conv1d(wav[:, None], w[:, None], bias, stride=stride).transpose(1, 2)                  # [B, L_out, C]
    want = F.gelu(F.layer_norm(conv, (C,), gamma, beta, float(torch.tensor(R.LN_EPS, dtype=F32))))
    torch.testing.assert_close(R.conv0_ln_gelu(wav, w, bias, gamma, beta, L_out, stride), want, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("cols", R.L2_COLS)
def test_l2norm_and_backward(cols):
    g = _g(cols)
    x = torch.randn(6, cols, generator=g, dtype=F64)
    x[1] = 0.0                                                # clamped by eps
    x[2] *= 1e-13 / float(x[2].norm())                        # below eps as well: y = x / eps
    x.requires_grad_()
    dy = torch.randn(6, cols, generator=g, dtype=F64)
    eps = float(torch.tensor(R.L2_EPS, dtype=F32))
    want = F.normalize(x, dim=1, eps=eps)
    y, n = R.l2norm(x.detach())
    torch.testing.assert_close(y, want.detach(), rtol=1e-12, atol=0)
    torch.testing.assert_close(n, x.detach().norm(dim=1), rtol=1e-12, atol=0)
    want.backward(dy)
    dx = R.l2norm_bwd(y, dy, n)
    live = torch.tensor([0, 3, 4, 5])
    torch.testing.assert_close(dx[live], x.grad[live], rtol=1e-9, atol=1e-9)
    # clamped rows: y = x / eps is linear, the kernel's formula keeps the projection term; state what it is
    torch.testing.assert_close(dx[1], dy[1] / eps, rtol=1e-12, atol=0)
    assert bool(torch.isfinite(dx).all())


def test_lse_rows_and_chunk_merge():
    g = _g(3)
    s = (torch.rand(7, 300, generator=g, dtype=F64) * 2 - 1) / 0.07
    lse, rsum = R.lse_rows(s)
    torch.testing.assert_close(lse, torch.logsumexp(s, 1), **TOL)
    torch.testing.assert_close(rsum, s.sum(1), **TOL)
    run = None
    for c0, c1 in ((0, 128), (128, 256), (256, 300)):
        part = R.lse_rows(s[:, c0:c1])[0]
        run = part if run is None else R.lse_merge(run, part)
    torch.testing.assert_close(run, lse, **TOL)


def test_contrastive_dsim_is_the_gradient_of_the_loss():
    g = _g(4)
    s = (torch.randn(5, 37, generator=g, dtype=F64) / 0.07).requires_grad_()
    (-torch.log_softmax(s, 1).mean()).backward()
    lse, _ = R.lse_rows(s.detach())
    d = R.contrastive_dsim(s.detach(), lse, 1.0 / 5, 37, ld=40)
    assert d.shape == (5, 40) and float(d[:, 37:].abs().sum()) == 0.0
    torch.testing.assert_close(d[:, :37], s.grad, rtol=1e-6, atol=1e-9)           # coef goes through float32, as the kernel's argument does
    # a column chunk of a wider matrix: the uniform term keeps the total width
    d2 = R.contrastive_dsim(s.detach()[:, :16], lse, 1.0 / 5, 37)
    torch.testing.assert_close(d2, s.grad[:, :16], rtol=1e-6, atol=1e-9)


def test_loss_combine():
    g = _g(5)
    nll, w = torch.rand(6, generator=g, dtype=F64) * 50, torch.rand(6, generator=g, dtype=F64)
    c1, c2 = torch.tensor([0.7], dtype=F64), torch.tensor([-0.2], dtype=F64)
    out, mag = R.loss_combine(nll, w, c1, c2, 0.25)
    v = nll * w
    torch.testing.assert_close(out, torch.stack([v.sum() + 0.25 * 0.5, 2 * v[:3].sum(), 2 * v[3:].sum()]), **TOL)
    torch.testing.assert_close(R.loss_combine(nll, w, None, c2, 0.25)[0][0], v.sum() + 0.25 * -0.2, **TOL)
    torch.testing.assert_close(R.loss_combine(nll, w, None, None, 0.25)[0][0], v.sum(), **TOL)
    assert bool((mag >= out.abs()).all())


def test_glue_statements():
    g = _g(6)
    mask = torch.randint(-1, 6, (1025,), generator=g)
    rank = torch.where(mask == 1, 0, torch.where(mask == 2, 1, torch.where(mask <= 0, 2, 3)))
    assert torch.equal(R.class_order(mask), torch.sort(rank, stable=True).indices)
    x = torch.randn(3, 5, 7, generator=g)
    assert torch.equal(R.permute(R.permute(x)), x) and R.permute(x).shape == (5, 3, 7) and torch.equal(R.permute(x)[4, 2], x[2, 4])
    src, perm = torch.randn(9, 4, generator=g, dtype=F64), torch.randperm(9, generator=g)
    out0 = torch.randn(9, 4, generator=g, dtype=F64)
    assert torch.equal(R.gather(R.scatter(src, perm, out0, 1.0, False), perm), src)
    torch.testing.assert_close(R.scatter(src, perm, out0, 0.5, True)[perm], 0.5 * src + out0[perm], **TOL)


def test_dropout_multiplier_law():
    u = torch.arange(65536, dtype=F32) / 65536
    for p, thr in ((0.1, 6554), (0.5, 32768)):
        m = R.drop_mult(u, p)
        assert int((m == 0).sum()) == thr and float(m.max()) == float(torch.tensor(65536.0) / torch.tensor(65536.0 - thr))
        assert abs(float(m.double().mean()) - 1.0) < 1e-6                      # an unbiased mask


def test_cast_specials_hit_ties_and_infinities():
    v = R.cast_values(1027, _g(7))
    assert float(v[0].to(torch.bfloat16)) == 1.0 and float(v[1].to(torch.bfloat16)) == 1 + 2.0 ** -6              # ties to even, both ways
    assert float(v[2].to(torch.float16)) == 1.0 and float(v[3].to(torch.float16)) == 1 + 2.0 ** -9
    assert bool(torch.isinf(v[5])) and bool(torch.isinf(v[6])) and bool(torch.isinf(v[11].to(torch.float16))) and float(v[10].to(torch.float16)) == 65504.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the float32 interpolation laws
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tin,Tout", R.MASK_DOWN)
def test_nearest_law_equals_interpolate(Tin, Tout):
    m = torch.randint(0, 4, (2, Tin), generator=_g(Tin))
    assert torch.equal(R.mask_downsample(m, Tout), R.mask_downsample_torch(m, Tout))


def _interp(x, Tv):
    return x if x.shape[0] == Tv else F.interpolate(x.t()[None], size=Tv, mode="linear", align_corners=True)[0].t()


@pytest.mark.parametrize("Tm,Tv", R.LERP_PAIRS_EXACT + R.LERP_PAIRS_FMA)
def test_lerp_law_equals_interpolate(Tm, Tv):
    """Indices and weights bit for bit on every pair (an identity matrix through F.interpolate IS its weight matrix: w0 * 1 + w1 * 0); the
    interpolated values bit for bit where the weights make a fused multiply-add round like a multiply and an add, within one rounding of the
    larger product elsewhere."""
    assert torch.equal(R.lerp_weights(Tm, Tv), _interp(torch.eye(Tm), Tv))
    x = torch.randn(Tm, 37, generator=_g(Tm * 1000 + Tv))
    i0, i1, lam = R.lerp_table(Tm, Tv)
    mine = (1 - lam)[:, None] * x[i0] + lam[:, None] * x[i1]
    if (Tm, Tv) in R.LERP_PAIRS_EXACT:
        assert torch.equal(mine, _interp(x, Tv))
    else:
        assert float((mine - _interp(x, Tv)).abs().max()) <= EPS32 * float(x.abs().max())


def test_gather_lerp_lists_use_checked_pairs():
    used = R.gather_pairs(R.GATHER_LERP)
    assert all(Tm == Tv or (Tm, Tv) in R.LERP_PAIRS_EXACT + R.LERP_PAIRS_FMA for Tm, Tv in used), used
    kinds = {("eq" if Tm == Tv else "up" if Tm < Tv else "down") for Tm, Tv in used}
    assert kinds == {"eq", "up", "down"} and any(Tm == 1 for Tm, _ in used) and any(Tv == 1 for _, Tv in used)
    assert {g for _, _, _, g, _ in R.GATHER_LERP} == {1, 2} and {Ta > 256 for _, Ta, _, _, _ in R.GATHER_LERP} == {True, False}
    assert any(0 in c and max(c) > 0 for _, _, _, _, c in R.GATHER_LERP)                         # an item without speech beside items with some
    assert all(min(Tm for Tm, _ in R.gather_pairs([c])) == 0 for c in R.GATHER_LERP_EMPTY)
    assert all(min(Tm for Tm, _ in R.gather_pairs([c])) > 0 for c in R.GATHER_LERP)


@pytest.mark.parametrize("case", R.GATHER_LERP + R.GATHER_LERP_EMPTY, ids=lambda c: c[0])
def test_gather_lerp_restatement_equals_the_torch_path(case):
    name, Ta, Tv, groups, counts = case
    g = _g(Ta * 100 + Tv)
    mask = R.speech_mask(Ta, counts, g)
    assert ((mask == 1) | (mask == 2)).sum(1).tolist() == counts
    feat, dout = torch.randn(len(counts), Ta, 3, generator=g), torch.randn(len(counts), Tv, 3, generator=g)
    out_t, mout_t, lens_t, df_t = R.gather_lerp_torch(feat, mask, Tv, groups, dout)
    out, mout, lens, df = R.gather_lerp(feat, mask, Tv, groups, dout)
    assert torch.equal(mout, mout_t) and torch.equal(lens, lens_t)
    tol = EPS32 * float(feat.abs().max())
    assert float((out - out_t).abs().max()) <= tol
    mag = R.gather_lerp(feat.abs(), mask, Tv, groups, dout.abs())[3]
    assert bool(((df - df_t).abs() <= 8 * EPS32 * mag).all())
    if case in R.GATHER_LERP_EMPTY:
        gs = len(counts) // groups
        for gi in range(groups):
            if max(counts[gi * gs:(gi + 1) * gs]) == 0:
                sl = slice(gi * gs, (gi + 1) * gs)
                assert float(out[sl].abs().sum()) == 0 and int(mout[sl].abs().sum()) == 0 and int(lens[sl].sum()) == 0 and float(df[sl].abs().sum()) == 0
                assert float(out_t[sl].abs().sum()) == 0 and int(lens_t[sl].sum()) == 0 and float(df_t[sl].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the shape lists reach every branch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_layernorm_lists_reach_every_form():
    fwd = {R.ln_fwd_form(c, al) for c, al in R.LN_FWD}
    assert fwd == {("generic", n) for n in (1, 2, 8, 16, 32)} | {("vec", n) for n in (1, 3, 5, 6, 7, 8)}
    assert R.ln_fwd_form(512, False) == ("generic", 8) and (512, False) in R.LN_FWD                  # the misaligned fall-back
    assert {R.ln_fwd_form(c) for c, _ in R.LN_SHIFT} == {("vec", n) for n in (1, 3, 5, 6, 7, 8)}
    assert {w for _, w in R.LN_SHIFT} == {"x", "y", "gamma"}
    assert {R.ln_fwd_form(c) for c in R.LN_OFFSET_COLS} == {("generic", 1), ("vec", 1)}
    bwd = {R.ln_bwd_form(c, al) for c, al in R.LN_BWD}
    assert bwd == {("generic", n) for n in (1, 2, 8, 16, 32)} | {("vec", n) for n in (1, 2, 4, 8)}
    assert any(R.ln_fwd_form(c)[0] == "vec" and R.ln_bwd_form(c)[0] == "generic" for c, al in R.LN_BWD if al)      # 768 / 1280
    assert {R.ln_bwd_form(c)[0] for c, _ in R.LN_DROP} == {"vec", "generic"} and {p for _, p in R.LN_DROP} == {0.1, 0.5}
    for rows in R.LN_BWD_ROWS:                                 # ragged rows per block, a short last block
        nblk = R.ln_nblk(rows)
        rpb = (rows + nblk - 1) // nblk
        assert (nblk - 1) * rpb < rows
    last = [rows - (R.ln_nblk(rows) - 1) * ((rows + R.ln_nblk(rows) - 1) // R.ln_nblk(rows)) for rows in R.LN_BWD_ROWS]
    rpbs = [(rows + R.ln_nblk(rows) - 1) // R.ln_nblk(rows) for rows in R.LN_BWD_ROWS]
    assert any(l < r for l, r in zip(last, rpbs)) and any(r % 4 for r in rpbs) and max(R.ln_nblk(r) for r in R.LN_BWD_ROWS) > 1


def test_conv0_lists_reach_every_form():
    assert R.conv0_form(512, 10, True) == "c512" and R.conv0_form(512, 10, True, al=False) == "generic_lp"
    forms = {(R.conv0_form(C, k, lp), C % 64 == 0, k) for C in R.CONV0_C for k, _ in R.CONV0_KS for lp in (True, False)}
    assert {f for f, _, _ in forms} == {"c512", "generic_lp", "generic_f32"}
    assert any(not m for _, m, _ in forms) and {k for _, _, k in forms} == {10, 3, 16}
    assert ("generic_f32", True, 10) in forms                # C = 512, k = 10 in float32: beside the fast form
    fpb = 64
    assert {min(3, (L + fpb - 1) // fpb) for L in R.CONV0_C512_LOUT} == {1, 2, 3}
    assert 1 in R.CONV0_C512_LOUT and any(L % fpb == 0 for L in R.CONV0_C512_LOUT) and any(L % fpb == 1 for L in R.CONV0_C512_LOUT)
    assert any(0 < L < 4 for L in R.CONV0_C512_LOUT) and max(R.CONV0_C) == 1024 and max(k for k, _ in R.CONV0_KS) == 16


def test_colsum_cast_sum_slices_lists_reach_every_form():
    for kind, cols in R.COLSUM_COLS.items():
        for c in cols:
            for is_lp in ((True,) if kind == "lp_vec" else (False,) if kind == "f32_vec" else (True, False)):
                assert R.colsum_form(is_lp, c, c) == kind, (kind, c)
        rpb = R.COLSUM_ROWS[kind]
        assert set(R.colsum_rows(kind)) == {1, rpb - 1, rpb + 1, 3 * rpb + 5}
    assert R.colsum_form(True, 200, 208) == "lp_vec" and R.colsum_form(False, 200, 204) == "f32_vec"            # the column slices of the GPU file
    assert R.colsum_form(True, 200, 200, al=False) == "scalar" and R.colsum_form(False, 200, 200, al=False) == "scalar"
    assert {R.cast_form(s, d, n, al) for s in (True, False) for d in (True, False) for n in R.CAST_N for al in (True, False)} == {"vec", "scalar"}
    assert R.cast_form(False, True, 4) == "vec" and R.cast_form(False, True, 1027) == "scalar" and R.cast_form(False, True, 4, al=False) == "scalar"
    forms = [(R.sum_slices_form(n, st, al), S, st > n, n % 4 == 0, st % 4 == 0, al) for S, n, st, al in R.SUM_SLICES]
    assert {(f, S) for f, S, *_ in forms} >= {("vec", 1), ("vec", 2), ("vec", 7), ("scalar", 1), ("scalar", 2), ("scalar", 7)}
    assert any(f == "vec" and wide for f, _, wide, *_ in forms) and any(f == "scalar" and wide for f, _, wide, *_ in forms)
    assert any(f == "scalar" and n4 and s4 and not al for f, _, _, n4, s4, al in forms)                         # scalar by alignment alone


def test_remaining_lists():
    assert R.LSM_COLS == [1, 64, 65, 800, 2048] and R.LSM_ROWS == [1, 51]
    assert {(c + p - 1) // p * p if p else c for c, p in R.LSM_BWD} >= {832, 2048, 1}
    assert R.L2_COLS == [1, 65, 128, 130] and R.REDUCE_N == [1, 255, 257, 12736] and R.COMBINE_N == [2, 6, 514]
    assert R.MASK_DOWN == [(7, 7), (5, 9), (1, 3), (19200, 59), (64000, 199)] and R.PERMUTE == [(1, 1, 1), (3, 5, 7), (2, 130, 512)]
