"""CPU: the measuring stick of the GEMM matrix (gemm_ref.py) is itself right, and its gates are neither vacuous nor impossible:
the fp64 statement equals torch.nn.functional.linear / gelu / autograd at every activation; float32 accumulation in three orders stays inside
the gate_sum floor at every K of the matrix; the 16-bit rule passes the emulation and fails just over its bound; the exact law holds for the
emulation; the operand builders put NaN and canaries where they claim; and every planted defect is rejected by a gate or by the exact law,
while the earlier 2e-2 gate lets at least a dropped k element and a stale 8-column chunk through (printed with -s)."""
import math

import pytest
import torch

import gemm_ref as G

LPS = list(G.LIBS.values())


def _rand_case(M, N, K, lp, seed=0, small_rows=0):
    g = torch.Generator().manual_seed(seed + K)
    rn = G.rounder(lp)
    A = rn(torch.randn(M, K, generator=g))
    if small_rows:
        A[:small_rows] *= 2.0 ** -9                       # a small-magnitude row tile (a power of two keeps the operands 16-bit values)
    B = rn(torch.randn(K, N, generator=g) / math.sqrt(K))
    bias = torch.randn(1, N, generator=g)
    res = torch.randn(M, N, generator=g)
    aux = rn(torch.randn(M, N, generator=g))
    u = torch.randint(0, 65536, (M * (N + 8) + 8,), generator=g).float() / 65536.0     # draws by element index, ldc up to N + 8
    return A, B, bias, res, aux, u


# -------------------------------------------------------------------------------------------------------------------------------------------
# the statement against torch
# -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", range(5))
def test_reference_equals_torch_linear_gelu_and_autograd(act):
    F = torch.nn.functional
    M, N, K = 37, 29, 50
    A, B, bias, res, aux, u = _rand_case(M, N, K, torch.bfloat16)
    A, W, bias, res, aux = A.double(), B.double().t().contiguous(), bias.double(), res.double(), aux.double()
    mult = G.mult_from_uniform(u, 0.25, G.drop_index(1, 0, 0, 0, M, N, N + 3, "cpu"))[0]
    assert 0.6 < float((mult > 0).double().mean()) < 0.9 and abs(float(mult.max()) - 1.0 / 0.75) < 1e-6
    for alpha, use_res, use_mult in ((1.0, False, False), (0.5, True, True)):
        C, C2 = G.ref_gemm(A, W.t(), torch.float64, alpha=alpha, bias=bias, act=act, aux=aux, mult=mult if use_mult else None,
                           res=res if use_res else None)
        pre = (F.linear(A, W) * alpha + bias).requires_grad_(True)
        m = mult if use_mult else torch.ones_like(mult)
        if act == G.ACT_NONE:
            want, want2 = pre * m, pre
        elif act == G.ACT_GELU:
            want, want2 = F.gelu(pre) * m, pre
        elif act == G.ACT_MUL_GELU_GRAD:
            a = aux.clone().requires_grad_(True)
            F.gelu(a).sum().backward()
            want, want2 = pre * a.grad * m, pre
        elif act == G.ACT_GELU_GF:
            F.gelu(pre).sum().backward()
            want, want2 = F.gelu(pre) * m, pre.grad * m
        else:
            want, want2 = pre * aux * m, pre
        if use_res:
            want = want + res
        torch.testing.assert_close(C, want.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(C2, want2.detach(), rtol=1e-12, atol=1e-12)


def test_split_k_and_sum_slices_are_the_whole_product():
    A, B, _, res, _, _ = _rand_case(24, 40, 777, torch.bfloat16)
    parts = G.split_k(A, B, 320, torch.float64)
    assert parts.shape[0] == 3                            # 320 + 320 + a ragged 137
    torch.testing.assert_close(G.sum_slices(parts, 0.5, res), res.double() + 0.5 * (A.double() @ B.double()), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(G.sum_slices(parts[:1], 1.0), A[:, :320].double() @ B[:320].double(), rtol=0, atol=0)


def test_drop_index_counts_the_batch_offset():
    idx = G.drop_index(6, 2, 1000, 5000, 3, 4, 10, "cpu")
    assert int(idx[0, 0, 0]) == 0 and int(idx[1, 2, 3]) == 1000 + 23 and int(idx[2, 0, 0]) == 5000 and int(idx[5, 1, 1]) == 2 * 5000 + 1000 + 11
    assert int(G.drop_index(3, 0, 1000, 0, 3, 4, 10, "cpu")[2, 1, 0]) == 2010
    assert abs(G.inv_keep(0.1) - 65536.0 / (65536.0 - 6554.0)) < 1e-7


# -------------------------------------------------------------------------------------------------------------------------------------------
# the float32 floor is a condition float32 accumulation meets
# -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", G.all_ks())
def test_float32_accumulation_stays_inside_the_floor(K):
    """64 EPS32 sum_k |a b| per element bounds the error of a float32 sum of the K products in sequential order, pairwise order and in blocks of
    64 (the worst-case bound of a sequential sum is (K - 1) EPS32 / 2 times that sum; rounding errors do not line up, and the largest ratio
    seen is printed).  The gate is FACTOR times this floor."""
    for lp in LPS:
        A, B, *_ = _rand_case(32, 32, K, lp, seed=7)
        r64 = A.double() @ B.double()
        floor = 64.0 * G.EPS32 * (A.double().abs() @ B.double().abs())
        for name, prod in (("sequential", G.prod_sequential), ("pairwise", G.prod_pairwise), ("blocks64", G.prod_blocks64), ("reversed32", G.prod_blocks_reversed)):
            d = (prod(A, B).double() - r64).abs()
            ratio = float((d / floor).max())
            print(f"K={K} {lp} {name}: worst err / floor = {ratio:.3f}")
            assert ratio <= 1.0, (K, lp, name, ratio)


# -------------------------------------------------------------------------------------------------------------------------------------------
# builders
# -------------------------------------------------------------------------------------------------------------------------------------------
def _uniform(n):
    return torch.randint(0, 65536, (n + 8,), generator=torch.Generator().manual_seed(n)).float() / 65536.0


@pytest.mark.parametrize("lp", LPS)
def test_builders_put_nan_and_canaries_where_they_claim(lp):
    """The two-level batch is laid out as the model lays out heads: items interleaved inside the rows, outer groups after the pad rows, so that
    zo * outer + zi * item differs from z * item and a kernel (or a dropout index) that ignores batch_inner is told apart."""
    c = G.case("demo", 50, 36, 64, a="km", b="kn", c2=True, act=G.ACT_GELU, drop=0.1, batch=6, inner=2, a_pad=16, b_pad=24, c_off=4)
    bt = G.Built(c, lp, "cpu", _uniform)
    assert (bt.lda, bt.sA, bt.oA) == (132, 66, 72 * 132) and bt.sa.shape == (3, 2, 64, 50) and bt.sa.stride() == (72 * 132, 66, 132, 1)
    assert (bt.ldb, bt.sB, bt.oB) == (120, 60, 72 * 120) and (bt.ldc, bt.sC, bt.oC) == (88, 44, 58 * 88)
    assert bt.C.shape == (3, 2, 50, 36) and bt.C.stride() == (58 * 88, 44, 88, 1) and bt.C.storage_offset() == 4
    for o, s_, rows, ld in ((bt.oA, bt.sA, 64, bt.lda), (bt.oB, bt.sB, 64, bt.ldb), (bt.oC, bt.sC, 50, bt.ldc)):
        assert o != 2 * s_ and s_ < rows * ld                                  # neither level is a multiple of the other
    torch.testing.assert_close(bt.sa.float().reshape(6, 64, 50), bt.A.transpose(1, 2), rtol=0, atol=0)
    base = bt.sa._base if bt.sa._base is not None else bt.sa
    whole = base.flatten()[:3 * bt.oA].view(3, 72, 2, 66)
    assert bool(torch.isnan(whole[:, 64:]).all()) and bool(torch.isnan(whole[..., 50:]).all())          # 8 NaN rows, NaN tail of every item's row
    assert bool(torch.isnan(bt.C).all()) and bool(torch.isnan(bt.C2).all()) and bt.canaries() == []
    bt.store(bt.emul())
    assert bt.canaries() == [] and bool(torch.isfinite(bt.C.float()).all())
    rows, bad, gate = G.verdict(bt, bt.outputs())
    assert bad == [] and gate == "judge"
    # the dropout index of a kernel that ignores batch_inner (z * sC) gives another mask, and the judge sees it
    flat_idx = G.drop_index(6, 0, bt.sC, 0, 50, 36, bt.ldc, "cpu")
    true_idx = G.drop_index(6, 2, bt.sC, bt.oC, 50, 36, bt.ldc, "cpu")
    assert torch.equal(flat_idx[:2], true_idx[:2]) and not bool((flat_idx[2:] == true_idx[2:]).any())
    wrong = G.ref_gemm(bt.A, bt.B, torch.float32, act=G.ACT_GELU, mult=G.mult_from_uniform(_uniform(int(true_idx.max()) + 1), 0.1, flat_idx),
                       rnd=G.rounder(lp), prod=G.prod_blocks_reversed)
    assert G.verdict(bt, dict(C=wrong[0], C2=wrong[1]))[1] != []
    for where in ((0, 0, 0, 36), (2, 50, 1, 0), (1, 49, 1, 43), (1, 57, 0, 5)):    # one past N, the first row past M, the end of a live row's share, the gap between outer groups
        bt2 = G.Built(c, lp, "cpu", _uniform)
        bt2.cflat[4:4 + 3 * bt2.oC].view(3, 58, 2, 44)[where] = 1.0
        assert bt2.canaries() != [], where
    bt3 = G.Built(c, lp, "cpu", _uniform)
    bt3.c2flat[0] = 0.0                                                  # the 4 elements in front of a C2 that starts 4 elements in
    assert bt3.canaries() != []
    # one level: items one after the other, bias with a NaN tail after every item
    c1 = G.case("demo1", 50, 36, 64, bias=True, res="f32", batch=3)
    b1 = G.Built(c1, lp, "cpu")
    assert (b1.lda, b1.sA, b1.oA) == (72, 58 * 72, 0) and b1.sBias == 44 and b1.sbias.stride() == (44, 44, 1)
    assert bool(torch.isnan(b1.sbias._base[:3 * 44].view(3, 44)[:, 36:]).all()) and torch.equal(b1.sbias, b1.bias)
    b1.store(b1.emul())
    assert b1.canaries() == [] and G.verdict(b1, b1.outputs())[1] == []
    b1.cflat[:3 * b1.sC].view(3, 58, 44)[1, 50, 0] = 1.0
    assert b1.canaries() != []


def test_case_lists_are_well_formed():
    seen = set()
    for gname, (env, fn) in G.GROUPS.items():
        for c in fn():
            key = (gname, G.case_id(c))
            assert key not in seen, key
            seen.add(key)
            assert c["expect"] and "kernel" in c["expect"], key
            if c["exact"]:
                assert c["act"] in (G.ACT_NONE, G.ACT_MUL_AUX) and c["drop"] == 0 and c["alpha"] in (1.0, 0.5), key
                assert c["K"] * 6 * 3 + 6000 < 2 ** 24
            if c["out"] == "f32" and c["inp"] == "lp":
                assert c["act"] in (G.ACT_NONE, G.ACT_MUL_AUX), key         # gate_sum is stated for sums and exact multiplies only
            if c["M"] * c["N"] > 2.1e6:                                   # the largest shape the other groups need is 2048 x 1024
                assert gname in ("v4", "v4_notail") and c["M"] == 4300, key  # the quadrant-job shapes are the only large ones
    v7 = {(c["expect"]["act"], c["expect"]["out_dtype"], c["expect"]["nm1"]) for g in ("v7_nm4", "v7_nm3") for c in G.GROUPS[g][1]() if "act" in c["expect"]}
    assert len(v7) == 10                                                     # all ten instantiations of the persistent kernel


# -------------------------------------------------------------------------------------------------------------------------------------------
# the rules accept the emulation and reject what lies just over the bound
# -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lp", LPS)
@pytest.mark.parametrize("K", [64, 1300])
def test_judge_passes_the_emulation_and_fails_just_over_the_bound(lp, K):
    c = G.case("j", 80, 72, K, bias=True, act=G.ACT_GELU, c2=True, drop=0.1, res="f32")
    bt = G.Built(c, lp, "cpu", _uniform)
    r64, em = bt.ref64(), bt.emul()
    for prod in (G.prod_blocks64, G.prod_matmul, G.prod_sequential):
        rows, bad = G.judge(lp, bt.emul(prod), r64, em)
        assert bad == [], bad
    e_ref = G.max_err(em["C"], r64["C"])
    for f, ok in ((0.98, True), (1.02, False)):
        ours = {k: v.clone() for k, v in r64.items()}
        ours["C"][0, 5, 7] += f * G.FACTOR * e_ref
        assert (G.judge(lp, ours, r64, em)[1] == []) == ok, f
    ours = {k: v * (1.0 + 1.5 * G.SCALE_TOL[lp]) for k, v in r64.items()}          # a scale error the max-error gate cannot see at small values
    assert any("scale" in b for b in G.judge(lp, ours, r64, em)[1])
    ours = {k: v.clone() for k, v in em.items()}
    ours["C2"][0, 1, 1] = float("nan")
    assert any("non-finite" in b for b in G.judge(lp, ours, r64, em)[1])
    # float32 output: gate_sum per element
    c = G.case("s", 80, 72, K, out="f32", bias=True, res="f32", act=G.ACT_MUL_AUX, aux="f32", drop=0.1)
    bt = G.Built(c, lp, "cpu", _uniform)
    r64, em, sa = bt.ref64(), bt.emul(), bt.sum_abs()
    for prod in (G.prod_blocks64, G.prod_sequential, G.prod_pairwise):
        assert G.gate_sum("C", bt.emul(prod)["C"], r64["C"], em["C"], sa["C"])[1] == []
    e_ref = G.max_err(em["C"], r64["C"])
    i = int(torch.argmin(sa["C"][0, :, 3]))                                          # the element with the smallest floor of a column
    gate = G.FACTOR * max(e_ref, 64.0 * G.EPS32 * float(sa["C"][0, i, 3]))
    for f, ok in ((0.98, True), (1.02, False)):
        ours = r64["C"].clone()
        ours[0, i, 3] += f * gate
        assert (G.gate_sum("C", ours, r64["C"], em["C"], sa["C"])[1] == []) == ok, f


@pytest.mark.parametrize("lp", LPS)
@pytest.mark.parametrize("K", [64, 100, 777, 1300])
def test_exact_law_holds_for_the_emulation(lp, K):
    for kw in (dict(out="f32", bias=True, res="alias", alpha=0.5), dict(bias=True, res="f32"), dict(act=G.ACT_MUL_AUX, aux="lp", alpha=0.5),
               dict(out="f32", act=G.ACT_MUL_AUX, aux="f32", bias=True), dict(batch=3, bias=True, res="f32")):
        bt = G.Built(G.case("x", 40, 48, K, exact=True, **kw), lp, "cpu")
        assert float(bt.A.abs().max()) == 3 and float(bt.B.abs().max()) == 2 and not torch.equal(bt.A[0, :40, :40], bt.A[0, :40, :40].t())
        for prod in (G.prod_blocks_reversed, G.prod_sequential, G.prod_blocks64):
            bt.store(bt.emul(prod))
            rows, bad, gate = G.verdict(bt, bt.outputs())
            assert gate == "exact" and bad == [], (kw, bad)
        bt.C[0, 3, 4] += 1 if lp == torch.float16 or kw.get("out") == "f32" else 64       # one unit in one element (one representable step at these sizes)
        assert G.verdict(bt, bt.outputs())[1] != []


# -------------------------------------------------------------------------------------------------------------------------------------------
# planted defects
# -------------------------------------------------------------------------------------------------------------------------------------------
M_, N_, SMALL = 48, 64, 16
DEFECTS = ("drop one k element", "drop one 64-wide K-tile", "swap two rows of a 16-row tile", "swap the 4-column halves of an 8-column chunk",
           "8-column chunk from the neighbouring tile", "bias omitted on one column", "dropout index shifted by one", "rounded twice")


def _scenario(lp, K, exact, out16, plain=False):
    """Operands + a function (defect) -> the emulated output with that defect planted.  The random scenario has a small-magnitude row tile
    (rows 0..15 of A scaled by 2^-9): that is where a 2e-2 gate is blind.  Defects 0..5 sit in that tile.  ``plain``: the product alone
    (no bias, dropout or residual), the case the earlier tests ran most."""
    rn = G.rounder(lp)
    if exact:
        A, B = G.exact_a(1, M_, K, "cpu")[0], G.exact_b(1, K, N_, "cpu")[0]
        bias = ((torch.arange(N_) * 37 % 41 - 20) * 300.0)[None]           # large integers: the 16-bit output type has to round
        res = G.exact_small((M_, N_), "cpu", 13, 6)
        u = None
    else:
        A, B, bias, res, _, u = _rand_case(M_, N_, K, lp, seed=3, small_rows=SMALL)
        if plain:
            bias, res = torch.zeros_like(bias), torch.zeros_like(res)
    ldc = N_ + 8
    idx = G.drop_index(1, 0, 0, 0, M_, N_, ldc, "cpu")[0]
    out_rnd = rn if out16 else G.ident

    def run(defect=None):
        a, b, bs = A.clone(), B, bias.expand(M_, N_).clone()
        mult = None if exact or plain else G.mult_from_uniform(u, 0.1, idx + (1 if defect == 6 else 0))
        if defect == 0:
            a[:SMALL, K // 2] = 0
        if defect == 1:
            a[:SMALL, :64] = 0
        if defect == 5:
            bs[:SMALL, int(bias.abs().argmax())] = 0
        v = G.prod_blocks64(a, b) + bs
        if mult is not None:
            v = v * mult.float()
        if defect == 7:
            v = rn(v)                                                     # the 16-bit value, then the residual, then 16 bits again
        v = out_rnd(v + res)
        if defect == 2:
            v[[3, 9]] = v[[9, 3]]
        if defect == 3:
            v[:SMALL, 8:16] = torch.cat([v[:SMALL, 12:16], v[:SMALL, 8:12]], 1)
        if defect == 4:
            v[:SMALL, 8:16] = v[:SMALL, 24:32]
        return v

    mult = None if exact or plain else G.mult_from_uniform(u, 0.1, idx)
    r64, _ = G.ref_gemm(A, B, torch.float64, bias=bias, mult=mult, res=res)
    em, _ = G.ref_gemm(A, B, torch.float32, bias=bias, mult=mult, res=res, rnd=out_rnd, prod=G.prod_blocks_reversed)
    sa, _ = G.sum_abs(A, B, bias=bias, mult=mult, res=res)
    return run, r64, em, sa


@pytest.mark.parametrize("lp", LPS)
@pytest.mark.parametrize("K", [min(G.all_ks()), max(G.all_ks())])
def test_planted_defects_fail(lp, K):
    """Each defect, planted on a correct result, is rejected by gate_sum (float32 output), by judge (16-bit output) or by the exact law; the table
    of who caught what is printed.  The earlier 2e-2 + 2e-2 |ref| gate accepts at least the first and the fifth."""
    gates = {}
    run, r64, em, sa = _scenario(lp, K, exact=False, out16=False)
    assert G.gate_sum("C", run(), r64, em, sa)[1] == [] and G.old_gate_passes(run(), r64)
    gates["gate_sum"] = lambda d, run=run, r64=r64, em=em, sa=sa: G.gate_sum("C", run(d), r64, em, sa)[1] != []
    runp, r64p, emp, sap = _scenario(lp, K, exact=False, out16=False, plain=True)
    assert G.gate_sum("C", runp(), r64p, emp, sap)[1] == [] and G.old_gate_passes(runp(), r64p)
    gates["gate_sum (product alone)"] = lambda d: d > 4 or G.gate_sum("C", runp(d), r64p, emp, sap)[1] != []
    old = lambda d: G.old_gate_passes(runp(d), r64p)
    run16, r64b, emb, _ = _scenario(lp, K, exact=False, out16=True)
    assert G.judge(lp, dict(C=run16()), dict(C=r64b), dict(C=emb))[1] == []
    gates["judge"] = lambda d: G.judge(lp, dict(C=run16(d)), dict(C=r64b), dict(C=emb))[1] != []
    for out16 in (False, True):
        runx, r64x, _, _ = _scenario(lp, K, exact=True, out16=out16)
        want = r64x.to(lp if out16 else torch.float32)
        assert torch.equal(runx().to(want.dtype), want)                       # the law holds without a defect
        gates["exact " + ("16-bit" if out16 else "float32")] = lambda d, runx=runx, want=want: not torch.equal(runx(d).to(want.dtype), want)
    print()
    for d, name in enumerate(DEFECTS):
        if d == 6:
            caught = [g for g in ("gate_sum", "judge") if gates[g](d)]          # the exact law runs without dropout
        elif d == 7:
            caught = [g for g in ("judge", "exact 16-bit") if gates[g](d)]      # only a 16-bit output can be rounded twice
        else:
            caught = [g for g, f in gates.items() if f(d) and not (d > 4 and "alone" in g)]
        was_ok = old(d) if d < 5 else None
        print(f"K={K} {lp}: {name:<48s} caught by {', '.join(caught) or 'NOTHING'}; the 2e-2 gate {'accepts' if was_ok else 'rejects' if was_ok is not None else 'n/a'}")
        assert caught, (name, K, lp)
        if d < 6:
            assert "gate_sum" in caught and "exact float32" in caught and "exact 16-bit" in caught, (name, caught)
        if d < 5:
            assert "gate_sum (product alone)" in caught, (name, caught)
        if d in (0, 4):
            assert was_ok, f"the 2e-2 gate was expected to accept: {name}"
