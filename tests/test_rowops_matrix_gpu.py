"""Every form of the kernels between the GEMMs that their dispatchers can reach - LayerNorm forward / backward, log_softmax, column sums, the
elementwise passes (rowops.hip), the fused feature-encoder layer 0 (audio_front.hip), the contrastive / loss helpers at the head of
loss_misc.hip and the data-dependent glue of the fusion module (fusion_misc.hip) - in both libraries (libavhip.so: bfloat16,
libavhip_f16.so: float16), against the plain float64 references of rowops_ref.py; never against another kernel of the library.

Gates (visual_ref.py, imported): 16-bit outputs by ``judge`` (max|ours - ref64| <= 4 x e_ref, e_ref = max|emul - ref64| of the
same-precision emulation; scale factor of outputs of >= 4096 elements; everything finite - output buffers start as NaN); float32 sums
(row mean, parameter gradients, column sums, slice sums, reductions, dfeat) by ``gate_sum`` (4 x max(e_ref, 64 eps32 sum|v|)); other
float32 results by ``gate_f32`` (4 x max(e_ref, eps32 |ref|)); float32-in / float32-out elementwise results by the project's float32 gate
(test_kernels_gpu._tol); indices, copies, casts and masks exactly.  A backward kernel is judged as a function of the operands it is
handed (the saved mean / rstd / y / norm are float32 tensors made by the emulation, and the reference reads the same numbers).
Each case prints family, shape and ours / e_ref = ratio (run with -s); the module prints the largest ratio per family at the end.  Which
branch a shape is for is written next to its list in rowops_ref.py."""
import pytest
import torch

import rowops_ref as R
import visual_ref as V
from conftest import pkg
from test_kernels_gpu import _tol
from test_visual_matrix_gpu import cu, library, nan, same_bits, shifted

pytestmark = pytest.mark.gpu

F64, F32, I64, U8 = torch.float64, torch.float32, torch.int64, torch.uint8
WORST = {}                                 # (family, library) -> largest ratio seen, printed when the module is done


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=list(V.LIBS))
def lib(request):
    with library(request.param) as lp:
        yield request.param, lp


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest ours / e_ref per family and library:")
        for (fam, mode), r in sorted(WORST.items()):
            print(f"  {fam:<22s} {mode}: {r:.2f}")


def call(name, *args):
    L = pkg("_lib")
    L.check(getattr(L.lib(), name)(*args), name)


def P(t, byte_offset=0):
    return None if t is None else t.data_ptr() + byte_offset


def S():
    return pkg("ops").stream()


def code(dtype):
    return 0 if dtype == F32 else 1                          # AV_F32 / "the library's 16-bit type"


def kinds(lp):
    return (("f32", F32), ("lp", lp))


class Case:
    """Collects the judged outputs of one case; ``done`` prints them, notes the ratios and fails on any message."""

    def __init__(self, family, libname, head):
        self.family, self.libname, self.head, self.rows, self.bad = family, libname, head, [], []

    def lp16(self, lp, name, ours, r64, em):
        rows, bad = V.judge(lp, {name: ours}, {name: r64}, {name: em})
        self.rows += rows; self.bad += bad

    def sums(self, name, ours, r64, em, sum_abs):
        row, bad = V.gate_sum(name, ours, r64, em, sum_abs)
        self.rows.append(row); self.bad += bad

    def f32(self, name, ours, r64, em):
        row, bad = V.gate_f32(name, ours, r64, em)
        self.rows.append(row); self.bad += bad

    def out(self, lp, dtype, name, ours, r64, em32):
        """An output that is float32 or 16-bit by ``dtype``: ``em32`` is the un-rounded float32 emulation."""
        if dtype == F32:
            self.f32(name, ours, r64, em32)
        else:
            self.lp16(lp, name, ours, r64, V.rounder(lp)(em32))

    def done(self):
        print(f"[{self.family} {self.libname}] {self.head}:", V.fmt(self.rows))
        for n, err, e_ref, ratio, sd in self.rows:
            if ratio == ratio and ratio != float("inf"):
                WORST[(self.family, self.libname)] = max(WORST.get((self.family, self.libname), 0.0), ratio)
        assert not self.bad, f"[{self.family} {self.libname}] {self.head}: " + "; ".join(self.bad)


def tol_case(family, libname, head, ours, r64):
    """float32 in, float32 out, elementwise: the project's float32 gate."""
    print(f"[{family} {libname}] {head}: float32 max err {V.max_err(ours, r64):.2e}")
    assert bool(torch.isfinite(ours).all()), f"[{family} {libname}] {head}: non-finite values"
    torch.testing.assert_close(ours, r64.to(F32), **_tol(F32))


def operand(values, dtype, aligned=True):
    """``values`` (float32, already holding values of ``dtype``) as a device tensor of ``dtype``; ``aligned`` False: one element off."""
    t = values.to(dtype).contiguous()
    if aligned:
        assert t.data_ptr() % 16 == 0
        return t
    t = shifted(t, off=1)
    assert t.data_ptr() % 8 != 0
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm forward (av_layernorm_fwd): R.LN_FWD x rows {1, 5, 77} x x {f32, 16-bit} x y {f32, 16-bit} x {none, GELU}
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_params(cols, g):
    return cu(1 + 0.3 * torch.randn(cols, generator=g)), cu(0.2 * torch.randn(cols, generator=g))


def run_ln_fwd(x, gamma, beta, y, act):
    rows, cols = y.shape
    mean, rstd = nan((rows,), F32), nan((rows,), F32)
    call("av_layernorm_fwd", P(x), code(x.dtype), P(gamma), P(beta), P(y), code(y.dtype), P(mean), P(rstd), rows, cols, R.LN_EPS, int(act), S())
    return mean, rstd


def ln_fwd_judge(c, lp, xv, gamma, beta, act, y, mean, rstd):
    r64 = R.layernorm(xv, gamma, beta, act)
    em = R.layernorm(xv, gamma, beta, act, F32)
    c.out(lp, y.dtype, "y", y, r64[0], em[0])
    c.sums("mean", mean, r64[1], em[1], xv.double().abs().mean(1))
    c.f32("rstd", rstd, r64[2], em[2])


@pytest.mark.parametrize("cols,al", R.LN_FWD)
def test_layernorm_forward(lib, cols, al):
    libname, lp = lib
    for rows in R.LN_FWD_ROWS:
        g = R.gen(cols, rows)
        gamma, beta = ln_params(cols, g)
        for xk, xdt in kinds(lp):
            xv = cu(R.randn((rows, cols), g, None if xk == "f32" else lp))
            x = operand(xv, xdt, al)
            for act in (False, True):
                for yk, ydt in kinds(lp):
                    y = nan((rows, cols), ydt)
                    mean, rstd = run_ln_fwd(x, gamma, beta, y, act)
                    c = Case("layernorm_fwd", libname, f"cols{cols} rows{rows} x={xk} y={yk} gelu={act} aligned={al}")
                    ln_fwd_judge(c, lp, xv, gamma, beta, act, y, mean, rstd)
                    c.done()


@pytest.mark.parametrize("cols,which", R.LN_SHIFT)
def test_layernorm_forward_vector_width_falls_back_when_misaligned(lib, cols, which):
    """One operand off 16-byte alignment at every vector width: the generic kernel runs and passes the same gate."""
    libname, lp = lib
    rows, g = 5, R.gen(cols, 3)
    gamma, beta = ln_params(cols, g)
    for xk, dt_ in kinds(lp):
        xv = cu(R.randn((rows, cols), g, None if xk == "f32" else lp))
        x = operand(xv, dt_, which != "x")
        gm = shifted(gamma, off=1) if which == "gamma" else gamma
        y = shifted(nan((rows, cols), dt_), off=1) if which == "y" else nan((rows, cols), dt_)
        assert any(t.data_ptr() % (16 if t.dtype == F32 else 8) for t in (x, gm, y))
        mean, rstd = run_ln_fwd(x, gm, beta, y, True)
        c = Case("layernorm_fwd", libname, f"cols{cols} rows{rows} {xk} {which} misaligned")
        ln_fwd_judge(c, lp, xv, gamma, beta, True, y, mean, rstd)
        c.done()


@pytest.mark.parametrize("cols", R.LN_OFFSET_COLS)
def test_layernorm_forward_large_common_offset(lib, cols):
    """Values 1000 +- 1 in float32: a variance taken as E[x^2] - mean^2 loses every digit; about the mean it does not."""
    libname, lp = lib
    xv = cu(R.offset_row(cols))
    gamma, beta = ln_params(cols, R.gen(cols, 9))
    y = nan((1, cols), F32)
    mean, rstd = run_ln_fwd(xv, gamma, beta, y, False)
    c = Case("layernorm_fwd", libname, f"cols{cols} values 1000 +- 1")
    ln_fwd_judge(c, lp, xv, gamma, beta, False, y, mean, rstd)
    c.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward (av_layernorm_bwd / av_layernorm_bwd_drop): R.LN_BWD x rows {1, 5, 77, 1030} x x, dy {f32, 16-bit} x dres x
# parameter gradients; the 16-bit copy of dx with the residual cases (both PG instantiations see it and see it absent)
# ---------------------------------------------------------------------------------------------------------------------------------
def run_ln_bwd(x, dy, gamma, mean, rstd, dres, want_pg, lp_copy, lp, drop=None):
    rows, cols = x.shape
    nblk = R.ln_nblk(rows)
    dx = nan((rows, cols), F32)
    part = nan((nblk, 2, cols), F32) if want_pg else None
    dxl = nan((rows, cols), lp) if lp_copy else None
    args = (P(x), code(x.dtype), P(dy), code(dy.dtype), P(gamma), P(mean), P(rstd), P(dres), P(dx), P(part), nblk, rows, cols, P(dxl))
    if drop is None:
        call("av_layernorm_bwd", *args, S())
    else:
        call("av_layernorm_bwd_drop", *args, float(drop[0]), int(drop[1]), int(drop[2]), S())
    return dx, part, dxl


def ln_bwd_operands(lp, rows, cols, xk, dk, g, al=True):
    gamma, beta = ln_params(cols, g)
    xv = cu(R.randn((rows, cols), g, None if xk == "f32" else lp))
    dyv = cu(R.randn((rows, cols), g, None if dk == "f32" else lp))
    dres = cu(R.randn((rows, cols), g))
    _, mean, rstd = R.layernorm(xv, gamma, beta, False, F32)                     # the saved statistics: float32 tensors
    x = operand(xv, F32 if xk == "f32" else lp, al)
    dy = operand(dyv, F32 if dk == "f32" else lp)
    return gamma, xv, dyv, dres, mean.contiguous(), rstd.contiguous(), x, dy


def ln_bwd_judge(c, xv, dyv, gamma, mean, rstd, dres, dx, part):
    r64 = R.layernorm_bwd(xv, dyv, gamma, mean, rstd, dres)
    em = R.layernorm_bwd(xv, dyv, gamma, mean, rstd, dres, F32)
    c.f32("dx", dx, r64[0], em[0])
    if part is not None:
        tot = part.double().sum(0)
        c.sums("dgamma", tot[0], r64[1], em[1], r64[3])
        c.sums("dbeta", tot[1], r64[2], em[2], r64[4])


@pytest.mark.parametrize("cols,al", R.LN_BWD)
def test_layernorm_backward(lib, cols, al):
    libname, lp = lib
    for rows in R.LN_BWD_ROWS:
        for xk, _ in kinds(lp):
            for dk, _ in kinds(lp):
                gamma, xv, dyv, dres, mean, rstd, x, dy = ln_bwd_operands(lp, rows, cols, xk, dk, R.gen(cols, rows, len(xk + dk)), al)
                for with_res in (False, True):
                    for want_pg in (False, True):
                        dx, part, dxl = run_ln_bwd(x, dy, gamma, mean, rstd, dres if with_res else None, want_pg, with_res, lp)
                        c = Case("layernorm_bwd", libname, f"cols{cols} rows{rows} x={xk} dy={dk} dres={with_res} param_grads={want_pg} aligned={al}")
                        ln_bwd_judge(c, xv, dyv, gamma, mean, rstd, dres if with_res else None, dx, part)
                        c.done()
                        if dxl is not None:
                            same_bits(dxl, dx.to(lp), f"cols{cols} rows{rows}: the 16-bit copy is not the rounding of dx")


@pytest.mark.parametrize("cols,p", R.LN_DROP)
def test_layernorm_backward_dropout_copy(lib, cols, p):
    """The copy is round16(dx * m) with m rebuilt from av_dropout_uniform; dx itself is what the call without dropout writes."""
    libname, lp = lib
    rows, seed, stream_id = 77, 0x1234567890AB, 7
    gamma, xv, dyv, dres, mean, rstd, x, dy = ln_bwd_operands(lp, rows, cols, "lp", "f32", R.gen(cols, 11))
    for want_pg in (True, False):
        dx0, _, dxl0 = run_ln_bwd(x, dy, gamma, mean, rstd, dres, want_pg, True, lp)
        dx, part, dxl = run_ln_bwd(x, dy, gamma, mean, rstd, dres, want_pg, True, lp, drop=(p, seed, stream_id))
        u = nan((rows, cols), F32)
        call("av_dropout_uniform", P(u), u.numel(), seed, stream_id, S())
        m = R.drop_mult(u, p)
        dropped = float((m == 0).float().mean())
        print(f"[layernorm_bwd {libname}] cols{cols} p={p} param_grads={want_pg}: dropped fraction {dropped:.4f}")
        assert abs(dropped - p) < 0.02
        same_bits(dx, dx0, "dropout changed dx itself")
        # equal as numbers (torch.equal: no NaN, every non-zero value bit for bit).  Not same_bits: a dropped negative element is -0 in
        # torch's product and +0 in the float16 library's vector form (measured: 509 / 2451 elements at p = 0.1 / 0.5, all of them dropped
        # ones with dx < 0, nothing else) - there the compiler turns the multiply and the conversion into one mixed-precision fused
        # multiply-add with an addend of +0, and (-0) + (+0) = +0.  The sign of a zero gradient changes nothing downstream.
        assert torch.equal(dxl, (dx * m).to(lp)), "the dropped-out copy is not round16(dx * m)"
        assert bool((dxl[m == 0] == 0).all()) and bool((dxl[m != 0].view(torch.int16) == (dx * m).to(lp)[m != 0].view(torch.int16)).all())
        same_bits(dxl0, dx0.to(lp), "the plain copy is not round16(dx)")
        c = Case("layernorm_bwd", libname, f"cols{cols} rows{rows} dropout p={p} param_grads={want_pg}")
        ln_bwd_judge(c, xv, dyv, gamma, mean, rstd, dres, dx, part)
        c.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# av_conv0_ln_gelu (audio_front.hip).  Weights differ along channel and tap (drawn per element; and one case with a single non-zero
# (c, j)), so a transposed LDS layout cannot pass.
# ---------------------------------------------------------------------------------------------------------------------------------
def conv0_operands(C, k, stride, L_out, g, single=False, B=2):
    T_in = (L_out - 1) * stride + k                                              # exactly: the clamped prefetch must not read past the last tap
    wav = cu(torch.randn(B, T_in, generator=g))
    w = torch.randn(C, k, generator=g) * k ** -0.5
    if single:
        w = torch.zeros(C, k)
        w[(5 * C) // 7, (2 * k) // 3] = 1.5
    bias, gamma, beta = (cu(torch.randn(C, generator=g) * s + o) for s, o in ((0.1, 0), (0.3, 1), (0.2, 0)))
    return wav, cu(w), bias, gamma, beta


def run_conv0(wav, w, bias, gamma, beta, out, L_out, stride):
    B, T_in = wav.shape
    C, k = w.shape
    call("av_conv0_ln_gelu", P(wav), P(w), P(bias), P(gamma), P(beta), P(out), code(out.dtype), B, T_in, L_out, C, k, stride, R.LN_EPS, S())
    return out


@pytest.mark.parametrize("L_out", R.CONV0_C512_LOUT)
def test_conv0_ln_gelu_c512(lib, L_out):
    libname, lp = lib
    C, k, stride = 512, 10, 5
    for single in (False, True):
        for with_bias in (True, False):
            wav, w, bias, gamma, beta = conv0_operands(C, k, stride, L_out, R.gen(L_out, single), single)
            b = bias if with_bias else None
            r64 = R.conv0_ln_gelu(wav, w, b, gamma, beta, L_out, stride)
            em = R.conv0_ln_gelu(wav, w, b, gamma, beta, L_out, stride, F32, V.rounder(lp))
            fast = run_conv0(wav, w, b, gamma, beta, nan((2, L_out, C), lp), L_out, stride)
            slow = run_conv0(wav, w, b, gamma, beta, shifted(nan((2, L_out, C), lp)), L_out, stride)       # 8 bytes off: the generic 16-bit kernel
            assert fast.data_ptr() % 16 == 0 and slow.data_ptr() % 16 == 8
            c = Case("conv0_c512", libname, f"L_out{L_out} bias={with_bias} single_weight={single}")
            c.lp16(lp, "c512", fast, r64, em)
            c.lp16(lp, "generic", slow, r64, em)
            c.done()


@pytest.mark.parametrize("C", R.CONV0_C)
def test_conv0_ln_gelu_generic(lib, C):
    libname, lp = lib
    for k, stride in R.CONV0_KS:
        for L_out in R.CONV0_LOUT:
            for with_bias in (True, False):
                single = (k, L_out, with_bias) == (3, 65, False)
                wav, w, bias, gamma, beta = conv0_operands(C, k, stride, L_out, R.gen(C, k, L_out), single)
                b = bias if with_bias else None
                r64 = R.conv0_ln_gelu(wav, w, b, gamma, beta, L_out, stride)
                em = R.conv0_ln_gelu(wav, w, b, gamma, beta, L_out, stride, F32)
                for ok, odt in kinds(lp):
                    if R.conv0_form(C, k, ok == "lp") == "c512":
                        continue                             # the fast form has its own test
                    out = run_conv0(wav, w, b, gamma, beta, nan((2, L_out, C), odt), L_out, stride)
                    c = Case("conv0_generic", libname, f"C{C} k{k} s{stride} L_out{L_out} out={ok} bias={with_bias} single_weight={single}")
                    c.out(lp, odt, "out", out, r64, em)
                    c.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# log_softmax
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", R.LSM_COLS)
def test_log_softmax_forward(lib, cols):
    libname, lp = lib
    for rows in R.LSM_ROWS:
        for xk, xdt in kinds(lp):
            xv = cu(R.randn((rows, cols), R.gen(cols, rows), None if xk == "f32" else lp, 3.0))
            if xk == "f32" and cols > 1:                     # a row whose spread needs the max subtraction
                xv[0] = cu(torch.linspace(-1e4, 1e4, cols)[torch.randperm(cols, generator=R.gen(cols))])
            x, y = xv.to(xdt), nan((rows, cols), F32)
            call("av_log_softmax_fwd", P(x), code(xdt), P(y), rows, cols, S())
            c = Case("log_softmax_fwd", libname, f"rows{rows} cols{cols} x={xk}")
            c.f32("y", y, R.log_softmax(xv), R.log_softmax(xv, F32))
            c.done()


@pytest.mark.parametrize("cols,pad_to", R.LSM_BWD)
def test_log_softmax_backward(lib, cols, pad_to):
    libname, lp = lib
    ldx = (cols + pad_to - 1) // pad_to * pad_to if pad_to else cols
    for rows in R.LSM_ROWS:
        g = R.gen(cols, rows, 5)
        y = R.log_softmax(cu(R.randn((rows, cols), g, None, 3.0))).to(F32).contiguous()
        dy = cu(R.randn((rows, cols), g))
        r64, em = R.log_softmax_bwd(y, dy, ldx), R.log_softmax_bwd(y, dy, ldx, F32)
        for ok, odt in kinds(lp):
            dx = nan((rows, ldx), odt)
            call("av_log_softmax_bwd_ld", P(y), P(dy), P(dx), code(odt), rows, cols, ldx, S())
            c = Case("log_softmax_bwd", libname, f"rows{rows} cols{cols} ldx{ldx} out={ok}")
            c.out(lp, odt, "dx", dx, r64, em)
            c.done()
            assert ldx == cols or bool((dx[:, cols:].float().view(torch.int32) == 0).all()), "the padding columns are not exact zeros"
            if ldx == cols:                                  # the entry point without a row stride
                dx2 = nan((rows, cols), odt)
                call("av_log_softmax_bwd", P(y), P(dy), P(dx2), code(odt), rows, cols, S())
                same_bits(dx2, dx, "av_log_softmax_bwd differs from av_log_softmax_bwd_ld with ldx = cols")


# ---------------------------------------------------------------------------------------------------------------------------------
# av_colsum: three kernels x rows {1, rows-per-block - 1, + 1, 3 x + 5} x the kernel's column counts x {plain, column slice (ld > cols),
# accumulate into a non-zero out, misaligned input (vector forms: falls back to the scalar kernel)}
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(R.COLSUM_COLS))
def test_colsum(lib, kind):
    libname, lp = lib
    dts = {"lp_vec": [("lp", lp)], "f32_vec": [("f32", F32)], "scalar": list(kinds(lp))}[kind]
    step = {"lp_vec": 8, "f32_vec": 4, "scalar": 3}[kind]
    for cols in R.COLSUM_COLS[kind]:
        for rows in R.colsum_rows(kind):
            for dk, dt_ in dts:
                for variant in ("plain", "slice", "accumulate") + (("misaligned",) if kind != "scalar" else ()):
                    g = R.gen(cols, rows, len(variant))
                    ld = cols + step if variant == "slice" else cols
                    assert R.colsum_form(dk == "lp", cols, ld, variant != "misaligned") == ("scalar" if variant == "misaligned" else kind)
                    full = cu(R.randn((rows, ld), g, None if dk == "f32" else lp))
                    x = operand(full, dt_, variant != "misaligned")
                    xv = full[:, :cols]
                    out0 = cu(torch.randn(cols, generator=g)) if variant == "accumulate" else None
                    out = out0.clone() if out0 is not None else nan((cols,), F32)
                    call("av_colsum", P(x), code(dt_), P(out), rows, cols, ld, int(out0 is not None), S())
                    r64, em, sabs = xv.double().sum(0), xv.sum(0), xv.double().abs().sum(0)
                    if out0 is not None:
                        r64, em, sabs = r64 + out0.double(), em + out0, sabs + out0.double().abs()
                    c = Case("colsum_" + kind, libname, f"rows{rows} cols{cols} ld{ld} {dk} {variant}")
                    c.sums("out", out, r64, em, sabs)
                    c.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# elementwise passes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slices,n,stride,al", R.SUM_SLICES)
def test_sum_slices(lib, n_slices, n, stride, al):
    libname, lp = lib
    g = R.gen(n_slices, n, stride)
    parts = operand(cu(torch.randn(n_slices * stride, generator=g)), F32, al)
    live = parts.view(n_slices, stride)[:, :n]
    for alpha in (1.0, -0.5):
        for acc in (False, True):
            out0 = cu(torch.randn(n, generator=g))
            out = out0.clone() if acc else nan((n,), F32)
            call("av_sum_slices", P(parts), n_slices, n, stride, alpha, P(out), int(acc), S())
            r64, em, sabs = alpha * live.double().sum(0), alpha * live.sum(0), abs(alpha) * live.double().abs().sum(0)
            if acc:
                r64, em, sabs = r64 + out0.double(), em + out0, sabs + out0.double().abs()
            c = Case("sum_slices", libname, f"S{n_slices} n{n} stride{stride} aligned={al} alpha={alpha} accumulate={acc} ({R.sum_slices_form(n, stride, al)})")
            c.sums("out", out, r64, em, sabs)
            c.done()


@pytest.mark.parametrize("n", R.CAST_N)
def test_cast_is_torchs_rounding(lib, n):
    """All four type pairs, aligned and one element off on either side: bit for bit torch's conversion, on rounding ties (both ways of
    "to even"), overflow to infinity, both infinities and signed zeros besides random values."""
    libname, lp = lib
    v = cu(R.cast_values(n, R.gen(n)))
    for sk, sdt in kinds(lp):
        for dk, ddt in kinds(lp):
            for where in ("aligned", "src", "dst"):
                src = operand(v.to(sdt).to(F32), sdt, where != "src")
                dst = shifted(nan((n,), ddt), off=1) if where == "dst" else nan((n,), ddt)
                call("av_cast", P(src), code(sdt), P(dst), code(ddt), n, S())
                same_bits(dst, v.to(sdt).to(ddt), f"av_cast {sk} -> {dk} n{n} {where}")
    print(f"[cast {libname}] n{n}: exact")


def test_axpby_and_mul_scalar(lib):
    libname, lp = lib
    n, g = 1027, R.gen(17)
    for xk, xdt in kinds(lp):
        xv = cu(R.randn((n,), g, None if xk == "f32" else lp))
        x, y0 = xv.to(xdt), cu(torch.randn(n, generator=g))
        y = y0.clone()
        call("av_axpby", 2.0, P(x), code(xdt), 0.5, P(y), n, S())
        tol_case("axpby", libname, f"x={xk} a=2 b=0.5", y, 2.0 * xv.double() + 0.5 * y0.double())
        y = nan((n,), F32)                                    # b == 0 must not read y
        call("av_axpby", -1.5, P(x), code(xdt), 0.0, P(y), n, S())
        tol_case("axpby", libname, f"x={xk} a=-1.5 b=0 onto NaN", y, -1.5 * xv.double())
    for m in (1, n):
        x, sc, y = cu(torch.randn(m, generator=g)), cu(torch.tensor([0.37])), nan((m,), F32)
        call("av_mul_scalar_dev", P(x), P(sc), P(y), m, S())
        tol_case("mul_scalar_dev", libname, f"n{m}", y, x.double() * sc.double())


def test_row_and_column_masks_are_exact(lib):
    """av_mask_rows, av_overwrite_rows, av_zero_feature_cols in float32 and 16-bit, sizes that are multiples of nothing, a random pattern,
    nothing masked and everything masked."""
    libname, lp = lib
    g = R.gen(23)
    rows, cols, B, T, H = 37, 13, 3, 5, 7
    embed = cu(torch.randn(cols, generator=g))
    for dk, dt_ in kinds(lp):
        x = cu(torch.randn(rows, cols, generator=g)).to(dt_)
        xb = cu(torch.randn(B, T, H, generator=g)).to(dt_)
        for pattern in ("random", "none", "all"):
            hit = {"random": cu(torch.rand(rows, generator=g) < 0.4), "none": torch.zeros(rows, dtype=torch.bool, device="cuda"),
                   "all": torch.ones(rows, dtype=torch.bool, device="cuda")}[pattern]
            y, keep, hit8 = x.clone(), (~hit).to(U8), hit.to(U8)
            call("av_mask_rows", P(y), code(dt_), P(keep), rows, cols, S())                          # the argument says which rows are KEPT
            same_bits(y, torch.where(hit[:, None], torch.zeros_like(x), x), f"av_mask_rows {dk} {pattern}")
            y = x.clone()
            call("av_overwrite_rows", P(y), code(dt_), P(hit8), P(embed), rows, cols, S())
            same_bits(y, torch.where(hit[:, None], embed.to(dt_)[None, :].expand(rows, cols), x), f"av_overwrite_rows {dk} {pattern}")
            hb = {"random": cu(torch.rand(B, H, generator=g) < 0.4), "none": torch.zeros(B, H, dtype=torch.bool, device="cuda"),
                  "all": torch.ones(B, H, dtype=torch.bool, device="cuda")}[pattern]
            y, hb8 = xb.clone(), hb.to(U8).contiguous()
            call("av_zero_feature_cols", P(y), code(dt_), P(hb8), B, T, H, S())
            same_bits(y, torch.where(hb[:, None, :], torch.zeros_like(xb), xb), f"av_zero_feature_cols {dk} {pattern}")
    print(f"[masks {libname}] exact")


# ---------------------------------------------------------------------------------------------------------------------------------
# loss side (loss_misc.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", R.L2_COLS)
def test_l2norm_forward_backward(lib, cols):
    libname, lp = lib
    rows, g = 6, R.gen(cols, 31)
    xc = torch.randn(rows, cols, generator=g)
    xc[1] = 0.0                                               # clamped by eps
    xc[2] *= 1e-13 / float(xc[2].norm())                      # a norm below eps
    x, dy = cu(xc), cu(torch.randn(rows, cols, generator=g))
    y, nrm = nan((rows, cols), F32), nan((rows,), F32)
    call("av_l2norm_fwd", P(x), P(y), P(nrm), rows, cols, R.L2_EPS, S())
    r64, em = R.l2norm(x), R.l2norm(x, F32)
    c = Case("l2norm", libname, f"cols{cols} forward")
    c.f32("y", y, r64[0], em[0]); c.f32("norm", nrm, r64[1], em[1])
    c.done()
    y_in, n_in = em[0].contiguous(), em[1].contiguous()      # the saved tensors of the backward: float32
    dx = nan((rows, cols), F32)
    call("av_l2norm_bwd", P(y_in), P(dy), P(n_in), P(dx), rows, cols, R.L2_EPS, S())
    c = Case("l2norm", libname, f"cols{cols} backward")
    c.f32("dx", dx, R.l2norm_bwd(y_in, dy, n_in), R.l2norm_bwd(y_in, dy, n_in, F32))
    c.done()


def test_lse_rows_chunked_merge(lib):
    """7 x 300 logits up to +-1 / 0.07 in a buffer of row stride 320 (the padding holds NaN): column chunks 128, 128, 44 merged by
    ``accumulate`` against ONE float64 log-sum-exp; the whole matrix in one call through both entry points; one column."""
    libname, lp = lib
    rows, cols, ld = 7, 300, 320
    buf = nan((rows, ld), F32)
    buf[:, :cols] = cu((torch.rand(rows, cols, generator=R.gen(41)) * 2 - 1) / 0.07)
    s = buf[:, :cols]
    lse64, sum64 = R.lse_rows(s)
    sabs = s.double().abs().sum(1)
    lse, rsum = nan((rows,), F32), nan((rows,), F32)
    em_l = em_s = None
    for i, (c0, c1) in enumerate(((0, 128), (128, 256), (256, 300))):
        call("av_lse_rows_chunk", P(buf, 4 * c0), P(lse), P(rsum), rows, c1 - c0, ld, int(i > 0), S())
        pl, ps = R.lse_rows(s[:, c0:c1], F32)
        em_l, em_s = (pl, ps) if i == 0 else (R.lse_merge(em_l, pl), em_s + ps)
    c = Case("lse_rows", libname, "7x300 ld320 chunks 128+128+44")
    c.f32("lse", lse, lse64, em_l); c.sums("rowsum", rsum, sum64, em_s, sabs)
    c.done()
    em_l, em_s = R.lse_rows(s, F32)
    for name, extra in (("av_lse_rows_chunk", (0,)), ("av_lse_rows", ())):
        lse, rsum = nan((rows,), F32), nan((rows,), F32)
        call(name, P(buf), P(lse), P(rsum), rows, cols, ld, *extra, S())
        c = Case("lse_rows", libname, f"7x300 ld320 one call ({name})")
        c.f32("lse", lse, lse64, em_l); c.sums("rowsum", rsum, sum64, em_s, sabs)
        c.done()
    lse, rsum = nan((rows,), F32), nan((rows,), F32)
    call("av_lse_rows_chunk", P(buf), P(lse), P(rsum), rows, 1, ld, 0, S())
    c = Case("lse_rows", libname, "one column")
    c.f32("lse", lse, s[:, 0].double(), s[:, 0]); c.sums("rowsum", rsum, s[:, 0].double(), s[:, 0], s[:, 0].double().abs())
    c.done()


def test_contrastive_dsim_chunk(lib):
    """A 7 x 300 chunk (row stride 320, NaN in the padding of the input) of a similarity matrix that is 428 columns wide in total: the uniform
    term is 1 / 428, the columns from 300 to 320 of the output are exact zeros."""
    libname, lp = lib
    rows, cols, ld, total, coef = 7, 300, 320, 428, 0.5 / 7
    buf = nan((rows, ld), F32)
    buf[:, :cols] = cu((torch.rand(rows, cols, generator=R.gen(43)) * 2 - 1) / 0.07)
    s = buf[:, :cols]
    lse = (R.lse_rows(s)[0] + 0.3).to(F32).contiguous()       # the row LSE of the whole matrix: larger than the chunk's
    for tc, name in ((total, "av_contrastive_dsim_chunk"), (cols, "av_contrastive_dsim")):
        r64, em = R.contrastive_dsim(s, lse, coef, tc, ld), R.contrastive_dsim(s, lse, coef, tc, ld, F32)
        for ok, odt in kinds(lp):
            out = nan((rows, ld), odt)
            call(name, P(buf), P(lse), P(out), code(odt), rows, cols, ld, coef, *((tc,) if tc != cols else ()), S())
            c = Case("contrastive_dsim", libname, f"7x300 ld320 total_cols{tc} out={ok}")
            c.out(lp, odt, "dsim", out, r64, em)
            c.done()
            assert bool((out[:, cols:].float().view(torch.int32) == 0).all()), "the columns beyond cols are not exact zeros"


@pytest.mark.parametrize("n", R.REDUCE_N)
def test_reduce_sum(lib, n):
    libname, lp = lib
    g = R.gen(n, 47)
    x = cu(torch.randn(n, generator=g))
    for scale in (1.0, 0.25):
        for acc in (False, True):
            out0 = cu(torch.randn(1, generator=g))
            out = out0.clone() if acc else nan((1,), F32)
            call("av_reduce_sum", P(x), n, P(out), scale, int(acc), S())
            r64, em, sabs = scale * x.double().sum().view(1), (scale * x.sum()).view(1), scale * x.double().abs().sum().view(1)
            if acc:
                r64, em, sabs = r64 + out0.double(), em + out0, sabs + out0.double().abs()
            c = Case("reduce_sum", libname, f"n{n} scale={scale} accumulate={acc}")
            c.sums("out", out, r64, em, sabs)
            c.done()


@pytest.mark.parametrize("n", R.COMBINE_N)
def test_loss_combine(lib, n):
    libname, lp = lib
    g = R.gen(n, 53)
    nll, w = cu(torch.rand(n, generator=g) * 80 + 1), cu(torch.rand(n, generator=g) / n)
    c1, c2 = cu(torch.tensor([0.83])), cu(torch.tensor([-1.7]))
    for a, b in ((c1, c2), (c1, None), (None, c2), (None, None)):
        out = nan((3,), F32)
        call("av_loss_combine", P(nll), P(w), P(a), P(b), 0.05, n, P(out), S())
        r64, sabs = R.loss_combine(nll, w, a, b, 0.05)
        c = Case("loss_combine", libname, f"n{n} c1={a is not None} c2={b is not None}")
        c.sums("total,l1,l2", out, r64, R.loss_combine(nll, w, a, b, 0.05, F32)[0], sabs)
        c.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# glue (fusion_misc.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,D", R.PERMUTE)
def test_permute_bt(lib, B, T, D):
    libname, lp = lib
    xv = cu(torch.randn(B, T, D, generator=R.gen(B, T, D)))
    for sdt, ddt in ((F32, lp), (lp, lp)):
        x = xv.to(sdt).contiguous()
        out = nan((T, B, D), ddt)
        call("av_permute_bt", P(x), code(sdt), P(out), code(ddt), B, T, D, S())
        same_bits(out, R.permute(x).to(ddt), f"av_permute_bt B{B} T{T} D{D} {sdt} -> {ddt}")
        back = nan((B, T, D), ddt)
        call("av_permute_bt", P(out), code(ddt), P(back), code(ddt), T, B, D, S())
        same_bits(back, x.to(ddt), f"av_permute_bt: the inverse call does not restore the input (B{B} T{T} D{D})")
    print(f"[permute_bt {libname}] B{B} T{T} D{D}: exact")


def test_gather_scatter_rows_and_class_order(lib):
    libname, lp = lib
    g = R.gen(61)
    n_src, n, D = 41, 57, 13
    src = cu(torch.randn(n_src, D, generator=g))
    idx = cu(torch.randint(0, n_src, (n,), generator=g))
    for ddt in (lp, F32):
        out = nan((n, D), ddt)
        call("av_gather_rows", P(src), code(F32), P(idx), P(out), code(ddt), n, D, S())
        same_bits(out, R.gather(src, idx).to(ddt), f"av_gather_rows f32 -> {ddt}")
    perm = cu(torch.randperm(n_src, generator=g))
    for alpha, acc in ((1.0, False), (-0.75, False), (0.5, True)):
        out0 = cu(torch.randn(n_src, D, generator=g))
        out = out0.clone() if acc else nan((n_src, D), F32)
        call("av_scatter_rows", P(src), P(perm), P(out), n_src, D, alpha, int(acc), S())
        tol_case("scatter_rows", libname, f"alpha={alpha} accumulate={acc}", out, R.scatter(src, perm, out0, alpha, acc))
    for m in R.CLASS_ORDER_N:
        mask = cu(torch.randint(-1, 6, (m,), generator=g))
        order = torch.full((m,), -1, dtype=I64, device="cuda")
        call("av_class_order", P(mask), m, P(order), S())
        assert torch.equal(order, R.class_order(mask)), f"av_class_order n{m}"
    print(f"[gather / class_order {libname}] exact")


@pytest.mark.parametrize("Tin,Tout", R.MASK_DOWN)
def test_mask_downsample(lib, Tin, Tout):
    libname, lp = lib
    m = torch.randint(0, 4, (3, Tin), generator=R.gen(Tin, Tout))
    out = torch.full((3, Tout), -1, dtype=I64, device="cuda")
    md = cu(m)
    call("av_mask_downsample", P(md), P(out), 3, Tin, Tout, S())
    assert torch.equal(out.cpu(), R.mask_downsample_torch(m, Tout)), f"av_mask_downsample {Tin} -> {Tout} is not F.interpolate(nearest)"
    print(f"[mask_downsample {libname}] {Tin} -> {Tout}: exact")


def run_gather_lerp(feat, mask, Tv, groups, dout):
    B, Ta, D = feat.shape
    ws = torch.zeros(B * Ta + B + groups, dtype=torch.int32, device="cuda")
    out, mout = nan((B, Tv, D), F32), torch.full((B, Tv), -1, dtype=I64, device="cuda")
    lens, dfeat = torch.full((B,), -1, dtype=I64, device="cuda"), nan((B, Ta, D), F32)
    fd, md, dd = cu(feat), cu(mask), cu(dout)
    call("av_fusion_gather_lerp_fwd", P(fd), P(md), P(ws), P(out), P(mout), P(lens), B, Ta, Tv, D, groups, S())
    call("av_fusion_gather_lerp_bwd", P(dd), P(ws), P(dfeat), B, Ta, Tv, D, groups, S())
    return out, mout, lens, dfeat


def host_lengths(mask, Ta, Tv, groups):
    T = pkg("model.trainer").MultimodalTrainer
    gs = mask.shape[0] // groups
    return torch.cat([T._fusion_lengths_host(mask[g * gs:(g + 1) * gs], Ta, Tv) for g in range(groups)])


def gather_lerp_operands(case, D):
    name, Ta, Tv, groups, counts = case
    g = R.gen(Ta, Tv, D, len(counts))
    mask = R.speech_mask(Ta, counts, g)
    return mask, torch.randn(len(counts), Ta, D, generator=g), torch.randn(len(counts), Tv, D, generator=g)


@pytest.mark.parametrize("D", R.GATHER_D)
@pytest.mark.parametrize("case", R.GATHER_LERP, ids=lambda c: c[0])
def test_fusion_gather_lerp(lib, case, D):
    libname, lp = lib
    name, Ta, Tv, groups, counts = case
    mask, feat, dout = gather_lerp_operands(case, D)
    want = R.gather_lerp_torch(feat, mask, Tv, groups, dout)                     # float32 F.interpolate path + autograd, on the CPU
    em = R.gather_lerp(feat, mask, Tv, groups, dout)
    mag = R.gather_lerp(feat.abs(), mask, Tv, groups, dout.abs())[3]
    out, mout, lens, dfeat = run_gather_lerp(feat, mask, Tv, groups, dout)
    assert torch.equal(mout.cpu(), want[1]), f"{name}: mask_out"
    assert torch.equal(lens.cpu(), want[2]) and torch.equal(lens.cpu(), host_lengths(mask, Ta, Tv, groups)), f"{name}: lens {lens.tolist()} != {want[2].tolist()}"
    tol_case("gather_lerp", libname, f"{name} Ta{Ta} Tv{Tv} D{D} groups{groups} counts{counts} out", out, cu(want[0]))
    c = Case("gather_lerp", libname, f"{name} Ta{Ta} Tv{Tv} D{D} groups{groups} backward")
    c.sums("dfeat", dfeat, cu(want[3]), cu(em[3]), cu(mag))
    c.done()


@pytest.mark.parametrize("D", R.GATHER_D)
@pytest.mark.parametrize("case", R.GATHER_LERP_EMPTY, ids=lambda c: c[0])
def test_fusion_gather_lerp_group_without_speech(lib, case, D):
    """Every item of a group (or of a batch of one) has no speech frame, Tm = 0: the defined result is zero rows, mask_out 0, length 0 and a
    zero gradient; the other group is untouched by it."""
    libname, lp = lib
    name, Ta, Tv, groups, counts = case
    mask, feat, dout = gather_lerp_operands(case, D)
    want = R.gather_lerp_torch(feat, mask, Tv, groups, dout)
    out, mout, lens, dfeat = run_gather_lerp(feat, mask, Tv, groups, dout)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dfeat).all())
    assert torch.equal(mout.cpu(), want[1]) and torch.equal(lens.cpu(), want[2]) and torch.equal(lens.cpu(), host_lengths(mask, Ta, Tv, groups))
    gs = len(counts) // groups
    for gi in range(groups):
        sl = slice(gi * gs, (gi + 1) * gs)
        if max(counts[sl]) == 0:
            assert float(out[sl].abs().sum()) == 0.0 and int(mout[sl].abs().sum()) == 0 and int(lens[sl].abs().sum()) == 0 and float(dfeat[sl].abs().sum()) == 0.0
    tol_case("gather_lerp", libname, f"{name} Ta{Ta} Tv{Tv} D{D} groups{groups} counts{counts} out", out, cu(want[0]))
    tol_case("gather_lerp", libname, f"{name} backward", dfeat, cu(want[3]))
