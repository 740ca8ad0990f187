"""The measuring stick of the GEMM tests (test_gemm_matrix_gpu.py judges the kernels with it, test_gemm_ref_cpu.py checks the stick itself): the
av_gemm contract of include/av_hip.h in plain PyTorch, device-agnostic, with no call into the library.

    v = alpha * A x B;  v += bias[n];  C2 = v;  activation;  v *= dropout multiplier;  v += R;  C = v
    AV_ACT_GELU_GF instead: C2 = gelu'(v) * mult, v = gelu(v) * mult

``ref_gemm`` is that statement in a working type; ref64 = float64 with nothing rounded; the emulation = the same operands, float32 accumulation
in an order that is not a kernel's (K blocks of 32 taken from the last to the first) and ONE rounding to the output type.  Its distance to ref64
is e_ref, the error a correct kernel of this precision is expected to have.

Gates (attention_ref.py / visual_ref.py; constants and functions are imported, not restated):
    judge       16-bit outputs: max|ours - ref64| <= FACTOR x e_ref, least-squares scale within SCALE_TOL for >= SCALE_MIN_NUMEL elements, finite;
    gate_sum    float32 outputs per element: FACTOR x max(e_ref, 64 EPS32 sum|v|), sum|v| = |alpha| (|A| @ |B|) + |bias| (times |aux| and the
                dropout multiplier where the epilogue multiplies) + |R| in float64.  That floor is a condition on float32 accumulation, not a
                measurement of a kernel: test_gemm_ref_cpu.py shows sequential, pairwise and 64-blocked float32 sums inside it at every K here;
    F32_TOL     float32 operands keep the float32 gate of test_kernels_gpu._tol;
    exact law   small asymmetric integer operands (i % 7 - 3 against j % 5 - 2, i = 3 m + k, j = k + 2 n), integer bias / aux / residual, alpha in {1, 0.5}: every partial
                sum stays below 2^24, so a float32 output equals the reference bit for bit and a 16-bit output equals the float64 result rounded
                once.  For AV_ACT_NONE, AV_ACT_MUL_AUX and the residual, without dropout.

Operands are handed to a kernel as views into larger allocations (``build``): lda / ldb wider than the logical row with NaN in the tail, 8 NaN rows
after the last operand row, outputs in [M + 8][ldc > N] buffers filled with a canary bit pattern whose live region starts as NaN; after a call the
canary must be bit-identical (``canary_intact``).  The case lists of the GPU matrix live here so that the CPU file runs over the same shapes."""
import math

import numpy as np
import torch

from attention_ref import EPS32, FACTOR, SCALE_MIN_NUMEL, SCALE_TOL, max_err, scale_dev  # noqa: F401  (re-exported for the two test files)
from visual_ref import LIBS, fmt, gate_sum, gelu, ident, judge, rounder  # noqa: F401

ACT_NONE, ACT_GELU, ACT_MUL_GELU_GRAD, ACT_GELU_GF, ACT_MUL_AUX = range(5)
ACT_NAMES = ("none", "gelu", "mul_gelu_grad", "gelu_gf", "mul_aux")
F32_TOL = dict(rtol=2e-5, atol=2e-5)                     # test_kernels_gpu._tol(torch.float32)
OLD_TOL = dict(rtol=2e-2, atol=2e-2)                     # the gate the GEMM tests had before this matrix; kept to show what it lets through
CANARY16, CANARY32 = 0x5A5B, 0x5A5B5A5B                  # finite in every type (bf16 / fp16 / fp32), so an aliased residual may start from it
PAD_ROWS = 8
P_DROP, SEED, STREAM = 0.1, 4242, 5


def gelu_grad(v):
    return 0.5 * (1.0 + torch.erf(v * (0.5 ** 0.5))) + v * torch.exp(-0.5 * v * v) * (1.0 / math.sqrt(2.0 * math.pi))


# -------------------------------------------------------------------------------------------------------------------------------------------
# the statement
# -------------------------------------------------------------------------------------------------------------------------------------------
def prod_matmul(a, b):
    return a @ b


def prod_blocks_reversed(a, b, blk=32):
    """float32 sum over K in blocks of ``blk`` taken from the last block to the first: no kernel's order."""
    K = a.shape[-1]
    acc = None
    for k0 in reversed(range(0, K, blk)):
        t = a[..., k0:k0 + blk] @ b[..., k0:k0 + blk, :]
        acc = t if acc is None else acc + t
    return acc


def prod_sequential(a, b):
    """One element of K after the other (what a scalar loop does)."""
    acc = torch.zeros(a.shape[:-1] + (b.shape[-1],), dtype=a.dtype, device=a.device)
    for k in range(a.shape[-1]):
        acc = acc + a[..., k:k + 1] * b[..., k:k + 1, :]
    return acc


def prod_pairwise(a, b):
    """Pairwise (tree) summation of the K products."""
    t = a.unsqueeze(-1) * b.unsqueeze(-3)                # [.., M, K, N]
    while t.shape[-2] > 1:
        if t.shape[-2] % 2:
            t = torch.cat([t, torch.zeros_like(t[..., :1, :])], -2)
        t = t[..., 0::2, :] + t[..., 1::2, :]
    return t[..., 0, :]


def prod_blocks64(a, b):
    """64-wide K-tiles first to last, each tile summed by matmul: the shape of a tiled kernel's sum."""
    acc = None
    for k0 in range(0, a.shape[-1], 64):
        t = a[..., k0:k0 + 64] @ b[..., k0:k0 + 64, :]
        acc = t if acc is None else acc + t
    return acc


def ref_gemm(A, B, wt, *, alpha=1.0, bias=None, act=ACT_NONE, aux=None, mult=None, res=None, rnd=ident, prod=prod_matmul):
    """-> (C, C2).  A [..., M, K], B [..., K, N] logical operands, bias [..., 1, N] or [N], aux / mult / res [..., M, N] (None = absent),
    everything converted to ``wt``; ``rnd`` is the one rounding to the output type."""
    c = lambda t: None if t is None else t.to(wt)
    v = prod(A.to(wt), B.to(wt)) * alpha
    if bias is not None:
        v = v + c(bias)
    m = c(mult)
    if act == ACT_GELU_GF:
        c2, v = gelu_grad(v), gelu(v)
        if m is not None:
            c2, v = c2 * m, v * m
    else:
        c2 = v
        if act == ACT_GELU:
            v = gelu(v)
        elif act == ACT_MUL_GELU_GRAD:
            v = v * gelu_grad(c(aux))
        elif act == ACT_MUL_AUX:
            v = v * c(aux)
        if m is not None:
            v = v * m
    if res is not None:
        v = v + c(res)
    return rnd(v), rnd(c2)


def sum_abs(A, B, *, alpha=1.0, bias=None, act=ACT_NONE, aux=None, mult=None, res=None):
    """float64 sum of the magnitudes of the summands of C (the gate_sum floor).  Only for epilogues that are sums and exact multiplies."""
    assert act in (ACT_NONE, ACT_MUL_AUX)
    s = (A.double().abs() @ B.double().abs()) * abs(alpha)
    if bias is not None:
        s = s + bias.double().abs()
    c2 = s
    if act == ACT_MUL_AUX:
        s = s * aux.double().abs()
    if mult is not None:
        s = s * mult.double()
    if res is not None:
        s = s + res.double().abs()
    return s, c2


def split_k(A, B, chunk, wt, prod=prod_matmul):
    """Partial products [S, M, N] of K slices of ``chunk`` (the last may be ragged): what av_gemm writes with k_total."""
    K = A.shape[-1]
    return torch.stack([prod(A[..., k0:k0 + chunk].to(wt), B[..., k0:k0 + chunk, :].to(wt)) for k0 in range(0, K, chunk)])


def sum_slices(parts, alpha, out=None):
    """av_sum_slices in the type of ``parts``: out = (out if accumulate) + alpha * sum_s parts[s]."""
    s = parts[0]
    for t in parts[1:]:
        s = s + t
    s = s * alpha
    return s if out is None else out.to(parts.dtype) + s


# -------------------------------------------------------------------------------------------------------------------------------------------
# dropout multiplier
# -------------------------------------------------------------------------------------------------------------------------------------------
def inv_keep(p):
    """The factor of a survivor: 65536 / (65536 - ceil(65536 p)) in float32 (the kept fraction the 16-bit keep test realises)."""
    thr = min(np.ceil(np.float32(p) * np.float32(65536.0)), np.float32(65535.0))
    return float(np.float32(65536.0) / (np.float32(65536.0) - np.float32(thr)))


def drop_index(Z, inner, sC, oC, M, N, ldc, device):
    """Element index of (z, m, n): batch offset (zo oC + zi sC; z sC with one level) + m ldc + n -> int64 [Z, M, N]."""
    z = torch.arange(Z, device=device)
    base = (z // inner) * oC + (z % inner) * sC if inner > 0 else z * sC
    return base[:, None, None] + torch.arange(M, device=device)[None, :, None] * ldc + torch.arange(N, device=device)[None, None, :]


def mult_from_uniform(u, p, idx):
    """u: the stream's draws in [0, 1) by element index (av_dropout_uniform); -> float64 multiplier of the elements ``idx``."""
    return (u[idx] >= p).double() * inv_keep(p)


# -------------------------------------------------------------------------------------------------------------------------------------------
# cases
# -------------------------------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(inp="lp", out="lp", a="rm", b="nk", act=ACT_NONE, bias=False, c2=False, drop=0.0, res=None, aux=None, alpha=1.0, batch=1,
                inner=0, exact=False, a_pad=8, b_pad=8, c_pad=8, r_pad=None, a_off=0, c_off=0, aux_off=0, stats=False, expect=None)


def case(name, M, N, K, **kw):
    """One problem.  inp / out: "lp" (the library's 16-bit type) or "f32"; a: "rm" [M][K] / "km" [K][M]; b: "nk" [N][K] / "kn" [K][N];
    res: None / "f32" / "alias" (R is C itself); aux: None / "lp" / "f32"; *_pad: leading dimension minus the logical row; *_off: elements the
    pointer starts into its buffer; expect: fields of the launch record the case asserts."""
    d = dict(DEFAULTS)
    unknown = set(kw) - set(d)
    assert not unknown, unknown
    d.update(kw, name=name, M=M, N=N, K=K)
    if d["act"] in (ACT_MUL_GELU_GRAD, ACT_MUL_AUX) and d["aux"] is None:
        d["aux"] = "lp"
    return d


def case_id(c):
    return "%s-%dx%dx%d" % (c["name"], c["M"], c["N"], c["K"])


def epilogue_classes(prefix, M, N, K, expect, exact=True):
    """The epilogue classes of the persistent kernel's ten instantiations (five per NM1) at one shape, each with the exact law where it applies."""
    E = dict(expect)
    mk = lambda n, **kw: case(prefix + n, M, N, K, expect=dict(E, act=kw.get("act", ACT_NONE), out_dtype=0 if kw.get("out") == "f32" else 1), **kw)
    out = [mk("f32", out="f32"), mk("f32_bias", out="f32", bias=True), mk("f32_alias_half", out="f32", bias=True, res="alias", alpha=0.5),
           mk("lp", bias=True), mk("lp_res", bias=True, res="f32"),
           mk("gelu_c2", act=ACT_GELU, bias=True, c2=True), mk("gelu_c2_drop", act=ACT_GELU, bias=True, c2=True, drop=P_DROP),
           mk("gf_c2_drop", act=ACT_GELU_GF, bias=True, c2=True, drop=P_DROP),
           mk("mulaux_lp", act=ACT_MUL_AUX, aux="lp"), mk("mulaux_f32_drop", act=ACT_MUL_AUX, aux="f32", drop=P_DROP),
           mk("mulaux_lp_drop", act=ACT_MUL_AUX, aux="lp", drop=P_DROP), mk("mulaux_f32", act=ACT_MUL_AUX, aux="f32")]
    if exact:
        out += [mk("x_f32_alias_half", out="f32", bias=True, res="alias", alpha=0.5, exact=True), mk("x_lp_res", bias=True, res="f32", exact=True),
                mk("x_mulaux", act=ACT_MUL_AUX, aux="lp", exact=True)]
    return out


V7_KS = (64, 128, 192, 320)
V7 = dict(kernel="v7")
# v7, NM1 = 4 (AVAMD_GEMM_V7=2, AVAMD_GEMM_V4_BM=256, AVAMD_GEMM_V7_G=12): 300 x 264 = 2 x 2 tiles < G (no walk); 2100 x 712 = 9 x 3 = 27 tiles,
# 27 % 12 = 3 <= 6 so nfull = 24 and three tiles run as quadrant jobs, workgroups walk 1, 2 and 3 tiles, last row group gsz = 1, last row tile 52
# rows; 4700 x 256 = 19 tiles, 19 % 12 = 7 > 6: a full extra round.  Every epilogue class at the walked shape and K = 192 (odd number of K-tiles),
# the three shapes at every K with the two plainest classes.
V7_NM4_ENV = dict(AVAMD_GEMM_V7="2", AVAMD_GEMM_V4_BM="256", AVAMD_GEMM_V7_G="12")


def _v7_shapes(nm1, bm):
    e = dict(V7, nm1=nm1, bm_eff=bm)
    out = []
    for K in V7_KS:
        out.append(case("small_f32", 300, 264, K, out="f32", bias=True, expect=dict(e, nbM=2, nbN=2, nfull=4, grid_x=4)))
        out.append(case("walk_lp", 2100, 712, K, bias=True, res="f32", expect=dict(e, nbM=9, nbN=3, nfull=24, grid_x=12)))
        out.append(case("walk_x_f32", 2100, 712, K, out="f32", bias=True, exact=True, expect=dict(e, nbM=9, nbN=3, nfull=24, grid_x=12)))
        out.append(case("round_gelu", 4700, 256, K, act=ACT_GELU, bias=True, c2=True, expect=dict(e, nbM=19, nbN=1, nfull=19, grid_x=12)))
    return out


def v7_nm4_cases():
    e = dict(V7, nm1=4, bm_eff=256)
    out = _v7_shapes(4, 256)
    out += epilogue_classes("cls_", 2100, 712, 192, dict(e, nfull=24, grid_x=12))
    out += epilogue_classes("cls64_", 2100, 712, 64, dict(e, nfull=24, grid_x=12), exact=False)
    out.append(case("batch3", 300, 264, 128, batch=3, bias=True, res="f32", out="f32", expect=dict(e, grid_z=3, grid_x=4)))
    out.append(case("batch3_walk", 1100, 712, 128, batch=3, bias=True, res="f32", expect=dict(e, grid_z=3, grid_x=12, nfull=15)))
    out.append(case("batch6_inner2", 300, 264, 128, batch=6, inner=2, act=ACT_GELU, c2=True, drop=P_DROP, expect=dict(e, grid_z=6)))
    out.append(case("batch6_inner2_aux", 300, 264, 128, batch=6, inner=2, act=ACT_MUL_AUX, aux="lp", drop=P_DROP, expect=dict(e, grid_z=6)))
    return out


# v7, NM1 = 3 (AVAMD_GEMM_V4_BM=208): 1700 x 712 = 9 row tiles (36 rows in the last) x 3 = 27 tiles; the tile stages 256 rows and owns 208, so the
# canary rows below M and the NaN rows of A below M are what this group is about.  One case at 160 rows (V4_BM=160: 11 x 3 = 33 tiles, 33 % 12 = 9).
V7_NM3_ENV = dict(AVAMD_GEMM_V7="2", AVAMD_GEMM_V4_BM="208", AVAMD_GEMM_V7_G="12")


def v7_nm3_cases():
    e = dict(V7, nm1=3, bm_eff=208, nbM=9, nbN=3, nfull=24, grid_x=12)
    out = epilogue_classes("cls_", 1700, 712, 192, e) + epilogue_classes("cls64_", 1700, 712, 64, e, exact=False)
    out += [case("k128_lp", 1700, 712, 128, bias=True, res="f32", expect=e), case("k320_x_f32", 1700, 712, 320, out="f32", bias=True, exact=True, expect=e)]
    return out


def v7_bm160_cases():
    return [case("bm160", 1700, 712, 192, bias=True, res="f32", expect=dict(V7, nm1=3, bm_eff=160, nbM=11, nbN=3, nfull=33, grid_x=12))]


# v4 (AVAMD_GEMM_V7=0, AVAMD_GEMM_V4=2): every activation; the scalar epilogues with the FastFlags asserted; bm_eff by default and forced;
# quadrant jobs need > 256 tiles here (no G override): 4300 x 4040 = 17 x 16 = 272 tiles, nfull = 256, ragged M and N, with and without the tail.
V4_ENV = dict(AVAMD_GEMM_V7="0", AVAMD_GEMM_V4="2")


def v4_cases():
    e = dict(kernel="v4", bm_eff=256, c_vec=1)
    M, N = 600, 520
    out = []
    for K in (64, 192):
        out += [case("f32_alias_half", M, N, K, out="f32", bias=True, res="alias", alpha=0.5, expect=dict(e, r_vec=1)),
                case("x_lp_res", M, N, K, bias=True, res="f32", exact=True, expect=dict(e, r_vec=1)),
                case("gelu_c2_drop", M, N, K, act=ACT_GELU, bias=True, c2=True, drop=P_DROP, expect=e),
                case("gf_c2_drop", M, N, K, act=ACT_GELU_GF, bias=True, c2=True, drop=P_DROP, expect=e),
                case("mulgrad_drop", M, N, K, act=ACT_MUL_GELU_GRAD, aux="lp", drop=P_DROP, expect=dict(e, aux_vec=1)),
                case("mulaux_f32", M, N, K, act=ACT_MUL_AUX, aux="f32", out="f32", expect=dict(e, aux_vec=1)),
                case("x_mulaux", M, N, K, act=ACT_MUL_AUX, aux="lp", exact=True, expect=dict(e, aux_vec=1))]
    s = dict(kernel="v4", bm_eff=256)
    out += [case("n700_scalar", 600, 700, 128, bias=True, c_pad=3, act=ACT_GELU, c2=True, drop=P_DROP, expect=dict(s, c_vec=0)),
            case("n700_x_scalar", 600, 700, 128, bias=True, c_pad=3, res="f32", r_pad=4, exact=True, expect=dict(s, c_vec=0, r_vec=1)),
            case("c_off4", 600, 520, 128, bias=True, c_off=4, c2=True, act=ACT_GELU, expect=dict(s, c_vec=0)),
            case("ldr_odd", 600, 520, 128, bias=True, res="f32", r_pad=3, expect=dict(s, c_vec=1, r_vec=0)),
            case("aux_off4", 600, 520, 128, act=ACT_MUL_AUX, aux="lp", aux_off=4, expect=dict(s, c_vec=1, aux_vec=0)),
            case("batch3", 600, 520, 128, batch=3, bias=True, res="f32", expect=dict(s, grid_z=3)),
            case("batch6_inner2", 300, 264, 64, batch=6, inner=2, act=ACT_GELU, c2=True, drop=P_DROP, expect=dict(s, grid_z=6)),
            case("batch6_inner2_aux", 300, 264, 64, batch=6, inner=2, act=ACT_MUL_AUX, aux="f32", out="f32", drop=P_DROP, expect=dict(s, grid_z=6))]
    q = dict(kernel="v4", bm_eff=256, nbM=17, nbN=16, nfull=256, grid_x=256 + 4 * 16)
    out += [case("quadrants", 4300, 4040, 64, bias=True, res="f32", expect=q), case("quadrants_x", 4300, 4040, 192, bias=True, exact=True, out="f32", expect=q)]
    return out


def v4_bm176_cases():
    return [case("bm176", 600, 520, 128, bias=True, res="f32", expect=dict(kernel="v4", bm_eff=176, nbM=4, nbN=3))]


def v4_notail_cases():
    return [case("no_tail", 4300, 4040, 64, bias=True, res="f32", expect=dict(kernel="v4", bm_eff=256, nbM=17, nbN=16, nfull=272, grid_x=272))]


# v2 and the 128 x 128 kernel (AVAMD_GEMM_V4=0, AVAMD_GEMM_V2=1): v2 needs M >= 512; below that the same epilogues land on the 128 x 128 kernel.
V2_ENV = dict(AVAMD_GEMM_V4="0", AVAMD_GEMM_V2="1")


def _all_epilogues(M, N, K, e):
    return [case("f32_alias_half", M, N, K, out="f32", bias=True, res="alias", alpha=0.5, expect=e),
            case("x_lp_res", M, N, K, bias=True, res="f32", exact=True, expect=e),
            case("gelu_c2_drop", M, N, K, act=ACT_GELU, bias=True, c2=True, drop=P_DROP, expect=e),
            case("gf_c2_drop", M, N, K, act=ACT_GELU_GF, bias=True, c2=True, drop=P_DROP, expect=e),
            case("mulgrad", M, N, K, act=ACT_MUL_GELU_GRAD, aux="lp", expect=e),
            case("x_mulaux", M, N, K, act=ACT_MUL_AUX, aux="lp", exact=True, expect=e),
            case("batch3", M, N, K, batch=3, bias=True, res="f32", expect=dict(e, grid_z=3))]


def v2_cases():
    out = []
    for K in (64, 192):
        out += _all_epilogues(600, 264, K, dict(kernel="v2", nbM=3, nbN=3)) + _all_epilogues(1000, 520, K, dict(kernel="v2", nbM=4, nbN=5))
        out += _all_epilogues(500, 264, K, dict(kernel="fast128", bn=128, akm=0, bkm=0, conv=0))
    return out


# default process: the 128 x 128 kernel and its fast_tail store path (full column tile, 16-bit output, no C2 / activation / dropout / R) against
# its ragged-N neighbour; the 64-wide form; the three k-major forms with ragged K where the form allows it (both operands k-major) and the exact law.
def default_cases():
    f = dict(kernel="fast128", bn=128, conv=0, akm=0, bkm=0)
    out = []
    for K in (64, 192):
        out += [case("tail_store", 300, 256, K, expect=f), case("tail_store_x", 300, 256, K, exact=True, expect=f),
                case("tail_neighbour", 300, 264, K, expect=f), case("tail_neighbour_x", 300, 264, K, exact=True, expect=f)]
        out += _all_epilogues(300, 264, K, f)
    for N in (8, 40, 64):
        e64 = dict(kernel="fast128", bn=64)
        out += [case("narrow", 300, N, 128, bias=True, res="f32", expect=e64), case("narrow_x_f32", 300, N, 64, out="f32", bias=True, exact=True, expect=e64),
                case("narrow_gelu", 300, N, 192, act=ACT_GELU, bias=True, c2=True, drop=P_DROP, expect=e64)]
    ka, kb, kab = dict(f, akm=1), dict(f, bkm=1), dict(f, akm=1, bkm=1)
    out += [case("akm", 264, 200, 128, a="km", out="f32", bias=True, expect=ka), case("akm_x", 264, 200, 192, a="km", out="f32", exact=True, a_pad=24, expect=ka),
            case("akm_narrow_b", 264, 64, 64, a="km", bias=True, res="f32", expect=dict(kernel="fast128", bn=128, akm=1, bkm=0)),
            case("bkm", 300, 264, 128, b="kn", bias=True, res="f32", expect=kb), case("bkm_x", 300, 264, 192, b="kn", out="f32", exact=True, b_pad=24, expect=kb),
            case("bkm_narrow_a", 64, 264, 64, b="kn", out="f32", bias=True, expect=kb),
            case("abkm", 264, 520, 100, a="km", b="kn", out="f32", expect=kab), case("abkm_x", 264, 520, 777, a="km", b="kn", out="f32", exact=True, a_pad=24, b_pad=40, expect=kab),
            case("abkm_x_half", 136, 200, 100, a="km", b="kn", out="f32", exact=True, alpha=0.5, res="alias", expect=kab),
            case("abkm_lp", 520, 1024, 64, a="km", b="kn", bias=True, expect=kab)]
    return out


# v6 (AVAMD_GEMM_V6=1): the three shapes of test_four_wavefront_gemm_kernel_behind_its_switch under these gates.
V6_ENV = dict(AVAMD_GEMM_V6="1")


def v6_cases():
    out = []
    for M, N, K in ((1000, 520, 192), (2048, 1024, 1024), (300, 264, 64)):
        e = dict(kernel="v6")
        out += [case("f32", M, N, K, out="f32", expect=e), case("f32_bias_res", M, N, K, out="f32", bias=True, res="f32", expect=e),
                case("gelu", M, N, K, act=ACT_GELU, bias=True, expect=e), case("x_lp_res", M, N, K, bias=True, res="f32", exact=True, expect=e)]
    return out


# fallbacks to gemm.hip: one case per refusal of av_gemm_fast_try, with the generic kernel asserted; then the fp32 generic kernel over
# {row-major, k-major A} x {NK, KN} x {N <= 64, N > 64} x {vector, scalar loads} (the generic kernel has no k-major A with an NK B).
def fallback_cases():
    g = dict(kernel="generic", in16=1)
    out = [case("k72", 200, 136, 72, bias=True, res="f32", expect=dict(g, bn=128)), case("k40", 200, 136, 40, bias=True, act=ACT_GELU, c2=True, expect=dict(g, bn=128)),
           case("lda_odd", 200, 136, 64, a_pad=4, bias=True, expect=dict(g, bn=128)), case("a_off4", 200, 136, 64, a_off=4, out="f32", exact=True, expect=dict(g, bn=128)),
           case("akm_m_odd", 204, 136, 64, a="km", b="kn", a_pad=4, out="f32", bias=True, expect=dict(g, bn=128, akm=1, bkm=1)),
           case("bkm_narrow", 200, 64, 64, b="kn", bias=True, res="f32", expect=dict(g, bn=64, bkm=1)),
           case("stats", 200, 136, 64, bias=True, stats=True, expect=dict(g, bn=128))]
    for M, N, K in ((70, 50, 33), (257, 129, 95)):
        for a, b in (("rm", "nk"), ("rm", "kn"), ("km", "kn")):
            for vec in (True, False):                     # ld a multiple of four floats (16-byte loads) or one more than that
                pad = lambda row: 8 + (4 - row % 4) % 4 + (0 if vec else 1)
                out.append(case("f32_%s_%s_%s" % (a, b, "vec" if vec else "scalar"), M, N, K, inp="f32", out="f32", a=a, b=b, bias=True, res="f32",
                                a_pad=pad(M if a == "km" else K), b_pad=pad(N if b == "kn" else K),
                                expect=dict(kernel="generic", in16=0, bn=64 if N <= 64 else 128, akm=int(a == "km"), bkm=int(b == "kn"))))
    return out


GROUPS = {                                               # name -> (switches of the child process or None for this process, case list)
    "v7_nm4": (V7_NM4_ENV, v7_nm4_cases), "v7_nm3": (V7_NM3_ENV, v7_nm3_cases), "v7_bm160": (dict(V7_NM3_ENV, AVAMD_GEMM_V4_BM="160"), v7_bm160_cases),
    "v4": (V4_ENV, v4_cases), "v4_bm176": (dict(V4_ENV, AVAMD_GEMM_V4_BM="176"), v4_bm176_cases),
    "v4_notail": (dict(V4_ENV, AVAMD_GEMM_V4_TAIL="0"), v4_notail_cases), "v2": (V2_ENV, v2_cases), "v6": (V6_ENV, v6_cases),
    "km8": (dict(AVAMD_GEMM_KM8="2"), lambda: []),       # matmul_tn cases: KM8_SHAPES x KM8_KS, built by the GPU file
    "default": (None, default_cases), "fallback": (None, fallback_cases),
}
KM8_SHAPES = [(264, 520), (520, 1024)]                   # matmul_tn under AVAMD_GEMM_KM8=2
KM8_KS = [64, 100, 777, 1300]
SUM_SLICES = [(S, acc) for S in (1, 2, 8) for acc in (False, True)]
TRANSPOSE = [(999, 1024), (7, 13)]


def all_ks():
    ks = set(KM8_KS)
    for _, fn in GROUPS.values():
        ks |= {c["K"] for c in fn()}
    return sorted(ks)


# -------------------------------------------------------------------------------------------------------------------------------------------
# operand and output builders
# -------------------------------------------------------------------------------------------------------------------------------------------
def _gen(seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return g


def _randn(shape, g, device, scale=1.0):
    return torch.randn(shape, generator=g, device=device, dtype=torch.float32) * scale


def _ar(n, device):
    return torch.arange(n, device=device)


def exact_a(Z, M, K, device):
    """A[z][m][k] = i % 7 - 3 with i = z + 3 m + k: asymmetric at every K (a flat index m K + k is symmetric where K % 7 == 1, as at K = 64), and
    rows 16, 64, 128 or 256 apart, and k 64 apart, all differ."""
    return ((_ar(Z, device)[:, None, None] + 3 * _ar(M, device)[None, :, None] + _ar(K, device)[None, None, :]) % 7 - 3).float()


def exact_b(Z, K, N, device):
    """B[z][k][n] = j % 5 - 2 with j = z + k + 2 n: columns 4, 8, 16 or 128 apart differ."""
    return ((_ar(Z, device)[:, None, None] + _ar(K, device)[None, :, None] + 2 * _ar(N, device)[None, None, :]) % 5 - 2).float()


def exact_small(shape, device, mod, sub):
    n = int(np.prod(shape))
    return ((torch.arange(n, device=device).reshape(shape) * 7 % mod) - sub).float()


def geometry(Z, inner, rows, width):
    """-> (leading dimension, item stride, outer stride, elements) of Z items of ``rows`` (+ PAD_ROWS) rows of ``width`` elements.  One level
    (inner = 0): the items lie one after the other.  Two levels: the ``inner`` items of an outer group are interleaved inside the rows, as the
    heads of a packed projection are (ld = inner * width, item stride = width < rows * ld), and the outer groups follow each other after the
    pad rows - so zo * outer + zi * item is NOT z * item, and a kernel that ignores batch_inner reads and writes elsewhere."""
    if inner:
        assert Z % inner == 0
        ld = inner * width
        o = (rows + PAD_ROWS) * ld
        return ld, width, o, (Z // inner) * o
    s = (rows + PAD_ROWS) * width
    return width, s, 0, Z * s


def _live(flat, Z, rows, cols, width, off, inner=0):
    """The live region as a view: [Z, rows, cols] with one level, [Z / inner, inner, rows, cols] with two."""
    ld, s, o, total = geometry(Z, inner, rows, width)
    if inner:
        return flat.as_strided((Z // inner, inner, rows, cols), (o, s, ld, 1), flat.storage_offset() + off)
    return flat[off:off + total].view(Z, rows + PAD_ROWS, ld)[:, :rows, :cols]


def padded_operand(logical, dtype, width, off=0, inner=0):
    """logical [Z, rows, cols] -> (view of it (see _live) inside a NaN-filled allocation with PAD_ROWS more rows per item and ``width`` - cols
    NaN elements after every row, item stride in elements).  ``off``: elements the view starts into the allocation."""
    Z, rows, cols = logical.shape
    assert width >= cols
    _, s, _, total = geometry(Z, inner, rows, width)
    flat = torch.full((total + 8,), float("nan"), dtype=dtype, device=logical.device)
    v = _live(flat, Z, rows, cols, width, off, inner)
    v.copy_(logical.to(dtype).reshape(v.shape))
    return v, s


def canary_buffer(Z, M, N, width, dtype, inner=0):
    """-> (flat host allocation for Z outputs of [M + PAD_ROWS][width] (+ 8 elements) filled with the canary bit pattern, item stride)."""
    _, s, _, total = geometry(Z, inner, M, width)
    it = torch.int32 if dtype == torch.float32 else torch.int16
    flat = torch.full((total + 8,), CANARY32 if dtype == torch.float32 else CANARY16, dtype=it).view(dtype)
    return flat, s


def canary_intact(flat, Z, M, N, width, off, inner=0):
    """Everything of the allocation outside the live region still holds the canary bit pattern."""
    it = torch.int32 if flat.dtype == torch.float32 else torch.int16
    bits = flat.view(it).clone()
    _live(bits, Z, M, N, width, off, inner).fill_(CANARY32 if it == torch.int32 else CANARY16)
    return bool((bits == (CANARY32 if it == torch.int32 else CANARY16)).all())


class Built:
    """Operands of one case on ``device``: logical tensors (A [Z, M, K], B [Z, K, N], bias [Z, 1, N], aux / res [Z, M, N]; float32 holding values
    of the operand types), their padded storage views, the canary output buffers and the strides av_gemm needs (in elements)."""

    def __init__(self, c, lp, device, uniform=None):
        self.c, self.lp, self.device = c, lp, device
        M, N, K, Z = c["M"], c["N"], c["K"], c["batch"]
        self.Z = Z
        idt = lp if c["inp"] == "lp" else torch.float32
        self.odt = lp if c["out"] == "lp" else torch.float32
        g = _gen(M * 31 + N * 17 + K + c["act"], device)
        rin = rounder(idt)
        if c["exact"]:
            A, B = exact_a(Z, M, K, device), exact_b(Z, K, N, device)
        else:
            A, B = rin(_randn((Z, M, K), g, device)), rin(_randn((Z, K, N), g, device, 1.0 / math.sqrt(K)))
        self.A, self.B = A, B
        self.bias = self.aux = self.res = None
        if c["bias"]:
            self.bias = exact_small((Z, 1, N), device, 11, 5) if c["exact"] else _randn((Z, 1, N), g, device)
        if c["aux"]:
            adt = lp if c["aux"] == "lp" else torch.float32
            self.aux = exact_small((Z, M, N), device, 7, 3) if c["exact"] else rounder(adt)(_randn((Z, M, N), g, device))
        if c["res"]:
            self.res = exact_small((Z, M, N), device, 13, 6) if c["exact"] else _randn((Z, M, N), g, device)
        # storage
        inner = self.inner = c["inner"]
        assert not (inner and (c["bias"] or c["res"])), "bias and R have no outer stride in av_gemm_args"
        km, kn = c["a"] == "km", c["b"] == "kn"
        wa, wb, wc = (M if km else K) + c["a_pad"], (N if kn else K) + c["b_pad"], N + c["c_pad"]
        self.lda, self.sA, self.oA, _ = geometry(Z, inner, K if km else M, wa)
        self.ldb, self.sB, self.oB, _ = geometry(Z, inner, K if kn else N, wb)
        self.ldc, self.sC, self.oC, _ = geometry(Z, inner, M, wc)
        self.wc = wc
        self.sa, _ = padded_operand(A.transpose(1, 2) if km else A, idt, wa, c["a_off"], inner)
        self.sb, _ = padded_operand(B if kn else B.transpose(1, 2), idt, wb, 0, inner)
        self.c_off = c["c_off"]
        self.cflat = canary_buffer(Z, M, N, wc, self.odt, inner)[0].to(device)
        self.C = _live(self.cflat, Z, M, N, wc, self.c_off, inner)
        self.C.fill_(float("nan"))
        self.c2flat = self.C2 = None
        if c["c2"]:
            self.c2flat = canary_buffer(Z, M, N, wc, self.odt, inner)[0].to(device)
            self.C2 = _live(self.c2flat, Z, M, N, wc, self.c_off, inner)
            self.C2.fill_(float("nan"))
        self.sbias = self.saux = self.sr = None
        self.sBias = self.sR = 0
        if self.bias is not None:                         # [Z][N + 8]: a NaN tail after every item's bias
            self.sBias = N + 8
            bflat = torch.full((Z * self.sBias + 8,), float("nan"), device=device)
            self.sbias = bflat[:Z * self.sBias].view(Z, 1, self.sBias)[:, :, :N]
            self.sbias.copy_(self.bias)
        if self.aux is not None:                          # aux shares ldc and the batch strides of C
            self.saux, _ = padded_operand(self.aux, lp if c["aux"] == "lp" else torch.float32, wc, c["aux_off"], inner)
        self.ldr = self.ldc
        if c["res"] == "alias":
            assert self.odt == torch.float32
            self.C.copy_(self.res)
            self.sr, self.sR = self.C, self.sC
        elif c["res"]:
            self.ldr = N + (c["r_pad"] if c["r_pad"] is not None else 8 + (4 - N % 4) % 4)
            self.sr, self.sR = padded_operand(self.res, torch.float32, self.ldr)
        self.mult = None
        if c["drop"] > 0:
            assert uniform is not None, "a dropout case needs the stream's draws"
            idx = drop_index(Z, self.inner, self.sC, self.oC, M, N, self.ldc, device)
            self.mult = mult_from_uniform(uniform(int(idx.max()) + 1), c["drop"], idx)

    # ---- references -------------------------------------------------------------------------------------------------------------------
    def _kw(self):
        c = self.c
        return dict(alpha=c["alpha"], bias=self.bias, act=c["act"], aux=self.aux, mult=self.mult, res=self.res)

    def ref64(self):
        C, C2 = ref_gemm(self.A, self.B, torch.float64, **self._kw())
        return dict(C=C, C2=C2)

    def emul(self, prod=prod_blocks_reversed):
        rnd = rounder(self.lp) if self.c["out"] == "lp" else ident
        C, C2 = ref_gemm(self.A, self.B, torch.float32, rnd=rnd, prod=prod, **self._kw())
        return dict(C=C, C2=C2)

    def sum_abs(self):
        kw = self._kw()
        C, C2 = sum_abs(self.A, self.B, **kw)
        return dict(C=C, C2=C2)

    def exact_expected(self):
        """The float64 result rounded once to the output type (the exact law)."""
        r = self.ref64()
        return {k: v.to(self.odt) for k, v in r.items()}

    def _views(self):
        return dict(C=self.C) if self.C2 is None else dict(C=self.C, C2=self.C2)

    def outputs(self):
        """The live regions as [Z, M, N] tensors (a copy where the two-level layout cannot be viewed that way)."""
        c = self.c
        return {k: v.reshape(self.Z, c["M"], c["N"]) for k, v in self._views().items()}

    def store(self, res):
        """Write a result dict into the live regions (what a correct kernel does; the CPU file's stand-in for a launch)."""
        for k, v in self._views().items():
            v.copy_(res[k].to(v.dtype).reshape(v.shape))

    def canaries(self):
        c = self.c
        bad = []
        if not canary_intact(self.cflat, self.Z, c["M"], c["N"], self.wc, self.c_off, self.inner):
            bad.append("C: bytes outside the live M x N region changed")
        if self.c2flat is not None and not canary_intact(self.c2flat, self.Z, c["M"], c["N"], self.wc, self.c_off, self.inner):
            bad.append("C2: bytes outside the live M x N region changed")
        return bad


def verdict(bt, ours):
    """Judge the outputs ``ours`` (dict C, C2 -> tensors [Z, M, N]) of the built case ``bt``.  -> (rows, failures, name of the gate)."""
    c, lp = bt.c, bt.lp
    ours = {k: v for k, v in ours.items() if v is not None}
    if c["exact"]:
        exp = bt.exact_expected()
        it = torch.int32 if bt.odt == torch.float32 else torch.int16
        bad = []
        for k, v in ours.items():
            same = v.contiguous().view(it) == exp[k].contiguous().view(it)
            same |= (v == 0) & (exp[k] == 0)                         # +0 and -0 are the same number
            if not bool(same.all()):
                bad.append(f"{k}: {int((~same).sum())} of {same.numel()} elements differ from the once-rounded exact result (exact law)")
        return [(k, max_err(v, exp[k]), 0.0, 0.0, None) for k, v in ours.items()], bad, "exact"
    r64, em = bt.ref64(), bt.emul()
    if c["inp"] == "f32":
        bad = []
        for k, v in ours.items():
            try:
                torch.testing.assert_close(v.double(), r64[k], **F32_TOL)
            except AssertionError as e:
                bad.append(f"{k}: {str(e).splitlines()[0]} {str(e).splitlines()[-1]}")
        frac = lambda v, r: float(((v.double() - r).abs() / (F32_TOL["atol"] + F32_TOL["rtol"] * r.abs())).max())      # share of the tolerance used
        return [(k, max_err(v, r64[k]), max_err(em[k], r64[k]), frac(v, r64[k]), None) for k, v in ours.items()], bad, "f32_tol"
    if c["out"] == "lp":
        rows, bad = judge(lp, ours, r64, em)
        return rows, bad, "judge"
    sa = bt.sum_abs()
    rows, bad = [], []
    for k, v in ours.items():
        row, b = gate_sum(k, v, r64[k], em[k], sa[k])
        rows.append(row); bad += b
    return rows, bad, "gate_sum"


def old_gate_passes(ours, r64):
    """The 2e-2 + 2e-2 |ref| gate of the earlier GEMM tests."""
    try:
        torch.testing.assert_close(ours.double(), r64.double(), **OLD_TOL)
        return True
    except AssertionError:
        return False
