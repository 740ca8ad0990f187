"""Every attention kernel variant the dispatcher can launch (av_attention_short_fwd_try / _bwd_try, launch_fwd_short2, dispatch_d,
ops.attention_fwd / _bwd, fusion_xattn_fwd / _bwd), in both libraries (libavhip.so: bfloat16, libavhip_f16.so: float16), against the
plain-PyTorch references of attention_ref.py - never against another kernel of the library.

Rule for 16-bit operands (attention_ref.judge): max|ours - ref64| <= 4 x e_ref per output, e_ref = max|emul - ref64| of the
same-precision emulation; the least-squares scale factor of every output of >= 4096 elements within half an ulp of the output type
(2^-9 / 2^-12) of one; lse within max(4 e_ref, 64 eps32 max(1, max|S|)); an output whose exact value is identically zero (one valid
key) within 64 eps32 A.  float32 operands keep the project's float32 gates (1e-4 forward, 2e-4 backward, 1e-3 lse).  Every case also
asserts: all outputs finite (gradient buffers start as NaN), dk / dv rows >= klen exactly zero, and outputs bit-identical when the
K / V rows >= klen change from 1e4 to 0.  Each case prints family, shape and ours / e_ref = ratio per output (run with -s).

Which dispatcher branch a group of parameters is for is written next to it.  The dropout multiplier is built from av_dropout_uniform
as test_stochastic_gpu._mask does (that generator has its own tests and is not an attention kernel)."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

LIBS = {"bf16": torch.bfloat16, "fp16": torch.float16}
P_DROP, SEED, STREAM = 0.1, 4242, 11
MODES = ("none", "gen", "bits")            # no dropout / masks generated in-kernel (DROP 1) / ops.attention_dropmask keep bits (DROP 2)
PAD_VALUE = 1.0e4                          # what lies in K / V rows >= klen: large, finite (0 x NaN is NaN in the reference too)
WORST = {}                                 # (family, library) -> largest ratio seen, printed when the module is done
_warmed = set()


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def library(mode):
    """Precision mode ``mode`` for the duration of the block.  Before a library's first case one forward + backward runs on NaN operands and
    is thrown away, so that stale LDS / registers are more likely to hold NaN than zeros afterwards (hardening against reads of unstaged
    padding rows; nothing is asserted about it)."""
    P = pkg("precision")
    old = P.get_precision()
    P.set_precision(mode)
    try:
        if mode not in _warmed:
            _warmed.add(mode)
            ops = pkg("ops")
            lp = LIBS[mode]
            for T, D in ((256, 64), (300, 64), (100, 128)):
                x = torch.full((2, T, 3, 2, D), float("nan"), device="cuda", dtype=lp)
                o, lse = ops.attention_fwd(x[:, :, 0], x[:, :, 1], x[:, :, 2], None, D ** -0.5)
                d = torch.empty_like(x)
                ops.attention_bwd(x[:, :, 0], x[:, :, 1], x[:, :, 2], o, d[:, :, 0], d[:, :, 1], d[:, :, 2], None, D ** -0.5, o=o, lse=lse)
            torch.cuda.synchronize()
        yield LIBS[mode]
    finally:
        P.set_precision(old)


@pytest.fixture(params=list(LIBS))
def lib(request):
    with library(request.param) as lp:
        yield request.param, lp


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest ours / e_ref per family and library:")
        for (fam, mode), r in sorted(WORST.items()):
            print(f"  {fam:<18s} {mode}: {r:.2f}")


def _buf(shape, dtype, off, fill=None):
    """A tensor of ``shape`` that starts ``off`` elements into its allocation (off = 4 sixteen-bit elements: 8-byte aligned, not 16)."""
    n = int(np.prod(shape))
    flat = torch.empty(n + 8, device="cuda", dtype=dtype)
    t = flat[off:off + n].view(shape)
    if fill is None:
        t.copy_(torch.randn(shape, device="cuda").to(dtype))
    else:
        t.fill_(fill)
    return t


_klens, _bh = R.klens, R.batch_heads


def _mult(B, H, Tq, Tk, p=P_DROP, seed=SEED, stream=STREAM):
    """Dropout multiplier [B, H, Tq, Tk]: element (b, h, q, k) is draw ((b H + h) Tq + q) Tk4 + k of the stream, Tk4 = Tk rounded up to 4;
    survivors are scaled by the inverse of the realised keep fraction (thr = ceil(65536 p) sixteen-bit steps, in float32 like the kernels)."""
    L = pkg("_lib"); ops = pkg("ops")
    T4 = (Tk + 3) // 4 * 4
    n = B * H * Tq * T4
    u = torch.empty(n, device="cuda")
    L.check(L.lib().av_dropout_uniform(ops.ptr(u), n, seed, stream, ops.stream()))
    thr = np.ceil(np.float32(p) * np.float32(65536.0))
    inv = float(np.float32(65536.0) / (np.float32(65536.0) - np.float32(thr)))
    return ((u >= p).double() * inv).view(B, H, Tq, T4)[..., :Tk].contiguous()


class Case:
    """Operands of one problem in the layouts the model uses: self-attention from a packed [B, T, 3, H, D] buffer with the gradients
    written into packed views (w2v2.py), cross shapes from q [B, Tq, H, D] and a packed [B, Tk, 2, H, D] (fusion_module.py).  ``off`` = 4
    starts q / k / v / dq / dk / dv 4 elements into their buffers (the alignment fallback); o and do stay 16-byte aligned."""

    def __init__(self, dtype, B, H, Tq, Tk, D, klen=None, off=0, packed=None, seed=0):
        torch.manual_seed(1000 * Tq + Tk + D + seed)
        self.dtype, self.B, self.H, self.Tq, self.Tk, self.D = dtype, B, H, Tq, Tk, D
        self.scale = D ** -0.5
        packed = (Tq == Tk) if packed is None else packed
        if packed:
            qkv = _buf((B, Tq, 3, H, D), dtype, off); g = _buf((B, Tq, 3, H, D), dtype, off, float("nan"))
            self.q, self.k, self.v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
            self.dq, self.dk, self.dv = g[:, :, 0], g[:, :, 1], g[:, :, 2]
        else:
            self.q = _buf((B, Tq, H, D), dtype, off); self.dq = _buf((B, Tq, H, D), dtype, off, float("nan"))
            kv = _buf((B, Tk, 2, H, D), dtype, off); g = _buf((B, Tk, 2, H, D), dtype, off, float("nan"))
            self.k, self.v, self.dk, self.dv = kv[:, :, 0], kv[:, :, 1], g[:, :, 0], g[:, :, 1]
        self.do = torch.randn(B, Tq, H, D, device="cuda").to(dtype)
        self.klen_list = None if klen is None else [int(x) for x in klen]
        self.klen = None if klen is None else torch.tensor(self.klen_list, device="cuda", dtype=torch.int32)
        self.valid = [Tk] * B if klen is None else [min(max(1, x), Tk) for x in self.klen_list]
        self.fill_padding(PAD_VALUE)

    def fill_padding(self, value):
        for b, c in enumerate(self.valid):
            if c < self.Tk:
                self.k[b, c:] = value; self.v[b, c:] = value

    def run(self, mode, fused=True, bits_in_bwd=True):
        """Forward + backward of the library -> dict(o, lse, dq, dk, dv) (copies)."""
        ops = pkg("ops")
        dr = (P_DROP, SEED, STREAM) if mode != "none" else None
        mask = ops.attention_dropmask(self.B, self.H, self.Tq, self.Tk, dr, self.q.device) if mode == "bits" else None
        o, lse = ops.attention_fwd(self.q, self.k, self.v, self.klen, self.scale, drop=dr, drop_mask=mask)
        for g in (self.dq, self.dk, self.dv):
            g.fill_(float("nan"))
        kw = dict(o=o, lse=lse) if fused else {}
        ops.attention_bwd(self.q, self.k, self.v, self.do, self.dq, self.dk, self.dv, self.klen, self.scale, drop=dr,
                          drop_mask=mask if bits_in_bwd else None, **kw)
        return dict(o=o, lse=lse, dq=self.dq.clone(), dk=self.dk.clone(), dv=self.dv.clone())

    def refs(self, mode):
        mult = _mult(self.B, self.H, self.Tq, self.Tk) if mode != "none" else None
        a = (self.q, self.k, self.v, self.do, self.klen, self.scale, mult)
        return R.ref64(*a), (R.emul(self.dtype, *a) if self.dtype != torch.float32 else None)


def _same_bits(a, b, what):
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(a[n].view(torch.uint8), b[n].view(torch.uint8)), f"{what}: {n} differs"


def check(family, libname, c, mode, fused=True):
    """One case: run, judge against ref64 / emul, padding rules.  Returns the library's outputs."""
    ours = c.run(mode, fused)
    r64, em = c.refs(mode)
    head = f"[{family} {libname}] B{c.B} H{c.H} Tq{c.Tq} Tk{c.Tk} D{c.D} klen={c.klen_list} {mode}:"
    bad = []
    if c.dtype == torch.float32:                                           # the project's float32 gates
        line = []
        for n, tol in (("o", 1e-4), ("lse", 1e-3), ("dq", 2e-4), ("dk", 2e-4), ("dv", 2e-4)):
            err = R.max_err(ours[n], r64[n])
            line.append(f"{n} {err:.2e}")
            if not bool(torch.isfinite(ours[n]).all()):
                bad.append(f"{n}: non-finite values")
            elif not bool(((ours[n].double() - r64[n]).abs() <= tol + tol * r64[n].abs()).all()):
                bad.append(f"{n}: beyond rtol = atol = {tol:g} (max err {err:.3e})")
        print(head, "  ".join(line))
    else:
        rows, bad = R.judge(c.dtype, ours, r64, em, R.zero_bound(c.q, c.k, c.v, c.do, c.scale))
        print(head, R.fmt(rows))
        for n, err, e_ref, ratio, sd in rows:
            if n != "lse" and ratio == ratio and ratio != float("inf"):
                WORST[(family, libname)] = max(WORST.get((family, libname), 0.0), ratio)
    for b, cv in enumerate(c.valid):                                       # gradients of masked keys: exactly zero
        if cv < c.Tk and not (float(ours["dk"][b, cv:].float().abs().max()) == 0.0 and float(ours["dv"][b, cv:].float().abs().max()) == 0.0):
            bad.append(f"dk / dv rows >= klen of item {b} are not exactly zero")
    assert not bad, head + " " + "; ".join(bad)
    if any(cv < c.Tk for cv in c.valid):                                   # what lies in keys >= klen does not matter
        c.fill_padding(0.0)
        _same_bits(c.run(mode, fused), ours, head + " padding 1e4 -> 0")
        c.fill_padding(PAD_VALUE)
    return ours


# ---------------------------------------------------------------------------------------------------------------------------------
# whole-sequence kernels (16-bit, D = 64, T <= 256): attn_fwd_short2_kernel<NKP, 0 / 2>, attn_fwd_short_kernel<NKP, 1>,
# attn_bwd_short_kernel<0 / 1 / 2>.  NKP = ceil(Tk / 32): every NKP 1..8 at both edges.
# ---------------------------------------------------------------------------------------------------------------------------------
WHOLE_TK, WHOLE_CROSS = R.WHOLE_TK, R.WHOLE_CROSS


def whole_case(libname, lp, Tq, Tk, mode, family=None):
    B, H = _bh(min(Tq, Tk), 64)
    c = Case(lp, B, H, Tq, Tk, 64, klen=_klens(Tk, B))
    ours = check(family or f"whole/{mode}", libname, c, mode)
    if mode == "bits":                                                     # DROP 2 and DROP 1 backward: the same arithmetic, bit for bit
        other = c.run("bits", bits_in_bwd=False)
        for n in ("dq", "dk", "dv"):
            assert torch.equal(other[n].view(torch.int16), ours[n].view(torch.int16)), f"keep-bit and in-kernel-mask backward differ in {n}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Tk", WHOLE_TK)
def test_whole_sequence_self_attention(lib, Tk, mode):
    whole_case(*lib, Tk, Tk, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Tq,Tk", WHOLE_CROSS)
def test_whole_sequence_cross_shapes(lib, Tq, Tk, mode):
    whole_case(*lib, Tq, Tk, mode)


# ---------------------------------------------------------------------------------------------------------------------------------
# chunked kernels (16-bit, D = 64, T > 256, chunks of 128): attn_fwd_long_kernel<DROP>, attn_bwd_long_kv / _q_kernel<DROP>.
# klen: whole, one key into the second chunk, exactly a chunk edge, inside the first chunk.
# ---------------------------------------------------------------------------------------------------------------------------------
CHUNKED, CHUNKED_KLEN = R.CHUNKED, R.CHUNKED_KLEN


def chunked_case(libname, lp, Tq, Tk, mode, family="chunked"):
    c = Case(lp, 4, 2, Tq, Tk, 64, klen=[Tk] + CHUNKED_KLEN)
    check(family, libname, c, mode)


@pytest.mark.parametrize("mode", ("none", "gen"))
@pytest.mark.parametrize("Tq,Tk", CHUNKED)
def test_chunked(lib, Tq, Tk, mode):
    chunked_case(*lib, Tq, Tk, mode)


# ---------------------------------------------------------------------------------------------------------------------------------
# tiled kernels: attn_fwd_kernel<16-bit, D>, attn_bwd_kv / _q_kernel<D>, D in {16, 32, 128} (dispatch_d / launch_bwd); D = 128 at
# T = 375 is the fusion path of BASELINE configs[2] (T_v > 112)
# ---------------------------------------------------------------------------------------------------------------------------------
TILED = [(D, Tq, Tk, "none") for D, Tq, Tk in R.TILED] + [(128, 100, 100, "gen"), (128, 70, 130, "gen"), (128, 375, 375, "gen")]


@pytest.mark.parametrize("D,Tq,Tk,mode", TILED)
def test_tiled(lib, D, Tq, Tk, mode):
    B, H = _bh(min(Tq, Tk), D)
    check(f"tiled-D{D}", lib[0], Case(lib[1], B, H, Tq, Tk, D, klen=_klens(Tk, B)), mode)


# ---------------------------------------------------------------------------------------------------------------------------------
# tiled kernels with 16-bit operands at D = 64: the fallback when a view is not 16-byte aligned (vec_ok / al8 of the dispatcher).
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("none", "gen"))
@pytest.mark.parametrize("T", R.MISALIGNED_T)
def test_tiled_d64_through_the_alignment_fallback(lib, T, mode):
    c = Case(lib[1], 3, 2, T, T, 64, klen=_klens(T, 3), off=4)
    for t in (c.q, c.k, c.v, c.dq, c.dk, c.dv):
        assert t.data_ptr() % 16 == 8
    check("tiled-D64", lib[0], c, mode)


def test_keep_bits_are_refused_where_the_whole_sequence_kernel_does_not_run(lib):
    ops = pkg("ops")
    c = Case(lib[1], 2, 2, 49, 49, 64, off=4)
    dr = (P_DROP, SEED, STREAM)
    mask = ops.attention_dropmask(2, 2, 49, 49, dr, "cuda")
    with pytest.raises(RuntimeError, match="keep bits cannot be used"):
        ops.attention_fwd(c.q, c.k, c.v, None, c.scale, drop=dr, drop_mask=mask)
    o, lse = ops.attention_fwd(c.q, c.k, c.v, None, c.scale, drop=dr)
    with pytest.raises(RuntimeError, match="stored mask cannot be used"):
        ops.attention_bwd(c.q, c.k, c.v, c.do, c.dq, c.dk, c.dv, None, c.scale, o=o, lse=lse, drop=dr, drop_mask=mask)


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 (parity mode): attn_fwd_kernel<float, D> + the unfused backward (av_gemm, av_softmax_rows, av_softmax_bwd_rows, cast_dropout);
# and the unfused backward on 16-bit operands (ops.attention_bwd without o / lse)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [49, 199, 300, 749])
def test_float32_forward_and_unfused_backward(lib, T, D):
    B = 3 if T <= 300 else 2
    check(f"float32-D{D}", lib[0], Case(torch.float32, B, 2, T, T, D, klen=_klens(T, B)), "gen", fused=False)


@pytest.mark.parametrize("mode", ("none", "gen"))
def test_unfused_backward_on_16_bit_operands(lib, mode):
    check("unfused", lib[0], Case(lib[1], 3, 2, 199, 199, 64, klen=_klens(199, 3)), mode, fused=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# key lengths at the edges, one case per kernel family: 1, 15, 16, 17, Tk - 1, and the out-of-range 0 and Tk + 5 (clamped to [1, Tk])
# ---------------------------------------------------------------------------------------------------------------------------------
KLEN_EDGES = [("whole/none", 64, 199, "none", 0), ("whole/gen", 64, 199, "gen", 0), ("whole/bits", 64, 199, "bits", 0), ("whole/none", 64, 17, "none", 0),
              ("chunked", 64, 300, "none", 0), ("chunked", 64, 300, "gen", 0), ("tiled-D16", 16, 100, "none", 0), ("tiled-D32", 32, 100, "none", 0),
              ("tiled-D128", 128, 100, "gen", 0), ("tiled-D64", 64, 199, "gen", 4), ("float32-D64", 64, 199, "gen", 0), ("unfused", 64, 199, "gen", 0)]


@pytest.mark.parametrize("family,D,T,mode,off", KLEN_EDGES)
def test_key_length_edges(lib, family, D, T, mode, off):
    dtype = torch.float32 if family.startswith("float32") else lib[1]
    c = Case(dtype, 7, 2, T, T, D, klen=[1, 15, 16, 17, T - 1, 0, T + 5], off=off)
    assert c.valid == [1, 15, 16, min(17, T), T - 1, 1, T]
    check(family, lib[0], c, mode, fused=family not in ("float32-D64", "unfused"))


def test_one_valid_key_everywhere(lib):
    """Every klen = 1: softmax is 1, dq and dk are identically zero in ref64 (the exact-zero corner), in every family."""
    for family, D, Tq, Tk, off in (("whole/none", 64, 70, 130, 0), ("chunked", 64, 300, 300, 0), ("tiled-D128", 128, 100, 100, 0), ("tiled-D64", 64, 49, 49, 4)):
        check(family, lib[0], Case(lib[1], 3, 2, Tq, Tk, D, klen=[1, 1, 1], off=off), "none")


# ---------------------------------------------------------------------------------------------------------------------------------
# structure, bit-exact: the instantiation depends on T only, so a batch equals its items and its heads; nothing accumulates with float
# atomics, so a second call returns the same bits
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Tq,Tk,off", [(64, 33, 33, 0), (64, 199, 199, 0), (64, 70, 130, 0), (64, 300, 300, 0), (64, 130, 600, 0), (128, 100, 100, 0),
                                         (64, 199, 199, 4)])
def test_batch_and_head_slices_and_repeat_are_bit_identical(lib, D, Tq, Tk, off):
    ops = pkg("ops")
    B, H = 3, 2
    c = Case(lib[1], B, H, Tq, Tk, D, klen=_klens(Tk, B), off=off)
    full = c.run("none")
    _same_bits(c.run("none"), full, "second identical call")

    def part(sb, sh):
        q, k, v, do = (t[sb, :, sh] for t in (c.q, c.k, c.v, c.do))
        kl = c.klen[sb]
        o, lse = ops.attention_fwd(q, k, v, kl, c.scale)
        dq, dk, dv = (_buf(t.shape, t.dtype, off, float("nan")) for t in (q, k, v))
        ops.attention_bwd(q, k, v, do, dq, dk, dv, kl, c.scale, o=o, lse=lse)
        want = dict(o=full["o"][sb, :, sh], lse=full["lse"][sb, sh], dq=full["dq"][sb, :, sh], dk=full["dk"][sb, :, sh], dv=full["dv"][sb, :, sh])
        for n, got in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
            assert torch.equal(got.contiguous().view(torch.uint8), want[n].contiguous().view(torch.uint8)), (n, sb, sh)

    for b in range(B):
        part(slice(b, b + 1), slice(None))
    for h in range(H):
        part(slice(None), slice(h, h + 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# fusion attention (csrc/fusion_attn.hip: packed in-projection + 4 x 128 attention core per (item, head), T <= 112)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("T", [1, 7, 15, 16, 17, 96, 97, 111, 112])
def test_fusion_attention(lib, T, B):
    """The three projections against float64 with e_ref from a float32 product rounded to the 16-bit type; the attention core (which
    consumes the ROUNDED projections, as the unfused path does) and fusion_xattn_bwd under the common rule, fed the projections the
    forward stored."""
    ops = pkg("ops")
    libname, lp = lib
    E, nh, hd = 512, 4, 128
    torch.manual_seed(100 * T + B)
    rn = lambda *s: torch.randn(*s, device="cuda")
    a, v = rn(B, T, E).to(lp), rn(B, T, E).to(lp)
    w = (rn(3 * E, E) / E ** 0.5).to(lp); bias = rn(3 * E) * 0.1
    scale = hd ** -0.5
    o, q, kv, lse = ops.fusion_xattn_fwd(a, v, w, bias, nh, scale, True)
    head = f"[fusion {libname}] B{B} T{T}:"
    bad, line = [], []
    for name, x, got, lo in (("q", a, q, 0), ("k", v, kv[:, :, 0], E), ("v", v, kv[:, :, 1], 2 * E)):
        r64 = (x.double() @ w[lo:lo + E].double().t() + bias[lo:lo + E].double()).view(B, T, nh, hd)
        em = (x.float() @ w[lo:lo + E].float().t() + bias[lo:lo + E]).view(B, T, nh, hd).to(lp)
        err, e_ref = R.max_err(got, r64), R.max_err(em, r64)
        line.append(f"{name} {err:.2e}/{e_ref:.2e}={err / e_ref:.2f}")
        WORST[("fusion", libname)] = max(WORST.get(("fusion", libname), 0.0), err / e_ref)
        if not (bool(torch.isfinite(got.float()).all()) and err <= R.FACTOR * e_ref):
            bad.append(f"projection {name}: err {err:.3e} > 4 x e_ref {e_ref:.3e}")
        if got.numel() >= R.SCALE_MIN_NUMEL and not R.scale_dev(got, r64) <= R.SCALE_TOL[lp]:
            bad.append(f"projection {name}: scale factor off by {R.scale_dev(got, r64):.3e}")
    do = rn(B, T, nh, hd).to(lp)
    dq, dkv = ops.fusion_xattn_bwd(q, kv, o, do, lse, scale)
    args = (q, kv[:, :, 0], kv[:, :, 1], do, None, scale, None)
    r64, em = R.ref64(*args), R.emul(lp, *args)
    rows, bad2 = R.judge(lp, dict(o=o, lse=lse, dq=dq, dk=dkv[:, :, 0], dv=dkv[:, :, 1]), r64, em, R.zero_bound(q, kv[:, :, 0], kv[:, :, 1], do, scale))
    print(head, "  ".join(line), R.fmt(rows))
    for n, err, e_ref, ratio, sd in rows:
        if n != "lse" and ratio == ratio and ratio != float("inf"):
            WORST[("fusion", libname)] = max(WORST.get(("fusion", libname), 0.0), ratio)
    assert not (bad + bad2), head + " " + "; ".join(bad + bad2)
    o2, q2, kv2, lse2 = ops.fusion_xattn_fwd(a, v, w, bias, nh, scale, False)
    assert q2 is None and kv2 is None and lse2 is None and torch.equal(o2.view(torch.int16), o.view(torch.int16))


def test_fusion_attention_refuses_t_113(lib):
    ops = pkg("ops")
    lp = lib[1]
    a = torch.zeros(2, 113, 512, device="cuda", dtype=lp); w = torch.zeros(1536, 512, device="cuda", dtype=lp); b = torch.zeros(1536, device="cuda")
    with pytest.raises(RuntimeError, match="out of range"):
        ops.fusion_xattn_fwd(a, a, w, b, 4, 128 ** -0.5, True)
    x = torch.zeros(2, 113, 4, 128, device="cuda", dtype=lp); kv = torch.zeros(2, 113, 2, 4, 128, device="cuda", dtype=lp)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.fusion_xattn_bwd(x, kv, x, x, torch.zeros(2, 4, 113, device="cuda"), 128 ** -0.5)


# ---------------------------------------------------------------------------------------------------------------------------------
# drop probabilities that resolve to "keep nothing" (p >= 1 - 2^-16: thr = 65536): the survivors' factor used to be +inf
# ---------------------------------------------------------------------------------------------------------------------------------
def test_drop_probability_next_to_one_never_gives_nan(lib):
    """p = 1 - 2^-17 passes every drop_p < 1 check.  Each op either raises the library's error or returns finite values."""
    ops = pkg("ops"); L = pkg("_lib")
    libname, lp = lib
    p = 1.0 - 2.0 ** -17
    dr = (p, SEED, STREAM)

    def finite_or_error(what, fn):
        try:
            outs = fn()
        except RuntimeError as e:
            assert "libavhip" in str(e), (what, e)
            return
        torch.cuda.synchronize()
        for t in outs:
            assert bool(torch.isfinite(t.float()).all()), f"{what}: non-finite values at p = 1 - 2^-17"

    def attn(dtype, T, D, bits, off=0):
        c = Case(dtype, 2, 2, T, T, D, off=off)
        mask = ops.attention_dropmask(2, 2, T, T, dr, "cuda") if bits else None
        o, lse = ops.attention_fwd(c.q, c.k, c.v, None, c.scale, drop=dr, drop_mask=mask)
        kw = dict(o=o, lse=lse) if dtype != torch.float32 else {}
        ops.attention_bwd(c.q, c.k, c.v, c.do, c.dq, c.dk, c.dv, None, c.scale, drop=dr, drop_mask=mask, **kw)
        return o, lse, c.dq, c.dk, c.dv

    for what, a in (("whole/bits", (lp, 70, 64, True)), ("whole/gen", (lp, 70, 64, False)), ("chunked", (lp, 300, 64, False)),
                    ("tiled-D128", (lp, 100, 128, False)), ("tiled-D64", (lp, 49, 64, False, 4)), ("float32", (torch.float32, 49, 64, False))):
        finite_or_error(what, lambda: attn(*a))
    x = torch.randn(300, 257, device="cuda")
    finite_or_error("cast_dropout", lambda: (ops.cast_dropout(x, torch.float32, dr), ops.cast_dropout(x, lp, dr)))
    xa = torch.randn(300, 128, device="cuda"); wa = torch.randn(256, 128, device="cuda") / 128 ** 0.5
    bias = torch.randn(256, device="cuda"); res = torch.randn(300, 256, device="cuda")
    for dtype in (torch.float32, lp):
        finite_or_error(f"GEMM epilogue {dtype}", lambda: (ops.linear(xa.to(dtype), wa.to(dtype), bias, out_dtype=torch.float32, act=L.ACT_GELU, R=res, drop=dr),
                                                           ops.linear(xa.to(dtype), wa.to(dtype), bias, drop=dr)))


# ---------------------------------------------------------------------------------------------------------------------------------
# paths behind environment switches that are read once per process: one child process each, one at a time, stop at the first failure
#   AVAMD_ATTN_V2=0     attn_fwd_short_kernel<NKP, 0 / 2> (register-staging forward) instead of attn_fwd_short2_kernel
#   AVAMD_ATTN_SHORT=0  T <= 256 at D = 64 goes to the tiled kernels attn_fwd_kernel<16-bit, 64>, attn_bwd_kv / _q_kernel<64>; keep bits raise
#   AVAMD_ATTN_LONG=0   T > 256 at D = 64 goes to the same tiled kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def child_main(switch):
    """Body of the child process of ``test_paths_behind_environment_switches`` (the switch is already in the environment)."""
    ops = pkg("ops")
    assert os.environ.get("AVAMD_ATTN_" + switch) == "0"
    for libname in LIBS:
        with library(libname) as lp:
            if switch == "V2":
                for Tk in (33, 128, 199, 256):
                    for mode in MODES:
                        whole_case(libname, lp, Tk, Tk, mode, family=f"V2=0 whole/{mode}")
            elif switch == "SHORT":
                assert not ops.attention_mask_shape_ok(lp, 3, 49, 49, 64)
                for T in (49, 199):
                    for mode in ("none", "gen"):
                        check("SHORT=0 tiled-D64", libname, Case(lp, 3, 2, T, T, 64, klen=_klens(T, 3)), mode)
                    c = Case(lp, 3, 2, T, T, 64)
                    dr = (P_DROP, SEED, STREAM)
                    mask = ops.attention_dropmask(3, 2, T, T, dr, "cuda")
                    with pytest.raises(RuntimeError, match="keep bits cannot be used"):
                        ops.attention_fwd(c.q, c.k, c.v, None, c.scale, drop=dr, drop_mask=mask)
                    o, lse = ops.attention_fwd(c.q, c.k, c.v, None, c.scale, drop=dr)
                    with pytest.raises(RuntimeError, match="stored mask cannot be used"):
                        ops.attention_bwd(c.q, c.k, c.v, c.do, c.dq, c.dk, c.dv, None, c.scale, o=o, lse=lse, drop=dr, drop_mask=mask)
            else:
                for T in (300, 749):
                    for mode in ("none", "gen"):
                        chunked_case(libname, lp, T, T, mode, family="LONG=0 tiled-D64")
    torch.cuda.synchronize()
    for (fam, mode), r in sorted(WORST.items()):
        print(f"  largest ratio {fam:<20s} {mode}: {r:.2f}")
    print("child ok")


def test_paths_behind_environment_switches():
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import test_attention_matrix_gpu as M; M.child_main(sys.argv[1])" % here
    for switch in ("V2", "SHORT", "LONG"):
        env = dict(os.environ, **{"AVAMD_ATTN_" + switch: "0"})
        out = subprocess.run([sys.executable, "-c", code, switch], env=env, capture_output=True, text=True, timeout=600)
        print(out.stdout)
        # a failed child ends the test here: nothing more is started on the GPU after a fault, an abort or a timeout
        assert out.returncode == 0 and out.stdout.strip().endswith("child ok"), f"AVAMD_ATTN_{switch}=0:\n" + out.stdout[-4000:] + out.stderr[-4000:]
