"""Every lip-encoder kernel form the dispatchers can reach - the Conv3d front end with and without its fused window max / min
(frontend3d.hip), the BatchNorm / PReLU / pooling glue (visual.hip) and the implicit-GEMM convolution forms of av_gemm (a_mode = A_CONV2D:
frame-major, position-major, positional conv) - in both libraries (libavhip.so: bfloat16, libavhip_f16.so: float16), against the plain
float64 references of visual_ref.py; never against another kernel of the library.

Rule for 16-bit outputs (visual_ref.judge): max|ours - ref64| <= 4 x e_ref per output, e_ref = max|emul - ref64| of the same-precision
emulation; least-squares scale factor of every output of >= 4096 elements within half an ulp of the type; everything finite (output
buffers start as NaN).  float32 sums (BatchNorm partials, average pool, the float32 output of the positional conv) within
4 x max(e_ref, 64 eps32 sum|v|); float32 results of av_bn_finalize within 4 x max(e_ref, eps32 |ref|); float32 operands keep the project's
float32 gate (test_kernels_gpu._tol).  Each case prints family, shape and ours / e_ref = ratio (run with -s); the module prints the largest
ratio per family at the end.  Which branch a group of parameters is for is written next to it (shape lists: visual_ref.py)."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch

import visual_ref as V
from conftest import pkg
from test_kernels_gpu import _tol

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
WORST = {}                                 # (family, library) -> largest ratio seen, printed when the module is done


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def library(mode):
    P = pkg("precision")
    old = P.get_precision()
    P.set_precision(mode)
    try:
        yield V.LIBS[mode]
    finally:
        P.set_precision(old)


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


def _api():
    return pkg("ops"), pkg("_lib")


def cu(t, dtype=None):
    return t.to("cuda", dtype) if dtype is not None else t.to("cuda")


def nan(shape, dtype):
    return torch.full(tuple(shape), float("nan"), device="cuda", dtype=dtype)


def shifted(t, off=4):
    """A copy of ``t`` that starts ``off`` elements into its allocation (4 sixteen-bit elements: 8-byte aligned, not 16)."""
    flat = torch.empty(t.numel() + 8, device="cuda", dtype=t.dtype)
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def settle(family, libname, head, rows, bad):
    """Print one case, note its ratios, fail on any message."""
    print(f"[{family} {libname}] {head}:", V.fmt(rows))
    for n, err, e_ref, ratio, sd in rows:
        if ratio == ratio and ratio != float("inf"):
            WORST[(family, libname)] = max(WORST.get((family, libname), 0.0), ratio)
    assert not bad, f"[{family} {libname}] {head}: " + "; ".join(bad)


def f32_case(family, libname, head, ours, r64):
    """float32 operands: the project's float32 gate."""
    print(f"[{family} {libname}] {head}: float32 max err {V.max_err(ours, r64):.2e}")
    assert bool(torch.isfinite(ours).all())
    torch.testing.assert_close(ours, r64.to(F32), **_tol(F32))


def same_bits(a, b, what):
    assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what


# ---------------------------------------------------------------------------------------------------------------------------------
# front end: av_conv3d_front, av_conv3d_front_pool (frontend3d.hip).  V.FRONT, (B, T, H, W):
#   (1,1,16,32)   one 8 x 16 tile, one strip; T = 1: four of the five temporal taps are padding
#   (1,2,16,32)   the smallest T above 1
#   (3,1,32,32)   three workgroups: the XCD remap has total % 8 != 0 and q = 0; two row tiles: the carry row is used
#   (1,5,16,96)   three strips: the halo column is used, with one row tile
#   (2,7,48,64)   non-square frames, carry row and halo column together
#   (13,1,16,64)  26 workgroups: the remap has q > 0 and rem > 0
#   (1,3,96,32)   H > W, six row tiles
# ---------------------------------------------------------------------------------------------------------------------------------
def pack_front_w(w, lp):
    """[64, 5, 7, 7] -> [64][288]: k = (kt * 7 + ky) * 8 + kx, kx padded 7 -> 8 and K 280 -> 288 with zeros (the kernel's weight image)."""
    p = torch.zeros(64, 36, 8, device=w.device)
    p[:, :35, :7] = w.reshape(64, 35, 7)
    return p.reshape(64, 288).to(lp).contiguous()


def run_front(x, wk, lp, pool, stats):
    ops, L = _api()
    B, T, H, W = x.shape
    N, Ho, Wo = B * T, H // 2, W // 2
    st = nan((N * (Ho // 8) * (Wo // 16), 2, 64), F32) if stats else None
    if pool:
        ymax, ymin = nan((N, Ho // 2, Wo // 2, 64), lp), nan((N, Ho // 2, Wo // 2, 64), lp)
        L.check(L.lib().av_conv3d_front_pool(ops.ptr(x), ops.ptr(wk), ops.ptr(ymax), ops.ptr(ymin), ops.ptr(st), B, T, H, W, ops.stream()), "av_conv3d_front_pool")
        return ymax, ymin, st
    y = nan((N, Ho, Wo, 64), lp)
    L.check(L.lib().av_conv3d_front(ops.ptr(x), ops.ptr(wk), ops.ptr(y), ops.ptr(st), B, T, H, W, ops.stream()), "av_conv3d_front")
    return y, st


def front_case(libname, lp, shape, family="front"):
    x, w = (cu(t) for t in V.front_operands(shape, lp))
    wk = pack_front_w(w, lp)
    y, st = run_front(x, wk, lp, False, True)
    y_nostats, _ = run_front(x, wk, lp, False, False)
    ymax, ymin, stp = run_front(x, wk, lp, True, True)
    ymax2, ymin2, _ = run_front(x, wk, lp, True, False)
    r64, em, (s64, sem, sabs) = V.front_refs(x, w, lp)
    rows, bad = V.judge(lp, dict(y=y, ymax=ymax, ymin=ymin), r64, em)
    for name, s in (("partials", st), ("partials/pool", stp)):
        row, b = V.gate_sum(name, s.sum(0), s64, sem, sabs)
        rows.append(row); bad += b
    settle(family, libname, f"B{shape[0]} T{shape[1]} H{shape[2]} W{shape[3]}", rows, bad)
    same_bits(y_nostats, y, "y with stats = None differs from y with stats")
    same_bits(ymax2, ymax, "ymax with stats = None differs"); same_bits(ymin2, ymin, "ymin with stats = None differs")
    mx, mn = V.window_maxmin(y.float())                      # the fused form pools exactly what the plain form stores
    assert torch.equal(ymax.float(), mx), "ymax is not the window maximum of the plain kernel's y"
    assert torch.equal(ymin.float(), mn), "ymin is not the window minimum of the plain kernel's y"
    # exact integers: a swapped axis, a flipped tap or a wrong seam is a whole-number error
    x, w = (cu(t) for t in V.front_operands(shape, lp, exact=True))
    wk = pack_front_w(w, lp)
    want = V.conv3d_front(x, w, F64).view(y.shape)
    wmx, wmn = V.window_maxmin(want)
    y, _ = run_front(x, wk, lp, False, False)
    ymax, ymin, _ = run_front(x, wk, lp, True, False)
    for name, got, ref in (("y", y, want), ("ymax", ymax, wmx), ("ymin", ymin, wmn)):
        torch.testing.assert_close(got.double(), ref, rtol=0, atol=0, msg=lambda m, name=name: f"exact-integer {name} {shape}: {m}")


@pytest.mark.parametrize("shape", V.FRONT)
def test_front_end(lib, shape):
    front_case(*lib, shape)


def child_main():
    """Body of the child process of ``test_front_end_without_prefetch`` (AVAMD_FRONT_PREFETCH=0 is already in the environment: the flag
    is read once per process): the whole front-end group on the form that loads each tile's patch when it needs it."""
    assert os.environ.get("AVAMD_FRONT_PREFETCH") == "0"
    for libname in V.LIBS:
        with library(libname) as lp:
            for shape in V.FRONT:
                front_case(libname, lp, shape, family="front/PREFETCH=0")
    torch.cuda.synchronize()
    for (fam, mode), r in sorted(WORST.items()):
        print(f"  largest ratio {fam:<20s} {mode}: {r:.2f}")
    print("child ok")


def test_front_end_without_prefetch():
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import test_visual_matrix_gpu as M; M.child_main()" % here
    env = dict(os.environ, AVAMD_FRONT_PREFETCH="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(out.stdout)
    # a failed child ends the test here: nothing more is started on the GPU after a fault, an abort or a timeout
    assert out.returncode == 0 and out.stdout.strip().endswith("child ok"), "AVAMD_FRONT_PREFETCH=0:\n" + out.stdout[-4000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------
# av_bn_prelu_maxpool (visual.hip) and av_bn_prelu_minmax (frontend3d.hip).  V.bn_params holds a positive, a negative and a zero scale
# and a slope in (0, 1), a negative slope and a slope above 1, in every combination of sign and kind.  V.MAXPOOL, (N, H, W, C, kind):
#   (2,5,7,64)        odd H and W in the vector form          (1,1,1,64)   one pixel: eight of the nine taps are padding
#   (3,8,16,64)       even sizes, more than one workgroup     (2,5,7,24)   C / 8 does not divide 256: the scalar 16-bit kernel
#   (2,6,6,64) "off"  input 8 bytes off 16-byte alignment: the scalar 16-bit kernel          (2,5,7,64) "f32"   float32
# ---------------------------------------------------------------------------------------------------------------------------------
def run_maxpool(x, sc, sh, sl, out_dtype):
    ops, L = _api()
    N, H, W, C = x.shape
    out = nan((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), out_dtype)
    L.check(L.lib().av_bn_prelu_maxpool(ops.ptr(x), ops.ptr(sc), ops.ptr(sh), ops.ptr(sl), ops.ptr(out), ops.dt(x), N, H, W, C, ops.stream()), "av_bn_prelu_maxpool")
    return out


def run_minmax(mx, mn, sc, sh, sl):
    ops, L = _api()
    out = nan(mx.shape, mx.dtype)
    L.check(L.lib().av_bn_prelu_minmax(ops.ptr(mx), ops.ptr(mn), ops.ptr(sc), ops.ptr(sh), ops.ptr(sl), ops.ptr(out), mx.numel(), ops.stream()), "av_bn_prelu_minmax")
    return out


@pytest.mark.parametrize("N,H,W,C,kind", V.MAXPOOL)
def test_bn_prelu_maxpool(lib, N, H, W, C, kind):
    libname, lp = lib
    g = torch.Generator().manual_seed(N * H * W * C)
    dtype = F32 if kind == "f32" else lp
    xv = cu(V.randn((N, H, W, C), g, None if kind == "f32" else lp))
    sc, sh, sl = (cu(t) for t in V.bn_params(C, g))
    x = shifted(xv.to(dtype)) if kind == "off" else xv.to(dtype)
    assert x.data_ptr() % 16 == (8 if kind == "off" else 0)
    out = run_maxpool(x, sc, sh, sl, dtype)
    head = f"N{N} H{H} W{W} C{C} {kind}"
    r64 = V.bn_prelu_maxpool(xv, sc, sh, sl, F64)
    if kind == "f32":
        return f32_case("maxpool", libname, head, out, r64)
    settle("maxpool", libname, head, *V.judge(lp, dict(out=out), dict(out=r64), dict(out=V.bn_prelu_maxpool(xv, sc, sh, sl, F32, V.rounder(lp)))))
    if C == 64:                                               # the same max / min pair through av_bn_prelu_minmax: the same bits
        mx, mn = (t.to(lp) for t in V.window_maxmin(xv))
        same_bits(run_minmax(mx, mn, sc, sh, sl), out, "av_bn_prelu_minmax and av_bn_prelu_maxpool differ on the same y")


# n = 64: one chunk group; 64 x 1000: a ragged single sweep; the last: just above one sweep of the capped grid (2048 x 256 x 4 chunks) plus a
# remainder that is no multiple of four strides - the second loop iteration and its clamped tail
@pytest.mark.parametrize("n", V.MINMAX_N)
def test_bn_prelu_minmax(lib, n):
    libname, lp = lib
    g = torch.Generator().manual_seed(n)
    a, b = cu(V.randn((n // 64, 64), g, lp)), cu(V.randn((n // 64, 64), g, lp))
    mx, mn = torch.maximum(a, b), torch.minimum(a, b)
    sc, sh, sl = (cu(t) for t in V.bn_params(64, g))
    out = run_minmax(mx.to(lp), mn.to(lp), sc, sh, sl)
    settle("minmax", libname, f"n{n}", *V.judge(lp, dict(out=out), dict(out=V.bn_prelu_minmax(mx, mn, sc, sh, sl, F64)),
                                                dict(out=V.bn_prelu_minmax(mx, mn, sc, sh, sl, F32, V.rounder(lp)))))


# ---------------------------------------------------------------------------------------------------------------------------------
# av_bn_finalize (visual.hip): train mode is ONE launch whose last workgroup (a ticket behind the 2C double accumulators) finalizes and
# leaves the workspace zeroed.  C: 24 (one column block, ragged), 64, 100 (2C = 200: four column blocks, the last ragged), 512;
# nblk: 1, 63 / 64 / 65 (the 64-row split of the partials), 1000 (16 row blocks)
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_inputs(C, nblk, seed, rows=8):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(nblk, rows, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g)
    part = torch.stack([y.sum(1), (y * y).sum(1)], 1)         # [nblk][2][C] float32
    return (cu(part.contiguous()), nblk * rows) + tuple(cu(t) for t in (torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g),
                                                                          torch.rand(C, generator=g) + 0.5))


def run_finalize(part, count, gamma, beta, rm, rv, training, ws, ws_zeroed):
    ops, L = _api()
    C = gamma.numel()
    sc, sh = nan((C,), F32), nan((C,), F32)
    L.check(L.lib().av_bn_finalize(ops.ptr(part), 0 if part is None else part.shape[0], count, ops.ptr(gamma), ops.ptr(beta), ops.ptr(rm), ops.ptr(rv),
                                   V.BN_MOMENTUM, V.BN_EPS, int(training), ops.ptr(sc), ops.ptr(sh), C, ops.ptr(ws), ws_zeroed, ops.stream()), "av_bn_finalize")
    return sc, sh


def finalize_case(libname, head, part, count, gamma, beta, rm, rv, training, ws, ws_zeroed):
    """One call, judged: scale, shift and (train mode, running pointers given) both running statistics by the float32-result gate."""
    rm0, rv0 = (None, None) if rm is None else (rm.clone(), rv.clone())
    sc, sh = run_finalize(part, count, gamma, beta, rm, rv, training, ws, ws_zeroed)
    want = V.bn_from_partials(part, count, gamma, beta, rm0, rv0, training)
    emul = V.bn_from_partials(part, count, gamma, beta, rm0, rv0, training, f32=True)
    rows, bad = [], []
    names = ("scale", "shift") + (("running_mean", "running_var") if training and rm is not None else ())
    for name, got, w, e in zip(names, (sc, sh, rm, rv), want, emul):
        row, b = V.gate_f32(name, got, w, e)
        rows.append(row); bad += b
    settle("bn_finalize", libname, head, rows, bad)
    if not training:
        same_bits(rm, rm0, "eval mode changed running_mean"); same_bits(rv, rv0, "eval mode changed running_var")


@pytest.mark.parametrize("nblk", V.BN_NBLK)
@pytest.mark.parametrize("C", V.BN_C)
def test_bn_finalize_train_mode(lib, C, nblk):
    part, count, gamma, beta, rm, rv = bn_inputs(C, nblk, 100 * C + nblk)
    ws = torch.zeros(2 * C + 1, device="cuda", dtype=F64)
    finalize_case(lib[0], f"C{C} nblk{nblk}", part, count, gamma, beta, rm, rv, True, ws, 1)
    finalize_case(lib[0], f"C{C} nblk{nblk} no running statistics", part, count, gamma, beta, None, None, True, ws, 1)
    assert bool((ws.view(torch.int64) == 0).all()), "the workspace (accumulators + ticket) is not left zeroed"


@pytest.mark.parametrize("C", V.BN_C)
def test_bn_finalize_count_one(lib, C):
    """One row: the variance is zero and the running variance takes the biased one (no division by count - 1 = 0)."""
    part, _, gamma, beta, rm, rv = bn_inputs(C, 1, C, rows=1)
    finalize_case(lib[0], f"C{C} count 1", part, 1, gamma, beta, rm, rv, True, torch.zeros(2 * C + 1, device="cuda", dtype=F64), 1)


@pytest.mark.parametrize("C,nblk", [(64, 65), (100, 1000), (512, 63)])
def test_bn_finalize_workspace_protocol(lib, C, nblk):
    """Three calls back to back on one workspace with ws_zeroed = 1 and different partials: every call right, the workspace all zero
    afterwards including the ticket word behind 2C; then one call with ws_zeroed = 0 on a workspace filled with garbage."""
    ws = torch.zeros(2 * C + 1, device="cuda", dtype=F64)
    for i, nb in enumerate((nblk, 1, nblk + 7)):
        part, count, gamma, beta, rm, rv = bn_inputs(C, nb, 7 * C + i)
        finalize_case(lib[0], f"C{C} nblk{nb} call {i}", part, count, gamma, beta, rm, rv, True, ws, 1)
        assert bool((ws.view(torch.int64) == 0).all()), f"call {i} did not leave the workspace (accumulators + ticket) zeroed"
    ws.view(torch.int64).fill_(0x7ff8dead0000beef)            # NaN accumulators, a non-zero ticket
    part, count, gamma, beta, rm, rv = bn_inputs(C, nblk, 9 * C)
    finalize_case(lib[0], f"C{C} nblk{nblk} garbage workspace", part, count, gamma, beta, rm, rv, True, ws, 0)
    assert bool((ws.view(torch.int64) == 0).all())


@pytest.mark.parametrize("C", V.BN_C)
def test_bn_finalize_eval_mode(lib, C):
    _, _, gamma, beta, rm, rv = bn_inputs(C, 1, 3 * C)
    finalize_case(lib[0], f"C{C} eval", None, 0, gamma, beta, rm, rv, False, None, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# av_bn_act (visual.hip).  V.BNACT_FORMS x residual {none, identity (rscale null), with its own BatchNorm} x {PReLU, none}:
#   vecC64 / vecC512   vector form                            small      n8 = 64 chunks: less than one workgroup
#   sweep              just above one sweep of the 512-block grid (512 x 256 x 4 chunks) + one stride + 168 chunks: second loop iteration, clamped tail
#   scalarC24          C / 8 does not divide 256: scalar 16-bit   scalar_res_off   residual 8 bytes off 16-byte alignment: scalar 16-bit   float32
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prelu", [True, False])
@pytest.mark.parametrize("resmode", V.BNACT_RES)
@pytest.mark.parametrize("name,C,n,kind", V.BNACT_FORMS)
def test_bn_act(lib, name, C, n, kind, resmode, prelu):
    ops, L = _api()
    libname, lp = lib
    g = torch.Generator().manual_seed(n + len(resmode))
    dtype = F32 if kind == "f32" else lp
    xv, rv_ = (cu(V.randn((n // C, C), g, None if kind == "f32" else lp)) for _ in range(2))
    sc, sh, sl = (cu(t) for t in V.bn_params(C, g))
    rs, rb, _ = (cu(t) for t in V.bn_params(C, g))
    x = xv.to(dtype)
    res = None if resmode == "none" else (shifted(rv_.to(dtype)) if kind == "res_off" else rv_.to(dtype))
    if kind == "res_off" and res is not None:
        assert res.data_ptr() % 16 == 8
    out = nan(x.shape, dtype)
    a = (None if res is None else rv_, rs if resmode == "bn" else None, rb if resmode == "bn" else None, sl if prelu else None)
    L.check(L.lib().av_bn_act(ops.ptr(x), ops.ptr(sc), ops.ptr(sh), ops.ptr(res), ops.ptr(a[1]), ops.ptr(a[2]), ops.ptr(a[3]), ops.ptr(out), ops.dt(x), n, C,
                              ops.stream()), "av_bn_act")
    head = f"{name} C{C} n{n} res={resmode} prelu={prelu}"
    r64 = V.bn_act(xv, sc, sh, *a, F64)
    if kind == "f32":
        return f32_case("bn_act", libname, head, out, r64)
    settle("bn_act", libname, head, *V.judge(lp, dict(out=out), dict(out=r64), dict(out=V.bn_act(xv, sc, sh, *a, F32, V.rounder(lp)))))


# ---------------------------------------------------------------------------------------------------------------------------------
# av_avgpool (visual.hip), V.AVGPOOL (N, HW, C, FB): frame-major (5,9,512) and HW = 1 (3,1,64); position-major (input built with
# to_pos_major) two blocks of 256 (512,9,512), small blocks (8,6,64, FB = 4), HW = 1 where both orders coincide (256,1,64)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("N,HW,C,FB", V.AVGPOOL)
def test_avgpool(lib, N, HW, C, FB, f32):
    ops, L = _api()
    libname, lp = lib
    xv = cu(V.randn((N, HW, C), torch.Generator().manual_seed(N + HW + C), None if f32 else lp))
    rows = xv.reshape(N * HW, C)
    x = (V.to_pos_major(rows, N, HW, FB) if FB else rows).to(F32 if f32 else lp).contiguous()
    out = nan((N, C), F32)
    L.check(L.lib().av_avgpool(ops.ptr(x), ops.dt(x), ops.ptr(out), N, HW, C, FB, ops.stream()), "av_avgpool")
    head = f"N{N} HW{HW} C{C} FB{FB}"
    r64 = V.avgpool(xv, F64)
    if f32:
        return f32_case("avgpool", libname, head, out, r64)
    row, bad = V.gate_sum("out", out, r64, V.avgpool(xv, F32), xv.double().abs().sum(1) / HW)
    settle("avgpool", libname, head, [row], bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# implicit-GEMM convolution forms: ops.gemm with a_mode = A_CONV2D (gemm_fast.hip conv_decode / conv_pixel / tap_seq / conv_rows_init /
# stage_conv), against the float64 convolution of the frame-major data; position-major sides are permuted with to_pos_major.
# V.CONV_PM (cNF = 256), Cin -> Cout, k, stride, input H x W, frames, cPM:
#   l2_fm_to_pm        64 -> 128, 3x3, s2, 6x6, 256, pm 2    128 x 128 kernel; reads frame-major, writes position-major
#   l2_two_blocks      128 -> 128, 3x3, s1, 3x3, 512, pm 3   two image blocks; corner positions keep 4 of 9 taps
#   l2_1x1_nonsquare   64 -> 128, 1x1, s2, 6x4, 256, pm 2    one tap, non-square
#   narrow             64 -> 64, 3x3, s1, 3x3, 256, pm 3     N <= 64: the narrow kernel
#   l3_8phase          128 -> 256, 3x3, s2, 6x6, 512, pm 3   M = 4608, N = 256, K = 1152: the 8-phase conv kernel with skipped K-tiles
#   l4_two_col_tiles   256 -> 512, 3x3, s2, 3x3, 1024, pm 3  M = 4096, two column tiles
#   pm_to_fm           128 -> 128, 3x3, s1, 3x2, 256, pm 1   reads position-major, writes frame-major
#   cin192_no_table    192 -> 128, 3x3, s1, 3x3, 256, pm 3   Cin / 64 no power of two: tap_seq has no table
# V.CONV_SMALL_NF: cNF = 128 on the 4608-row layer3 case (256-row tiles) and cNF = 64 on the 128-row kernel: tiles span positions, every tap stays.
# V.CONV_FM (frame-major gaps): non-square 12 x 6 at stride 2; channel slice cCtot = 192, cCin = 64, cCoff = 64; Cin = 192.
# ---------------------------------------------------------------------------------------------------------------------------------
def run_conv(c, x, w, lp, in_dtype=None, stats=True, out=None, raw=False):
    """x [n, H, W, Ctot] and w [Cout, k, k, Cin] frame-major values on the device -> (y [M, Cout] in the order cPM asks for, partials)."""
    ops, L = _api()
    dtype = in_dtype or lp
    P_in, P_out = c["H"] * c["W"], c["Ho"] * c["Wo"]
    rows = x.reshape(c["n"] * P_in, c["ctot"])
    xd = (V.to_pos_major(rows, c["n"], P_in, c["nf"]) if c["pm"] & 1 and not raw else rows).to(dtype).contiguous()       # raw: refusal tests, no valid order exists
    K = c["k"] * c["k"] * c["cin"]
    wk = w.reshape(c["cout"], K).to(dtype).contiguous()
    M = c["n"] * P_out
    y = nan((M, c["cout"]), dtype) if out is None else out
    st = nan(((M + 127) // 128, 2, c["cout"]), F32) if stats else None
    geo = dict(cT=1, cH=c["H"], cW=c["W"], cCtot=c["ctot"], cCin=c["cin"], cCoff=c["coff"], cKt=1, cKh=c["k"], cKw=c["k"], cSh=c["s"], cSw=c["s"], cPt=0,
               cPh=c["pad"], cPw=c["pad"], cOh=c["Ho"], cOw=c["Wo"], cNF=c["nf"], cPM=c["pm"])
    ops.gemm(xd, wk, y, M=M, N=c["cout"], K=K, lda=0, ldb=K, ldc=c["cout"], a_mode=L.A_CONV2D, conv=geo, stats=st)
    return y, st


def conv_case(libname, lp, c, family):
    x, w = (cu(t) for t in V.conv_operands(c, lp))
    y, st = run_conv(c, x, w, lp)
    y_fm = V.from_pos_major(y, c["n"], c["Ho"] * c["Wo"], c["nf"]) if c["pm"] & 2 else y
    y64, yem, (s64, sem, sabs) = V.conv_refs(c, x, w, lp)
    rows, bad = V.judge(lp, dict(y=y_fm), dict(y=y64), dict(y=yem))
    row, b = V.gate_sum("partials", st.sum(0), s64, sem, sabs)
    settle(family, libname, f"{c['name']} {c['cin']}->{c['cout']} k{c['k']} s{c['s']} {c['H']}x{c['W']} n{c['n']} pm{c['pm']} nf{c['nf']}", rows + [row], bad + b)
    x, w = (cu(t) for t in V.conv_operands(c, lp, exact=True))
    y, _ = run_conv(c, x, w, lp, stats=False)
    y_fm = V.from_pos_major(y, c["n"], c["Ho"] * c["Wo"], c["nf"]) if c["pm"] & 2 else y
    torch.testing.assert_close(y_fm.double(), V.conv_case_ref(c, x, w, F64), rtol=0, atol=0, msg=lambda m: f"exact-integer {c['name']}: {m}")


@pytest.mark.parametrize("c", V.CONV_PM, ids=lambda c: c["name"])
def test_conv_position_major(lib, c):
    conv_case(*lib, c, "conv/pos-major")


@pytest.mark.parametrize("c", V.CONV_SMALL_NF, ids=lambda c: c["name"])
def test_conv_position_major_blocks_below_the_row_tile(lib, c):
    conv_case(*lib, c, "conv/pos-major")


@pytest.mark.parametrize("c", V.CONV_FM, ids=lambda c: c["name"])
def test_conv_frame_major_gaps(lib, c):
    conv_case(*lib, c, "conv/frame-major")


def test_conv_position_major_refusals(lib):
    """float32 operands with cPM != 0, and a row count that is no whole number of image blocks: an error, nothing computed."""
    libname, lp = lib
    c = V.conv_case("refuse_f32", 64, 64, 3, 1, 3, 3, 256, 3, 256)
    x, w = (cu(t) for t in V.conv_operands(c, lp))
    out = nan((c["n"] * 9, 64), F32)
    with pytest.raises(RuntimeError, match="position-major"):
        run_conv(c, x, w, lp, in_dtype=F32, stats=False, out=out, raw=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    c = V.conv_case("refuse_ragged", 64, 64, 3, 1, 3, 3, 300, 3, 256)           # 300 images: M % (cOh cOw cNF) != 0
    x, w = (cu(t) for t in V.conv_operands(c, lp))
    out = nan((c["n"] * 9, 64), lp)
    with pytest.raises(RuntimeError, match="position-major"):
        run_conv(c, x, w, lp, stats=False, out=out, raw=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# positional-conv form (the call of model/w2v2.py): G = 2 groups of Cg = 64 in Hd = 128 through batch = G, sA = sC = sR = sBias = Cg,
# sB = Cg kp Cg, ldc = ldr = Hd, bias + GELU + float32 residual, float32 output.  kp 32 / 33: both sides of the bit-mask / range switch of
# conv_rows_init (cKh cKw > 32), even and odd; kp 128: the model's.  (B, T): (2, 49) T < kp / 2 clips every row at kp = 128, (3, 200) a tap
# that leaks across items shows, (1, 1) M = 1.
# ---------------------------------------------------------------------------------------------------------------------------------
def run_posconv(x, w, bias, res, lp, act):
    ops, L = _api()
    B, T, Hd = x.shape
    G, Cg, kp, _ = w.shape
    hT, wk = x.to(lp).contiguous(), w.reshape(G, Cg, kp * Cg).to(lp).contiguous()
    out = nan((B, T, Hd), F32)
    conv = dict(cT=1, cH=T, cW=1, cCtot=Hd, cCin=Cg, cCoff=0, cKt=1, cKh=kp, cKw=1, cSh=1, cSw=1, cPt=0, cPh=kp // 2, cPw=0, cOh=T, cOw=1)
    ops.gemm(hT, wk, out, M=B * T, N=Cg, K=kp * Cg, lda=0, ldb=kp * Cg, ldc=Hd, a_mode=L.A_CONV2D, conv=conv, bias=bias, act=act, R=res, ldr=Hd, batch=G,
             sA=Cg, sB=Cg * kp * Cg, sC=Cg, sR=Cg, sBias=Cg)
    return out


@pytest.mark.parametrize("B,T", V.POSCONV_BT)
@pytest.mark.parametrize("kp", V.POSCONV_KP)
def test_positional_conv(lib, kp, B, T):
    _, L = _api()
    libname, lp = lib
    x, w, bias, res = (cu(t) for t in V.posconv_operands(kp, B, T, lp))
    out = run_posconv(x, w, bias, res, lp, L.ACT_GELU)
    r64, em, sabs = V.posconv_refs(x, w, bias, res, True)
    row, bad = V.gate_sum("out", out, r64, em, sabs)
    settle("posconv", libname, f"kp{kp} B{B} T{T}", [row], bad)
    x, w, bias, res = (cu(t) for t in V.posconv_operands(kp, B, T, lp, exact=True))
    out = run_posconv(x, w, bias, res, lp, L.ACT_NONE)
    torch.testing.assert_close(out.double(), V.pos_conv(x, w, bias, res, False, F64), rtol=0, atol=0, msg=lambda m: f"exact-integer kp{kp} B{B} T{T}: {m}")
