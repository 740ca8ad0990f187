"""Every kernel form av_gemm can launch outside the implicit-im2col ones (gemm_fast.hip: the 128 x 128 kernel's four non-conv forms and its
64-wide form, v2, v4, v4 k-major, v6, the ten v7 instantiations; gemm.hip: the generic kernels), av_sum_slices and av_transpose, in both
libraries (libavhip.so: bfloat16, libavhip_f16.so: float16), against the plain-PyTorch statement of gemm_ref.py - never against another kernel.

Every case asserts the launch record (av_gemm_last_launch): a case whose shape no longer reaches the kernel it was written for fails instead of
testing something else.  Gates (gemm_ref.verdict): 16-bit outputs by the 4 x e_ref rule + scale + finite, float32 outputs by gate_sum per element,
float32 operands by the float32 tolerance, integer cases by the exact law (bit for bit).  Operands are views into larger NaN-padded allocations,
outputs live in canary buffers that must come back bit-identical outside M x N.  Each case prints family, shape, kernel id and ours / e_ref
(run with -s); the module prints the worst ratio per family and library and the kernel ids seen.

The dispatch switches are read once per process, so a forced group runs in a child pytest of this file (one driver test per group, one child at
a time, each under its own timeout); the child is told its group through AVAMD_GEMM_MATRIX_GROUP and collects that group's cases only.  A driver
asserts that the child reported exactly the expected number of passed cases and nothing failed or skipped; after a child that ended by signal,
abort or timeout the remaining drivers fail without starting anything."""
import contextlib
import ctypes
import os
import re
import subprocess
import sys
import time

import pytest
import torch

import gemm_ref as G
from conftest import pkg

pytestmark = pytest.mark.gpu

GROUP = os.environ.get("AVAMD_GEMM_MATRIX_GROUP")          # set for a child process only
IN_PROCESS = ("default", "fallback")
FORCED = [g for g in G.GROUPS if g not in IN_PROCESS]
# seconds: (run time of the child measured on an MI355X, the largest of four runs; its timeout = three times that, rounded up to 5 s).  2.5 to 2.7 s
# of every child's time pass before its first case (interpreter, torch, library load, first launch; each driver prints that share).
CHILD_TIME = {"v7_nm4": (6.4, 20), "v7_nm3": (4.7, 15), "v7_bm160": (4.1, 15), "v4": (4.8, 15), "v4_bm176": (4.7, 15), "v4_notail": (4.8, 15),
              "v2": (5.0, 15), "v6": (4.6, 15), "km8": (4.9, 15)}
WORST, KERNELS = {}, set()
_warmed = set()
_dead = []                                                 # a child that ended by signal / abort / timeout: later drivers do not start


def _cases_here():
    if GROUP is None:
        return [(g, c) for g in IN_PROCESS for c in G.GROUPS[g][1]()]
    return [(GROUP, c) for c in G.GROUPS[GROUP][1]()]


CASES = _cases_here()


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def library(mode):
    """Precision mode ``mode`` for the block.  Before a library's first case one product runs on NaN operands and is thrown away, so that stale
    LDS is more likely to hold NaN than zeros afterwards (hardening against reads of unstaged rows; nothing is asserted about it)."""
    P = pkg("precision")
    old = P.get_precision()
    P.set_precision(mode)
    try:
        if mode not in _warmed:
            _warmed.add(mode)
            ops = pkg("ops")
            x = torch.full((512, 256), float("nan"), device="cuda", dtype=G.LIBS[mode])
            ops.linear(x, x[:256].contiguous())
            torch.cuda.synchronize()
        yield G.LIBS[mode]
    finally:
        P.set_precision(old)


@pytest.fixture(params=list(G.LIBS))
def lib(request):
    assert not _dead, f"not run: {_dead[0]} left the GPU in a failed state"
    with library(request.param) as lp:
        try:
            yield request.param, lp
        finally:
            try:
                torch.cuda.synchronize()
            except RuntimeError as e:                  # a fault of the device, not a wrong number: nothing more runs on it from this process
                _dead.append(f"{request.node.name} ({str(e).splitlines()[0]})")
                raise


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest ours / e_ref per family and library:")
        for (fam, mode), r in sorted(WORST.items()):
            print(f"  GEMM-MATRIX-WORST {fam:<12s} {mode}: {r:.2f}")
    if KERNELS:
        print("kernel ids seen:")
        for k in sorted(KERNELS):
            print(f"  GEMM-MATRIX-KERNEL {k}")


def _report_start():
    """A child prints once, in front of its first case, how long it took to get there (interpreter, torch, library load, first launch): the
    start is most of a child's run time, and it is what varies between machines."""
    t0 = os.environ.pop("AVAMD_GEMM_MATRIX_T0", None)
    if t0 is not None:
        print(f"\nGEMM-MATRIX-START {time.time() - float(t0):.1f} s")


def _uniform(n):
    L, ops = pkg("_lib"), pkg("ops")
    n4 = (n + 3) // 4 * 4
    u = torch.empty(n4, device="cuda")
    L.check(L.lib().av_dropout_uniform(ops.ptr(u), n4, G.SEED, G.STREAM, ops.stream()))
    return u


def kernel_id(r):
    k = r["kernel"]
    lp = lambda code: "f32" if code == 0 else "lp"
    if k == "generic":
        return f"generic<{'lp' if r['in16'] else 'f32'},bn={r['bn']},akm={r['akm']},bkm={r['bkm']}>"
    if k == "fast128":
        return f"fast128<bnt={r['bn']},conv={r['conv']},akm={r['akm']},bkm={r['bkm']}>"
    if k == "v7":
        return f"v7<{G.ACT_NAMES[r['act']]},{lp(r['out_dtype'])},nm1={r['nm1']}>"
    return k


def check_record(expect, what):
    """Assert the fields ``expect`` of the calling thread's launch record; -> (kernel id, record)."""
    r = pkg("_lib").gemm_last_launch()
    got = {k: r[k] for k in expect}
    assert got == expect, f"{what}: launch record {got} != expected {expect} (whole record: {r})"
    kid = kernel_id(r)
    KERNELS.add(kid)
    return kid, r


def launch(bt, stats=None):
    """av_gemm on the storage of the built case ``bt``."""
    L, ops = pkg("_lib"), pkg("ops")
    c = bt.c
    a = L.GemmArgs()
    p = lambda t: None if t is None else t.data_ptr()
    a.A, a.B, a.C, a.C2 = p(bt.sa), p(bt.sb), p(bt.C), p(bt.C2)
    a.bias, a.R, a.aux, a.stats = p(bt.sbias), p(bt.sr), p(bt.saux), p(stats)
    a.M, a.N, a.K, a.batch = c["M"], c["N"], c["K"], c["batch"]
    a.lda, a.ldb, a.ldc, a.ldr = bt.lda, bt.ldb, bt.ldc, bt.ldr
    a.sA, a.sB, a.sC, a.sR, a.sBias = bt.sA, bt.sB, bt.sC, bt.sR, bt.sBias
    a.batch_inner, a.oA, a.oB, a.oC = bt.inner, bt.oA, bt.oB, bt.oC
    a.a_mode = L.A_TRANS if c["a"] == "km" else L.A_ROWMAJOR
    a.b_mode = L.B_KN if c["b"] == "kn" else L.B_NK
    a.in_dtype = 0 if c["inp"] == "f32" else 1
    a.out_dtype = 0 if c["out"] == "f32" else 1
    a.aux_dtype = 0 if c["aux"] == "f32" else 1
    a.act, a.alpha = c["act"], c["alpha"]
    if c["drop"] > 0:
        a.drop_p, a.drop_seed, a.drop_stream = c["drop"], G.SEED, G.STREAM
    L.check(L.lib().av_gemm(ctypes.byref(a), ops.stream()), "av_gemm")


def note(fam, mode, rows):
    for _, err, e_ref, ratio, _ in rows:
        if ratio == ratio and ratio != float("inf"):
            WORST[(fam, mode)] = max(WORST.get((fam, mode), 0.0), ratio)


def stats_check(bt, stats):
    """[ceil(M / 128)][2][N] column sums and sums of squares of the float32 values before the output rounding, per block of 128 rows."""
    c = bt.c
    M, N = c["M"], c["N"]
    nblk = (M + 127) // 128
    kw = bt._kw()
    v64 = G.ref_gemm(bt.A, bt.B, torch.float64, **kw)[0][0]
    v32 = G.ref_gemm(bt.A, bt.B, torch.float32, prod=G.prod_blocks_reversed, **kw)[0][0]
    va = G.sum_abs(bt.A, bt.B, **kw)[0][0]
    blk = lambda t: torch.stack([torch.stack([t[i * 128:(i + 1) * 128].sum(0), (t[i * 128:(i + 1) * 128] ** 2).sum(0)]) for i in range(nblk)])
    rows, bad = [], []
    for j, n in enumerate(("colsum", "colsumsq")):
        row, b = G.gate_sum("stats." + n, stats[:, j], blk(v64)[:, j], blk(v32)[:, j], blk(va)[:, j])
        rows.append(row); bad += b
    return rows, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of this process: the default dispatch and the fallbacks in the parent, one forced group in a child
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,c", CASES, ids=[g + "-" + G.case_id(c) for g, c in CASES])
def test_case(lib, group, c):
    mode, lp = lib
    _report_start()
    bt = G.Built(c, lp, "cuda", _uniform)
    stats = None
    if c["stats"]:
        stats = torch.full(((c["M"] + 127) // 128, 2, c["N"]), float("nan"), device="cuda")
    launch(bt, stats)
    torch.cuda.synchronize()
    kid, rec = check_record(dict(c["expect"]), G.case_id(c))
    rows, bad, gate = G.verdict(bt, bt.outputs())
    bad += bt.canaries()
    if stats is not None:
        r2, b2 = stats_check(bt, stats)
        rows += r2; bad += b2
    fam = group if c["inp"] == "lp" else group + "_f32"
    note(fam, mode, rows)
    print(f"\n{fam} {mode} {G.case_id(c)} batch={c['batch']} {kid} bm_eff={rec['bm_eff']} tiles={rec['nbM']}x{rec['nbN']} nfull={rec['nfull']} "
          f"grid={rec['grid_x']}x{rec['grid_z']} flags={rec['c_vec']}{rec['r_vec']}{rec['aux_vec']} [{gate}] {G.fmt(rows)}")
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# k-major 8-phase form (AVAMD_GEMM_KM8=2): dW = A^T B with K split over the batch, the partial products summed by av_sum_slices
# ---------------------------------------------------------------------------------------------------------------------------------
KM8 = [(M, N, K, split, exact, True) for M, N in G.KM8_SHAPES for K in G.KM8_KS for split in ("rule", "three") for exact in (False, True)
       if not (split == "three" and K < 128)]
KM8 += [(264, 520, K, "rule", exact, False) for K in (64, 1300) for exact in (False, True)]      # accumulate = 0 into an output that starts as NaN


def _km8(lib, M, N, K, split, exact, acc):
    """matmul_tn's call (ops.matmul_tn: k_total, batch = slices, then av_sum_slices with alpha and accumulate) on padded operands: ``rule`` = the
    slice count ops._split_k8 picks, ``three`` = three slices whatever the rule says.  One slice goes straight to the output with alpha and the
    output as residual; without ``acc`` nothing is accumulated and the output starts as NaN.  The partial-product buffer has canary rows after every slice and must come back finite inside, untouched outside."""
    mode, lp = lib
    _report_start()
    L, ops = pkg("_lib"), pkg("ops")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    if exact:
        A, B = G.exact_a(1, M, K, dev), G.exact_b(1, K, N, dev)
        out0 = G.exact_small((M, N), dev, 13, 6)
    else:
        rn = G.rounder(lp)
        A = rn(torch.randn((1, M, K), generator=g, device=dev) / K ** 0.5)
        B = rn(torch.randn((1, K, N), generator=g, device=dev))
        out0 = torch.randn((M, N), generator=g, device=dev)
    alpha = 0.5
    lda, ldb = M + 24, N + 8
    sa, _ = G.padded_operand(A.transpose(1, 2), lp, lda)
    sb, _ = G.padded_operand(B, lp, ldb)
    t8 = ((M + 255) // 256) * ((N + 255) // 256)
    if split == "rule":
        S, chunk = ops._split_k8(t8, K, M * N)
    else:
        chunk = ((K + 2) // 3 + 63) // 64 * 64
        S = (K + chunk - 1) // chunk
    oflat, _ = G.canary_buffer(1, M, N, N, torch.float32)
    oflat = oflat.to(dev)
    out = G._live(oflat, 1, M, N, N, 0)
    out.copy_(out0 if acc else torch.full_like(out0, float("nan")))
    a = L.GemmArgs()
    a.A, a.B = sa.data_ptr(), sb.data_ptr()
    a.M, a.N, a.lda, a.ldb, a.ldc, a.ldr = M, N, lda, ldb, N, N
    a.a_mode, a.b_mode, a.in_dtype, a.out_dtype = L.A_TRANS, L.B_KN, 1, 0
    pflat = None
    if S > 1:
        pflat, sC = G.canary_buffer(S, M, N, N, torch.float32)
        pflat = pflat.to(dev)
        parts = G._live(pflat, S, M, N, N, 0)
        parts.fill_(float("nan"))
        a.C, a.K, a.batch, a.k_total, a.alpha = parts.data_ptr(), chunk, S, K, 1.0
        a.sA, a.sB, a.sC = chunk * lda, chunk * ldb, sC
    else:
        a.C, a.R, a.K, a.batch, a.alpha = out.data_ptr(), out.data_ptr() if acc else None, K, 1, alpha
    L.check(L.lib().av_gemm(ctypes.byref(a), ops.stream()), "av_gemm")
    nb = ((M + 255) // 256) * ((N + 255) // 256)
    kid, rec = check_record(dict(kernel="v4_km", akm=1, bkm=1, nbM=(M + 255) // 256, nbN=(N + 255) // 256, grid_x=nb * S, nfull=nb * S), f"km8 {M}x{N}x{K}")
    bad = []
    if S > 1:
        torch.cuda.synchronize()
        if not bool(torch.isfinite(parts).all()):
            bad.append("partial products: non-finite values")
        if not G.canary_intact(pflat, S, M, N, N, 0):
            bad.append("partial products: bytes outside the live regions changed")
        L.check(L.lib().av_sum_slices(parts.data_ptr(), S, M * N, sC, alpha, out.data_ptr(), int(acc), ops.stream()), "av_sum_slices")
    torch.cuda.synchronize()
    if not G.canary_intact(oflat, 1, M, N, N, 0):
        bad.append("output: bytes outside the live region changed")
    ck = chunk if S > 1 else K
    r64 = G.sum_slices(G.split_k(A[0], B[0], ck, torch.float64), alpha, out0.double() if acc else None)
    if exact:
        rows = [("out", G.max_err(out[0], r64), 0.0, 0.0, None)]
        if not torch.equal(out[0], r64.float()):
            bad.append(f"out: {int((out[0] != r64.float()).sum())} elements differ from the exact result (exact law)")
    else:
        em = G.sum_slices(G.split_k(A[0], B[0], ck, torch.float32, G.prod_blocks_reversed), alpha, out0 if acc else None)
        sa_ = (A[0].double().abs() @ B[0].double().abs()) * alpha + (out0.double().abs() if acc else 0.0)
        row, b = G.gate_sum("out", out[0], r64, em, sa_)
        rows = [row]; bad += b
    note("km8", mode, rows)
    print(f"\nkm8 {mode} {M}x{N}x{K} slices={S} chunk={ck} {'exact' if exact else 'random'} accumulate={int(acc)} {kid} grid={rec['grid_x']} {G.fmt(rows)}")
    assert not bad, "; ".join(bad)


if GROUP == "km8":                                         # collected in that child only (an empty parameter list would count as a skip)
    test_km8 = pytest.mark.parametrize("M,N,K,split,exact,acc", KM8)(_km8)


# ---------------------------------------------------------------------------------------------------------------------------------
# av_sum_slices and av_transpose (a child deselects them)
# ---------------------------------------------------------------------------------------------------------------------------------
IN_PARENT = GROUP is None


def test_kmajor_a_with_nk_b_has_no_generic_kernel(lib):
    """{k-major A, NK B} is the one operand pair of the fp32 cross product that gemm.hip does not have (dispatch_modes): av_gemm returns
    AV_ERR_ARG with a message, launches nothing, and the launch record reads "none".  The fp32 matrix of fallback_cases leaves it out for that reason."""
    mode, lp = lib
    L, ops = pkg("_lib"), pkg("ops")
    bt = G.Built(G.case("refused", 70, 50, 33, inp="f32", out="f32", a="km", b="nk"), lp, "cuda")
    a = L.GemmArgs()
    a.A, a.B, a.C = bt.sa.data_ptr(), bt.sb.data_ptr(), bt.C.data_ptr()
    a.M, a.N, a.K, a.batch, a.lda, a.ldb, a.ldc, a.alpha = 70, 50, 33, 1, bt.lda, bt.ldb, bt.ldc, 1.0
    a.a_mode, a.b_mode = L.A_TRANS, L.B_NK
    rc = L.lib().av_gemm(ctypes.byref(a), ops.stream())
    torch.cuda.synchronize()
    assert rc == 1 and b"unsupported operand mode pair" in L.lib().av_last_error()
    assert L.gemm_last_launch()["kernel"] == "none"
    assert bool(torch.isnan(bt.C).all()) and bt.canaries() == []


@pytest.mark.parametrize("S,acc", G.SUM_SLICES)
def test_sum_slices(lib, S, acc):
    """n not a multiple of 4, stride > n: exact on small integers (every order gives the same sum), canaries after each slice and the output."""
    mode, lp = lib
    L, ops = pkg("_lib"), pkg("ops")
    M, N = 37, 27                                          # n = 999
    pflat, stride = G.canary_buffer(S, M, N, N, torch.float32)
    pflat = pflat.cuda()
    parts = G._live(pflat, S, M, N, N, 0)
    parts.copy_(torch.stack([G.exact_small((M, N), "cuda", 11 + s, 5) for s in range(S)]))
    oflat = G.canary_buffer(1, M, N, N, torch.float32)[0].cuda()
    out = G._live(oflat, 1, M, N, N, 0)
    out0 = G.exact_small((M, N), "cuda", 13, 6) if acc else torch.full((M, N), float("nan"), device="cuda")
    out.copy_(out0)
    L.check(L.lib().av_sum_slices(parts.data_ptr(), S, M * N, stride, 0.5, out.data_ptr(), int(acc), ops.stream()), "av_sum_slices")
    torch.cuda.synchronize()
    want = G.sum_slices(parts.double(), 0.5, out0.double() if acc else None).float()
    assert torch.equal(out[0], want) and G.canary_intact(oflat, 1, M, N, N, 0) and G.canary_intact(pflat, S, M, N, N, 0)


@pytest.mark.parametrize("R,C", G.TRANSPOSE)
@pytest.mark.parametrize("pad_to", [1, 64])
@pytest.mark.parametrize("pair", ["lp-lp", "f32-lp", "f32-f32", "lp-f32"])
def test_transpose(lib, R, C, pad_to, pair):
    """out[C][Rpad] = in[R][C]^T with ldi > C: exact (the input holds 16-bit values), the pad columns zero, the NaN tail of the input rows and the
    NaN rows after the input never reach the output, nothing is written outside out."""
    mode, lp = lib
    L, ops = pkg("_lib"), pkg("ops")
    idt, odt = ((lp if s == "lp" else torch.float32) for s in pair.split("-"))
    x = G.rounder(lp)(torch.randn((1, R, C), generator=torch.Generator(device="cuda").manual_seed(R), device="cuda"))
    sx, _ = G.padded_operand(x, idt, C + 5)
    Rp = (R + pad_to - 1) // pad_to * pad_to
    oflat = G.canary_buffer(1, C, Rp, Rp, odt)[0].cuda()
    out = G._live(oflat, 1, C, Rp, Rp, 0)
    out.fill_(float("nan"))
    code = lambda d: 0 if d == torch.float32 else 1
    L.check(L.lib().av_transpose(sx.data_ptr(), code(idt), out.data_ptr(), code(odt), R, C, C + 5, Rp, ops.stream()), "av_transpose")
    torch.cuda.synchronize()
    assert torch.equal(out[0, :, :R].float(), x[0].t()), "transposed values differ"
    assert bool((out[0, :, R:] == 0).all()), "the pad is not zero"
    assert G.canary_intact(oflat, 1, C, Rp, Rp, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# drivers of the forced groups (parent only)
# ---------------------------------------------------------------------------------------------------------------------------------
def _expected(group):
    return (len(KM8) if group == "km8" else len(G.GROUPS[group][1]())) * len(G.LIBS)


if IN_PARENT:
    @pytest.mark.parametrize("group", FORCED)
    def test_forced_group(group):
        """One child pytest of this file under the group's switches; exactly the group's cases pass in it."""
        assert not _dead, f"not started: the child of group {_dead[0]} ended by signal, abort or timeout"
        env = dict(os.environ, AVAMD_GEMM_MATRIX_GROUP=group, AVAMD_GEMM_MATRIX_T0=repr(time.time()), **G.GROUPS[group][0])
        measured, limit = CHILD_TIME[group]
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-p", "no:cacheprovider", "-k", "test_km8" if group == "km8" else "test_case"],
                               env=env, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired as e:
            _dead.append(group)
            seen = e.stdout.decode("utf-8", "replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
            raise AssertionError(f"group {group}: child exceeded its {limit} s (measured {measured} s)\n{seen[-3000:]}")
        dt = time.time() - t0
        out = r.stdout
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            _dead.append(group)
        for line in out.splitlines():
            m = re.match(r"\s*GEMM-MATRIX-WORST (\S+)\s+(\S+): ([0-9.]+)", line)
            if m:
                WORST[(m.group(1), m.group(2))] = max(WORST.get((m.group(1), m.group(2)), 0.0), float(m.group(3)))
            m = re.match(r"\s*GEMM-MATRIX-KERNEL (\S+)", line)
            if m:
                KERNELS.add(m.group(1))
        start = re.search(r"GEMM-MATRIX-START ([0-9.]+) s", out)
        print(f"\ngroup {group}: child took {dt:.1f} s, {start.group(1) if start else '?'} s of it before its first case (timeout {limit} s)")
        print("\n".join(l for l in out.splitlines() if l.startswith(group) or l.startswith("km8")))
        tail = out[-6000:] + r.stderr[-2000:]
        assert r.returncode == 0, f"group {group}: child exit status {r.returncode}\n{tail}"
        summary = [l for l in out.splitlines() if re.search(r"\d+ passed", l)]
        assert summary, tail
        counts = {k: int(n) for n, k in re.findall(r"(\d+) (passed|failed|skipped|error|errors|xfailed|xpassed)", summary[-1])}
        assert counts == {"passed": _expected(group)}, f"group {group}: {summary[-1]!r}, expected exactly {_expected(group)} passed\n{tail}"
