"""Torch-tensor wrappers over the C-ABI of libavhip.so (plumbing only: pointers, shapes, current stream).

PyTorch provides device memory and streams; every arithmetic op on the path is a HIP kernel of ours.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _lib as L
from . import precision
from ._lib import AV_BF16, AV_F32

Tensor = torch.Tensor


def _lp() -> torch.dtype:
    """The 16-bit operand type of the library in use: float16 in precision mode "fp16" (libavhip_f16.so), bfloat16 otherwise."""
    return torch.float16 if precision.get_precision() == "fp16" else torch.bfloat16


def dt(t: Tensor) -> int:
    if t.dtype == torch.float32:
        return AV_F32
    if t.dtype == _lp():
        return AV_BF16                                              # dtype code 1 = "the library's 16-bit type"
    raise TypeError(f"unsupported dtype {t.dtype} (the library of precision mode {precision.get_precision()!r} handles float32 / {_lp()})")


def tdt(code: int) -> torch.dtype:
    return torch.float32 if code == AV_F32 else _lp()


def ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_dev = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def stream():
    """hipStream_t of torch's current stream on the current device (raw handle: ~10x cheaper than building a Stream object
    per kernel launch, which at ~950 launches per step was 3 ms of host time)."""
    if _raw_stream is not None:
        return _raw_stream(_cur_dev())                      # torch._C._cuda_getDevice: current_device() without the lazy-init checks
    return torch.cuda.current_stream().cuda_stream


def h2d_async(arr, device) -> Tensor:
    """numpy array -> device tensor without draining the stream: staged through the caching pinned-host allocator and copied with
    non_blocking=True (a plain ``torch.tensor(host_data, device=cuda)`` synchronises the stream it runs on)."""
    return torch.from_numpy(arr).pin_memory().to(device, non_blocking=True)


def _req(t: Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor must live on the GPU (no CPU fallback in libavhip)")


class GemmProbe:
    """Optional live timing of ONE av_gemm instantiation with events on the launch stream (bench.py roofline leg)."""
    active = None            # dict(key=(in_dtype, a_mode, b_mode, wide), records=[(start, end, flops)])

    @classmethod
    def start(cls, in_dtype: int, a_mode: int, b_mode: int, wide: bool):
        cls.active = dict(key=(in_dtype, a_mode, b_mode, wide), records=[])

    @classmethod
    def stop(cls):
        a, cls.active = cls.active, None
        return a


class AttnProbe:
    """Optional live timing of the attention launches with events on the launch stream (bench.py ``attention`` report).
    Records (start, end, tag, flops, bytes); tag = "fwd"/"bwd" + head_dim (64 = wav2vec2 self-attention K7, 128 = fusion K17)."""
    active = None

    @classmethod
    def start(cls):
        cls.active = []

    @classmethod
    def stop(cls):
        a, cls.active = cls.active, None
        return a


def _probed(tag, flops, nbytes, fn):
    pr = AttnProbe.active
    if pr is None:
        return fn()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    pr.append((e0, e1, tag, float(flops), float(nbytes)))
    return r


def gemm(A: Tensor, B: Tensor, C_: Tensor, *, M: int, N: int, K: int, lda: int, ldb: int, ldc: int,
         a_mode: int = L.A_ROWMAJOR, b_mode: int = L.B_NK, bias: Optional[Tensor] = None, act: int = L.ACT_NONE,
         R: Optional[Tensor] = None, ldr: int = 0, aux: Optional[Tensor] = None, C2: Optional[Tensor] = None,
         stats: Optional[Tensor] = None, alpha: float = 1.0, batch: int = 1, sA: int = 0, sB: int = 0, sC: int = 0,
         sR: int = 0, sBias: int = 0, conv: Optional[dict] = None, a_off: int = 0, b_off: int = 0, c_off: int = 0,
         batch_inner: int = 0, oA: int = 0, oB: int = 0, oC: int = 0, drop: Optional[tuple] = None, k_total: int = 0) -> Tensor:
    """Raw av_gemm call.  Offsets are in elements."""
    _req(A, "gemm A"); _req(B, "gemm B"); _req(C_, "gemm C")
    if A.dtype != B.dtype:
        raise TypeError(f"gemm: A {A.dtype} and B {B.dtype} must match")
    a = L.GemmArgs()
    a.A = A.data_ptr() + a_off * A.element_size()
    a.B = B.data_ptr() + b_off * B.element_size()
    a.C = C_.data_ptr() + c_off * C_.element_size()
    a.C2 = ptr(C2) if C2 is None else C2.data_ptr() + c_off * C2.element_size()
    a.bias = ptr(bias); a.R = ptr(R) if R is None else R.data_ptr() + c_off * 4
    a.aux = ptr(aux); a.stats = ptr(stats)
    a.M, a.N, a.K, a.batch = M, N, K, batch
    a.lda, a.ldb, a.ldc, a.ldr = lda, ldb, ldc, (ldr or ldc)
    a.sA, a.sB, a.sC, a.sR, a.sBias = sA, sB, sC, sR, sBias
    a.batch_inner, a.oA, a.oB, a.oC = batch_inner, oA, oB, oC
    a.k_total = k_total
    if drop is not None and drop[0] > 0:
        a.drop_p, a.drop_seed, a.drop_stream = float(drop[0]), int(drop[1]), int(drop[2])     # (p, seed, stream id)
    a.a_mode, a.b_mode = a_mode, b_mode
    a.in_dtype, a.out_dtype = dt(A), dt(C_)
    a.aux_dtype = dt(aux) if aux is not None else 0
    a.act, a.alpha = act, alpha
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError("gemm: bias must be float32")
    if R is not None and R.dtype != torch.float32:
        raise TypeError("gemm: residual must be float32")
    if conv:
        for k, v in conv.items():
            setattr(a, k, v)
    pr = GemmProbe.active
    if pr is not None and pr["key"] == (a.in_dtype, a_mode, b_mode, N > 64):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(L.lib().av_gemm(C.byref(a), stream()), "av_gemm")
        e1.record()
        es, oes = A.element_size(), C_.element_size()
        nbytes = batch * ((M * K + N * K) * es + M * N * (oes + (4 if R is not None else 0) + (aux.element_size() if aux is not None else 0)
                                                          + (oes if C2 is not None else 0)))
        pr["records"].append((e0, e1, 2.0 * M * N * K * batch, float(nbytes),
                              (M, N, K, batch, act, bias is not None, R is not None, aux is not None, C2 is not None,
                               drop is not None and drop[0] > 0, bool(conv), stats is not None)))
        return C_
    L.check(L.lib().av_gemm(C.byref(a), stream()), "av_gemm")
    return C_


def linear(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, *, out_dtype: Optional[torch.dtype] = None,
           act: int = L.ACT_NONE, R: Optional[Tensor] = None, out: Optional[Tensor] = None, C2: Optional[Tensor] = None,
           aux: Optional[Tensor] = None, alpha: float = 1.0, drop: Optional[tuple] = None) -> Tensor:
    """y[M,N] = epilogue(x[M,K] @ w[N,K]^T + bias)  (nn.Linear layout).  x may be any [..., K] contiguous tensor."""
    K = x.shape[-1]
    M = x.numel() // K
    N = w.shape[0]
    assert w.shape[1] == K and x.is_contiguous() and w.is_contiguous()
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), dtype=out_dtype or x.dtype, device=x.device)
    gemm(x, w, out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, act=act, R=R, aux=aux, C2=C2, alpha=alpha, drop=drop)
    return out


def transpose(x: Tensor, out_dtype: Optional[torch.dtype] = None, pad_to: int = 1) -> Tensor:
    """[R, C] -> [C, Rpad] (Rpad = R rounded up to ``pad_to``, zero-filled)."""
    R, Cc = x.shape
    assert x.stride(1) == 1
    Rp = (R + pad_to - 1) // pad_to * pad_to
    out = torch.empty((Cc, Rp), dtype=out_dtype or x.dtype, device=x.device)
    L.check(L.lib().av_transpose(ptr(x), dt(x), ptr(out), dt(out), R, Cc, x.stride(0), Rp, stream()), "av_transpose")
    return out


_WT_CACHE = {}


def transpose_cached(b: Tensor, hot_ok: bool = False) -> Optional[Tensor]:
    """W^T of a weight-like operand, cached on (storage, version): frozen layers transpose once.  A weight that keeps changing (a
    trained layer: new version after every optimizer step) is *hot*: with ``hot_ok`` the caller gets None from its third version on and
    feeds the k-major operand to the GEMM directly instead of paying a transpose pass per step."""
    key = (b.data_ptr(), tuple(b.shape), b.dtype)
    ver = b._version
    hit = _WT_CACHE.get(key)
    if hit is None or hit[2]() is not b:
        import weakref
        hit = [ver, transpose(b), weakref.ref(b), 0]
        if len(_WT_CACHE) > 512:
            _WT_CACHE.clear()
        _WT_CACHE[key] = hit
    elif hit[0] != ver:
        hit[3] += 1
        if hot_ok and hit[3] >= 2:
            hit[0], hit[1] = None, None                          # hot: no transposed copy is kept
            return None
        hit[0], hit[1] = ver, transpose(b)
    elif hit[1] is None:
        if hot_ok:
            return None
        hit[0], hit[1] = ver, transpose(b)
    return hit[1]


def _fast_ok(t: Tensor, K: int, N: int) -> bool:
    return precision.is_lp(t.dtype) and K >= 64 and N > 64


# k-major operands straight into the fast GEMM (transposed LDS reads) instead of a transpose pass; AVAMD_GEMM_KMAJOR=0 = old path
KMAJOR = os.environ.get("AVAMD_GEMM_KMAJOR", "1") != "0"
KM8 = int(os.environ.get("AVAMD_GEMM_KM8", "1"))         # dW products of >= 32 tiles of 256 x 256 on the 8-phase kernel's k-major form (0: never, 2: from one tile on)
# dX of a weight that changes every step: 0 (default) = transpose the weight once per version (one 12 us pass, shared by both audio passes)
# and run the row-major 8-phase kernel; 1 = feed the k-major weight to the 128 x 128 kernel (no transpose pass)
KMAJOR_DX_HOT = os.environ.get("AVAMD_GEMM_KMAJOR_DX", "0") != "0"


def matmul_nn(a: Tensor, b: Tensor, *, out_dtype: Optional[torch.dtype] = None, act: int = L.ACT_NONE,
              aux: Optional[Tensor] = None, R: Optional[Tensor] = None, out: Optional[Tensor] = None, alpha: float = 1.0,
              b_is_weight: bool = False, drop: Optional[tuple] = None) -> Tensor:
    """y[M,N] = a[M,K] @ b[K,N]  (b row-major, e.g. dX = dY @ W with W [N_out,K_in])."""
    K = a.shape[-1]
    M = a.numel() // K
    N = b.shape[1]
    assert b.shape[0] == K and a.is_contiguous() and b.is_contiguous()
    if out is None:
        out = torch.empty(a.shape[:-1] + (N,), dtype=out_dtype or a.dtype, device=a.device)
    kmajor_ok = KMAJOR and N % 8 == 0
    if _fast_ok(a, K, N) and K % 64 == 0 and (b_is_weight or not kmajor_ok):
        bt = transpose_cached(b, hot_ok=kmajor_ok and KMAJOR_DX_HOT) if b_is_weight else transpose(b)   # [N, K]: K-contiguous operand for the fast kernel
        if bt is not None:
            gemm(a, bt, out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, act=act, aux=aux, R=R, alpha=alpha, drop=drop)
            return out
    # bf16, K % 64 == 0, N % 8 == 0, b not a (cached) weight: the fast kernel reads the k-major B through transposed LDS reads
    gemm(a, b, out, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, b_mode=L.B_KN, act=act, aux=aux, R=R, alpha=alpha, drop=drop)
    return out


def _split_k(tiles: int, Kk: int, mn: int, slots: int = 512) -> int:
    """Number of K slices for dW-shaped products: minimise rounds(tiles * S over 2 workgroups per CU) * K / S plus the
    partial-sum traffic (S fp32 slices written and read once)."""
    best, best_cost = 1, None
    for S in range(1, 9):
        if S > 1 and Kk // S < 512:
            break
        rounds = (tiles * S + slots - 1) // slots
        cost = rounds * (Kk / S) * 22e-9 + (S * mn * 8 / 5e12 if S > 1 else 0.0)
        if best_cost is None or cost < best_cost * 0.97:
            best, best_cost = S, cost
    return best


def _split_k8(tiles: int, Kk: int, mn: int, slots: int = 256):
    """(slices, k per slice) for the 8-phase kernel's k-major form (256 x 256 tiles, one workgroup per CU): rounds x (K-tiles x 1.55 us + 7 us of
    prologue / epilogue) plus the partial-sum traffic (S fp32 slices written and read once)."""
    best = (1, Kk, None)
    for S in range(1, 33):
        chunk = ((Kk + S - 1) // S + 63) // 64 * 64
        if S > 1 and chunk < 512:
            break
        Se = (Kk + chunk - 1) // chunk
        rounds = (tiles * Se + slots - 1) // slots
        cost = rounds * (chunk / 64 * 1.55e-6 + 7e-6) + (Se * mn * 8 / 5e12 if Se > 1 else 0.0)
        if best[2] is None or cost < best[2] * 0.97:
            best = (Se, chunk, cost)
    return best[0], best[1]


def matmul_tn(a: Tensor, b: Tensor, *, out: Optional[Tensor] = None, alpha: float = 1.0, accumulate: bool = False) -> Tensor:
    """y[M,N] (fp32) = a[K,M]^T @ b[K,N]   (dW = dY^T X: a = dY [tokens, out], b = X [tokens, in]).
    a / b may be row-strided views (last dim contiguous)."""
    Kk, M = a.shape
    N = b.shape[1]
    assert b.shape[0] == Kk and a.stride(1) == 1 and b.stride(1) == 1
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    if _fast_ok(a, Kk, N) and M > 64 and not (KMAJOR and M % 8 == 0 and N % 8 == 0 and N > 64 and a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0):
        at = transpose(a, pad_to=64)             # [M, Kp]  token dimension becomes the contiguous K (zero padded)
        bt = transpose(b, pad_to=64)             # [N, Kp]
        Kp = at.shape[1]
        gemm(at, bt, out, M=M, N=N, K=Kp, lda=Kp, ldb=Kp, ldc=N, alpha=alpha, R=out if accumulate else None)
        return out
    km = KMAJOR and _fast_ok(a, Kk, N) and M > 64 and M % 8 == 0 and N % 8 == 0 and a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0
    t8 = ((M + 255) // 256) * ((N + 255) // 256)
    if km and KM8 and M >= 256 and N >= 256 and (KM8 >= 2 or t8 >= 32):         # 8-phase kernel, k-major form (gemm_fast.hip: the same conditions)
        S, chunk = _split_k8(t8, Kk, M * N)
    else:
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        S = _split_k(tiles, Kk, M * N) if km else 1  # few output tiles, long K (tokens): split K over the batch dimension
        if S > 1:
            chunk = ((Kk + S - 1) // S + 63) // 64 * 64
            S = (Kk + chunk - 1) // chunk
    if S > 1:
        parts = torch.empty((S, M, N), dtype=torch.float32, device=a.device)
        gemm(a, b, parts, M=M, N=N, K=chunk, lda=a.stride(0), ldb=b.stride(0), ldc=N, a_mode=L.A_TRANS, b_mode=L.B_KN, batch=S,
             sA=chunk * a.stride(0), sB=chunk * b.stride(0), sC=M * N, k_total=Kk)
        L.check(L.lib().av_sum_slices(ptr(parts), S, M * N, M * N, float(alpha), ptr(out), int(accumulate), stream()), "av_sum_slices")
        return out
    gemm(a, b, out, M=M, N=N, K=Kk, lda=a.stride(0), ldb=b.stride(0), ldc=N, a_mode=L.A_TRANS, b_mode=L.B_KN, alpha=alpha,
         R=out if accumulate else None)
    return out


def layernorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, *, out_dtype: torch.dtype, eps: float = 1e-5, act: int = L.ACT_NONE,
                  save_stats: bool = False):
    cols = x.shape[-1]
    rows = x.numel() // cols
    assert x.is_contiguous()
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    mean = rstd = None
    if save_stats:
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    L.check(L.lib().av_layernorm_fwd(ptr(x), dt(x), ptr(gamma), ptr(beta), ptr(y), dt(y), ptr(mean), ptr(rstd), rows, cols,
                                     eps, act, stream()), "av_layernorm_fwd")
    return (y, mean, rstd) if save_stats else y


def layernorm_bwd(x: Tensor, dy: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, dres: Optional[Tensor] = None,
                  want_param_grads: bool = False, lp_copy: bool = False, lp_drop: Optional[tuple] = None, gb_acc: Optional[Tensor] = None,
                  packed_gb: bool = False):
    """dx (fp32) [, dgamma, dbeta]; with ``lp_copy`` the last element returned is a bf16 copy of dx written by the same kernel;
    ``lp_drop`` = (p, seed, stream id) makes that copy dx o dropout-mask / (1 - p).  ``gb_acc`` (a [2 cols] tensor from an earlier call) /
    ``packed_gb``: the parameter gradients come back as ONE packed tensor [dgamma | dbeta], accumulated into ``gb_acc`` when given (an
    earlier pass's tensor, or a zeroed view of a gradient bucket)."""
    cols = x.shape[-1]
    rows = x.numel() // cols
    assert x.is_contiguous() and dy.is_contiguous()
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dxl = torch.empty(x.shape, dtype=_lp(), device=x.device) if lp_copy else None
    nblk = max(1, min(512, (rows + 15) // 16))
    part = torch.empty((nblk, 2 * cols), dtype=torch.float32, device=x.device) if want_param_grads else None
    if lp_copy and lp_drop is not None and lp_drop[0] > 0:
        L.check(L.lib().av_layernorm_bwd_drop(ptr(x), dt(x), ptr(dy), dt(dy), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dx),
                                              ptr(part), nblk, rows, cols, ptr(dxl), float(lp_drop[0]), int(lp_drop[1]), int(lp_drop[2]), stream()),
                "av_layernorm_bwd_drop")
    else:
        L.check(L.lib().av_layernorm_bwd(ptr(x), dt(x), ptr(dy), dt(dy), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dx),
                                         ptr(part), nblk, rows, cols, ptr(dxl), stream()), "av_layernorm_bwd")
    res = (dx,)
    if want_param_grads:
        if gb_acc is not None:
            gb = colsum(part, out=gb_acc, accumulate=True)
            res = (dx, gb)
        elif packed_gb:
            res = (dx, colsum(part))
        else:
            gb = colsum(part)
            res = (dx, gb[:cols], gb[cols:])
    if lp_copy:
        return res + (dxl,)
    return res if want_param_grads else dx


def log_softmax_fwd(x: Tensor) -> Tensor:
    cols = x.shape[-1]
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    L.check(L.lib().av_log_softmax_fwd(ptr(x), dt(x), ptr(y), x.numel() // cols, cols, stream()), "av_log_softmax_fwd")
    return y


def log_softmax_bwd(y: Tensor, dy: Tensor, out_dtype: torch.dtype, pad_to: int = 0) -> Tensor:
    """dx = dy - exp(y) * sum(dy).  ``pad_to`` > 0: the rows of dx are padded with zero columns to a multiple of it (returned tensor
    [..., ceil(cols / pad_to) * pad_to]: a K-padded operand for the dX product of the layer below)."""
    cols = y.shape[-1]
    ldx = (cols + pad_to - 1) // pad_to * pad_to if pad_to > 0 else cols
    dx = torch.empty(y.shape[:-1] + (ldx,), dtype=out_dtype, device=y.device)
    L.check(L.lib().av_log_softmax_bwd_ld(ptr(y), ptr(dy), ptr(dx), dt(dx), y.numel() // cols, cols, ldx, stream()), "av_log_softmax_bwd")
    return dx


def colsum(x: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    cols = x.shape[-1]
    if x.is_contiguous():
        rows, ld = x.numel() // cols, cols
    else:                                                   # a column slice of a wider matrix (rows strided, last dim contiguous)
        assert x.dim() == 2 and x.stride(1) == 1
        rows, ld = x.shape[0], x.stride(0)
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=x.device)
        accumulate = False
    L.check(L.lib().av_colsum(ptr(x), dt(x), ptr(out), rows, cols, ld, int(accumulate), stream()), "av_colsum")
    return out


def colsum_into(x: Tensor, zeroed_view: Optional[Tensor]) -> Tensor:
    """Column sums accumulated into a pre-zeroed view of a gradient bucket (no clear launch), or into a fresh tensor when there is none."""
    return colsum(x, out=zeroed_view, accumulate=True) if zeroed_view is not None else colsum(x)


def cast(x: Tensor, dtype: torch.dtype) -> Tensor:
    if x.dtype == dtype:
        return x
    assert x.is_contiguous()
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    L.check(L.lib().av_cast(ptr(x), dt(x), ptr(y), dt(y), x.numel(), stream()), "av_cast")
    return y


def cast_dropout(x: Tensor, dtype: torch.dtype, drop: Optional[tuple]) -> Tensor:
    """cast(x * mask): ``drop`` = (p, seed, stream id) or None (plain cast)."""
    if drop is None or drop[0] <= 0:
        return cast(x, dtype)
    assert x.is_contiguous()
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    L.check(L.lib().av_cast_dropout(ptr(x), dt(x), ptr(y), dt(y), x.numel(), float(drop[0]), int(drop[1]), int(drop[2]), stream()), "av_cast_dropout")
    return y


def axpby(a: float, x: Tensor, b: float, y: Tensor) -> Tensor:
    """y = a*x + b*y  (y fp32, in place)."""
    assert x.is_contiguous() and y.is_contiguous() and y.dtype == torch.float32 and x.numel() == y.numel()
    L.check(L.lib().av_axpby(a, ptr(x), dt(x), b, ptr(y), x.numel(), stream()), "av_axpby")
    return y


def mask_rows_(x: Tensor, keep_u8: Tensor) -> Tensor:
    cols = x.shape[-1]
    L.check(L.lib().av_mask_rows(ptr(x), dt(x), ptr(keep_u8), x.numel() // cols, cols, stream()), "av_mask_rows")
    return x


# ---------------------------------------------------------------------------------------------------------------
# attention.  q/k/v/o are [B, T, H, D] views (last dim contiguous, head stride == D), e.g. slices of a packed
# [B, T, 3, H, D] projection buffer — no copies are made.
# ---------------------------------------------------------------------------------------------------------------
def _chk_view(t: Tensor, name: str):
    if t.dim() != 4 or t.stride(3) != 1 or t.stride(2) != t.shape[3]:
        raise ValueError(f"{name}: expected a [B,T,H,D] view with contiguous D and head stride D, got {tuple(t.shape)} / {t.stride()}")


_ATTN_SHORT = os.environ.get("AVAMD_ATTN_SHORT", "1") != "0"


def attention_mask_shape_ok(dtype, B: int, Tq: int, Tk: int, D: int) -> bool:
    return _ATTN_SHORT and precision.is_lp(dtype) and D == 64 and Tq <= 256 and Tk <= 256 and B <= 65535


def attention_dropmask(B: int, H: int, Tq: int, Tk: int, drop: tuple, device) -> Tensor:
    """Keep bits of the attention-probability dropout of a [B, H, Tq, Tk] problem, evaluated once for the whole-sequence forward and both
    phases of its backward (check ``attention_mask_shape_ok`` first)."""
    mask = torch.empty((B, H, (Tq + 15) // 16, 64), dtype=torch.int64, device=device)
    L.check(L.lib().av_attention_dropmask(ptr(mask), B, H, Tq, Tk, float(drop[0]), int(drop[1]), int(drop[2]), stream()), "av_attention_dropmask")
    return mask


def attention_fwd(q: Tensor, k: Tensor, v: Tensor, klen: Optional[Tensor], scale: float, need_lse: bool = True,
                  drop: Optional[tuple] = None, drop_mask: Optional[Tensor] = None):
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk_view(t, n)
    B, Tq, H, D = q.shape
    Tk = k.shape[1]
    o = torch.empty((B, Tq, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, Tq), dtype=torch.float32, device=q.device) if need_lse else None
    dp, dseed, dstream = (float(drop[0]), int(drop[1]), int(drop[2])) if (drop is not None and drop[0] > 0) else (0.0, 0, 0)
    es = q.element_size()
    _probed(f"fwd{D}", 4.0 * B * H * Tq * Tk * D, B * H * D * es * (2 * Tq + 2 * Tk),
            lambda: L.check(L.lib().av_attention_fwd_mask(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), dt(q), B, H, Tq, Tk, D,
                                                          q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                                                          o.stride(0), o.stride(1), ptr(klen), scale, dp, dseed, dstream,
                                                          ptr(drop_mask) if dp > 0 else None, stream()), "av_attention_fwd"))
    return o, lse


def fusion_xattn_fwd(a: Tensor, v: Tensor, w_in: Tensor, b_in: Tensor, nh: int, scale: float, save: bool):
    """Fused in-projection + cross-attention core (csrc/fusion_attn.hip): a, v [B, T, E] bf16 -> (o [B,T,nh,hd], q [B,T,nh,hd] | None,
    kv [B,T,2,nh,hd] | None, lse [B,nh,T] | None)."""
    B, T, E = a.shape
    hd = E // nh
    assert a.is_contiguous() and v.is_contiguous() and w_in.is_contiguous() and w_in.shape == (3 * E, E) and b_in.dtype == torch.float32
    o = torch.empty((B, T, nh, hd), dtype=a.dtype, device=a.device)
    q = torch.empty((B, T, nh, hd), dtype=a.dtype, device=a.device) if save else None
    kv = torch.empty((B, T, 2, nh, hd), dtype=a.dtype, device=a.device) if save else None
    lse = torch.empty((B, nh, T), dtype=torch.float32, device=a.device) if save else None
    fl = B * (6.0 * T * E * E + 4.0 * T * T * E)
    by = a.element_size() * (2 * B * T * E + 3 * E * E + B * T * E * (4 if save else 1))
    _probed("blockfwd", fl, by,
            lambda: L.check(L.lib().av_fusion_xattn_fwd(ptr(a), ptr(v), ptr(w_in), ptr(b_in), ptr(q), ptr(kv), ptr(o), ptr(lse), B, T, E, nh, scale,
                                                        stream()), "av_fusion_xattn_fwd"))
    return o, q, kv, lse


def fusion_xattn_bwd(q: Tensor, kv: Tensor, o: Tensor, do: Tensor, lse: Tensor, scale: float):
    """Backward of the fused cross-attention core (csrc/fusion_attn.hip): q, o, do [B,T,nh,hd], kv [B,T,2,nh,hd] bf16 -> (dq, dkv)."""
    B, T, nh, hd = q.shape
    E = nh * hd
    assert q.is_contiguous() and kv.is_contiguous() and o.is_contiguous() and do.is_contiguous()
    dq = torch.empty_like(q); dkv = torch.empty_like(kv)
    es = q.element_size()
    _probed("blockbwd", 10.0 * B * T * T * E, es * B * T * E * 8,
            lambda: L.check(L.lib().av_fusion_xattn_bwd(ptr(q), ptr(kv), ptr(o), ptr(do), ptr(lse), ptr(dq), ptr(dkv), B, T, E, nh, scale, stream()),
                            "av_fusion_xattn_bwd"))
    return dq, dkv


def attention_bwd(q: Tensor, k: Tensor, v: Tensor, do: Tensor, dq: Tensor, dk: Tensor, dv: Tensor, klen: Optional[Tensor],
                  scale: float, o: Optional[Tensor] = None, lse: Optional[Tensor] = None, drop: Optional[tuple] = None,
                  drop_mask: Optional[Tensor] = None) -> None:
    """Backward of attention_fwd from batched MFMA GEMMs + row kernels (P is re-materialised, T x T is small here):
    P = softmax(scale QK^T); dV = P^T dO; dP = dO V^T; dS = scale P o (dP - rowsum(dP o P)); dQ = dS K; dK = dS^T Q.
    dq/dk/dv are [B,T,H,D] output views (written in place)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (do, "do"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
        _chk_view(t, n)
    B, Tq, H, D = q.shape
    Tk = k.shape[1]
    dp, dseed, dstream = (float(drop[0]), int(drop[1]), int(drop[2])) if (drop is not None and drop[0] > 0) else (0.0, 0, 0)
    if precision.is_lp(q.dtype) and o is not None and lse is not None:     # fused flash-style backward (attention_bwd.hip)
        _chk_view(o, "o")
        st = (C.c_longlong * 16)(*[x for t in (q, k, v, o, do, dq, dk, dv) for x in (t.stride(0), t.stride(1))])
        delta = torch.empty((B, H, Tq), dtype=torch.float32, device=q.device)
        es = q.element_size()
        _probed(f"bwd{D}", 10.0 * B * H * Tq * Tk * D, B * H * D * es * (4 * Tq + 4 * Tk),
                lambda: L.check(L.lib().av_attention_bwd_mask(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv),
                                                              B, H, Tq, Tk, D, st, ptr(klen), scale, dp, dseed, dstream,
                                                              ptr(drop_mask) if dp > 0 else None, stream()), "av_attention_bwd"))
        return
    # unfused form (fp32 parity mode).  With dropout the row pitch equals the Philox row pitch of the attention kernels (keys padded
    # to 4, attn_common.h), so the mask of element (b, h, q, k) is the mask of linear index row * ld + k of these buffers
    ld = (Tk + 3) // 4 * 4 if dp > 0 else (Tk + 7) // 8 * 8
    dev = q.device
    drop_t = (dp, dseed, dstream)
    S = torch.empty((B, H, Tq, ld), dtype=torch.float32, device=dev)
    bh = dict(batch=B * H, batch_inner=H)
    gemm(q, k, S, M=Tq, N=Tk, K=D, lda=q.stride(1), ldb=k.stride(1), ldc=ld, sA=D, oA=q.stride(0), sB=D, oB=k.stride(0),
         sC=Tq * ld, oC=H * Tq * ld, **bh)
    P = torch.empty((B, H, Tq, ld), dtype=q.dtype, device=dev)
    L.check(L.lib().av_softmax_rows(ptr(S), ptr(P), dt(P), B * H * Tq, Tk, scale, ptr(klen), H * Tq, ld, stream()), "av_softmax_rows")
    # dV[key, d] = sum_q Pd[q, key] dO[q, d]   (Pd = P o mask / (1 - p): what the forward multiplied V with, hf:457)
    Pd = cast_dropout(P, P.dtype, drop_t) if dp > 0 else P
    gemm(Pd, do, dv, M=Tk, N=D, K=Tq, lda=ld, ldb=do.stride(1), ldc=dv.stride(1), a_mode=L.A_TRANS, b_mode=L.B_KN,
         sA=Tq * ld, oA=H * Tq * ld, sB=D, oB=do.stride(0), sC=D, oC=dv.stride(0), **bh)
    # dP = dO V^T  (into S)
    gemm(do, v, S, M=Tq, N=Tk, K=D, lda=do.stride(1), ldb=v.stride(1), ldc=ld, sA=D, oA=do.stride(0), sB=D, oB=v.stride(0),
         sC=Tq * ld, oC=H * Tq * ld, **bh)
    if dp > 0:
        S = cast_dropout(S, torch.float32, drop_t)           # dP = dPd o mask / (1 - p)
    dS = torch.empty((B, H, Tq, ld), dtype=q.dtype, device=dev)
    L.check(L.lib().av_softmax_bwd_rows(ptr(P), dt(P), ptr(S), ptr(dS), dt(dS), B * H * Tq, Tk, scale, ld, stream()), "av_softmax_bwd_rows")
    # dQ = dS K ; dK = dS^T Q
    gemm(dS, k, dq, M=Tq, N=D, K=Tk, lda=ld, ldb=k.stride(1), ldc=dq.stride(1), b_mode=L.B_KN, sA=Tq * ld, oA=H * Tq * ld,
         sB=D, oB=k.stride(0), sC=D, oC=dq.stride(0), **bh)
    gemm(dS, q, dk, M=Tk, N=D, K=Tq, lda=ld, ldb=q.stride(1), ldc=dk.stride(1), a_mode=L.A_TRANS, b_mode=L.B_KN,
         sA=Tq * ld, oA=H * Tq * ld, sB=D, oB=q.stride(0), sC=D, oC=dk.stride(0), **bh)


# ---------------------------------------------------------------------------------------------------------------
# CTC loss on the device (csrc/ctc_loss.hip): opt-in replacement of nn.CTCLoss (model/trainer.py:25,116-117).  Lengths and targets stay
# on the device, nothing in the call synchronises.
# ---------------------------------------------------------------------------------------------------------------
def native_ctc_default() -> bool:
    """The environment switch AVAMD_NATIVE_CTC (default "0": nn.CTCLoss on PyTorch-ROCm, as BASELINE north_star prescribes), read when a
    CTCDecoder / MultimodalTrainer is constructed with ``native_ctc=None``."""
    return os.environ.get("AVAMD_NATIVE_CTC", "0") != "0"


def _ctc_rows(who: str, log_probs, batch_first: bool, *, max_T: Optional[int] = None, min_V: int = 1):
    """The validated fp32 GPU block [B, T, V] (``batch_first``) or [T, B, V] of a CTC call -> (detached view with contiguous rows, B, T, V,
    stride_b, stride_t); a view whose last dimension is not contiguous is copied.  ``max_T``: also V >= ``min_V`` and 1 <= T <= ``max_T``."""
    if not isinstance(log_probs, Tensor) or not log_probs.is_cuda:
        raise RuntimeError(f"{who} (HIP): log_probs must be on the GPU; there is no CPU fallback (the host paths take host tensors)")
    if log_probs.dim() != 3:
        raise ValueError(f"{who}: log_probs must be [B, T, V] with batch_first, [T, B, V] without, got shape {tuple(log_probs.shape)}")
    if log_probs.dtype != torch.float32:
        raise TypeError(f"{who}: log_probs must be float32 (the CTC kernels have no low-precision operand), got {log_probs.dtype}")
    lp = log_probs.detach()
    if lp.stride(2) != 1:
        lp = lp.contiguous()
    if batch_first:
        (B, T, V), sb, st = lp.shape, lp.stride(0), lp.stride(1)
    else:
        (T, B, V), st, sb = lp.shape, lp.stride(0), lp.stride(1)
    if max_T is not None and (V < min_V or not 1 <= T <= max_T):
        raise ValueError(f"{who}: need V >= {min_V} and 1 <= T <= {max_T}, got T={T} V={V}")
    return lp, B, T, V, sb, st


def _ctc_lengths(who: str, name: str, t, B: int, device, optional: bool = False) -> Optional[Tensor]:
    """An integer length vector of B items -> int64 on ``device``; a host tensor is copied without blocking."""
    if t is None and optional:
        return None
    if not isinstance(t, Tensor):
        t = torch.as_tensor(t, dtype=torch.long)
    if t.dim() != 1 or t.numel() != B:
        raise ValueError(f"{who}: {name} must hold one length per batch item ({B}), got shape {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError(f"{who}: {name} must be an integer tensor, got {t.dtype}")
    return t.to(device=device, dtype=torch.long, non_blocking=True).contiguous()


def _ctc_targets(targets: Tensor, B: int, device):
    """Padded integer targets [B, Lmax] -> (int64 rows on ``device`` with a unit inner stride and a row stride >= Lmax, Lmax); Lmax = 0
    gives one column of zeros, which the kernels never read."""
    Lmax = targets.shape[1]
    tg = targets.to(device=device, dtype=torch.long, non_blocking=True)
    if Lmax == 0:
        tg = torch.zeros((B, 1), dtype=torch.long, device=device)
    elif tg.stride(1) != 1 or tg.stride(0) < Lmax:
        tg = tg.contiguous()
    return tg, Lmax


class _CtcLossFn(torch.autograd.Function):
    """nll [B] = av_ctc_loss_fwd; d nll / d log_probs = av_ctc_loss_bwd (torch's form: grad_nll (exp(lp) - occupancy)).  ``rows`` is
    ``_ctc_rows`` of ``log_probs``, ``tg`` the targets of ``_ctc_targets``."""

    @staticmethod
    def forward(fctx, log_probs, rows, tg, Lmax, input_lengths, target_lengths, blank, zero_infinity, batch_first):
        lp, B, T, V, sb, st = rows
        S_max = 2 * Lmax + 1
        need = fctx.needs_input_grad[0]
        nll = torch.empty(B, dtype=torch.float32, device=lp.device)
        la = torch.empty((B, T, S_max), dtype=torch.float32, device=lp.device) if need else None
        lb = torch.empty((B, T, S_max), dtype=torch.float32, device=lp.device) if need else None
        L.check(L.lib().av_ctc_loss_fwd(ptr(lp), sb, st, ptr(tg), tg.stride(0), ptr(input_lengths), ptr(target_lengths), B, T, V, S_max,
                                        int(blank), int(bool(zero_infinity)), ptr(nll), ptr(la), ptr(lb), stream()), "av_ctc_loss_fwd")
        if need:
            fctx.save_for_backward(lp, tg, input_lengths, target_lengths, nll, la, lb)
            fctx.cfg = (B, T, V, S_max, sb, st, int(blank), bool(batch_first))
        return nll

    @staticmethod
    def backward(fctx, g):
        lp, tg, il, tl, nll, la, lb = fctx.saved_tensors
        B, T, V, S_max, sb, st, blank, batch_first = fctx.cfg
        g = g.contiguous().float()
        grad = torch.empty((B, T, V), dtype=torch.float32, device=lp.device)
        L.check(L.lib().av_ctc_loss_bwd(ptr(lp), sb, st, ptr(tg), tg.stride(0), ptr(il), ptr(tl), B, T, V, S_max, blank, ptr(nll), ptr(la),
                                        ptr(lb), ptr(g), ptr(grad), stream()), "av_ctc_loss_bwd")
        return (grad if batch_first else grad.transpose(0, 1)), None, None, None, None, None, None, None, None


def ctc_loss(log_probs: Tensor, targets: Tensor, input_lengths, target_lengths, blank: int = 0, reduction: str = "mean",
             zero_infinity: bool = False, batch_first: bool = False) -> Tensor:
    """torch.nn.functional.ctc_loss on the HIP kernels: same argument order, defaults and reductions ("mean" = mean over the batch of
    nll_i / max(L_i, 1), "sum", "none").  ``log_probs`` fp32 [T, B, V] (``batch_first``: [B, T, V]); any view with a contiguous last
    dimension is taken without a copy.  ``targets`` int64 [B, Lmax], padded (the 1-D concatenated form is not supported).  The
    lengths may live on the device (nothing is read back) or on the host (copied without blocking).  With ``zero_infinity=False`` an
    infeasible item returns +inf and its gradient is unspecified (here: zero)."""
    rows = _ctc_rows("ctc_loss", log_probs, batch_first)
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"ctc_loss: reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
    B, dev = rows[1], log_probs.device
    if targets.dim() != 2:
        raise NotImplementedError("ctc_loss (HIP): targets must be the padded 2-D form [B, Lmax]; 1-D concatenated targets are not supported")
    if targets.shape[0] != B:
        raise ValueError(f"ctc_loss: targets has {targets.shape[0]} rows for a batch of {B}")
    if targets.dtype.is_floating_point or targets.dtype == torch.bool:
        raise TypeError(f"ctc_loss: targets must be an integer tensor, got {targets.dtype}")
    tg, Lmax = _ctc_targets(targets, B, dev)
    il = _ctc_lengths("ctc_loss", "input_lengths", input_lengths, B, dev)
    tl = _ctc_lengths("ctc_loss", "target_lengths", target_lengths, B, dev)
    nll = _CtcLossFn.apply(log_probs, rows, tg, Lmax, il, tl, int(blank), bool(zero_infinity), bool(batch_first))
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum()
    return (nll / tl.clamp_min(1).to(torch.float32)).mean()


class _CtcNbestFn(torch.autograd.Function):
    """nll [B, N] = av_ctc_nbest_fwd; d (sum g nll) / d log_probs = av_ctc_nbest_bwd: one [B, T, V] gradient for the N hypotheses."""

    @staticmethod
    def forward(fctx, log_probs, rows, hyp_ids, hyp_lengths, input_lengths, blank, batch_first, S_max):
        lp, B, T, V, sb, st = rows
        N, Lh = hyp_ids.shape[1], hyp_ids.shape[2]
        Lmax = (S_max - 1) // 2
        ld_n = hyp_ids.stride(1) if N > 1 else max(Lh, 1)
        ld_b = hyp_ids.stride(0) if B > 1 else (N - 1) * ld_n + max(Lh, 1)
        need = fctx.needs_input_grad[0]
        nll = torch.empty((B, N), dtype=torch.float32, device=lp.device)
        la = torch.empty((B, N, T, S_max), dtype=torch.float32, device=lp.device) if need else None
        lb = torch.empty((B, N, T, S_max), dtype=torch.float32, device=lp.device) if need else None
        L.check(L.lib().av_ctc_nbest_fwd(ptr(lp), sb, st, ptr(hyp_ids), ld_b, ld_n, ptr(hyp_lengths), ptr(input_lengths), B, N, T, V, S_max,
                                         int(blank), ptr(nll), ptr(la), ptr(lb), stream()), "av_ctc_nbest_fwd")
        if need:
            fctx.save_for_backward(lp, hyp_ids, hyp_lengths, input_lengths, nll, la, lb)
            fctx.cfg = (B, N, T, V, S_max, sb, st, ld_b, ld_n, int(blank), bool(batch_first))
        return nll

    @staticmethod
    def backward(fctx, g):
        lp, hi, hl, il, nll, la, lb = fctx.saved_tensors
        B, N, T, V, S_max, sb, st, ld_b, ld_n, blank, batch_first = fctx.cfg
        g = g.contiguous().float()
        grad = torch.empty((B, T, V), dtype=torch.float32, device=lp.device)
        L.check(L.lib().av_ctc_nbest_bwd(ptr(lp), sb, st, ptr(hi), ld_b, ld_n, ptr(hl), ptr(il), B, N, T, V, S_max, blank, ptr(nll), ptr(la),
                                         ptr(lb), ptr(g), ptr(grad), stream()), "av_ctc_nbest_bwd")
        return (grad if batch_first else grad.transpose(0, 1)), None, None, None, None, None, None, None


def ctc_nbest_nll(log_probs: Tensor, hyp_ids: Tensor, hyp_lengths, input_lengths, blank: int = 0, batch_first: bool = True,
                  max_len: Optional[int] = None) -> Tensor:
    """CTC negative log-likelihood of N label sequences per utterance against one shared block of log-probs (csrc/ctc_loss.hip, the n-best
    form): fp32 [B, N], differentiable with respect to ``log_probs`` - the N hypotheses' gradients arrive as ONE [B, T, V] tensor, the
    log-probs are never expanded.  ``log_probs`` fp32 [B, T, V] (``batch_first=False``: [T, B, V]); any view with a contiguous last
    dimension is taken without a copy.  ``hyp_ids`` integer [B, N, Lh] (an int32 view with unit inner stride is taken without a copy: the
    beam kernel's id block as it is), ``hyp_lengths`` [B, N], ``input_lengths`` [B] (one per utterance, shared by its hypotheses); lengths
    on the host are copied without blocking, nothing synchronises.  A hypothesis is OUT - nll = +inf, no gradient, the incoming gradient at
    that position never read - when its length is < 0 (absent) or > ``max_len`` (not clamped), when an id is outside [0, V) or when no path
    exists.  ``max_len`` (default Lh) sets the lattice width S_max = 2 max_len + 1 for callers who want smaller workspaces; every other
    hypothesis' nll is bit for bit ``ctc_loss(..., reduction="none", zero_infinity=False)`` of that item."""
    rows = _ctc_rows("ctc_nbest_nll", log_probs, batch_first)
    B = rows[1]
    if not isinstance(hyp_ids, Tensor) or hyp_ids.dim() != 3 or hyp_ids.shape[0] != B:
        raise ValueError(f"ctc_nbest_nll: hyp_ids must be an integer tensor [B={B}, N, Lh], got "
                         f"{tuple(hyp_ids.shape) if isinstance(hyp_ids, Tensor) else type(hyp_ids).__name__}")
    if hyp_ids.dtype.is_floating_point or hyp_ids.dtype.is_complex or hyp_ids.dtype == torch.bool:
        raise TypeError(f"ctc_nbest_nll: hyp_ids must be an integer tensor, got {hyp_ids.dtype}")
    N, Lh = hyp_ids.shape[1], hyp_ids.shape[2]
    if not 1 <= N <= 64:
        raise ValueError(f"ctc_nbest_nll: N = {N} hypotheses per utterance outside [1, 64]")
    max_len = Lh if max_len is None else int(max_len)
    if not 0 <= max_len <= Lh:
        raise ValueError(f"ctc_nbest_nll: max_len {max_len} outside [0, Lh = {Lh}]")
    dev = log_probs.device
    hi = hyp_ids.to(device=dev, dtype=torch.int32, non_blocking=True)
    if Lh == 0:
        hi = torch.zeros((B, N, 1), dtype=torch.int32, device=dev)
    elif hi.stride(2) != 1 or (N > 1 and hi.stride(1) < Lh) or (B > 1 and hi.stride(0) < (N - 1) * (hi.stride(1) if N > 1 else Lh) + Lh):
        hi = hi.contiguous()
    if not isinstance(hyp_lengths, Tensor):
        hyp_lengths = torch.as_tensor(hyp_lengths, dtype=torch.long)
    if hyp_lengths.dtype.is_floating_point or hyp_lengths.dtype == torch.bool or hyp_lengths.numel() != B * N:
        raise ValueError(f"ctc_nbest_nll: hyp_lengths must hold [B={B}, N={N}] integer lengths, got {hyp_lengths.dtype} {tuple(hyp_lengths.shape)}")
    hl = hyp_lengths.reshape(B, N).to(device=dev, dtype=torch.long, non_blocking=True).contiguous()
    il = _ctc_lengths("ctc_nbest_nll", "input_lengths", input_lengths, B, dev)
    return _CtcNbestFn.apply(log_probs, rows, hi, hl, il, int(blank), bool(batch_first), 2 * max_len + 1)


def ctc_align(log_probs: Tensor, targets: Tensor, input_lengths, target_lengths, blank: int = 0, batch_first: bool = False):
    """CTC forced alignment on the kernel of csrc/ctc_align.hip, arguments as for ``ctc_loss``: ``log_probs`` fp32 [T, B, V]
    (``batch_first``: [B, T, V]), any view with a contiguous last dimension is taken without a copy; ``targets`` integer [B, Lmax], padded;
    lengths on the device (nothing is read back) or on the host (copied without blocking).  Returns (states int32 [B, T], spans int32
    [B, Lmax, 2], token_scores fp32 [B, Lmax], score fp32 [B]) on the device; the law and the outputs of an infeasible item: align.py."""
    lp, B, T, V, sb, st = _ctc_rows("ctc_align", log_probs, batch_first)
    if targets.dim() != 2 or targets.dtype.is_floating_point or targets.dtype == torch.bool:
        raise TypeError(f"ctc_align: targets must be an integer tensor [B, Lmax], got {targets.dtype} {tuple(targets.shape)}")
    if targets.shape[0] != B:
        raise ValueError(f"ctc_align: targets has {targets.shape[0]} rows for a batch of {B}")
    dev = lp.device
    tg, Lmax = _ctc_targets(targets, B, dev)
    il = _ctc_lengths("ctc_align", "input_lengths", input_lengths, B, dev)
    tl = _ctc_lengths("ctc_align", "target_lengths", target_lengths, B, dev)
    S_max = 2 * Lmax + 1
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    spans = torch.empty((B, Lmax, 2), dtype=torch.int32, device=dev)
    tok = torch.empty((B, Lmax), dtype=torch.float32, device=dev)
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    if B == 0:
        return states, spans, tok, score
    need = L.ll(0)
    L.check(L.lib().av_ctc_align_workspace_bytes(B, T, S_max, C.byref(need)), "av_ctc_align_workspace_bytes")
    ws = torch.empty((max(1, (need.value + 3) // 4),), dtype=torch.int32, device=dev)
    L.check(L.lib().av_ctc_align(ptr(lp), sb, st, ptr(tg), tg.stride(0), ptr(il), ptr(tl), B, T, V, S_max, int(blank), ptr(states),
                                 ptr(spans) if Lmax else None, ptr(tok) if Lmax else None, ptr(score), ptr(ws), ws.numel() * 4, stream()),
            "av_ctc_align")
    return states, spans, tok, score


def ctc_segment(log_probs: Tensor, targets: Tensor, input_lengths, target_lengths, utterances=None, blank: int = 0, free: int = 0,
                score_window: int = 30, batch_first: bool = True, max_workspace_bytes: int = 4 << 30):
    """CTC segmentation on the kernel of csrc/ctc_segment.hip: ``log_probs`` fp32 [B, T, V] (``batch_first=False``: [T, B, V]; any view with
    a contiguous last dimension is taken without a copy, T has no limit), ``targets`` integer [B, Lmax <= 8191] padded, ``utterances``
    integer [B, U, 2] token ranges or None; lengths, targets and utterances on the device (nothing is read back) or on the host (copied
    without blocking).  ``free``: bit 0 = free start, bit 1 = free end.  Returns (states int32 [B, T], spans int32 [B, Lmax, 2],
    token_scores fp32 [B, Lmax], score fp32 [B], frame_scores fp32 [B, T], utt_spans int32 [B, U, 2], utt_means fp32 [B, U], utt_scores
    fp32 [B, U]) on the device; the law: segmentation.py.  The workspace this call owns holds 2 bits per frame and state; a shape that
    needs more than ``max_workspace_bytes`` raises before anything is allocated."""
    lp, B, T, V, sb, st = _ctc_rows("ctc_segment", log_probs, batch_first)
    if targets.dim() != 2 or targets.dtype.is_floating_point or targets.dtype == torch.bool:
        raise TypeError(f"ctc_segment: targets must be an integer tensor [B, Lmax], got {targets.dtype} {tuple(targets.shape)}")
    if targets.shape[0] != B:
        raise ValueError(f"ctc_segment: targets has {targets.shape[0]} rows for a batch of {B}")
    dev = lp.device
    U = 0 if utterances is None else utterances.shape[1]
    if utterances is not None and (utterances.dim() != 3 or utterances.shape[0] != B or utterances.shape[2] != 2
                                   or utterances.dtype.is_floating_point or utterances.dtype == torch.bool):
        raise TypeError(f"ctc_segment: utterances must be an integer tensor [B={B}, U, 2], got {utterances.dtype} {tuple(utterances.shape)}")
    tg, Lmax = _ctc_targets(targets, B, dev)
    il = _ctc_lengths("ctc_segment", "input_lengths", input_lengths, B, dev)
    tl = _ctc_lengths("ctc_segment", "target_lengths", target_lengths, B, dev)
    S_max = 2 * Lmax + 1
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    spans = torch.empty((B, Lmax, 2), dtype=torch.int32, device=dev)
    tok = torch.empty((B, Lmax), dtype=torch.float32, device=dev)
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    frame = torch.empty((B, T), dtype=torch.float32, device=dev)
    usp = torch.empty((B, U, 2), dtype=torch.int32, device=dev)
    umean = torch.empty((B, U), dtype=torch.float32, device=dev)
    uscore = torch.empty((B, U), dtype=torch.float32, device=dev)
    if B == 0:
        return states, spans, tok, score, frame, usp, umean, uscore
    need = L.ll(0)
    L.check(L.lib().av_ctc_segment_workspace_bytes(B, T, S_max, C.byref(need)), "av_ctc_segment_workspace_bytes")
    if need.value > int(max_workspace_bytes):
        raise ValueError(f"ctc_segment: T = {T} frames against L = {Lmax} labels (B = {B}) needs a move workspace of {need.value} bytes, more "
                         f"than max_workspace_bytes = {int(max_workspace_bytes)}: split the recording or raise the limit")
    ut = utterances.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous() if U else None
    ws = torch.empty((max(1, (need.value + 3) // 4),), dtype=torch.int32, device=dev)
    L.check(L.lib().av_ctc_segment(ptr(lp), sb, st, ptr(tg), tg.stride(0), ptr(il), ptr(tl), ptr(ut) if U else None, B, T, V, S_max, U,
                                   int(blank), int(free), int(score_window), ptr(states), ptr(spans) if Lmax else None,
                                   ptr(tok) if Lmax else None, ptr(score), ptr(frame), ptr(usp) if U else None,
                                   ptr(umean) if U else None, ptr(uscore) if U else None, ptr(ws), ws.numel() * 4, stream()),
            "av_ctc_segment")
    return states, spans, tok, score, frame, usp, umean, uscore


def ctc_spot(log_probs: Tensor, keywords: Tensor, kw_lengths, input_lengths=None, blank: int = 0, max_hits: int = 4,
             min_score: float = float("-inf"), batch_first: bool = True):
    """CTC keyword spotting on the kernels of csrc/ctc_spot.hip: ``log_probs`` fp32 [B, T, V] (``batch_first=False``: [T, B, V]; any view
    with a contiguous last dimension is taken without a copy, T has no limit), ``keywords`` integer [K, Lmax <= 32] padded, ``kw_lengths``
    [K] and ``input_lengths`` [B] or None on the device (nothing is read back) or on the host (copied without blocking).  Returns (hits
    int32 [B, K, max_hits, 2] padded with -1, scores fp32 [B, K, max_hits] padded with -inf, counts int32 [B, K]) on the device; the
    law: spot.py."""
    lp, B, T, V, sb, st = _ctc_rows("ctc_spot", log_probs, batch_first)
    if not isinstance(keywords, Tensor) or keywords.dim() != 2 or keywords.dtype.is_floating_point or keywords.dtype == torch.bool:
        raise TypeError("ctc_spot: keywords must be an integer tensor [K, Lmax], got "
                        f"{(keywords.dtype, tuple(keywords.shape)) if isinstance(keywords, Tensor) else type(keywords).__name__}")
    K, Lmax = keywords.shape
    N, blank, min_score = int(max_hits), int(blank), float(min_score)
    if not 1 <= Lmax <= 32 or not 1 <= N <= 8 or min_score != min_score or not 0 <= blank < V:
        raise ValueError(f"ctc_spot: need 1 <= Lmax <= 32, 1 <= max_hits <= 8, 0 <= blank < V and a min_score that is not NaN, got Lmax={Lmax} "
                         f"max_hits={N} blank={blank} V={V} min_score={min_score}")
    dev = lp.device
    hits = torch.empty((B, K, N, 2), dtype=torch.int32, device=dev)
    scores = torch.empty((B, K, N), dtype=torch.float32, device=dev)
    counts = torch.empty((B, K), dtype=torch.int32, device=dev)
    if B == 0 or K == 0:
        return hits, scores, counts
    kw = keywords.to(device=dev, dtype=torch.int32, non_blocking=True)
    if kw.stride(1) != 1 or kw.stride(0) < Lmax:
        kw = kw.contiguous()
    kl = _ctc_lengths("ctc_spot", "kw_lengths", kw_lengths, K, dev).to(torch.int32)
    il = _ctc_lengths("ctc_spot", "input_lengths", input_lengths, B, dev, optional=True)
    need = L.ll(0)
    L.check(L.lib().av_ctc_spot_workspace_bytes(B, T, K, C.byref(need)), "av_ctc_spot_workspace_bytes")
    ws = torch.empty((need.value // 4,), dtype=torch.int32, device=dev)
    L.check(L.lib().av_ctc_spot(ptr(lp), sb, st, ptr(il), ptr(kw), kw.stride(0), ptr(kl), B, T, V, K, Lmax, blank, N, min_score, ptr(hits),
                                ptr(scores), ptr(counts), ptr(ws), ws.numel() * 4, stream()), "av_ctc_spot")
    return hits, scores, counts


# ---------------------------------------------------------------------------------------------------------------
# CTC confidences on the device (csrc/ctc_confidence.hip; the laws and the host path: confidence.py).  Lengths and spans stay on the
# device, nothing in a call synchronises.
# ---------------------------------------------------------------------------------------------------------------
def _conf_codes(who: str, method=None, alpha=None, aggregation=None):
    m = a = None
    if method is not None:
        if method not in L.CONF_METHODS:
            raise ValueError(f"{who}: method must be one of {sorted(L.CONF_METHODS)}, got {method!r}")
        m, alpha = L.CONF_METHODS[method], float(alpha)
        if method == "tsallis":
            if not 0.0 < alpha < float("inf"):                        # NaN fails both comparisons
                raise ValueError(f"{who}: the tsallis alpha must be finite and > 0, got {alpha}")
            if abs(alpha - 1.0) < 1.0 / 64.0:
                raise ValueError(f"{who}: tsallis alpha {alpha} is within 1/64 of 1, where the law loses its digits: use method='entropy', "
                                 "its alpha -> 1 limit")
    if aggregation is not None:
        if aggregation not in L.CONF_AGGREGATIONS:
            raise ValueError(f"{who}: aggregation must be one of {sorted(L.CONF_AGGREGATIONS)}, got {aggregation!r}")
        a = L.CONF_AGGREGATIONS[aggregation]
    return m, alpha, a


def ctc_frame_conf(log_probs: Tensor, lengths=None, method: str = "tsallis", alpha: float = 0.33, batch_first: bool = True) -> Tensor:
    """av_ctc_frame_conf: ``log_probs`` fp32 [B, T, V] (``batch_first=False``: [T, B, V]; any view with a contiguous last dimension is
    taken without a copy), ``lengths`` [B] on either side or None -> confidence fp32 [B, T] on the device, 0 for t >= T_b."""
    m, alpha, _ = _conf_codes("ctc_frame_conf", method, alpha)
    lp, B, T, V, sb, st = _ctc_rows("ctc_frame_conf", log_probs, batch_first, max_T=4096, min_V=2)
    ln = _ctc_lengths("ctc_frame_conf", "lengths", lengths, B, lp.device, optional=True)
    conf = torch.empty((B, T), dtype=torch.float32, device=lp.device)
    L.check(L.lib().av_ctc_frame_conf(ptr(lp), sb, st, ptr(ln), B, T, V, m, alpha, ptr(conf), stream()), "av_ctc_frame_conf")
    return conf


def ctc_span_conf(frame_conf: Tensor, spans: Tensor, lengths=None, aggregation: str = "min") -> Tensor:
    """av_ctc_span_conf: ``frame_conf`` fp32 [B, T] on the GPU, ``spans`` integer [B, L, 2] (first frame, end exclusive) and ``lengths`` [B]
    on either side -> fp32 [B, L] on the device."""
    _, _, a = _conf_codes("ctc_span_conf", aggregation=aggregation)
    if not isinstance(frame_conf, Tensor) or not frame_conf.is_cuda:
        raise RuntimeError("ctc_span_conf (HIP): frame_conf must be on the GPU; there is no CPU fallback (confidence.py runs host tensors)")
    if frame_conf.dim() != 2 or frame_conf.dtype != torch.float32:
        raise TypeError(f"ctc_span_conf: frame_conf must be float32 [B, T], got {frame_conf.dtype} {tuple(frame_conf.shape)}")
    B, T = frame_conf.shape
    if not isinstance(spans, Tensor) or spans.dim() != 3 or spans.shape[0] != B or spans.shape[2] != 2:
        raise ValueError(f"ctc_span_conf: spans must be [B={B}, L, 2], got "
                         f"{tuple(spans.shape) if isinstance(spans, Tensor) else type(spans).__name__}")
    if spans.dtype.is_floating_point or spans.dtype == torch.bool:
        raise TypeError(f"ctc_span_conf: spans must be an integer tensor, got {spans.dtype}")
    if not 1 <= T <= 4096:
        raise ValueError(f"ctc_span_conf: need 1 <= T <= 4096, got T={T}")
    dev = frame_conf.device
    Ls = spans.shape[1]
    cf = frame_conf.detach().contiguous()
    sp = spans.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
    ln = _ctc_lengths("ctc_span_conf", "lengths", lengths, B, dev, optional=True)
    out = torch.empty((B, Ls), dtype=torch.float32, device=dev)
    L.check(L.lib().av_ctc_span_conf(ptr(cf), ptr(sp), ptr(ln), B, T, Ls, a, ptr(out), stream()), "av_ctc_span_conf")
    return out


def ctc_greedy_timed(log_probs: Tensor, blank: int, lengths=None, method: str = "tsallis", alpha: float = 0.33, aggregation: str = "min",
                     batch_first: bool = True):
    """av_ctc_greedy_timed: one read of ``log_probs`` (as for ``ctc_frame_conf``) -> (ids int32 [B, T] padded with -1, lengths int32 [B],
    spans int32 [B, T, 2] padded with -1, token_conf fp32 [B, T], frame_conf fp32 [B, T]) on the device."""
    m, alpha, a = _conf_codes("ctc_greedy_timed", method, alpha, aggregation)
    lp, B, T, V, sb, st = _ctc_rows("ctc_greedy_timed", log_probs, batch_first, max_T=4096, min_V=2)
    blank = int(blank)
    if not 0 <= blank < V:
        raise ValueError(f"ctc_greedy_timed: blank {blank} outside [0, {V})")
    dev = lp.device
    ln = _ctc_lengths("ctc_greedy_timed", "lengths", lengths, B, dev, optional=True)
    ids = torch.empty((B, T), dtype=torch.int32, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    spans = torch.empty((B, T, 2), dtype=torch.int32, device=dev)
    tok = torch.empty((B, T), dtype=torch.float32, device=dev)
    conf = torch.empty((B, T), dtype=torch.float32, device=dev)
    L.check(L.lib().av_ctc_greedy_timed(ptr(lp), sb, st, ptr(ln), B, T, V, blank, m, alpha, a, ptr(ids), ptr(cnt), ptr(spans), ptr(tok),
                                        ptr(conf), stream()), "av_ctc_greedy_timed")
    return ids, cnt, spans, tok, conf


# ---------------------------------------------------------------------------------------------------------------
# Long-form transcription on the device (csrc/ctc_longform.hip; the window plan, the laws and the host path: longform.py).  Cuts and
# lengths stay on the device, nothing in a call synchronises.
# ---------------------------------------------------------------------------------------------------------------
def _longform_rows(who: str, lp, inner: int):
    """A float32 GPU block [S, ..., V] whose ``inner`` middle dimensions collapse into one row axis -> (view with contiguous rows, stride
    between speakers, stride between rows); a view that does not collapse, or whose rows are not contiguous, is copied."""
    if not isinstance(lp, Tensor) or not lp.is_cuda:
        raise RuntimeError(f"{who} (HIP): the log-probs must be on the GPU; there is no CPU fallback (longform.py runs host tensors)")
    if lp.dim() != 2 + inner:
        raise ValueError(f"{who}: the log-probs must have {2 + inner} dimensions, got shape {tuple(lp.shape)}")
    if lp.dtype != torch.float32:
        raise TypeError(f"{who}: the log-probs must be float32, got {lp.dtype}")
    lp = lp.detach()
    if lp.stride(-1) != 1 or lp.stride(-2) < lp.shape[-1] or (inner == 2 and lp.stride(1) != lp.shape[2] * lp.stride(2)) \
            or (lp.shape[0] > 1 and lp.stride(0) < lp.stride(-2) * lp.shape[1:-1].numel()):
        lp = lp.contiguous()
    return lp, lp.stride(0), lp.stride(-2)


def ctc_stitch(window_log_probs: Tensor, src_row: Tensor, src_weight: Tensor, F: int) -> Tensor:
    """av_ctc_stitch: ``window_log_probs`` fp32 [S, nw, W, V] (a view whose window rows are evenly spaced is taken without a copy),
    ``src_row`` int32 [F, 4] and ``src_weight`` fp32 [F, 4] on the device (longform.WindowPlan.table) -> fp32 [S, F, V]."""
    lp, ss, sr = _longform_rows("ctc_stitch", window_log_probs, 2)
    S, nw, W, V = lp.shape
    if V < 2 or nw * W < 1 or F < 1:
        raise ValueError(f"ctc_stitch: need V >= 2 and at least one window row and frame, got shape {tuple(lp.shape)} F={F}")
    if tuple(src_row.shape) != (F, 4) or src_row.dtype != torch.int32 or tuple(src_weight.shape) != (F, 4) or src_weight.dtype != torch.float32:
        raise ValueError(f"ctc_stitch: the source table must be int32 [F={F}, 4] and float32 [F={F}, 4]")
    _req(src_row, "ctc_stitch"); _req(src_weight, "ctc_stitch")
    out = torch.empty((S, F, V), dtype=torch.float32, device=lp.device)
    L.check(L.lib().av_ctc_stitch(ptr(lp), ss, sr, ptr(src_row.contiguous()), ptr(src_weight.contiguous()), S, nw * W, F, V, ptr(out), stream()),
            "av_ctc_stitch")
    return out


def ctc_cut_points(log_probs: Tensor, blank: int, segment: int, radius: int, nb: int) -> Tensor:
    """av_ctc_cut_points: ``log_probs`` fp32 [S, F, V] (any view with contiguous rows) -> cuts int32 [S, nb + 2] on the device; ``nb`` is
    longform.boundaries(F, segment, radius), which the library recomputes."""
    lp, ss, st = _longform_rows("ctc_cut_points", log_probs, 1)
    S, F, V = lp.shape
    cuts = torch.empty((S, nb + 2), dtype=torch.int32, device=lp.device)
    L.check(L.lib().av_ctc_cut_points(ptr(lp), ss, st, S, F, V, int(blank), int(segment), int(radius), ptr(cuts), stream()), "av_ctc_cut_points")
    return cuts


def ctc_segment_gather(log_probs: Tensor, cuts: Tensor, segment: int):
    """av_ctc_segment_gather: ``log_probs`` fp32 [S, F, V], ``cuts`` int32 [S, nb + 2] on the device -> (seg_lp fp32 [S (nb + 1), segment, V],
    seg_len int64 [S (nb + 1)]), both on the device and fully written."""
    lp, ss, st = _longform_rows("ctc_segment_gather", log_probs, 1)
    S, F, V = lp.shape
    _req(cuts, "ctc_segment_gather")
    if cuts.dim() != 2 or cuts.shape[0] != S or cuts.shape[1] < 2 or cuts.dtype != torch.int32:
        raise ValueError(f"ctc_segment_gather: cuts must be int32 [S={S}, nb + 2], got {cuts.dtype} {tuple(cuts.shape)}")
    nb = cuts.shape[1] - 2
    seg = torch.empty((S * (nb + 1), int(segment), V), dtype=torch.float32, device=lp.device)
    ln = torch.empty((S * (nb + 1),), dtype=torch.int64, device=lp.device)
    L.check(L.lib().av_ctc_segment_gather(ptr(lp), ss, st, ptr(cuts.contiguous()), S, F, V, nb, int(segment), ptr(seg), ptr(ln), stream()),
            "av_ctc_segment_gather")
    return seg, ln
