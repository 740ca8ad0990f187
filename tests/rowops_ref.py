"""The measuring stick of the row / glue / loss kernel tests (test_rowops_matrix_gpu.py judges the kernels with it, test_rowops_ref_cpu.py checks
the stick itself): every operation of rowops.hip, audio_front.hip, the head of loss_misc.hip and fusion_misc.hip written in plain PyTorch -
slices, sums, elementwise ops; no torch.nn layer and no call into the library.  As in visual_ref.py each operation exists once,
parameterised by a working type ``wt`` and a rounding function ``rnd``:

    ref64   wt = float64, nothing rounded;
    emul    wt = float32 (the kernels' arithmetic), ``rnd`` rounding to the 16-bit type where a kernel stores one.  Its distance to ref64
            is e_ref, the error a correct kernel of this precision is expected to have.

Two operations are stated with torch itself on CPU float32 tensors, because what they restate IS a float32 law (the index and weight
arithmetic of F.interpolate; a float64 interpolate differs from it by about 4e-5 in the weights): ``mask_downsample_torch`` and
``gather_lerp_torch``.  Their plain restatements (``nearest_index``, ``lerp_table``, ``gather_lerp``) follow lerp_coef / mask_down_kernel
and are checked against the torch path on the CPU.

The shape lists of the GPU matrix live here, each with the dispatcher branch it is for; the dispatch conditions of av_layernorm_fwd /
av_layernorm_bwd_drop / av_colsum / av_cast / av_sum_slices / av_conv0_ln_gelu are restated as ``*_form`` functions so that the CPU file can
assert that the lists reach every branch."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from visual_ref import LIBS, gelu, ident, rounder  # noqa: F401  (LIBS / rounder are re-exported to the two test files)

F32, F64 = torch.float32, torch.float64
LN_EPS, L2_EPS = 1e-5, 1e-12


# -------------------------------------------------------------------------------------------------------------------------------------------
# dispatch conditions, read from the launch code (rowops.hip, audio_front.hip).  ``al``: every pointer the condition looks at is aligned.
# -------------------------------------------------------------------------------------------------------------------------------------------
def _nit(cols):
    return 1 if cols <= 64 else 2 if cols <= 128 else 8 if cols <= 512 else 16 if cols <= 1024 else 32


def ln_fwd_form(cols, al=True):
    """av_layernorm_fwd: ("vec", NV) for cols % 256 == 0, cols <= 2048 and x / y / gamma / beta aligned, else ("generic", NIT)."""
    return ("vec", cols // 256) if cols % 256 == 0 and cols <= 2048 and al else ("generic", _nit(cols))


def ln_bwd_form(cols, al=True):
    """av_layernorm_bwd_drop: the vector form exists for 256, 512, 1024 and 2048 columns only."""
    return ("vec", cols // 256) if cols in (256, 512, 1024, 2048) and al else ("generic", _nit(cols))


COLSUM_ROWS = {"lp_vec": 256, "f32_vec": 128, "scalar": 512}          # rows per block of the three kernels (CSV_ROWS, CSVF_ROWS, CS_ROWS)


def colsum_form(is_lp, cols, ld, al=True):
    if is_lp and cols % 8 == 0 and ld % 8 == 0 and al:
        return "lp_vec"
    if not is_lp and cols % 4 == 0 and ld % 4 == 0 and al:
        return "f32_vec"
    return "scalar"


def cast_form(src_lp, dst_lp, n, al=True):
    return "vec" if not src_lp and dst_lp and n % 4 == 0 and al else "scalar"


def sum_slices_form(n, stride, al=True):
    return "vec" if n % 4 == 0 and stride % 4 == 0 and al else "scalar"


def conv0_form(C, k, out_lp, al=True):
    return "c512" if C == 512 and k == 10 and out_lp and al else ("generic_lp" if out_lp else "generic_f32")


# -------------------------------------------------------------------------------------------------------------------------------------------
# shapes of the GPU matrix
# -------------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm forward, (cols, aligned).  generic: 1 / 64 NIT = 1 (one lane; a full wave), 65 / 128 NIT = 2, 129 / 512-misaligned NIT = 8
# (512 falls back from the vector form because a pointer is off 16 bytes), 800 NIT = 16, 1025 / 2047 NIT = 32.  vector: NV = 1, 3, 5, 6, 7, 8.
LN_FWD = [(1, True), (64, True), (65, True), (128, True), (129, True), (512, False), (800, True), (1025, True), (2047, True),
          (256, True), (768, True), (1280, True), (1536, True), (1792, True), (2048, True)]
LN_FWD_ROWS = [1, 5, 77]                                    # one wave of a block; a second block with one row; 20 blocks, the last with one row
LN_SHIFT = [(256, "x"), (768, "y"), (1280, "gamma"), (1536, "x"), (1792, "y"), (2048, "gamma")]        # per vector width: the operand moved off 16 bytes
LN_OFFSET_COLS = [64, 256]                                  # rows of 1000 + k / 64: generic and vector form (every float32 sum of the row is exact)
# LayerNorm backward: the generic columns of the forward list; vector 256, 512, 1024, 2048; 768 (a vector width of the forward) is generic here.
LN_BWD = [(1, True), (64, True), (65, True), (128, True), (129, True), (512, False), (800, True), (1025, True), (2047, True),
          (256, True), (512, True), (1024, True), (2048, True), (768, True)]
LN_BWD_ROWS = [1, 5, 77, 1030]                              # nblk = 1, 1, 5, 65: rows per block 1, 5 (wave 0 takes two rows), 16 with a last block of 13 / of 6
LN_DROP = [(512, 0.1), (512, 0.5), (800, 0.1), (800, 0.5)]  # in-kernel dropout copy (vector form) and the av_cast_dropout pass (generic form)


def ln_nblk(rows):
    """The block count ops.layernorm_bwd asks for."""
    return max(1, min(512, (rows + 15) // 16))


# av_conv0_ln_gelu.  CONV0_C512: the production kernel (C = 512, k = 10, 16-bit output, 16-byte aligned), L_out: one frame (every prefetch clamped to
# fend - 1 = 0), 3 (waves 0..2 only), 63 / 64 / 65 (one block short of, exactly, one frame beyond frames_per_block = 64), 130 (three blocks, the last
# with two frames).  CONV0_GENERIC: C below one wave (32), one wave (64), C % 64 != 0 (96), the production width off the fast path (512 with
# k != 10 or float32 output) and the limit (1024); k = 10 / 3 / 16 (the limit).
CONV0_C512_LOUT = [1, 3, 63, 64, 65, 130]
CONV0_C, CONV0_KS, CONV0_LOUT = [32, 64, 96, 512, 1024], [(10, 5), (3, 2), (16, 1)], [1, 65]

# log_softmax, (rows, cols): one lane, a full wave, one element into the second sweep, the CTC vocabulary, the limit
LSM_COLS, LSM_ROWS = [1, 64, 65, 800, 2048], [1, 51]
LSM_BWD = [(1, 0), (64, 0), (65, 0), (800, 64), (2040, 64), (2048, 0)]         # (cols, pad_to): 800 -> 832, 2040 -> 2048 (the ldx limit)

# av_colsum: per kernel the column counts (vector f32: one lane, 200, one lane into the second 256-column block; vector 16-bit: one lane,
# 200 (two 128-column blocks, the second ragged), 136 (one lane into the second block); scalar: 1 and 203 (four 64-column blocks))
COLSUM_COLS = {"f32_vec": [4, 200, 260], "lp_vec": [8, 200, 136], "scalar": [1, 203]}


def colsum_rows(kind):
    r = COLSUM_ROWS[kind]
    return [1, r - 1, r + 1, 3 * r + 5]


SUM_SLICES = [(1, 8, 8, True), (2, 1024, 1032, True), (7, 1028, 1028, True), (1, 1027, 1027, True), (2, 1027, 1040, True), (7, 5, 9, True),
              (2, 1024, 1024, False)]                       # (S, n, stride, aligned): vector x {1, 2, 7} slices, scalar by n, by stride, by alignment
CAST_N = [1, 3, 4, 1027]
L2_COLS = [1, 65, 128, 130]
REDUCE_N = [1, 255, 257, 12736]
COMBINE_N = [2, 6, 514]
PERMUTE = [(1, 1, 1), (3, 5, 7), (2, 130, 512)]
MASK_DOWN = [(7, 7), (5, 9), (1, 3), (19200, 59), (64000, 199)]
CLASS_ORDER_N = [1, 1023, 1025, 12736]

# av_fusion_gather_lerp: (name, Ta, Tv, groups, speech-frame counts per item).  The group maxima give the (Tm, Tv) pairs of LERP_PAIRS.
GATHER_LERP = [("equal+empty_item", 9, 5, 1, [5, 3, 0]), ("up", 9, 11, 1, [3, 2]), ("down_to_one", 9, 1, 1, [7, 4]), ("from_one", 9, 7, 1, [1, 0, 1]),
               ("two_groups_eq_up", 9, 3, 2, [3, 1, 2, 0]), ("two_groups_down_eq", 9, 5, 2, [9, 4, 5, 5]),
               ("second_sweep_up", 300, 257, 1, [100, 37]), ("second_sweep_down", 300, 25, 2, [49, 12, 25, 0]), ("second_sweep_equal", 300, 280, 1, [280, 1])]
GATHER_LERP_EMPTY = [("empty_group", 9, 5, 2, [0, 0, 4, 5]), ("empty_batch_of_one", 9, 5, 1, [0]), ("empty_second_sweep", 300, 7, 2, [3, 7, 0, 0])]
GATHER_D = [3, 300]
# (Tm, Tv) whose weights (0, 1/2, 1 or whole-number source positions) make w0 x0 + w1 x1 the same float32 number with and without a fused
# multiply-add: there the restatement equals F.interpolate bit for bit on any data.  LERP_PAIRS_FMA: the weights and indices are equal bit for bit
# (interpolating an identity matrix shows them), the interpolated values differ by the rounding of a fused multiply-add in torch's CPU kernel.
LERP_PAIRS_EXACT = [(1, 7), (7, 1), (5, 5), (49, 25), (2, 3), (9, 5), (3, 5), (7, 3), (5, 9), (25, 49), (11, 3), (280, 280)]
LERP_PAIRS_FMA = [(3, 11), (100, 257)]


def gather_pairs(cases):
    out = set()
    for _, Ta, Tv, groups, counts in cases:
        gs = len(counts) // groups
        out |= {(max(counts[g * gs:(g + 1) * gs]), Tv) for g in range(groups)}
    return out


# -------------------------------------------------------------------------------------------------------------------------------------------
# operands (seeded, drawn on the CPU; values of 16-bit tensors already rounded)
# -------------------------------------------------------------------------------------------------------------------------------------------
def gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))


def randn(shape, g, lp=None, scale=1.0):
    t = torch.randn(shape, generator=g) * scale
    return t if lp is None else t.to(lp).to(F32)


def offset_row(cols):
    """One row of 1000 + k / 64, k in [-64, 64]: a large common offset, and every partial sum of up to 256 values fits 24 bits."""
    return 1000 + torch.randint(-64, 65, (1, cols), generator=gen(cols)).to(F32) / 64


def speech_mask(Ta, counts, g):
    """[B, Ta] int64: ``counts[b]`` positions (random, so also beyond 256 when Ta = 300) hold 1 or 2, the others 0 or 3."""
    m = torch.empty(len(counts), Ta, dtype=torch.int64)
    for b, n in enumerate(counts):
        m[b] = torch.where(torch.rand(Ta, generator=g) < 0.5, 0, 3)
        pos = torch.randperm(Ta, generator=g)[:n]
        m[b, pos] = torch.randint(1, 3, (n,), generator=g)
    return m


# -------------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# -------------------------------------------------------------------------------------------------------------------------------------------
def layernorm(x, gamma, beta, act=False, wt=F64, rnd=ident, eps=LN_EPS):
    """x [rows, cols] -> y = rnd(act((x - mean) rstd gamma + beta)), mean, rstd (biased variance about the mean, two passes)."""
    x = x.to(wt)
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + torch.tensor(eps, dtype=F32).to(wt))       # the kernel's eps is a float
    y = d * rstd * gamma.to(wt) + beta.to(wt)
    return rnd(gelu(y) if act else y), mean[:, 0], rstd[:, 0]


def layernorm_bwd(x, dy, gamma, mean, rstd, dres=None, wt=F64):
    """-> dx (+ dres), dgamma, dbeta and the magnitude sums of the two parameter gradients (for gate_sum).
    g = dy gamma; dx = rstd (g - mean(g) - xhat mean(g xhat)); dgamma = sum_rows dy xhat; dbeta = sum_rows dy."""
    x, dy, gamma = x.to(wt), dy.to(wt), gamma.to(wt)
    xh = (x - mean.to(wt)[:, None]) * rstd.to(wt)[:, None]
    g = dy * gamma
    dx = rstd.to(wt)[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + dres.to(wt)
    return dx, (dy * xh).sum(0), dy.sum(0), (dy * xh).abs().sum(0), dy.abs().sum(0)


# -------------------------------------------------------------------------------------------------------------------------------------------
# log_softmax
# -------------------------------------------------------------------------------------------------------------------------------------------
def log_softmax(x, wt=F64):
    x = x.to(wt)
    mx = x.max(1, keepdim=True).values
    return x - (mx + torch.log(torch.exp(x - mx).sum(1, keepdim=True)))


def log_softmax_bwd(y, dy, ldx=None, wt=F64, rnd=ident):
    """dx = dy - exp(y) sum(dy), zero-padded to ``ldx`` columns."""
    y, dy = y.to(wt), dy.to(wt)
    dx = dy - torch.exp(y) * dy.sum(1, keepdim=True)
    if ldx is not None and ldx > dx.shape[1]:
        dx = torch.cat([dx, torch.zeros(dx.shape[0], ldx - dx.shape[1], dtype=wt, device=dx.device)], 1)
    return rnd(dx)


# -------------------------------------------------------------------------------------------------------------------------------------------
# feature-encoder layer 0
# -------------------------------------------------------------------------------------------------------------------------------------------
def conv0_ln_gelu(wav, w, bias, gamma, beta, L_out, stride, wt=F64, rnd=ident, eps=LN_EPS):
    """wav [B, T_in], w [C, k] -> [B, L_out, C]: a[f, c] = bias[c] + sum_j w[c, j] wav[f stride + j]; LayerNorm over c; erf GELU."""
    C, k = w.shape
    wav, w = wav.to(wt), w.to(wt)
    a = torch.zeros(wav.shape[0], L_out, C, dtype=wt, device=wav.device)
    if bias is not None:
        a = a + bias.to(wt)
    for j in range(k):
        a = a + wav[:, j:j + (L_out - 1) * stride + 1:stride, None] * w[:, j]
    y, _, _ = layernorm(a.reshape(-1, C), gamma, beta, True, wt, rnd, eps)
    return y.view(wav.shape[0], L_out, C)


# -------------------------------------------------------------------------------------------------------------------------------------------
# loss side
# -------------------------------------------------------------------------------------------------------------------------------------------
def l2norm(x, wt=F64, eps=L2_EPS):
    """-> y = x / max(|x|, eps), |x| per row."""
    x = x.to(wt)
    n = torch.sqrt((x * x).sum(1))
    return x * (1.0 / n.clamp_min(float(torch.tensor(eps, dtype=F32))))[:, None], n


def l2norm_bwd(y, dy, nrm, wt=F64, eps=L2_EPS):
    """dx = (dy - y (y . dy)) / max(n, eps)."""
    y, dy = y.to(wt), dy.to(wt)
    return (dy - y * (y * dy).sum(1, keepdim=True)) * (1.0 / nrm.to(wt).clamp_min(float(torch.tensor(eps, dtype=F32))))[:, None]


def lse_rows(s, wt=F64):
    """-> log-sum-exp and sum of every row."""
    s = s.to(wt)
    mx = s.max(1).values
    return mx + torch.log(torch.exp(s - mx[:, None]).sum(1)), s.sum(1)


def lse_merge(a, b):
    """The running merge of two chunk results."""
    hi = torch.maximum(a, b)
    return hi + torch.log(torch.exp(a - hi) + torch.exp(b - hi))


def contrastive_dsim(s, lse, coef, total_cols, ld=None, wt=F64, rnd=ident):
    """coef (softmax - 1 / total_cols) with the given row LSE, zero-padded to ``ld`` columns."""
    s = s.to(wt)
    u = (torch.tensor(1.0, dtype=F32) / torch.tensor(float(total_cols), dtype=F32)).to(wt) if wt == F32 else 1.0 / total_cols
    d = torch.tensor(coef, dtype=F32).to(wt) * (torch.exp(s - lse.to(wt)[:, None]) - u)
    if ld is not None and ld > d.shape[1]:
        d = torch.cat([d, torch.zeros(d.shape[0], ld - d.shape[1], dtype=wt, device=d.device)], 1)
    return rnd(d)


def loss_combine(nll, w, c1, c2, half_lambda, wt=F64):
    """-> [total, l1, l2] and the magnitude sums: total = sum_i nll_i w_i + half_lambda (c1 + c2); l1 / l2 = twice the first / second half of
    the weighted sum (the comment of loss_combine_kernel)."""
    v = nll.to(wt) * w.to(wt)
    hn = v.numel() // 2
    a, b = v[:hn].sum(), v[hn:].sum()
    cs = [c.to(wt)[0] for c in (c1, c2) if c is not None]
    c = sum(cs) if cs else torch.zeros((), dtype=wt, device=v.device)
    hl = torch.tensor(half_lambda, dtype=F32).to(wt)
    aa, ab = v[:hn].abs().sum(), v[hn:].abs().sum()
    cabs = sum(x.abs() for x in cs) if cs else c
    return torch.stack([a + b + hl * c, 2 * a, 2 * b]), torch.stack([aa + ab + hl.abs() * cabs, 2 * aa, 2 * ab])


# -------------------------------------------------------------------------------------------------------------------------------------------
# glue
# -------------------------------------------------------------------------------------------------------------------------------------------
def class_order(mask):
    """Indices of mask == 1 ascending, then of 2, then of values <= 0, then of the rest."""
    rank = torch.where(mask == 1, 0, torch.where(mask == 2, 1, torch.where(mask <= 0, 2, 3)))
    idx = torch.arange(mask.numel(), device=mask.device)
    return torch.cat([idx[rank == r] for r in range(4)])


def gather(src, idx):
    return src[idx]


def scatter(src, idx, out, alpha, accumulate, wt=F64):
    o = out.to(wt).clone() if accumulate else torch.zeros_like(out, dtype=wt)
    base = o[idx] if accumulate else 0.0
    o[idx] = torch.tensor(alpha, dtype=F32).to(wt) * src.to(wt) + base
    return o                                                 # rows no index names: ``out`` (accumulate) / not judged (the kernel leaves them)


def permute(x):
    """[B, T, D] -> [T, B, D]."""
    return x.transpose(0, 1).contiguous()


def nearest_index(Tin, Tout):
    """mask_down_kernel and the nearest half of gather_lerp: floor(i * (float) Tin / (float) Tout) in float32, clamped to Tin - 1."""
    scale = np.float32(Tin) / np.float32(Tout)
    j = np.floor(np.arange(Tout, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(j, Tin - 1))


def mask_downsample(mask, Tout):
    return mask[:, nearest_index(mask.shape[1], Tout).to(mask.device)]


def mask_downsample_torch(mask, Tout):
    return F.interpolate(mask[:, None].to(F32), size=Tout, mode="nearest")[:, 0].long()


def lerp_table(Tm, Tv):
    """lerp_coef of fusion_misc.hip in float32 for i = 0 .. Tv - 1 -> i0, i1 (int64), lam (float32).  Tm == Tv: the identity."""
    i = np.arange(Tv, dtype=np.float32)
    if Tm == Tv:
        k = torch.arange(Tv)
        return k, k.clone(), torch.zeros(Tv)
    scale = np.float32(Tm - 1) / np.float32(Tv - 1) if Tv > 1 else np.float32(0)
    src = scale * i
    i0 = np.minimum(src.astype(np.int64), Tm - 1)
    lam = src - i0.astype(np.float32)
    i1 = i0 + (i0 < Tm - 1)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(lam.astype(np.float32))


def _groups(mask, groups):
    B = mask.shape[0]
    gs = B // groups
    for g in range(groups):
        sl = slice(g * gs, (g + 1) * gs)
        keep = (mask[sl] == 1) | (mask[sl] == 2)
        yield sl, keep, int(keep.sum(1).max())


def gather_lerp_torch(feat, mask, Tv, groups, dout=None):
    """The float32 statement with torch itself (CPU tensors): per group the speech frames (mask 1 / 2) of every item, padded to the group's
    maximum Tm, resampled to Tv frames with F.interpolate(linear, align_corners=True) and the mask with F.interpolate(nearest) - both skipped
    when Tm == Tv.  -> out [B, Tv, D], mask_out [B, Tv], lens [B] = count(mask_out != 0) (+ dfeat through autograd when ``dout`` is given).
    A group without a speech frame is treated by hand (F.interpolate rejects a zero-length input): zeros, length 0, zero gradient."""
    pad = torch.nn.utils.rnn.pad_sequence
    feat = feat.detach().clone().requires_grad_(dout is not None)
    outs, mouts = [], []
    for sl, keep, Tm in _groups(mask, groups):
        f, m = feat[sl], mask[sl]
        if Tm == 0:
            outs.append(torch.zeros(f.shape[0], Tv, f.shape[2]) + 0.0 * f.sum())
            mouts.append(torch.zeros(f.shape[0], Tv, dtype=torch.int64))
            continue
        a = pad([f[i][keep[i]] for i in range(f.shape[0])], batch_first=True)
        mm = pad([m[i][keep[i]] for i in range(f.shape[0])], batch_first=True)
        if Tm != Tv:
            a = F.interpolate(a.transpose(1, 2), size=Tv, mode="linear", align_corners=True).transpose(1, 2)
            mm = F.interpolate(mm[:, None].to(F32), size=Tv, mode="nearest")[:, 0].long()
        outs.append(a)
        mouts.append(mm)
    out, mout = torch.cat(outs), torch.cat(mouts)
    res = (out.detach(), mout, (mout != 0).sum(1))
    if dout is None:
        return res
    out.backward(dout)
    return res + (feat.grad,)


def gather_lerp(feat, mask, Tv, groups, dout=None):
    """The same operation on the restated float32 law (lerp_table / nearest_index), multiply, multiply, add per element.  With ``dout``:
    + dfeat, the transposed operation (every source frame sums w(i, j) dout[i]).  Tm == 0: zeros."""
    B, Ta, D = feat.shape
    out, mout = torch.zeros(B, Tv, D), torch.zeros(B, Tv, dtype=torch.int64)
    dfeat = None if dout is None else torch.zeros(B, Ta, D, dtype=dout.dtype)
    for sl, keep, Tm in _groups(mask, groups):
        if Tm == 0:
            continue
        i0, i1, lam = lerp_table(Tm, Tv)
        lam = lam.to(feat.dtype)
        jn = torch.arange(Tv) if Tm == Tv else nearest_index(Tm, Tv)
        for b in range(sl.start, sl.stop):
            pos = torch.nonzero(keep[b - sl.start])[:, 0]
            n = pos.numel()
            x = torch.zeros(Tm, D, dtype=feat.dtype)
            x[:n] = feat[b, pos]
            out[b] = ((1 - lam)[:, None] * x[i0] + lam[:, None] * x[i1]).to(out.dtype)
            mc = torch.zeros(Tm, dtype=torch.int64)
            mc[:n] = mask[b, pos]
            mout[b] = mc[jn]
            if dout is not None:
                dx = torch.zeros(Tm, D, dtype=dout.dtype)
                dx.index_add_(0, i0, (1 - lam.to(dout.dtype))[:, None] * dout[b])
                dx.index_add_(0, i1, lam.to(dout.dtype)[:, None] * dout[b])
                dfeat[b, pos] = dx[:n]
    res = (out, mout, (mout != 0).sum(1))
    return res if dout is None else res + (dfeat,)


def lerp_weights(Tm, Tv):
    """[Tv, Tm] float32: the weight of source frame j in output frame i under lerp_table."""
    i0, i1, lam = lerp_table(Tm, Tv)
    W = torch.zeros(Tv, Tm)
    r = torch.arange(Tv)
    W[r, i0] += 1 - lam
    W[r, i1] += lam
    return W


# -------------------------------------------------------------------------------------------------------------------------------------------
# dropout multiplier from the library's uniforms
# -------------------------------------------------------------------------------------------------------------------------------------------
def drop_mult(u, p):
    """u >= ceil(65536 p) / 65536 ? 65536 / (65536 - ceil(65536 p)) : 0, the product 65536 p taken in float32 as the kernel does."""
    thr = math.ceil(float(np.float32(p) * np.float32(65536.0)))
    keep = (torch.tensor(65536.0, dtype=F32) / torch.tensor(65536.0 - thr, dtype=F32)).to(u.device)
    return torch.where(u >= thr / 65536.0, keep, torch.zeros((), dtype=F32, device=u.device))


# values that sit on a rounding tie of bfloat16 (8 significant bits) and of float16 (11 bits), both ways of "to even", overflow to the largest
# exponent, and both infinities: what a cast has to get right beyond random numbers
CAST_SPECIALS = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -8), float("inf"), float("-inf"), 0.0, -0.0, 3.0e38, 65519.0,
                 65520.0, -70000.0, 2.0 ** -14, 1.0, -2.5]


def cast_values(n, g):
    v = torch.randn(n, generator=g) * 3
    k = min(n, len(CAST_SPECIALS))
    v[:k] = torch.tensor(CAST_SPECIALS[:k])
    return v
