"""The measuring stick of the lip-encoder tests (test_visual_matrix_gpu.py judges the kernels with it, test_visual_ref_cpu.py checks the stick
itself): every operation of the visual front end, the ResNet glue and the implicit-GEMM convolution forms, written in plain PyTorch - slices, matmul, elementwise ops; no torch.nn layer and no call
into the library.  Each operation exists once, parameterised by a working type ``wt`` and a rounding function ``rnd``:

    ref64   wt = float64, nothing rounded;
    emul    operands already rounded to the 16-bit type ``lp``, arithmetic in float32 (products of 16-bit operands are exact in float32, sums are
            float32: an MFMA's arithmetic), the result rounded to ``lp`` where a kernel must round: each convolution output and each stored
            activation.  Its distance to ref64 is e_ref, the error a correct kernel of this precision is expected to have.

Layouts are the library's: activations channel-last, a convolution output is [rows, Cout] with rows = (image, y, x) ("frame-major") or, in
position-major order with blocks of NF images, row ((q // NF) * P + pos) * NF + q % NF for pixel ``pos`` of image ``q`` of a P-pixel map (the rule
of the gemm_fast.hip comment).  BatchNorm partials are [nblk][2][C]: per block of rows the column sums and sums of squares.

Gates (the rule of attention_ref.py; its constants are imported, not copied):
    judge       16-bit outputs: max|ours - ref64| <= FACTOR x e_ref; least-squares scale factor of every output of >= SCALE_MIN_NUMEL elements
                within SCALE_TOL[lp]; everything finite (callers start output buffers as NaN);
    gate_sum    float32 sums (BatchNorm partials, average pool, a float32 convolution output): FACTOR x max(e_ref, 64 EPS32 sum|v|), sum|v| =
                the float64 sum of the magnitudes of the summands - the constant lse_gate uses;
    gate_f32    float32 results derived from double accumulators (av_bn_finalize): FACTOR x max(e_ref, EPS32 |ref64|), one ulp of the result;
    float32 operands keep the project's float32 gate (test_kernels_gpu._tol).
The shape lists of that GPU matrix live here (which dispatcher branch each shape reaches is written next to it), so that the CPU file can
run the emulation over the same shapes."""
import math

import torch

from attention_ref import EPS32, FACTOR, SCALE_MIN_NUMEL, SCALE_TOL, max_err, scale_dev

LIBS = {"bf16": torch.bfloat16, "fp16": torch.float16}
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def rounder(lp):
    return lambda t: t.to(lp).to(torch.float32)


def ident(t):
    return t


# -------------------------------------------------------------------------------------------------------------------------------------------
# shapes of the GPU matrix.  Which branch a shape reaches is READ FROM THE LAUNCH CODE, not observed in a trace: the grid caps from
# av_bn_prelu_minmax (frontend3d.hip: blocks > 2048), vec_grid / bn_act_cap (visual.hip: 2048, and 512 unless AVAMD_EW_BLOCKS is set), the
# vector-form conditions from the `vec` expressions of av_bn_act / av_bn_prelu_maxpool (16-bit, C % 8 == 0, 256 % (C / 8) == 0, x / out / res
# 16-byte aligned), the kernel choice of av_gemm from av_gemm_fast_try and "no table" from tap_seq ((1 << sh) != Cin / 64) in gemm_fast.hip.
# -------------------------------------------------------------------------------------------------------------------------------------------
# front end (av_conv3d_front, av_conv3d_front_pool), (B, T, H, W): one 8 x 16 tile and strip with T = 1 (four of five temporal taps are padding);
# the smallest T above 1; three workgroups (XCD remap with total % 8 != 0, q = 0) and two row tiles (carry row); three strips (halo column) with
# one row tile; non-square with carry row and halo column; 26 workgroups (remap with q > 0 and rem > 0); H > W with six row tiles
FRONT = [(1, 1, 16, 32), (1, 2, 16, 32), (3, 1, 32, 32), (1, 5, 16, 96), (2, 7, 48, 64), (13, 1, 16, 64), (1, 3, 96, 32)]
# (N, H, W, C, kind): kind "lp" = 16-bit, "off" = 16-bit with the input 8 bytes off 16-byte alignment, "f32" = float32
MAXPOOL = [(2, 5, 7, 64, "lp"), (1, 1, 1, 64, "lp"), (3, 8, 16, 64, "lp"), (2, 5, 7, 24, "lp"), (2, 6, 6, 64, "off"), (2, 5, 7, 64, "f32")]
MINMAX_SWEEP = 2048 * 256 * 4 * 8                          # elements of one sweep of the capped av_bn_prelu_minmax grid (2048 blocks x 256 x 4 x 8)
MINMAX_N = [64, 64 * 1000, MINMAX_SWEEP + (2048 * 256 + 8 * 37) * 8]       # the last: one more stride + 296 chunks, so u = 1 is clamped for most threads
BN_C, BN_NBLK = [24, 64, 100, 512], [1, 63, 64, 65, 1000]
BNACT_SWEEP = 512 * 256 * 4 * 8                            # one sweep of the 512-block av_bn_act grid
# (name, C, n elements, kind): kind "lp", "res_off" (16-bit, residual 8 bytes off 16-byte alignment -> scalar form), "f32"
BNACT_FORMS = [("vecC64", 64, 64 * 300, "lp"), ("vecC512", 512, 512 * 40, "lp"), ("small", 64, 64 * 8, "lp"),
               ("sweep", 64, BNACT_SWEEP + (512 * 256 + 8 * 21) * 8, "lp"), ("scalarC24", 24, 24 * 101, "lp"), ("scalar_res_off", 64, 64 * 37, "res_off"),
               ("float32", 64, 64 * 50, "f32")]
BNACT_RES = ["none", "identity", "bn"]
AVGPOOL = [(5, 9, 512, 0), (3, 1, 64, 0), (512, 9, 512, 256), (8, 6, 64, 4), (256, 1, 64, 256)]             # (N, HW, C, FB)


# implicit-GEMM convolution forms (av_gemm, a_mode = A_CONV2D): Cin -> Cout, k, stride, input H x W, frames, cPM, cNF.  CONV_PM: the 128 x 128 kernel
# reading frame-major and writing position-major; two image blocks with corner positions keeping 4 of 9 taps; one tap, non-square; the narrow kernel
# (N <= 64); M = 4608, N = 256, K = 1152 on the 8-phase kernel with skipped K-tiles; M = 4096 with two column tiles; position-major in, frame-major out;
# Cin / 64 no power of two (tap_seq has no table).  CONV_SMALL_NF: cNF below the row tile (256-row and 128-row kernels): tiles span positions, every
# tap stays.  CONV_FM: frame-major non-square at stride 2, a channel slice (cCtot = 192, cCin = 64, cCoff = 64), Cin = 192.
def conv_case(name, cin, cout, k, s, H, W, frames, pm=0, nf=0, ctot=None, coff=0):
    pad = k // 2
    return dict(name=name, cin=cin, cout=cout, k=k, s=s, H=H, W=W, n=frames, pm=pm, nf=nf if pm else 0, ctot=ctot or cin, coff=coff, pad=pad,
                Ho=(H + 2 * pad - k) // s + 1, Wo=(W + 2 * pad - k) // s + 1)


CONV_PM = [conv_case("l2_fm_to_pm", 64, 128, 3, 2, 6, 6, 256, 2, 256), conv_case("l2_two_blocks", 128, 128, 3, 1, 3, 3, 512, 3, 256),
           conv_case("l2_1x1_nonsquare", 64, 128, 1, 2, 6, 4, 256, 2, 256), conv_case("narrow", 64, 64, 3, 1, 3, 3, 256, 3, 256),
           conv_case("l3_8phase", 128, 256, 3, 2, 6, 6, 512, 3, 256), conv_case("l4_two_col_tiles", 256, 512, 3, 2, 3, 3, 1024, 3, 256),
           conv_case("pm_to_fm", 128, 128, 3, 1, 3, 2, 256, 1, 256), conv_case("cin192_no_table", 192, 128, 3, 1, 3, 3, 256, 3, 256)]
CONV_SMALL_NF = [conv_case("l3_8phase_nf128", 128, 256, 3, 2, 6, 6, 512, 3, 128), conv_case("l2_nf64", 128, 128, 3, 1, 3, 3, 256, 3, 64)]
CONV_FM = [conv_case("nonsquare_12x6", 64, 128, 3, 2, 12, 6, 5), conv_case("channel_slice", 64, 64, 3, 1, 5, 7, 3, ctot=192, coff=64),
           conv_case("cin192", 192, 128, 3, 1, 5, 7, 3)]
CONV_ALL = CONV_PM + CONV_SMALL_NF + CONV_FM
POSCONV_KP, POSCONV_BT, POSCONV_G, POSCONV_CG = [32, 33, 128], [(2, 49), (3, 200), (1, 1)], 2, 64


# -------------------------------------------------------------------------------------------------------------------------------------------
# operands: drawn on the CPU from a seeded generator (so the CPU file sees what the GPU file sees), values of 16-bit tensors already rounded
# -------------------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def randn(shape, g, lp=None, scale=1.0):
    t = torch.randn(shape, generator=g) * scale
    return t if lp is None else t.to(lp).to(torch.float32)


def exact_x(shape, prime=13, thr=1):
    """{0, 1} from the flat index modulo a prime that divides no stride of ``shape``: differs along every axis."""
    n = math.prod(shape)
    return ((torch.arange(n) % prime) < thr).to(torch.float32).view(shape)


def exact_w(shape):
    """{-1, 0, 1}: ((flat index mod 11) mod 3) - 1."""
    n = math.prod(shape)
    return (((torch.arange(n) % 11) % 3) - 1).to(torch.float32).view(shape)


def front_operands(shape, lp, exact=False):
    """x float32 [B, T, H, W] (the kernel rounds it), w [64, 5, 7, 7] with values of type lp."""
    B, T, H, W = shape
    if exact:
        return exact_x(shape, 13, 5), exact_w((64, 5, 7, 7))
    g = _gen(1000 * B + 100 * T + H + W)
    return randn(shape, g), randn((64, 5, 7, 7), g, lp, 245 ** -0.5)


def conv_operands(c, lp, exact=False):
    """x [n, H, W, Ctot], w [Cout, k, k, Cin] (tap-major K = the library's weight layout), both with values of type lp."""
    xs, ws = (c["n"], c["H"], c["W"], c["ctot"]), (c["cout"], c["k"], c["k"], c["cin"])
    if exact:                                                # the densest x (of 13 residues) that keeps sum|x||w| near 200: 7 of 11 weights are non-zero
        K = c["k"] * c["k"] * c["cin"]
        return exact_x(xs, 13, max(1, min(6, 200 * 13 * 11 // (7 * K)))), exact_w(ws)
    g = _gen(sum(ord(ch) for ch in c["name"]))
    return randn(xs, g, lp), randn(ws, g, lp, (c["k"] * c["k"] * c["cin"]) ** -0.5)


def posconv_operands(kp, B, T, lp, exact=False):
    """x [B, T, Hd] and w [G, Cg, kp, Cg] with values of type lp, bias [Hd] and residual [B, T, Hd] float32."""
    G, Cg = POSCONV_G, POSCONV_CG
    Hd = G * Cg
    if exact:
        bias = ((torch.arange(Hd) % 5) - 2).to(torch.float32)
        res = ((torch.arange(B * T * Hd) % 7) - 3).to(torch.float32).view(B, T, Hd)
        return exact_x((B, T, Hd), 29, 1), exact_w((G, Cg, kp, Cg)), bias, res
    g = _gen(10000 * kp + 100 * B + T)
    return randn((B, T, Hd), g, lp), randn((G, Cg, kp, Cg), g, lp, (kp * Cg) ** -0.5), randn((Hd,), g, None, 0.1), randn((B, T, Hd), g)


def bn_params(C, g):
    """scale / shift / slope [C] holding each of: a positive, a negative and a zero scale; a slope in (0, 1), a negative slope, a slope above 1."""
    scale = torch.randn(C, generator=g) * 0.7 + 0.2
    shift = torch.randn(C, generator=g) * 0.5
    slope = torch.rand(C, generator=g) * 0.5 + 0.1
    scale[0], scale[1], scale[2], scale[3 % C] = 0.8, -0.6, 0.0, -1.3
    slope[0], slope[1], slope[2], slope[3 % C], slope[4 % C], slope[5 % C] = 0.25, -0.5, 1.7, 1.7, -0.5, 0.25
    scale[4 % C], scale[5 % C] = 0.9, -0.9                 # channels 0..5: every sign of the scale under every kind of slope
    return scale, shift, slope


# -------------------------------------------------------------------------------------------------------------------------------------------
# pixel orders
# -------------------------------------------------------------------------------------------------------------------------------------------
def pos_major_index(n_img, P, NF):
    """Position-major row of every frame-major row q * P + pos: ((q // NF) * P + pos) * NF + q % NF."""
    q = torch.arange(n_img)[:, None]
    pos = torch.arange(P)[None, :]
    return (((q // NF) * P + pos) * NF + q % NF).reshape(-1)


def to_pos_major(rows, n_img, P, NF):
    out = torch.empty_like(rows)
    out[pos_major_index(n_img, P, NF).to(rows.device)] = rows
    return out


def from_pos_major(rows, n_img, P, NF):
    return rows[pos_major_index(n_img, P, NF).to(rows.device)]


# -------------------------------------------------------------------------------------------------------------------------------------------
# front end
# -------------------------------------------------------------------------------------------------------------------------------------------
def conv3d_front(x, w, wt, rnd=ident):
    """Conv3d(1 -> 64, k (5, 7, 7), stride (1, 2, 2), pad (2, 3, 3)): x [B, T, H, W], w [64, 5, 7, 7] -> [B T Ho Wo, 64] channel-last."""
    B, T, H, W = x.shape
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    xp = torch.zeros(B, T + 4, H + 6, W + 6, dtype=wt, device=x.device)
    xp[:, 2:2 + T, 3:3 + H, 3:3 + W] = x.to(wt)
    w = w.to(wt)
    out = torch.zeros(B, T, Ho, Wo, 64, dtype=wt, device=x.device)
    for kt in range(5):
        for ky in range(7):
            for kx in range(7):
                out += xp[:, kt:kt + T, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2].unsqueeze(-1) * w[:, kt, ky, kx]
    return rnd(out.reshape(-1, 64))


def window_maxmin(y):
    """Maximum and minimum over the 3 x 3 / stride 2 / pad 1 windows of a channel-last map y [N, H, W, C] -> 2 x [N, Hp, Wp, C]."""
    N, H, W, C = y.shape
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = []
    for fill, op in ((float("-inf"), torch.maximum), (float("inf"), torch.minimum)):
        yp = torch.full((N, 2 * Hp + 1, 2 * Wp + 1, C), fill, dtype=y.dtype, device=y.device)
        yp[:, 1:1 + H, 1:1 + W] = y                                                       # window rows 2 p - 1 .. 2 p + 1 = padded rows 2 p .. 2 p + 2
        m = None
        for dy in range(3):
            for dx in range(3):
                v = yp[:, dy:dy + 2 * Hp:2, dx:dx + 2 * Wp:2]
                m = v if m is None else op(m, v)
        out.append(m.contiguous())
    return out


def partial_sums(y, wt):
    """Column sums and sums of squares [2, C] of a convolution output y [rows, C] (what the summed BatchNorm partials must equal)."""
    y = y.to(wt)
    return torch.stack([y.sum(0), (y * y).sum(0)])


def bn_from_partials(part, count, gamma, beta, rmean, rvar, training, momentum=BN_MOMENTUM, eps=BN_EPS, f32=False):
    """BatchNorm scale / shift [C] from [nblk][2][C] partials and a count -> (scale, shift, running_mean, running_var).  Train mode: batch mean,
    BIASED variance for scale / shift, the UNBIASED variance (count = 1: the biased one) with momentum for the running statistics (None stays
    None).  Eval mode reads the running statistics and leaves them alone.  The partials are summed in float64 in both forms (the kernel keeps
    double accumulators); ``f32``: the emulation - mean and 1 / sqrt(var + eps) rounded to float32, every later operation in float32."""
    wt = torch.float32 if f32 else torch.float64
    gamma, beta = gamma.to(wt), beta.to(wt)
    if not training:
        sc = gamma / torch.sqrt(rvar.to(wt) + torch.tensor(eps, dtype=torch.float32).to(wt))          # the kernel's eps is a float
        return sc, beta - rmean.to(wt) * sc, rmean, rvar
    s = part.double().sum(0)
    mean = s[0] / count
    var = (s[1] / count - mean * mean).clamp_min(0.0)
    sc = gamma * (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))).to(wt)
    sh = beta - mean.to(wt) * sc
    if rmean is None:
        return sc, sh, None, None
    unb = var * count / (count - 1.0) if count > 1 else var
    m = torch.tensor(momentum, dtype=torch.float32).to(wt)                               # the kernel's momentum is a float
    one_m = (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(momentum, dtype=torch.float32)).to(wt) if f32 else 1.0 - m
    return sc, sh, one_m * rmean.to(wt) + m * mean.to(wt), one_m * rvar.to(wt) + m * unb.to(wt)


# -------------------------------------------------------------------------------------------------------------------------------------------
# glue
# -------------------------------------------------------------------------------------------------------------------------------------------
def _prelu(v, slope):
    return v if slope is None else torch.where(v >= 0, v, v * slope)


def bn_act(x, scale, shift, res, rscale, rshift, slope, wt, rnd=ident):
    """out = prelu(x scale + shift + residual), residual = res rscale + rshift (its own BatchNorm), res (rscale None) or nothing; x [..., C]."""
    v = x.to(wt) * scale.to(wt) + shift.to(wt)
    if res is not None:
        v = v + (res.to(wt) * rscale.to(wt) + rshift.to(wt) if rscale is not None else res.to(wt))
    return rnd(_prelu(v, None if slope is None else slope.to(wt)))


def bn_prelu_maxpool(x, scale, shift, slope, wt, rnd=ident):
    """x [N, H, W, C] -> [N, Hp, Wp, C]: BatchNorm-apply, PReLU, 3 x 3 / stride 2 / pad 1 maximum (rounding commutes with the maximum)."""
    return rnd(window_maxmin(_prelu(x.to(wt) * scale.to(wt) + shift.to(wt), slope.to(wt)))[0])


def bn_prelu_minmax(ymax, ymin, scale, shift, slope, wt, rnd=ident):
    a = _prelu(ymax.to(wt) * scale.to(wt) + shift.to(wt), slope.to(wt))
    b = _prelu(ymin.to(wt) * scale.to(wt) + shift.to(wt), slope.to(wt))
    return rnd(torch.maximum(a, b))


def avgpool(x, wt):
    """x [N, HW, C] frame-major -> [N, C]."""
    return x.to(wt).sum(1) / x.shape[1]


# -------------------------------------------------------------------------------------------------------------------------------------------
# convolutions
# -------------------------------------------------------------------------------------------------------------------------------------------
def conv2d_nhwc(x, w, stride, pad, wt, rnd=ident, coff=0):
    """x [N, H, W, Ctot], w [Cout, kh, kw, Cin] on channels [coff, coff + Cin) -> [N Ho Wo, Cout], rows (image, y, x)."""
    N, H, W, _ = x.shape
    Cout, kh, kw, Cin = w.shape
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    xp = torch.zeros(N, H + 2 * pad, W + 2 * pad, Cin, dtype=wt, device=x.device)
    xp[:, pad:pad + H, pad:pad + W] = x[..., coff:coff + Cin].to(wt)
    w = w.to(wt)
    out = torch.zeros(N, Ho, Wo, Cout, dtype=wt, device=x.device)
    for ky in range(kh):
        for kx in range(kw):
            out += xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] @ w[:, ky, kx].t()
    return rnd(out.reshape(-1, Cout))


def conv_case_ref(c, x, w, wt, rnd=ident):
    return conv2d_nhwc(x, w, c["s"], c["pad"], wt, rnd, c["coff"])


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * (0.5 ** 0.5)))


def pos_conv(x, w, bias, res, act, wt, pre=False):
    """The grouped 1-D positional convolution: x [B, T, Hd], w [G, Cg, kp, Cg] ([group][c_out][tap][c_in]), padding = kp // 2, the last output
    dropped for even kp; then + bias, GELU (``act``), + residual -> [B, T, Hd].  ``pre``: the convolution alone."""
    B, T, Hd = x.shape
    G, Cg, kp, _ = w.shape
    pad = kp // 2
    xp = torch.zeros(B, T + 2 * pad, Hd, dtype=wt, device=x.device)
    xp[:, pad:pad + T] = x.to(wt)
    w = w.to(wt)
    out = torch.zeros(B, T, Hd, dtype=wt, device=x.device)
    for g in range(G):
        gs = slice(g * Cg, (g + 1) * Cg)
        for k in range(kp):
            out[:, :, gs] += xp[:, k:k + T, gs] @ w[g, :, k].t()
    if pre:
        return out
    v = out + bias.to(wt)
    if act:
        v = gelu(v)
    return v + res.to(wt)


# -------------------------------------------------------------------------------------------------------------------------------------------
# ref64 + emulation of one case, as dicts (what both test files judge)
# -------------------------------------------------------------------------------------------------------------------------------------------
def _sums_refs(y64, yem_unrounded, yabs):
    """Summed BatchNorm partials [2, C]: ref64, emulation (float32 sums of the un-rounded float32 convolution) and sum|v|.  The summands of a
    column sum are all the products x w of its rows, so sum|v| = the column sums of conv(|x|, |w|); a sum of squares sums y^2 with
    |y| <= conv(|x|, |w|), so its sum|v| is the column sum of conv(|x|, |w|)^2."""
    return partial_sums(y64, torch.float64), partial_sums(yem_unrounded, torch.float32), partial_sums(yabs, torch.float64)


def front_refs(x, w, lp):
    """-> (r64, em, sums): r64 / em = dict(y [N, Ho, Wo, 64], ymax, ymin [N, Hp, Wp, 64]); the pooled reference pools the ROUNDED reference conv
    (what both forms of the kernel pool); sums = (ref64, emulation, sum|v|) of the summed partials of the un-rounded conv."""
    B, T, H, W = x.shape
    rn = rounder(lp)
    sh = (B * T, H // 2, W // 2, 64)
    y64 = conv3d_front(x, w, torch.float64)
    yem_raw = conv3d_front(rn(x), w, torch.float32)
    r64 = dict(y=y64.view(sh))
    em = dict(y=rn(yem_raw).view(sh))
    r64["ymax"], r64["ymin"] = window_maxmin(y64.to(lp).double().view(sh))
    em["ymax"], em["ymin"] = window_maxmin(em["y"])
    return r64, em, _sums_refs(y64, yem_raw, conv3d_front(x.abs(), w.abs(), torch.float64))


def conv_refs(c, x, w, lp):
    """-> (y64, y_em, sums) of one CONV_* case, rows frame-major."""
    rn = rounder(lp)
    y64 = conv_case_ref(c, x, w, torch.float64)
    yem_raw = conv_case_ref(c, x, w, torch.float32)
    return y64, rn(yem_raw), _sums_refs(y64, yem_raw, conv_case_ref(c, x.abs(), w.abs(), torch.float64))


def posconv_refs(x, w, bias, res, act):
    """-> (ref64, emulation, sum|v|) of the float32 output: a float32 sum of the products, the bias and the residual (GELU has slope <= 1.13 and
    g(0) = 0, so it does not enlarge the bound), hence sum|v| = conv(|x|, |w|) + |bias| + |res|."""
    r64 = pos_conv(x, w, bias, res, act, torch.float64)
    em = pos_conv(x, w, bias, res, act, torch.float32)
    return r64, em, pos_conv(x.abs(), w.abs(), bias.abs(), res.abs(), False, torch.float64)


# -------------------------------------------------------------------------------------------------------------------------------------------
# gates
# -------------------------------------------------------------------------------------------------------------------------------------------
def judge(lp, ours, r64, em):
    """The 16-bit rule on dicts name -> tensor.  Returns (rows, failures): rows = (name, err, e_ref, ratio, scale deviation or None)."""
    rows, bad = [], []
    for n, x in ours.items():
        if not bool(torch.isfinite(x.float()).all()):
            bad.append(f"{n}: non-finite values")
            continue
        err, e_ref = max_err(x, r64[n]), max_err(em[n], r64[n])
        ratio = err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))
        sd = scale_dev(x, r64[n]) if x.numel() >= SCALE_MIN_NUMEL else None
        rows.append((n, err, e_ref, ratio, sd))
        if not err <= FACTOR * e_ref:
            bad.append(f"{n}: err {err:.3e} > {FACTOR:g} x e_ref {e_ref:.3e} (ratio {ratio:.2f})")
        if sd is not None and not sd <= SCALE_TOL[lp]:
            bad.append(f"{n}: scale factor off by {sd:.3e} > {SCALE_TOL[lp]:.3e}")
    return rows, bad


def _floor_gate(name, ours, r64, em, floor, what):
    """|ours - ref64| <= FACTOR x max(e_ref, floor) elementwise (e_ref = max|emul - ref64|, one number; floor a tensor)."""
    if not bool(torch.isfinite(ours).all()):
        return (name, float("nan"), 0.0, float("inf"), None), [f"{name}: non-finite values"]
    e_ref = max_err(em, r64)
    gate = FACTOR * torch.maximum(floor.double(), torch.tensor(e_ref, dtype=torch.float64, device=floor.device))
    d = (ours.double() - r64.double()).abs()
    ratio = float((d / gate).max()) * FACTOR
    row = (name, float(d.max()), e_ref, ratio, None)
    return row, ([] if bool((d <= gate).all()) else [f"{name}: err {float(d.max()):.3e} beyond {FACTOR:g} x max(e_ref {e_ref:.3e}, {what}) (ratio {ratio:.2f})"])


def gate_sum(name, ours, r64, em, sum_abs):
    """A float32 sum: the floor is 64 EPS32 sum|v|, ``sum_abs`` = the float64 sum of the magnitudes of the summands (same shape as ours)."""
    return _floor_gate(name, ours, r64, em, 64.0 * EPS32 * sum_abs.double(), "64 eps32 sum|v|")


def gate_f32(name, ours, r64, em):
    """A plain float32 result: the floor is EPS32 |ref64|, one ulp of the result."""
    return _floor_gate(name, ours, r64, em, EPS32 * r64.double().abs(), "eps32 |ref|")


def fmt(rows):
    out = []
    for n, err, e_ref, ratio, sd in rows:
        s = f"{n} {err:.2e}/{e_ref:.2e}={ratio:.2f}"
        if sd is not None:
            s += f" |s-1|={sd:.1e}"
        out.append(s)
    return "  ".join(out)
