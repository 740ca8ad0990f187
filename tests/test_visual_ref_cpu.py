"""Checks of the measuring stick itself (visual_ref.py), on the CPU: the float64 references equal the torch.nn statements of the reference
model (model/encoder.py:57-75, hf:326-379), the pixel-order maps are the bijection the gemm_fast.hip comment states, the min/max identity
the fused front end rests on is exact, and the same-precision emulation is a usable yardstick on every 16-bit shape listed for the GPU matrix
(e_ref > 0, its own scale factor inside the gate).  No library call, no GPU."""
import pytest
import torch
import torch.nn as nn

import visual_ref as V

F64 = torch.float64
LPS = list(V.LIBS.items())


def _close(a, b, tol=1e-12):
    torch.testing.assert_close(a.double(), b.double(), rtol=tol, atol=tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# agreement with torch.nn in float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count_one", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 16, 32), (1, 1, 16, 32)])
def test_front_end_equals_conv3d_batchnorm_prelu_maxpool(shape, count_one):
    """Conv3d -> BatchNorm3d -> PReLU -> MaxPool3d, train mode (scale / shift from [nblk][2][C] partials, running statistics with the unbiased
    variance) and eval mode (from the running statistics), through both routes: BN + PReLU + max pool of the conv output, and the window
    max / min of the raw conv output finished by bn_prelu_minmax.  momentum = 0.125 is exact in float32, as the kernel's float argument."""
    B, T, H, W = shape
    g = torch.Generator().manual_seed(7)
    x = torch.randn(shape, generator=g, dtype=F64)
    eps = float(torch.tensor(V.BN_EPS, dtype=torch.float32))
    net = nn.Sequential(nn.Conv3d(1, 64, (5, 7, 7), (1, 2, 2), (2, 3, 3), bias=False), nn.BatchNorm3d(64, eps=eps, momentum=0.125), nn.PReLU(64),
                        nn.MaxPool3d((1, 3, 3), (1, 2, 2), (0, 1, 1))).double()
    with torch.no_grad():
        net[1].weight.copy_(torch.randn(64, generator=g)); net[1].bias.copy_(torch.randn(64, generator=g))
        net[1].running_mean.copy_(torch.randn(64, generator=g)); net[1].running_var.copy_(torch.rand(64, generator=g) + 0.5)
        net[2].weight.copy_(torch.randn(64, generator=g))                       # negative slopes and slopes above 1 included
        net[1].weight[:3] = torch.tensor([0.0, -1.0, 2.0], dtype=F64)
    w = net[0].weight.detach()[:, 0]
    y = V.conv3d_front(x, w, F64)
    _close(y.view(B, T, H // 2, W // 2, 64), net[0](x[:, None]).detach().permute(0, 2, 3, 4, 1))
    rm0, rv0 = net[1].running_mean.clone(), net[1].running_var.clone()
    nblk = 3
    part = torch.stack([V.partial_sums(c, F64) for c in y.chunk(nblk)])
    N, Ho, Wo = B * T, H // 2, W // 2
    for training in (True, False):
        net.train(training)
        with torch.no_grad():
            want = net(x[:, None]).permute(0, 2, 3, 4, 1).reshape(N, (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1, 64)
        rm_in = net[1].running_mean.clone() if not training else rm0
        rv_in = net[1].running_var.clone() if not training else rv0
        sc, sh, rm, rv = V.bn_from_partials(part, y.shape[0], net[1].weight.detach(), net[1].bias.detach(), rm_in, rv_in, training, momentum=0.125)
        slope = net[2].weight.detach()
        _close(V.bn_prelu_maxpool(y.view(N, Ho, Wo, 64), sc, sh, slope, F64), want, 1e-10)
        mx, mn = V.window_maxmin(y.view(N, Ho, Wo, 64))
        _close(V.bn_prelu_minmax(mx, mn, sc, sh, slope, F64), want, 1e-10)
        _close(rm, net[1].running_mean, 1e-12); _close(rv, net[1].running_var, 1e-12)
        if not training:
            assert torch.equal(rm, rm_in) and torch.equal(rv, rv_in)
    if count_one:                                                # count = 1 keeps the biased variance (zero) for the running statistics, no division by zero
        row = y[:1]
        part1 = V.partial_sums(row, F64)[None]
        sc, sh, rm, rv = V.bn_from_partials(part1, 1, torch.ones(64, dtype=F64), torch.zeros(64, dtype=F64), rm0, rv0, True, momentum=0.125)
        _close(rv, 0.875 * rv0); _close(rm, 0.875 * rm0 + 0.125 * row[0])
        _close(sc, torch.full((64,), eps ** -0.5, dtype=F64), 1e-9)
        assert V.bn_from_partials(part1, 1, torch.ones(64), torch.zeros(64), None, None, True)[2:] == (None, None)


@pytest.mark.parametrize("c", V.CONV_FM + [V.conv_case("pm_geometry", 64, 128, 1, 2, 6, 4, 3), V.conv_case("s2_even", 64, 64, 3, 2, 6, 6, 2)], ids=lambda c: c["name"])
def test_conv2d_equals_nn_conv2d(c):
    x, w = V.conv_operands(c, torch.bfloat16)
    ref = nn.functional.conv2d(x[..., c["coff"]:c["coff"] + c["cin"]].permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), None, c["s"], c["pad"])
    assert ref.shape[2:] == (c["Ho"], c["Wo"])
    _close(V.conv_case_ref(c, x, w, F64), ref.permute(0, 2, 3, 1).reshape(-1, c["cout"]))


@pytest.mark.parametrize("B,T", V.POSCONV_BT + [(2, 7)])
@pytest.mark.parametrize("kp", [4, 5] + V.POSCONV_KP)
def test_positional_conv_equals_grouped_conv1d_with_the_dropped_sample(kp, B, T):
    x, w, bias, res = V.posconv_operands(kp, B, T, torch.bfloat16)
    G, Cg = V.POSCONV_G, V.POSCONV_CG
    conv = nn.Conv1d(G * Cg, G * Cg, kp, padding=kp // 2, groups=G).double()
    with torch.no_grad():
        conv.weight.copy_(w.permute(0, 1, 3, 2).reshape(G * Cg, Cg, kp)); conv.bias.copy_(bias)          # [G, co, k, ci] -> [G co, ci, k]
        y = conv(x.double().transpose(1, 2))
        y = y[:, :, :-1] if kp % 2 == 0 else y                                                           # hf:336-343 Wav2Vec2SamePadLayer
        want = nn.functional.gelu(y).transpose(1, 2) + res.double()
    _close(V.pos_conv(x, w, bias, res, True, F64), want)
    _close(V.pos_conv(x, w, bias, res, False, F64), y.transpose(1, 2) + res.double())


@pytest.mark.parametrize("N,HW,C,FB", V.AVGPOOL)
def test_average_pool_equals_adaptive_avg_pool(N, HW, C, FB):
    x = torch.randn(N, HW, C, dtype=F64, generator=torch.Generator().manual_seed(HW))
    want = nn.AdaptiveAvgPool2d(1)(x.permute(0, 2, 1).reshape(N, C, HW, 1)).reshape(N, C)
    _close(V.avgpool(x, F64), want)
    if FB:                                                       # through the position-major order and back
        pm = V.to_pos_major(x.reshape(N * HW, C), N, HW, FB)
        _close(V.avgpool(V.from_pos_major(pm, N, HW, FB).view(N, HW, C), F64), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# pixel orders
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 6, 9])
@pytest.mark.parametrize("NF", [1, 64, 256])
def test_position_major_map_is_the_stated_bijection(NF, P):
    n_img = 2 * NF
    idx = V.pos_major_index(n_img, P, NF)
    assert sorted(idx.tolist()) == list(range(n_img * P))
    for q in (0, 1, NF - 1, NF, n_img - 1):
        for pos in (0, P - 1, P // 2):
            assert int(idx[q * P + pos]) == ((q // NF) * P + pos) * NF + q % NF
    rows = torch.arange(n_img * P * 3, dtype=torch.float32).view(n_img * P, 3)
    pm = V.to_pos_major(rows, n_img, P, NF)
    assert torch.equal(V.from_pos_major(pm, n_img, P, NF), rows)
    assert torch.equal(V.to_pos_major(V.from_pos_major(rows, n_img, P, NF), n_img, P, NF), rows)
    q, pos = n_img - 1, P - 1
    assert torch.equal(pm[((q // NF) * P + pos) * NF + q % NF], rows[q * P + pos])
    if NF == 1:
        assert torch.equal(pm, rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# the identity behind the fused front end
# ---------------------------------------------------------------------------------------------------------------------------------
def test_window_maximum_of_prelu_bn_needs_only_the_window_extremes():
    """max over a window of prelu(bn(x)) = max(prelu(bn(max x)), prelu(bn(min x))), exactly, for every sign of the scale and every slope
    (negative, inside (0, 1), above 1) and a zero scale: bn + prelu is monotone or V-shaped per channel."""
    g = torch.Generator().manual_seed(3)
    y = torch.randn(3, 9, 11, 64, generator=g, dtype=F64)
    scale, shift, slope = (t.double() for t in V.bn_params(64, g))
    assert (scale > 0).any() and (scale < 0).any() and (scale == 0).any()
    assert ((slope > 0) & (slope < 1)).any() and (slope < 0).any() and (slope > 1).any()
    for sc_sign in (1.0, -1.0):
        mx, mn = V.window_maxmin(y)
        a = V.bn_prelu_maxpool(y, sc_sign * scale, shift, slope, F64)
        b = V.bn_prelu_minmax(mx, mn, sc_sign * scale, shift, slope, F64)
        assert torch.equal(a, b)
    # and the window extremes themselves against a direct loop over one image
    mx, mn = V.window_maxmin(y[:1])
    for py in range(5):
        for px in range(6):
            win = y[0, max(0, 2 * py - 1):2 * py + 2, max(0, 2 * px - 1):2 * px + 2].reshape(-1, 64)
            assert torch.equal(mx[0, py, px], win.max(0).values) and torch.equal(mn[0, py, px], win.min(0).values)


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation as a yardstick: e_ref > 0 and its own scale factor inside the gate, on every 16-bit shape of the GPU matrix
# ---------------------------------------------------------------------------------------------------------------------------------
def _yardstick(lp, r64, em):
    for n in r64:
        e_ref = V.max_err(em[n], r64[n])
        assert e_ref > 0, f"{n}: the emulation equals the reference (nothing to measure against)"
        if r64[n].numel() >= V.SCALE_MIN_NUMEL:
            sd = V.scale_dev(em[n], r64[n])
            assert sd <= V.SCALE_TOL[lp], f"{n}: the emulation's own scale factor is off by {sd:.2e}"


@pytest.mark.parametrize("libname,lp", LPS)
@pytest.mark.parametrize("shape", V.FRONT)
def test_emulation_front_end(shape, libname, lp):
    x, w = V.front_operands(shape, lp)
    r64, em, (s64, sem, sabs) = V.front_refs(x, w, lp)
    _yardstick(lp, r64, em)
    assert bool((sabs >= s64.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("libname,lp", LPS)
@pytest.mark.parametrize("c", V.CONV_ALL, ids=lambda c: c["name"])
def test_emulation_convolutions(c, libname, lp):
    x, w = V.conv_operands(c, lp)
    y64, yem, (s64, sem, sabs) = V.conv_refs(c, x, w, lp)
    _yardstick(lp, dict(y=y64), dict(y=yem))
    assert bool((sabs >= s64.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("libname,lp", LPS)
def test_emulation_glue(libname, lp):
    rn = V.rounder(lp)
    for N, H, W, C, kind in V.MAXPOOL:
        if kind == "f32":
            continue
        g = torch.Generator().manual_seed(N * H * W * C)
        x = V.randn((N, H, W, C), g, lp)
        sc, sh, sl = V.bn_params(C, g)
        _yardstick(lp, dict(o=V.bn_prelu_maxpool(x, sc, sh, sl, F64)), dict(o=V.bn_prelu_maxpool(x, sc, sh, sl, torch.float32, rn)))
    for n in V.MINMAX_N:
        g = torch.Generator().manual_seed(n)
        a, b = V.randn((n // 64, 64), g, lp), V.randn((n // 64, 64), g, lp)
        mx, mn = torch.maximum(a, b), torch.minimum(a, b)
        sc, sh, sl = V.bn_params(64, g)
        _yardstick(lp, dict(o=V.bn_prelu_minmax(mx, mn, sc, sh, sl, F64)), dict(o=V.bn_prelu_minmax(mx, mn, sc, sh, sl, torch.float32, rn)))
    for name, C, n, kind in V.BNACT_FORMS:
        if kind == "f32":
            continue
        g = torch.Generator().manual_seed(n)
        x, res = V.randn((n // C, C), g, lp), V.randn((n // C, C), g, lp)
        sc, sh, sl = V.bn_params(C, g)
        rs, rb, _ = V.bn_params(C, g)
        for args in ((None, None, None, sl), (res, None, None, None), (res, rs, rb, sl)):
            _yardstick(lp, dict(o=V.bn_act(x, sc, sh, *args, F64)), dict(o=V.bn_act(x, sc, sh, *args, torch.float32, rn)))


@pytest.mark.parametrize("libname,lp", LPS)
def test_emulation_float32_outputs(libname, lp):
    """The outputs that the floor gates judge (positional conv and average pool: gate_sum; av_bn_finalize: gate_f32): the emulation differs from
    the reference (e_ref > 0), passes its own gate, and the floor is of the size of e_ref or above - it is the floor that decides there."""
    for kp in V.POSCONV_KP:
        for B, T in V.POSCONV_BT:
            x, w, bias, res = V.posconv_operands(kp, B, T, lp)
            r64, em, sabs = V.posconv_refs(x, w, bias, res, True)
            row, bad = V.gate_sum("out", em, r64, em, sabs)
            assert not bad and row[2] > 0 and bool((sabs >= r64.abs() * (1 - 1e-12)).all()), (kp, B, T, row)
            assert 64 * V.EPS32 * float(sabs.max()) >= row[2], "the floor does not cover the float32 summation error"
    for N, HW, C, FB in V.AVGPOOL:
        x = V.randn((N, HW, C), torch.Generator().manual_seed(N + HW + C), lp)
        r64, em, sabs = V.avgpool(x, F64), V.avgpool(x, torch.float32), x.double().abs().sum(1) / HW
        row, bad = V.gate_sum("out", em, r64, em, sabs)
        assert not bad and (row[2] > 0 or HW == 1) and 64 * V.EPS32 * float(sabs.max()) >= row[2], (N, HW, C, row)
    for C in V.BN_C:
        for nblk in V.BN_NBLK:
            g = torch.Generator().manual_seed(100 * C + nblk)
            y = torch.randn(nblk, 8, C, generator=g) * 1.5 + torch.randn(C, generator=g)
            part = torch.stack([y.sum(1), (y * y).sum(1)], 1)
            a = (torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5)
            for training in (True, False):
                want, em = V.bn_from_partials(part, 8 * nblk, *a, training), V.bn_from_partials(part, 8 * nblk, *a, training, f32=True)
                for name, w64, e32 in zip(("scale", "shift", "running_mean", "running_var")[:4 if training else 2], want, em):
                    assert e32.dtype == torch.float32 and w64.dtype == F64
                    row, bad = V.gate_f32(name, e32, w64, e32)
                    assert not bad and row[2] > 0, (C, nblk, training, name, row)
                    assert row[2] <= 64 * V.EPS32 * float(w64.abs().max() + 1), "the float32 emulation of av_bn_finalize is not at float32 precision"


# ---------------------------------------------------------------------------------------------------------------------------------
# the gates themselves: a good input passes, one just over the bound fails, a NaN fails, the floor is applied per element
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("libname,lp", LPS)
def test_judge_passes_the_emulation_and_fails_just_over_the_bound(libname, lp):
    g = torch.Generator().manual_seed(5)
    r64 = torch.randn(64, 128, generator=g, dtype=F64)
    em = r64.to(lp).double()
    e_ref = V.max_err(em, r64)
    rows, bad = V.judge(lp, dict(y=em), dict(y=r64), dict(y=em))
    assert not bad and rows[0][0] == "y" and rows[0][2] == e_ref and rows[0][3] == 1.0 and rows[0][4] is not None
    assert "y " in V.fmt(rows) and "|s-1|" in V.fmt(rows)
    for factor, fails in ((0.999 * V.FACTOR, False), (1.001 * V.FACTOR, True)):          # one element moved to factor x e_ref
        ours = r64.clone(); ours[3, 5] += factor * e_ref
        rows, bad = V.judge(lp, dict(y=ours), dict(y=r64), dict(y=em))
        assert bool(bad) == fails and abs(rows[0][3] - factor) < 1e-9, (factor, bad)
        assert not fails or "err" in bad[0]
    ours = em.clone(); ours[0, 0] = float("nan")
    assert "non-finite" in V.judge(lp, dict(y=ours), dict(y=r64), dict(y=em))[1][0]
    ours = em.clone(); ours[1, 1] = float("inf")
    assert "non-finite" in V.judge(lp, dict(y=ours), dict(y=r64), dict(y=em))[1][0]
    # a wrong overall factor that no single element shows: only the scale check sees it; below SCALE_MIN_NUMEL elements it does not apply
    ours = em * (1 + 2.5 * V.SCALE_TOL[lp])
    rows, bad = V.judge(lp, dict(y=ours), dict(y=r64), dict(y=em))
    assert any("scale factor" in b for b in bad)
    small = slice(0, V.SCALE_MIN_NUMEL // 128 - 1)
    assert V.judge(lp, dict(y=em[small]), dict(y=r64[small]), dict(y=em[small]))[0][0][4] is None
    # e_ref = 0 (an exactly representable reference): equal passes with ratio 0, anything else fails with ratio inf
    ex = torch.arange(8, dtype=F64)
    assert V.judge(lp, dict(y=ex), dict(y=ex), dict(y=ex)) == ([("y", 0.0, 0.0, 0.0, None)], [])
    rows, bad = V.judge(lp, dict(y=ex + 1e-9), dict(y=ex), dict(y=ex))
    assert bad and rows[0][3] == float("inf")


def test_floor_gates_apply_the_floor_per_element():
    r64 = torch.tensor([1.0, 1000.0, -3.0, 0.0], dtype=F64)
    em = r64.clone(); em[0] += 1e-6                                                   # e_ref = 1e-6
    sabs = torch.tensor([2.0, 2000.0, 1e6, 0.0], dtype=F64)
    floor = 64 * V.EPS32 * sabs                                                       # 1.5e-5, 1.5e-2, 7.6, 0
    ok = r64 + 0.99 * V.FACTOR * floor.clamp_min(1e-6)                                # every element just inside its own bound
    row, bad = V.gate_sum("s", ok, r64, em, sabs)
    assert not bad and row[0] == "s" and 0.9 * V.FACTOR < row[3] <= V.FACTOR, (row, bad)
    for i in range(4):                                                                # each element just over ITS bound fails, whatever the others allow
        ours = r64.clone()
        ours[i] += 1.01 * V.FACTOR * max(float(floor[i]), 1e-6)
        row, bad = V.gate_sum("s", ours, r64, em, sabs)
        assert bad and row[3] > V.FACTOR, (i, row)
        ours[i] = r64[i] + 0.99 * V.FACTOR * max(float(floor[i]), 1e-6)
        assert not V.gate_sum("s", ours, r64, em, sabs)[1], i
    ours = r64.clone(); ours[1] += 4.5 * floor[0]                                     # inside element 1's own floor although far over element 0's
    assert not V.gate_sum("s", ours, r64, em, sabs)[1]
    ours = r64.clone(); ours[2] = float("nan")
    assert "non-finite" in V.gate_sum("s", ours, r64, em, sabs)[1][0]
    # gate_f32: the floor is one ulp of each result
    for i, v in enumerate(r64.tolist()):
        bound = V.FACTOR * max(V.EPS32 * abs(v), 1e-6)
        for f, fails in ((0.99, False), (1.01, True)):
            ours = r64.clone(); ours[i] += f * bound
            assert bool(V.gate_f32("r", ours, r64, em)[1]) == fails, (i, f)
    ours = r64.clone(); ours[3] = float("inf")
    assert "non-finite" in V.gate_f32("r", ours, r64, em)[1][0]


# ---------------------------------------------------------------------------------------------------------------------------------
# exact-integer operands: every partial sum of every output is an integer of magnitude <= 256, exact in bfloat16 and float16 in any order
# ---------------------------------------------------------------------------------------------------------------------------------
def _is_exact(y64, yabs):
    assert float(yabs.max()) <= 256.0, f"sum of magnitudes {float(yabs.max())} > 256"
    assert bool((y64 == y64.round()).all()) and float(y64.abs().max()) >= 3.0 and len(torch.unique(y64)) >= 5, "pattern too tame"
    for lp in V.LIBS.values():
        assert torch.equal(y64.to(lp).double(), y64)


@pytest.mark.parametrize("shape", V.FRONT)
def test_exact_integer_front_end(shape):
    x, w = V.front_operands(shape, torch.bfloat16, exact=True)
    assert set(x.unique().tolist()) <= {0.0, 1.0} and set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
    _is_exact(V.conv3d_front(x, w, F64), V.conv3d_front(x.abs(), w.abs(), F64))
    for ax in range(4):                                          # the patterns differ along every axis: a swapped axis or flipped tap changes the result
        if x.shape[ax] > 1:
            assert not torch.equal(x, x.flip(ax))
    for ax in range(4):
        assert not torch.equal(w, w.flip(ax))
    assert not torch.equal(w.transpose(2, 3), w)


@pytest.mark.parametrize("c", V.CONV_ALL, ids=lambda c: c["name"])
def test_exact_integer_convolutions(c):
    x, w = V.conv_operands(c, torch.bfloat16, exact=True)
    _is_exact(V.conv_case_ref(c, x, w, F64), V.conv_case_ref(c, x.abs(), w.abs(), F64))
    if c["k"] > 1:
        assert not torch.equal(w.transpose(1, 2), w) and not torch.equal(w.flip(1), w) and not torch.equal(w.flip(2), w)
    if c["H"] == c["W"]:
        assert not torch.equal(x.transpose(1, 2), x)


@pytest.mark.parametrize("B,T", V.POSCONV_BT)
@pytest.mark.parametrize("kp", V.POSCONV_KP)
def test_exact_integer_positional_conv(kp, B, T):
    x, w, bias, res = V.posconv_operands(kp, B, T, torch.bfloat16, exact=True)
    y = V.pos_conv(x, w, bias, res, False, F64)
    yabs = V.pos_conv(x.abs(), w.abs(), bias.abs(), res.abs(), False, F64)
    assert float(yabs.max()) <= 256.0 and bool((y == y.round()).all())
    if T > 1:
        assert float(V.pos_conv(x, w, bias, res, False, F64, pre=True).abs().max()) >= 3.0
