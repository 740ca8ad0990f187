"""CPU: the host path of augment.py (lips, noise, plan) against the independent restatement tests/augment_ref.py, the settings'
validation, the statistics of the draws, and the argument checks of av_augment_lips / av_augment_noise (no kernel is launched)."""
import math

import numpy as np
import pytest
import torch

import augment_ref as R
from conftest import pkg

ENV = ("AVAMD_AUG_SHIFT", "AVAMD_AUG_FLIP", "AVAMD_AUG_TMASK", "AVAMD_AUG_TMASK_EVERY", "AVAMD_AUG_SNR", "AVAMD_AUG_SEED")


def A(**kw):
    return pkg("augment").Augment(**kw)


def clips(B, T, H, W, seed=0):
    return np.random.default_rng(seed).random((B, T, H, W), dtype=np.float32)


@pytest.mark.parametrize("step", [0, 1, 7])
@pytest.mark.parametrize("speaker", [1, 2])
def test_host_lips_and_plan_equal_the_reference(step, speaker):
    B, T, H, W, lengths = 3, 60, 12, 10, (60, 37, 1)
    a = A(max_shift=3, flip=0.5, mask_max=25, mask_every=25, seed=11)
    x = clips(B, T, H, W)
    want = R.lips(x, lengths, 11, step, speaker, 3, 32768, 25, 25)
    got = a.lips(torch.from_numpy(x), torch.tensor(lengths), step, speaker)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    dx, dy, flip, tsrc = a.plan(B, T, lengths, step, speaker)
    for b in range(B):
        rdx, rdy, rflip, rts = R.lip_plan(b, T, lengths[b], 11, step, speaker, 3, 32768, 25, 25)
        assert (int(dx[b]), int(dy[b]), bool(flip[b]), tsrc[b].tolist()) == (rdx, rdy, rflip, rts)
    assert not got.numpy()[1, 37:].any() and not got.numpy()[2, 1:].any()              # padded frames are zeros


def test_host_lips_frame_size_channel_axis_and_copy():
    x = clips(2, 5, 96, 96, seed=3)
    a = A(max_shift=4, flip=0.5, mask_max=2, mask_every=3, seed=5)
    want = R.lips(x, None, 5, 2, 1, 4, 32768, 2, 3)
    assert np.array_equal(a.lips(torch.from_numpy(x), None, 2, 1).numpy(), want)
    x5 = torch.from_numpy(x)[:, None]                                                  # [B, 1, T, H, W]: the trainer's view
    got = a.lips(x5, None, 2, 1)
    assert got.shape == x5.shape and np.array_equal(got.numpy()[:, 0], want)
    assert np.array_equal(A().lips(torch.from_numpy(x), None, 9, 2).numpy(), x)        # everything off: a copy


def test_host_noise_equals_the_reference():
    B, N, lengths = 4, 1003, (1003, 640, 1, 0)
    x = np.random.default_rng(1).standard_normal((B, N)).astype(np.float32) * np.float32(0.1)
    x[1] = 0                                                                           # a silent row among the non-empty ones
    x[3, :] = 0
    a = A(snr=(5, 25), seed=9)
    for step in (0, 3):
        y, sg = a.noise(torch.from_numpy(x), torch.tensor(lengths), step)
        wy, wsg = R.noise(x, lengths, 9, step, 5, 25)
        assert np.array_equal(sg.numpy(), wsg) and np.array_equal(y.numpy(), wy)
        assert sg[0] > 0 and sg[2] > 0 and sg[1] == 0 and sg[3] == 0
        assert np.array_equal(y.numpy()[1], x[1]) and np.array_equal(y.numpy()[2, 1:], x[2, 1:]) and not np.array_equal(y.numpy()[0], x[0])
        assert a.last_power[0] == R.power(x[0], 1003)


def test_settings_validation(monkeypatch):
    Aug = pkg("augment").Augment
    for bad in (dict(mask_max=26, mask_every=25), dict(flip=-0.1), dict(flip=1.5), dict(flip=float("nan")), dict(snr=(25, 5)),
                dict(max_shift=-1), dict(mask_every=0)):
        with pytest.raises(ValueError):
            Aug(**bad)
    x = torch.zeros((1, 2, 6, 8))
    with pytest.raises(ValueError):
        Aug(max_shift=6).lips(x, None, 0, 1)                                           # max_shift >= min(H, W)
    assert Aug(max_shift=5).lips(x, None, 0, 1).shape == x.shape
    with pytest.raises(ValueError):
        Aug(mask_max=1, mask_every=2).plan(1, 253, None, 0, 1)                         # 127 segments
    assert Aug(mask_max=1, mask_every=2).plan(1, 252, None, 0, 1)[3].shape == (1, 252)
    with pytest.raises(ValueError):
        Aug(max_shift=1).plan(1, 4, None, 1 << 24, 1)                                  # the step no longer fits the index packing
    with pytest.raises(ValueError):
        Aug(max_shift=1).plan(1, 4, None, 0, 3)                                        # speakers are 1 and 2
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert Aug.from_env() is None
    monkeypatch.setenv("AVAMD_AUG_SEED", "5")
    monkeypatch.setenv("AVAMD_AUG_TMASK_EVERY", "10")
    assert Aug.from_env() is None                                                      # a seed and a segment length switch nothing on
    monkeypatch.setenv("AVAMD_AUG_SHIFT", "4"); monkeypatch.setenv("AVAMD_AUG_FLIP", "0.5"); monkeypatch.setenv("AVAMD_AUG_TMASK", "10")
    monkeypatch.setenv("AVAMD_AUG_SNR", "5,25")
    a = Aug.from_env()
    assert (a.max_shift, a.flip, a.mask_max, a.mask_every, a.snr, a.seed) == (4, 0.5, 10, 10, (5.0, 25.0), 5)
    a.step = 12
    b = Aug(max_shift=1)
    b.load_state_dict(a.state_dict())
    assert (b.step, b.seed) == (12, 5) and all(type(v) is int for v in a.state_dict().values())


def test_stream_ids_are_unused_elsewhere():
    """The four augmentation streams differ from every dropout stream: S_FEATPROJ, S_POS and the per-layer ones (layer * 8 + 0 .. 3)."""
    aug = pkg("augment"); w2 = pkg("model.w2v2")
    ids = [aug.S_AUG_LIP1, aug.S_AUG_LIP2, aug.S_AUG_SNR, aug.S_AUG_NOISE]
    assert len(set(ids + [w2.S_FEATPROJ, w2.S_POS])) == 6
    assert all(i >= 1 << 16 for i in ids)                                              # the layer streams are below 8 * layers
    assert [R.S_LIP[1], R.S_LIP[2], R.S_SNR, R.S_NOISE] == ids


def test_plan_statistics_and_independence():
    a = A(max_shift=3, flip=0.5, mask_max=10, mask_every=25, seed=1)
    T = 60
    lengths = np.array([60, 37, 1, 25] * 1024)
    dx, dy, flip, tsrc = a.plan(4096, T, lengths, 5, 1)
    assert sorted(set(dx.tolist())) == list(range(-3, 4)) and sorted(set(dy.tolist())) == list(range(-3, 4))
    assert abs(flip.mean() - 0.5) <= 5 * math.sqrt(0.25 / 4096)
    t = np.arange(T)[None, :]
    valid = t < lengths[:, None]
    assert (tsrc[valid] <= np.broadcast_to(t, tsrc.shape)[valid]).all() and (tsrc[valid] >= 0).all()
    assert (tsrc < lengths[:, None]).all() and (tsrc[~valid] == -1).all()
    assert (tsrc[valid] != np.broadcast_to(t, tsrc.shape)[valid]).any()                 # some frame is frozen
    # clip b alone (as clip b of a batch that holds nothing else) gives the same plan: it does not depend on the batch's other clips
    for b in (0, 1, 777):
        want = R.lip_plan(b, T, int(lengths[b]), 1, 5, 1, 3, 32768, 10, 25)
        assert (int(dx[b]), int(dy[b]), bool(flip[b]), tsrc[b].tolist()) == want
        pad = np.full(b + 1, T); pad[b] = lengths[b]
        one = a.plan(b + 1, T, pad, 5, 1)
        assert (one[0][b], one[1][b], one[2][b], one[3][b].tolist()) == (dx[b], dy[b], flip[b], tsrc[b].tolist())
    # other speaker, next step: other plans
    full = np.full(64, T)
    p0 = a.plan(64, T, full, 5, 1)
    for other in (a.plan(64, T, full, 5, 2), a.plan(64, T, full, 6, 1)):
        assert any(not np.array_equal(u, v) for u, v in zip(p0[:2], other[:2])) and not np.array_equal(p0[3], other[3])


def test_noise_statistics_and_snr():
    n = 1 << 20
    z = R.noise_z(3, 2, 1, n).astype(np.float64)
    assert abs(z.mean()) <= 5 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * math.sqrt(1.7 / n)                                # a sum of four uniforms has kurtosis 2.7
    assert np.abs(z).max() <= 3.47
    # the host path draws the same samples: y - x = sigma z
    N = 64000
    x = np.random.default_rng(2).standard_normal((2, N)).astype(np.float32) * np.float32(0.05)
    a = A(snr=(5, 25), seed=3)
    y, sg = a.noise(torch.from_numpy(x), None, 2)
    for b in range(2):
        snr = float(R.snr_db(3, 2, b, 5, 25))
        assert 5 <= snr <= 25
        P = R.power(x[b], N)
        got = 10 * math.log10(P / np.mean((y.numpy()[b].astype(np.float64) - x[b]) ** 2))
        # mean((y - x)^2) = sigma^2 mean(z^2); mean(z^2) has standard deviation sqrt(1.7 / N), so 10 log10 of it has
        # (10 / ln 10) sqrt(1.7 / N); the float32 roundings of sigma, sigma z and x + . are below 1e-6 relative: far inside
        assert abs(got - snr) <= 5 * (10 / math.log(10)) * math.sqrt(1.7 / N), (got, snr)


def test_entry_points_report_bad_arguments():
    import ctypes
    L = pkg("_lib")
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    q = p + 2048 * 4

    def lips(src=p, dst=q, B=1, T=2, H=8, W=8, step=0, S=1, thr=0, wmax=0, E=25):
        return lib.av_augment_lips(src, dst, None, B, T, H, W, 0, step, 0xF0000011, S, thr, wmax, E, None)
    for kw, word in ((dict(dst=p), b"src == dst"), (dict(dst=p + 4), b"overlap"), (dict(S=8), b"max_shift"), (dict(src=None), b"null"),
                     (dict(dst=None), b"null"), (dict(wmax=26), b"mask_max"), (dict(T=253, E=2), b"segments"), (dict(step=1 << 24), b"step"),
                     (dict(thr=65537), b"flip_thr"), (dict(B=65537), b"bad shape")):
        assert lips(**kw) != 0 and word in lib.av_last_error(), (kw, lib.av_last_error())
    assert lips(B=0) == 0                                                              # nothing to do: no launch

    def noise(x=p, y=q, lens=p, B=1, N=16, step=0, lo=5.0, hi=25.0, ws=p, sg=p):
        return lib.av_augment_noise(x, y, lens, B, N, 0, step, lo, hi, ws, sg, None)
    for kw, word in ((dict(x=None), b"null"), (dict(lens=None), b"null"), (dict(ws=None), b"null"), (dict(sg=None), b"null"),
                     (dict(lo=25.0, hi=5.0), b"snr"), (dict(N=(1 << 24) + 1), b"bad shape"), (dict(step=-1), b"step"), (dict(y=p + 4), b"overlap")):
        assert noise(**kw) != 0 and word in lib.av_last_error(), (kw, lib.av_last_error())
    assert noise(B=0) == 0
