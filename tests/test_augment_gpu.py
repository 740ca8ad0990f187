"""GPU: av_augment_lips / av_augment_noise against the independent restatement tests/augment_ref.py (exact equality: the lip pass computes
nothing in floating point, the noise pass is checked with the device's own sigma), and the trainer's augment= option on the tiny
configuration of tests/test_step_gpu.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import augment_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu
ENV = ("AVAMD_AUG_SHIFT", "AVAMD_AUG_FLIP", "AVAMD_AUG_TMASK", "AVAMD_AUG_TMASK_EVERY", "AVAMD_AUG_SNR", "AVAMD_AUG_SEED")
SEED = 11
# (B, T, H, W), lengths, (S, flip, mask_max, mask_every), steps.  H != W catches an x / y swap; lengths 60 and 37 make a span spill into
# the next segment and a span clipped at the valid length; mask_max = mask_every = 25 puts frames under both their own segment's span and
# the previous one's; rows of 10 pixels are no multiple of four.  96 x 96: the real frame size.  5 x 7: 35 elements per frame, the path
# without 16-byte stores.
LIP_CASES = {
    "small": ((3, 60, 12, 10), (60, 37, 1), (3, 0.5, 25, 25), (0, 1, 7)),
    "frame": ((2, 5, 96, 96), (5, 3), (4, 0.5, 2, 3), (2,)),
    "odd": ((2, 7, 5, 7), (7, 4), (2, 0.5, 3, 3), (0, 3)),
}


def aug_of(cfg, **kw):
    S, flip, wmax, every = cfg
    return pkg("augment").Augment(max_shift=S, flip=flip, mask_max=wmax, mask_every=every, seed=SEED, **kw)


@functools.lru_cache(maxsize=None)
def lip_case(name, step, speaker):
    """(input, expected output) of a case, computed once and shared (read-only)."""
    shape, lengths, (S, flip, wmax, every), _ = LIP_CASES[name]
    x = np.random.default_rng(len(name)).random(shape, dtype=np.float32)
    want = R.lips(x, lengths, SEED, step, speaker, S, int(np.ceil(65536 * flip)), wmax, every)
    x.setflags(write=False); want.setflags(write=False)
    return x, want


@pytest.mark.parametrize("name,step,speaker", [(n, s, 1 + (i + len(n)) % 2) for n, c in LIP_CASES.items() for i, s in enumerate(c[3])])
def test_lips_equal_the_reference(name, step, speaker):
    shape, lengths, cfg, _ = LIP_CASES[name]
    x, want = lip_case(name, step, speaker)
    a = aug_of(cfg)
    xd = torch.from_numpy(x.copy()).cuda()
    got = a.lips(xd, torch.tensor(lengths), step, speaker)
    assert got.data_ptr() != xd.data_ptr() and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(xd.cpu().numpy(), x)                                          # the input is bit-unchanged
    g = got.cpu().numpy()
    for b, n in enumerate(lengths):
        assert not g[b, n:].any()                                                      # padded frames are 0
    assert any(not np.array_equal(g[b, :n], x[b, :n]) for b, n in enumerate(lengths))  # and something did happen
    # the host path of the package gives the same clips
    assert np.array_equal(a.lips(torch.from_numpy(x.copy()), torch.tensor(lengths), step, speaker).numpy(), want)


def test_lips_full_lengths_channel_view_own_buffer_and_copy():
    shape, _, cfg, _ = LIP_CASES["small"]
    x, _ = lip_case("small", 0, 1)
    a = aug_of(cfg)
    xd = torch.from_numpy(x.copy()).cuda()
    full = a.lips(xd, torch.full((shape[0],), shape[1]), 4, 2)
    assert torch.equal(a.lips(xd, None, 4, 2), full)                                    # lengths = None: every clip is T frames long
    assert np.array_equal(full.cpu().numpy(), R.lips(x, None, SEED, 4, 2, cfg[0], 32768, cfg[2], cfg[3]))
    view = xd[:, :, None].permute(0, 2, 1, 3, 4)                                        # the trainer's [B, 1, T, H, W] view: the same bytes
    buf = torch.full(view.shape, 7.0, device="cuda")
    out = a.lips(view, None, 4, 2, out=buf)
    assert out is buf and torch.equal(buf[:, 0], full)
    off = pkg("augment").Augment(seed=SEED)                                             # all off: a bit-exact copy (and zeros beyond the length)
    assert torch.equal(off.lips(xd, None, 3, 1).view(torch.int32), xd.view(torch.int32))


NOISE_CASES = {
    # N = 1003: rows that are no multiple of four samples; row 1 is silent among the non-empty ones, row 3 is empty
    "small": (1003, (1003, 640, 1, 0), 1),
    # N = 8204: two chunks of the power pass, 16-byte loads and stores; row 2 is silent
    "chunks": (8204, (8204, 8193, 4100, 0), 2),
}


@pytest.mark.parametrize("name", list(NOISE_CASES))
def test_noise_equals_the_law(name):
    N, lengths, silent = NOISE_CASES[name]
    lo, hi, step = 5.0, 25.0, 3
    x = (np.random.default_rng(N).standard_normal((4, N)) * 0.1).astype(np.float32)
    x[silent] = 0
    x[3] = 0                                                                           # padding stays 0
    for b, n in enumerate(lengths):
        x[b, n:] = 0
    x[1, -1] = -0.0                                                                    # in row 1's padding: a copy keeps the sign bit
    a = pkg("augment").Augment(snr=(lo, hi), seed=SEED)
    xd = torch.from_numpy(x.copy()).cuda()
    ld = torch.tensor(lengths).cuda()
    y, sg = a.noise(xd, ld, step)
    power = a.last_power.clone()
    y2, sg2 = a.noise(xd, ld, step, out=torch.empty_like(xd), sigma=torch.empty_like(sg))
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)) and torch.equal(sg.view(torch.int32), sg2.view(torch.int32))
    assert torch.equal(power.view(torch.int64), a.last_power.view(torch.int64))         # two runs: the same bits
    assert np.array_equal(xd.cpu().numpy().view(np.int32), x.view(np.int32))            # the input is bit-unchanged
    sg_h, p_h, y_h = sg.cpu().numpy(), power.cpu().numpy(), y.cpu().numpy()
    for b, n in enumerate(lengths):
        P = R.power(x[b], n)
        assert abs(p_h[b] - P) <= 1e-12 * P
        law = R.sigma64(x[b], n, SEED, step, b, lo, hi)
        assert abs(float(sg_h[b]) - law) <= float(np.spacing(np.float32(law))), (b, sg_h[b], law)     # within 1 float32 ulp
        assert (sg_h[b] == 0) == (b in (silent, 3))
    want, _ = R.noise(x, lengths, SEED, step, lo, hi, sigma=sg_h)
    assert np.array_equal(y_h, want)                                                   # y = fl(x + fl(sigma_dev z_ref)), exactly
    for b, n in enumerate(lengths):                                                    # padding and the silent row: bit-unchanged
        assert np.array_equal(y_h[b, n:].view(np.int32), x[b, n:].view(np.int32))
    assert np.array_equal(y_h[silent].view(np.int32), x[silent].view(np.int32))
    assert not np.array_equal(y_h[0, :lengths[0]], x[0, :lengths[0]])


def test_bad_arguments_are_status_codes():
    L = pkg("_lib"); ops = pkg("ops")
    lib = L.lib()
    x = torch.zeros((1, 2, 8, 8), device="cuda"); y = torch.empty_like(x)
    n = torch.tensor([2], device="cuda")

    def lips(src, dst, S=1):
        return lib.av_augment_lips(ops.ptr(src), ops.ptr(dst), ops.ptr(n), 1, 2, 8, 8, 0, 0, 0xF0000011, S, 0, 0, 25, ops.stream())
    assert lips(x, x) != 0 and b"src == dst" in lib.av_last_error()
    assert lips(x, y, S=8) != 0 and b"max_shift" in lib.av_last_error()
    assert lips(None, y) != 0 and b"null" in lib.av_last_error()
    assert lips(x, None) != 0 and b"null" in lib.av_last_error()
    w = torch.zeros((1, 16), device="cuda"); ws = torch.empty(2, dtype=torch.float64, device="cuda"); sg = torch.empty(1, device="cuda")
    for args in ((None, w, n, ws, sg), (w, None, n, ws, sg), (w, w, None, ws, sg), (w, w, n, None, sg), (w, w, n, ws, None)):
        xx, yy, ll, pp, ss = (ops.ptr(t) for t in args)
        assert lib.av_augment_noise(xx, yy, ll, 1, 16, 0, 0, 5.0, 25.0, pp, ss, ops.stream()) != 0 and b"null" in lib.av_last_error()
    with pytest.raises(ValueError):
        pkg("augment").Augment(max_shift=8).lips(x, None, 0, 1)
    with pytest.raises(RuntimeError, match="src == dst"):
        pkg("augment").Augment(max_shift=1).lips(x, None, 0, 1, out=x)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the trainer
KEYS = ("loss1", "loss2", "contrast1", "contrast2", "total")


@pytest.fixture(autouse=True)
def no_augment_environment(monkeypatch):
    """A trainer built with augment=None reads the environment: the tests decide what is on, not the shell."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def on_settings(seed=SEED):
    return pkg("augment").Augment(max_shift=4, flip=0.5, mask_max=10, mask_every=25, snr=(5, 25), seed=seed)


def trainer(aug):
    """The tiny fp32 trainer of tests/test_step_gpu.py, constructed again around the same modules with ``augment=``."""
    from test_step_gpu import build
    init = pkg("utils.init"); tr = pkg("model.trainer")
    t0 = build(init.W2V2_TINY, "fp32")
    t = tr.MultimodalTrainer(t0.visual_encoder, t0.audio_encoder, t0.fusion_module, t0.decoder1, t0.tokenizer, learning_rate=1e-4, device="cuda",
                             lambda_=0.1, augment=aug)
    t.fixed_projection = t0.fixed_projection
    return t


def batch_of(seed=5, ragged=False):
    return pkg("dataset.synthetic").make_batch(2, 1.0, seed=seed, ragged=ragged)


def losses(out):
    return tuple(float(out[k].detach()) for k in KEYS)


def test_trainer_feeds_the_encoders_the_host_law():
    aug = on_settings()
    t = trainer(aug)
    cpu = batch_of(seed=6, ragged=True)
    dev = {k: v.cuda() for k, v in cpu.items()}                                         # device-resident: the step sees the batch's own tensors
    seen = {"lips": [], "audio": []}
    vf, af = t.visual_encoder.forward, t.audio_encoder.forward

    def vis(x, *a, **kw):
        seen["lips"].append(x.detach().clone())
        return vf(x, *a, **kw)

    def aud(x, *a, **kw):
        seen["audio"].append(x.detach().clone())
        return af(x, *a, **kw)
    t.visual_encoder.forward, t.audio_encoder.forward = vis, aud
    host = on_settings()
    valid = (cpu["mask1"] != 3).sum(1)
    for k in range(2):
        seen["lips"].clear(); seen["audio"].clear()
        assert aug.step == k
        t.train_step(dev)
        assert aug.step == k + 1 and len(seen["lips"]) == 2 and len(seen["audio"]) == 1
        for spk in (1, 2):
            want = host.lips(cpu[f"lip{spk}"], cpu[f"lip{spk}_lengths"], k, spk)        # [B, T, 1, H, W] on the host
            got = seen["lips"][spk - 1].cpu()                                          # [B, 1, T, H, W]
            assert torch.equal(got.permute(0, 2, 1, 3, 4), want) and not torch.equal(want, cpu[f"lip{spk}"])
        y_host, sg_host = host.noise(cpu["audio"], valid, k)
        sg = t.last_aug_sigma.cpu().numpy()
        assert (np.abs(sg - sg_host.numpy()) <= np.spacing(sg_host.numpy())).all()
        want, _ = R.noise(cpu["audio"].numpy(), valid.tolist(), SEED, k, 5, 25, sigma=sg)
        assert np.array_equal(seen["audio"][0].cpu().numpy(), want) and not np.array_equal(want, cpu["audio"].numpy())
    for k, v in cpu.items():                                                           # the batch's own tensors are bit-unchanged
        assert torch.equal(dev[k].cpu(), v), k


@pytest.fixture(scope="module")
def uninterrupted(tmp_path_factory):
    """Four steps of one augmented trainer; a checkpoint after step 2 (the third step)."""
    ck = pkg("checkpoint")
    t = trainer(on_settings())
    b = [batch_of(seed=5 + i, ragged=bool(i % 2)) for i in range(4)]
    ls = [losses(t.train_step(b[i])) for i in range(3)]
    path = str(tmp_path_factory.mktemp("aug") / "aug.pt")
    ck.save_checkpoint(0, t, path)
    ls.append(losses(t.train_step(b[3])))
    return {"batches": b, "losses": ls, "path": path}


def test_same_seed_same_losses_other_seed_other_losses(uninterrupted):
    b = uninterrupted["batches"]
    same, other = trainer(on_settings()), trainer(on_settings(seed=SEED + 1))
    ls_same = [losses(same.train_step(b[i])) for i in range(3)]
    ls_other = [losses(other.train_step(b[i])) for i in range(3)]
    assert ls_same == uninterrupted["losses"][:3]                                      # bit for bit
    assert all(u[4] != v[4] for u, v in zip(ls_other, ls_same))


def test_resume_continues_bit_for_bit(uninterrupted, tmp_path):
    ck = pkg("checkpoint")
    t = trainer(on_settings(seed=99))                                                  # the file's seed and step replace these
    saved = torch.load(uninterrupted["path"], weights_only=True)["augment"]
    assert saved == {"step": 3, "seed": SEED} and all(type(v) is int for v in saved.values())
    assert ck.load_checkpoint(t, uninterrupted["path"], audio_encoder=True, optimizer=True) == 1
    assert (t.augment.step, t.augment.seed) == (3, SEED)
    assert losses(t.train_step(uninterrupted["batches"][3])) == uninterrupted["losses"][3]
    # a checkpoint written without augmentation has no entry and still loads, into either kind of trainer
    plain = trainer(None)
    path = str(tmp_path / "plain.pt")
    ck.save_checkpoint(2, plain, path)
    assert "augment" not in torch.load(path, weights_only=True)
    assert ck.load_checkpoint(t, path, audio_encoder=True, optimizer=True) == 3 and t.augment.step == 4
    assert ck.load_checkpoint(plain, uninterrupted["path"], optimizer=True) == 1 and plain.augment is None


def test_evaluate_never_augments_and_default_is_off(monkeypatch):
    from test_step_gpu import build
    plain = build(pkg("utils.init").W2V2_TINY, "fp32")                                 # augment=None, nothing in the environment
    assert plain.augment is None and plain._aug_buf == {}
    aug = trainer(on_settings())
    batch = batch_of(seed=8, ragged=True)
    l0, w0 = plain.evaluate([batch])
    l1, w1 = aug.evaluate([batch])
    assert l0 == l1 and w0 == w1 and aug._aug_buf == {} and aug.augment.step == 0
    monkeypatch.setenv("AVAMD_AUG_SHIFT", "2")
    env = build(pkg("utils.init").W2V2_TINY, "fp32")
    assert env.augment is not None and env.augment.max_shift == 2 and not env.augment.noise_on
