"""Training-time data augmentation: the lip clips are shifted, mirrored and have frames frozen, the waveform gets additive noise at a
drawn signal-to-noise ratio - on the kernels of csrc/augment.hip for GPU tensors (one read and one write of the tensor, nothing is drawn
on the host, nothing synchronises), in numpy for host tensors.  Both follow ONE law and agree bit for bit.

  generator: every choice is a draw of the dropout generator (``drop_draw`` of csrc/av_common.h), a pure function of (seed, stream,
    block); a block yields four 16-bit integers k0..k3 and an integer in 0..R-1 is ``(k * R) >> 16``.  Clip ``b`` at step ``k`` has the
    counter ``c = k * 65536 + b`` (b < 65536, k < 2^24): its plan does not depend on the other clips of the batch.
  lips, float32 [B, T, H, W] (or the same bytes with a channel axis of one), stream S_AUG_LIP1 / S_AUG_LIP2 for speaker 1 / 2:
      out[b, t, y, x] = in[b, tsrc(t), clamp(y - dy, 0, H-1), clamp((flip ? W-1-x : x) - dx, 0, W-1)],  0 for t >= lengths[b]
    block c * 64:  dx = draw(k0, 2S+1) - S,  dy = draw(k1, 2S+1) - S,  flip = k2 < ceil(65536 p)
    frame freeze (dropped video frames; needs no fill value): segment j = 0 .. ceil(n/E)-1 of the n valid frames takes uniforms 2 (j%2)
    and 2 (j%2) + 1 of block c * 64 + 1 + j/2: s_j = draw(., E), w_j = draw(., Wmax + 1), span_j = [jE + s_j, min(jE + s_j + w_j, n)).
    With Wmax <= E a frame lies at most in its own segment's span and the previous one's (the own one wins); inside a span it reads input
    frame max(start - 1, 0), every other frame reads itself; sources are input frames, freezes do not chain.  ceil(T/E) <= 126.
  noise, float32 [B, N], N <= 2^24:  P_b = mean square of the valid samples in double;  snr_b = fl(lo + fl(u fl(hi - lo))) in float32 with
    u = k0 / 65536 of block c of S_AUG_SNR;  sigma_b = float32(sqrt(P_b 10^(-snr_b / 10)));  y_i = fl(x_i + fl(sigma_b z_i)) for
    i < lengths[b] and x_i beyond, z_i = float32(k0 + k1 + k2 + k3 - 131070) * float32(1 / sqrt((65536^2 - 1) / 3)) of block (c << 24) + i
    of S_AUG_NOISE: a sum of four uniforms - zero mean, unit variance, |z| <= 3.47, exact in integers (a Box-Muller draw could not be
    restated bit for bit).  A silent or empty row has sigma 0 and is copied."""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch

S_AUG_LIP1, S_AUG_LIP2, S_AUG_SNR, S_AUG_NOISE = 0xF0000011, 0xF0000012, 0xF0000013, 0xF0000014      # AV_AUG_STREAM_* of include/av_hip.h
NOISE_CHUNK = 8192                                   # AV_AUG_NOISE_CHUNK
MAX_SEGMENTS, MAX_BATCH, MAX_STEP, MAX_SAMPLES = 126, 65536, 1 << 24, 1 << 24
_INV_STD = np.float32(1.0 / math.sqrt((65536.0 ** 2 - 1.0) / 3.0))
_M32 = 0xFFFFFFFF
_ENV = ("AVAMD_AUG_SHIFT", "AVAMD_AUG_FLIP", "AVAMD_AUG_TMASK", "AVAMD_AUG_TMASK_EVERY", "AVAMD_AUG_SNR", "AVAMD_AUG_SEED")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the generator on the host (csrc/av_common.h: drop_key, drop_key2, mix32, drop_draw)
def _rotl(x: int, r: int) -> int:
    return ((x << r) | (x >> (32 - r))) & _M32


def _keys(seed: int, stream: int):
    h = ((seed & _M32) * 0x9E3779B1) & _M32
    h ^= (((seed >> 32) & _M32) * 0x85EBCA77) & _M32
    h ^= (((stream + 0x165667B1) & _M32) * 0xC2B2AE3D) & _M32
    h ^= h >> 15; h = (h * 0x2C1B3C6D) & _M32; h ^= h >> 12; h = (h * 0x297A2D39) & _M32; h ^= h >> 15
    g = (_rotl(h, 16) * 0x9E3779B1 + 0x7F4A7C15) & _M32
    g ^= g >> 13; g = (g * 0x5BD1E995) & _M32; g ^= g >> 15
    return h, g


def _mix32(x: np.ndarray, k2: int) -> np.ndarray:
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7FEB352D); x = x ^ np.uint32(k2)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846CA68B); x = x ^ (x >> np.uint32(16))
    return x


def _draw4(seed: int, stream: int, blocks: np.ndarray) -> np.ndarray:
    """blocks uint64 [n] -> the four 16-bit integers of each block, int64 [n, 4]."""
    key, k2 = _keys(seed, stream)
    blocks = np.atleast_1d(np.asarray(blocks, dtype=np.uint64))
    lo = (blocks & np.uint64(_M32)).astype(np.uint32)
    c1 = (blocks >> np.uint64(32)).astype(np.uint32)
    rot = lambda v, r: (v << np.uint32(r)) | (v >> np.uint32(32 - r))
    x = lo ^ np.uint32(key) ^ c1 ^ rot(c1, 11) ^ rot(c1, 23)
    o0, o1 = _mix32(x, k2), _mix32(x + np.uint32(0x9E3779B9), k2)
    return np.stack([o0 & np.uint32(0xFFFF), o0 >> np.uint32(16), o1 & np.uint32(0xFFFF), o1 >> np.uint32(16)], axis=1).astype(np.int64)


def _host_lengths(lengths, B: int, full: int) -> np.ndarray:
    if lengths is None:
        return np.full(B, full, np.int64)
    n = lengths.detach().cpu().numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)
    n = n.astype(np.int64).reshape(-1)
    if n.size != B:
        raise ValueError(f"augment: {n.size} lengths for a batch of {B}")
    return np.clip(n, 0, full)


class Augment:
    """Settings of the augmentation and its step counter.  ``max_shift`` S: translation by dx, dy in -S..S pixels (border pixels repeat);
    ``flip``: probability of a horizontal mirror; ``mask_max`` / ``mask_every``: per segment of ``mask_every`` frames one run of up to
    ``mask_max`` frozen frames; ``snr``: (lo, hi) in dB, the range the mixture's signal-to-noise ratio is drawn from, None = no noise.
    ``step`` counts training steps (the trainer advances it); ``rank_offset`` is added to the seed (data parallelism)."""

    def __init__(self, max_shift: int = 0, flip: float = 0.0, mask_max: int = 0, mask_every: int = 25, snr=None, seed: int = 0):
        self.max_shift, self.mask_max, self.mask_every, self.seed = int(max_shift), int(mask_max), int(mask_every), int(seed)
        self.flip = float(flip)
        if self.max_shift < 0:
            raise ValueError(f"Augment: max_shift must be >= 0, got {max_shift}")
        if not 0.0 <= self.flip <= 1.0:                                        # NaN fails both comparisons
            raise ValueError(f"Augment: flip must be a probability in [0, 1], got {flip}")
        if self.mask_every < 1 or not 0 <= self.mask_max <= self.mask_every:
            raise ValueError(f"Augment: need 0 <= mask_max <= mask_every and mask_every >= 1, got mask_max={mask_max} mask_every={mask_every}")
        if snr is not None:
            lo, hi = (float(v) for v in snr)
            if not (lo <= hi and math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError(f"Augment: snr must be finite (lo, hi) with lo <= hi, got {snr}")
            snr = (lo, hi)
        self.snr = snr
        if not 0 <= self.seed < 1 << 64:
            raise ValueError(f"Augment: seed must fit 64 bits, got {seed}")
        self.flip_thr = min(65536, max(0, math.ceil(65536.0 * self.flip)))     # the resolution of the dropout keep test
        self.step = 0
        self.rank_offset = 0
        self.last_power = None                                                 # P_b of the last noise() call, float64 [B]
        self._ws = {}

    @classmethod
    def from_env(cls) -> Optional["Augment"]:
        """AVAMD_AUG_SHIFT, AVAMD_AUG_FLIP, AVAMD_AUG_TMASK, AVAMD_AUG_TMASK_EVERY (25), AVAMD_AUG_SNR ("lo,hi"), AVAMD_AUG_SEED (0);
        None when nothing is switched on."""
        env = os.environ
        snr = env.get("AVAMD_AUG_SNR") or None
        if snr is not None:
            parts = snr.split(",")
            if len(parts) != 2:
                raise ValueError(f'AVAMD_AUG_SNR must be "lo,hi", got {snr!r}')
            snr = (float(parts[0]), float(parts[1]))
        a = cls(max_shift=int(env.get("AVAMD_AUG_SHIFT", "0")), flip=float(env.get("AVAMD_AUG_FLIP", "0")),
                mask_max=int(env.get("AVAMD_AUG_TMASK", "0")), mask_every=int(env.get("AVAMD_AUG_TMASK_EVERY", "25")), snr=snr,
                seed=int(env.get("AVAMD_AUG_SEED", "0")))
        return a if (a.lips_on or a.noise_on) else None

    @property
    def lips_on(self) -> bool:
        return self.max_shift > 0 or self.flip_thr > 0 or self.mask_max > 0

    @property
    def noise_on(self) -> bool:
        return self.snr is not None

    def state_dict(self) -> dict:
        return {"step": int(self.step), "seed": int(self.seed)}

    def load_state_dict(self, sd: dict) -> None:
        self.step, self.seed = int(sd["step"]), int(sd["seed"])

    # -----------------------------------------------------------------------------------------------------------------------------------
    def _seed(self) -> int:
        return (self.seed + self.rank_offset) & ((1 << 64) - 1)

    def _step(self, step) -> int:
        step = self.step if step is None else int(step)
        if not 0 <= step < MAX_STEP:
            raise ValueError(f"augment: step {step} outside [0, 2^24)")
        return step

    @staticmethod
    def _lip_stream(speaker: int) -> int:
        if speaker not in (1, 2):
            raise ValueError(f"augment: speaker must be 1 or 2, got {speaker}")
        return S_AUG_LIP1 if speaker == 1 else S_AUG_LIP2

    def _check_clip(self, B: int, T: int) -> None:
        if B > MAX_BATCH:
            raise ValueError(f"augment: at most {MAX_BATCH} clips per batch, got {B}")
        if -(-T // self.mask_every) > MAX_SEGMENTS:
            raise ValueError(f"augment: {T} frames in segments of {self.mask_every} are more than {MAX_SEGMENTS} segments")

    def plan(self, B: int, T: int, lengths=None, step=None, speaker: int = 1):
        """(dx int64 [B], dy int64 [B], flip bool [B], tsrc int64 [B, T]) on the host; tsrc is the input frame an output frame reads, -1
        for a padded frame (written as zeros)."""
        self._check_clip(B, T)
        step, stream, seed = self._step(step), self._lip_stream(speaker), self._seed()
        n_all = _host_lengths(lengths, B, T)
        S, E = self.max_shift, self.mask_every
        dx, dy, flip = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, bool)
        tsrc = np.tile(np.arange(T, dtype=np.int64), (B, 1))
        for b in range(B):
            c = step * 65536 + b
            k = _draw4(seed, stream, np.uint64(c * 64) + np.arange(64, dtype=np.uint64))
            dx[b] = ((k[0, 0] * (2 * S + 1)) >> 16) - S
            dy[b] = ((k[0, 1] * (2 * S + 1)) >> 16) - S
            flip[b] = k[0, 2] < self.flip_thr
            n = int(n_all[b])
            if self.mask_max > 0:
                src = np.arange(T, dtype=np.int64)
                for j in range(-(-n // E)):                                    # ascending: the own segment's span overwrites the previous one's
                    blk, u = 1 + j // 2, 2 * (j % 2)
                    start = j * E + int((k[blk, u] * E) >> 16)
                    end = min(start + int((k[blk, u + 1] * (self.mask_max + 1)) >> 16), n)
                    if end > start:
                        src[start:end] = max(start - 1, 0)
                tsrc[b] = src
            tsrc[b, n:] = -1
        return dx, dy, flip, tsrc

    # -----------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _clip_shape(x: torch.Tensor):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise ValueError("augment.lips: the clips must be a float32 tensor")
        if x.dim() == 4:
            return tuple(x.shape)
        if x.dim() == 5 and x.shape[1] == 1:
            return (x.shape[0], x.shape[2], x.shape[3], x.shape[4])
        if x.dim() == 5 and x.shape[2] == 1:
            return (x.shape[0], x.shape[1], x.shape[3], x.shape[4])
        raise ValueError(f"augment.lips: clips must be [B, T, H, W], [B, 1, T, H, W] or [B, T, 1, H, W], got {tuple(x.shape)}")

    def lips(self, x: torch.Tensor, lengths=None, step=None, speaker: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The augmented clips, the shape of ``x``; ``x`` is not written.  ``lengths``: valid frames per clip (None = all).  A GPU tensor runs
        av_augment_lips on the current stream (``out``: the buffer to write, same shape, contiguous, not ``x``); a host tensor the numpy law."""
        B, T, H, W = self._clip_shape(x)
        self._check_clip(B, T)
        if self.max_shift >= min(H, W):
            raise ValueError(f"augment.lips: max_shift {self.max_shift} must be below min(H, W) = {min(H, W)}")
        step, stream = self._step(step), self._lip_stream(speaker)
        if not x.is_cuda:
            dx, dy, flip, tsrc = self.plan(B, T, lengths, step, speaker)
            src = x.detach().reshape(B, T, H, W).numpy()
            res = np.zeros_like(src)
            for b in range(B):
                xs = np.clip((W - 1 - np.arange(W) if flip[b] else np.arange(W)) - dx[b], 0, W - 1)
                ys = np.clip(np.arange(H) - dy[b], 0, H - 1)
                for t in np.flatnonzero(tsrc[b] >= 0):
                    res[b, t] = src[b, tsrc[b, t]][ys][:, xs]
            res = torch.from_numpy(res).reshape(x.shape)
            if out is not None:
                out.copy_(res)
                return out
            return res
        from . import _lib as L
        from . import ops
        x = x.detach()
        if not x.is_contiguous():
            x = x.contiguous()
        if out is None:
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
            raise ValueError("augment.lips: out must be a contiguous float32 tensor of the clips' shape on their device")
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=x.device, dtype=torch.long, non_blocking=True).contiguous()
            if lengths.numel() != B:
                raise ValueError(f"augment.lips: {lengths.numel()} lengths for a batch of {B}")
        L.check(L.lib().av_augment_lips(ops.ptr(x), ops.ptr(out), ops.ptr(lengths), B, T, H, W, self._seed(), step, stream, self.max_shift,
                                        self.flip_thr, self.mask_max, self.mask_every, ops.stream()), "av_augment_lips")
        return out

    def noise(self, x: torch.Tensor, lengths=None, step=None, out: Optional[torch.Tensor] = None, sigma: Optional[torch.Tensor] = None):
        """(y, sigma): the waveforms float32 [B, N] with noise at the drawn SNR on their valid samples (``lengths``, None = all) and the noise
        level float32 [B]; ``x`` is not written.  P_b is left in ``last_power``.  GPU tensors run av_augment_noise on the current stream."""
        if self.snr is None:
            raise ValueError("augment.noise: no snr range is set")
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2:
            raise ValueError("augment.noise: the waveforms must be a float32 tensor [B, N]")
        B, N = x.shape
        if B >= MAX_BATCH or N > MAX_SAMPLES:
            raise ValueError(f"augment.noise: B = {B} or N = {N} beyond the index packing (B < 65536, N <= 2^24)")
        step, seed = self._step(step), self._seed()
        lo, hi = np.float32(self.snr[0]), np.float32(self.snr[1])
        if not x.is_cuda:
            n_all = _host_lengths(lengths, B, N)
            src = x.detach().numpy()
            y = src.copy()
            sg = np.zeros(B, np.float32)
            power = np.zeros(B, np.float64)
            for b in range(B):
                n, c = int(n_all[b]), step * 65536 + b
                if n == 0:
                    continue
                power[b] = np.sum(src[b, :n].astype(np.float64) ** 2) / n
                if not power[b] > 0:
                    continue
                u = np.float32(_draw4(seed, S_AUG_SNR, np.uint64(c))[0, 0]) * np.float32(1.0 / 65536.0)
                snr = np.float32(lo + np.float32(u * np.float32(hi - lo)))
                sg[b] = np.float32(math.sqrt(power[b] * math.pow(10.0, -float(snr) / 10.0)))
                if sg[b] == 0:
                    continue
                k = _draw4(seed, S_AUG_NOISE, np.uint64(c << 24) + np.arange(n, dtype=np.uint64))
                z = (k.sum(1) - 131070).astype(np.float32) * _INV_STD
                y[b, :n] = src[b, :n] + sg[b] * z
            self.last_power = torch.from_numpy(power)
            y, sg = torch.from_numpy(y), torch.from_numpy(sg)
            if out is not None:
                out.copy_(y); y = out
            if sigma is not None:
                sigma.copy_(sg); sg = sigma
            return y, sg
        from . import _lib as L
        from . import ops
        x = x.detach()
        if not x.is_contiguous():
            x = x.contiguous()
        dev = x.device
        if out is None:
            out = torch.empty((B, N), dtype=torch.float32, device=dev)
        elif out.shape != x.shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError("augment.noise: out must be a contiguous float32 tensor [B, N] on the waveforms' device")
        if sigma is None:
            sigma = torch.empty((B,), dtype=torch.float32, device=dev)
        elif sigma.shape != (B,) or sigma.dtype != torch.float32 or sigma.device != dev or not sigma.is_contiguous():
            raise ValueError("augment.noise: sigma must be a contiguous float32 tensor [B] on the waveforms' device")
        if lengths is None:
            lengths = torch.full((B,), N, dtype=torch.long, device=dev)
        else:
            lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.long, non_blocking=True).contiguous()
            if lengths.numel() != B:
                raise ValueError(f"augment.noise: {lengths.numel()} lengths for a batch of {B}")
        words = max(1, B) * (1 + max(1, -(-N // NOISE_CHUNK)))
        ws = self._ws.get(dev)
        if ws is None or ws.numel() < words:
            ws = self._ws[dev] = torch.empty((words,), dtype=torch.float64, device=dev)
        L.check(L.lib().av_augment_noise(ops.ptr(x), ops.ptr(out), ops.ptr(lengths), B, N, seed, step, float(lo), float(hi), ops.ptr(ws),
                                         ops.ptr(sigma), ops.stream()), "av_augment_noise")
        self.last_power = ws[:B]
        return out, sigma
