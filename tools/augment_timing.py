"""The augmentation kernels on one MI355X at the headline shape (lips 64 x 100 x 96 x 96 fp32 for each of the two speakers, audio
64 x 64000), against their floor and against the only form available before:
  (a) av_augment_lips, both speakers / av_augment_noise                      (augment.Augment, output buffers reused),
  (b) a device-to-device copy of the same tensors: the floor of a pass that reads and writes the tensor once,
  (c) the torch composition: per clip index_select along time, replicate-pad + slice for the shift and flip where drawn, with the plan
      drawn on the host (the same plan (a) uses, so both move the same pixels) / randn-based noise at a drawn SNR.
Alternating rounds in steady state within one process, device events, median and range.  (c)'s host time (drawing the plan, launching
~4 ops per clip) is reported separately as wall time.  Writes profiles/augment_timing.txt; records, gates nothing.

    python tools/augment_timing.py [--out profiles/augment_timing.txt] [--rounds 20]
"""
from __future__ import annotations

import argparse
import importlib
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "multimodal-av-model_amd"


def fmt(ms):
    return f"median {statistics.median(ms):8.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_lips(x, out, plan, S):
    """x, out [B, T, H, W]; the plan of Augment.plan with full lengths."""
    dx, dy, flip, tsrc = plan
    H, W = x.shape[2], x.shape[3]
    for b in range(x.shape[0]):
        y = x[b].index_select(0, tsrc[b])
        if flip[b]:
            y = y.flip(2)
        y = F.pad(y[None], (S, S, S, S), mode="replicate")[0]
        ox = S + dx[b] if flip[b] else S - dx[b]                   # the shift is applied to the mirrored frame
        out[b] = y[:, S - dy[b]:S - dy[b] + H, ox:ox + W]
    return out


def torch_noise(x, valid, n, lo, hi):
    P = (x * x * valid).sum(1) / n
    snr = lo + (hi - lo) * torch.rand(x.shape[0], device=x.device)
    sigma = torch.sqrt(P * torch.pow(10.0, -snr / 10.0))
    return x + sigma[:, None] * torch.randn_like(x) * valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_timing.txt"))
    ap.add_argument("--rounds", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_timing: needs the GPU; there is nothing to time without it")
    Augment = importlib.import_module(PKG + ".augment").Augment
    B, T, H, W, N = 64, 100, 96, 96, 64000
    S = 4
    aug = Augment(max_shift=S, flip=0.5, mask_max=10, mask_every=25, snr=(5, 25), seed=1)
    g = torch.Generator(device="cuda").manual_seed(3)
    lips = [torch.rand((B, T, H, W), device="cuda", generator=g) for _ in range(2)]
    bufs = [torch.empty_like(l) for l in lips]
    audio = torch.randn((B, N), device="cuda", generator=g) * 0.1
    abuf, sg = torch.empty_like(audio), torch.empty(B, device="cuda")
    n = torch.full((B,), N, dtype=torch.long, device="cuda")
    valid = torch.ones((B, N), device="cuda")
    nf = n.float()
    state = {"step": 0}

    def lips_a():
        for s in (0, 1):
            aug.lips(lips[s], None, state["step"], s + 1, out=bufs[s])

    def lips_b():
        for s in (0, 1):
            bufs[s].copy_(lips[s])

    host = []

    def lips_c():
        t0 = time.perf_counter()
        for s in (0, 1):
            dx, dy, flip, tsrc = aug.plan(B, T, None, state["step"], s + 1)
            plan = (dx.tolist(), dy.tolist(), flip.tolist(), torch.from_numpy(tsrc).cuda())
            torch_lips(lips[s], bufs[s], plan, S)
        host.append(1e3 * (time.perf_counter() - t0))

    sides = {"la": lips_a, "lb": lips_b, "lc": lips_c,
             "na": lambda: aug.noise(audio, n, state["step"], out=abuf, sigma=sg),
             "nb": lambda: abuf.copy_(audio),
             "nc": lambda: torch_noise(audio, valid, nf, 5.0, 25.0)}
    # (a) and (c) move the same pixels: one check before timing
    lips_a(); ref = bufs[0].clone(); lips_c()
    same = bool(torch.equal(ref, bufs[0]))
    for _ in range(3):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    host.clear()
    ms = {k: [] for k in sides}
    for r in range(args.rounds):
        state["step"] = r
        for k, fn in sides.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    gl, ga = 2 * 2 * B * T * H * W * 4 / 1e9, 2 * B * N * 4 / 1e9
    lines = [f"# tools/augment_timing.py on {torch.cuda.get_device_name(0)}.  lips 2 x [{B}, {T}, {H}, {W}] fp32 ({gl / 2:.3f} GB read + {gl / 2:.3f} GB "
             f"written), audio [{B}, {N}] fp32 ({1e3 * ga / 2:.1f} MB each way).  max_shift {S}, flip 0.5, freeze up to 10 of every 25 frames, SNR 5..25 dB.",
             f"# {args.rounds} alternating rounds after 3 warm-up rounds, device events around each side, output buffers reused.",
             f"  lips  (a) av_augment_lips x 2                 {fmt(ms['la'])}   {gl / med['la'] * 1e3:7.0f} GB/s",
             f"  lips  (b) device-to-device copy x 2           {fmt(ms['lb'])}   {gl / med['lb'] * 1e3:7.0f} GB/s",
             f"  lips  (c) torch index_select / flip / pad     {fmt(ms['lc'])}   host wall time of a round: median {statistics.median(host):.1f} ms",
             f"  lips  (a) / (b) x{med['la'] / med['lb']:.3f};  (a) / (c) x{med['la'] / med['lc']:.3f};  (a) and (c) give the same clips: {same}",
             f"  audio (a) av_augment_noise (3 launches)       {fmt(ms['na'])}",
             f"  audio (b) device-to-device copy               {fmt(ms['nb'])}",
             f"  audio (c) torch randn noise at an SNR         {fmt(ms['nc'])}",
             f"  audio (a) / (b) x{med['na'] / med['nb']:.3f};  (a) / (c) x{med['na'] / med['nc']:.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
