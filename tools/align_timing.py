"""CTC forced alignment on one MI355X: device events around av_ctc_align, around av_ctc_loss_fwd (alpha only: the same serial lattice walk
with log-sum-exp for max and without a back-trace - the yardstick) on the same tensors, and the package's host path (float32 numpy, wall
clock).  B 64 / T 100 / V 800 and B 8 / T 375 / V 800, target lengths about T / 3; 20 repeats after 3 warm-ups, median and range.  Writes
profiles/ctc_align_timing.txt and fails only if the device path is not faster than the host path of the same run.

    python tools/align_timing.py [--out profiles/ctc_align_timing.txt] [--host-repeats 1]
"""
from __future__ import annotations

import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "multimodal-av-model_amd"


def events_ms(fn, repeats=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def fmt(ms):
    return f"median {statistics.median(ms):8.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_align_timing.txt"))
    ap.add_argument("--host-repeats", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_timing: needs the GPU; there is nothing to time without it")
    import align_ref as R
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops"); A = importlib.import_module(PKG + ".align")
    torch.set_num_threads(16)
    lib = L.lib()
    blank = 0
    lines = [f"# tools/align_timing.py on {torch.cuda.get_device_name(0)}: float32 log-probs from the tests' generator, full input lengths, target",
             "# lengths about T / 3 (labels from 5 classes: repeats abound).  device: events, 20 repeats after 3 warm-ups; both kernels run one",
             "# workgroup per utterance.  av_ctc_loss_fwd: loss only (no alpha / beta written).  host: align.forced_align on the host tensor",
             "# (float32 numpy), wall clock."]
    ok = True
    for B, T, V in ((64, 100, 800), (8, 375, 800)):
        Lmax = T // 3
        rng = np.random.default_rng(T)
        lens = [Lmax if b % 2 == 0 else int(rng.integers(max(1, Lmax - 8), Lmax + 1)) for b in range(B)]
        cases = [R.make_case(41000 + b, T, V, lens[b], blank) for b in range(B)]
        lp_h = torch.from_numpy(np.stack([c[0] for c in cases]))
        tg_h = torch.zeros((B, Lmax), dtype=torch.long)
        for b, (_, lab) in enumerate(cases):
            tg_h[b, :len(lab)] = torch.tensor(lab)
        il_h, tl_h = torch.full((B,), T, dtype=torch.long), torch.tensor(lens)
        lp, tg, il, tl = lp_h.cuda(), tg_h.cuda(), il_h.cuda(), tl_h.cuda()
        S_max = 2 * Lmax + 1
        need = L.ll(0)
        L.check(lib.av_ctc_align_workspace_bytes(B, T, S_max, L.C.byref(need)))
        ws = torch.empty(((need.value + 3) // 4,), dtype=torch.int32, device="cuda")
        states = torch.empty((B, T), dtype=torch.int32, device="cuda")
        spans = torch.empty((B, Lmax, 2), dtype=torch.int32, device="cuda")
        tok = torch.empty((B, Lmax), dtype=torch.float32, device="cuda")
        score = torch.empty((B,), dtype=torch.float32, device="cuda")
        nll = torch.empty((B,), dtype=torch.float32, device="cuda")
        align = events_ms(lambda: L.check(lib.av_ctc_align(ops.ptr(lp), T * V, V, ops.ptr(tg), Lmax, ops.ptr(il), ops.ptr(tl), B, T, V, S_max,
                                                           blank, ops.ptr(states), ops.ptr(spans), ops.ptr(tok), ops.ptr(score), ops.ptr(ws),
                                                           need.value, ops.stream())))
        loss = events_ms(lambda: L.check(lib.av_ctc_loss_fwd(ops.ptr(lp), T * V, V, ops.ptr(tg), Lmax, ops.ptr(il), ops.ptr(tl), B, T, V, S_max,
                                                             blank, 0, ops.ptr(nll), None, None, ops.stream())))
        host = []
        for _ in range(args.host_repeats):
            t0 = time.perf_counter()
            al_h = A.forced_align(lp_h, tg_h, il_h, tl_h, blank=blank)
            host.append((time.perf_counter() - t0) * 1e3)
        al_d = A.forced_align(lp, tg, il, tl, blank=blank)
        same = all(torch.equal(x.cpu().view(torch.int32), y.view(torch.int32)) for x, y in zip(al_d, al_h))
        am, lm, hm = statistics.median(align), statistics.median(loss), statistics.median(host)
        lines += [f"B {B:2d} T {T:3d} V {V}  Lmax {Lmax} (S_max {S_max}), workspace {need.value} bytes",
                  f"  av_ctc_align                     {fmt(align)}   = {1e3 * am / T:.2f} us per frame",
                  f"  av_ctc_loss_fwd (loss only)      {fmt(loss)}   = {1e3 * lm / T:.2f} us per frame",
                  f"  host path                        {fmt(host)}   device / host results bit-identical: {same}",
                  f"  align vs loss forward x{am / lm:.2f}, host vs device x{hm / am:.0f}"]
        ok = ok and am < hm
    lines.append(f"sanity (device faster than the host path of this run, both shapes): {'ok' if ok else 'FAILED'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
