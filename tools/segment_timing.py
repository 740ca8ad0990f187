"""CTC segmentation on one MI355X: device events around av_ctc_segment (fixed ends and both ends free), around a device copy of the same
log-probs (the bytes the kernel must at least read), and the package's host path (float32 numpy, wall clock, once) at B 2 / V 800 with
(T 15 000, L 3 000) and (T 90 000, L 8 000) - one hour of two speakers against a transcript of 8 000 tokens; then av_ctc_segment against
av_ctc_align at B 8 / T 375 / V 800, where both run.  Log-probs: log_softmax of seeded normal noise (x 3); labels random with no equal
neighbours; four utterances per item.  20 repeats after 3 warm-ups (5 after 1 at the long shapes), median and range.  Writes
profiles/ctc_segment_timing.txt and fails only if the device path is not faster than the host path of the same run.

    python tools/segment_timing.py [--out profiles/ctc_segment_timing.txt] [--no-host]
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
    return f"median {statistics.median(ms):9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})"


def labels(rng, V, L):
    out = rng.integers(1, V, size=L)
    for i in range(1, L):
        if out[i] == out[i - 1]:
            out[i] = 1 + (out[i] % (V - 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_segment_timing.txt"))
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_timing: needs the GPU; there is nothing to time without it")
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops"); S = importlib.import_module(PKG + ".segmentation")
    torch.set_num_threads(16)
    lib = L.lib()
    blank, w = 0, 30
    lines = [f"# tools/segment_timing.py on {torch.cuda.get_device_name(0)}: float32 log-probs (log_softmax of 3 x seeded normal noise), full input and",
             "# target lengths, labels random with no equal neighbours, four utterances per item, score_window 30.  device: events around the one",
             "# call (one workgroup per item); copy: a device-to-device copy of the log-probs.  host: segmentation.ctc_segment on the host tensor",
             "# (float32 numpy, fixed ends), wall clock, once."]
    ok = True

    def run(B, T, V, Lmax, repeats, warmup, host, against_align):
        nonlocal ok
        rng = np.random.default_rng(T + Lmax)
        g = torch.Generator(device="cuda").manual_seed(T)
        lp = torch.log_softmax(3.0 * torch.randn((B, T, V), generator=g, device="cuda"), dim=-1)
        tg = torch.from_numpy(np.stack([labels(rng, V, Lmax) for _ in range(B)])).cuda()
        il, tl = torch.full((B,), T, dtype=torch.long, device="cuda"), torch.full((B,), Lmax, dtype=torch.long, device="cuda")
        q = Lmax // 4
        ut = torch.tensor([[[0, q], [q, 2 * q], [2 * q, 3 * q], [3 * q, Lmax]]] * B, dtype=torch.int32, device="cuda")
        S_max, U = 2 * Lmax + 1, 4
        need = L.ll(0)
        L.check(lib.av_ctc_segment_workspace_bytes(B, T, S_max, L.C.byref(need)))
        ws = torch.empty(((need.value + 3) // 4,), dtype=torch.int32, device="cuda")
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")          # noqa: E731
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")        # noqa: E731
        out = (i32(B, T), i32(B, Lmax, 2), f32(B, Lmax), f32(B), f32(B, T), i32(B, U, 2), f32(B, U), f32(B, U))

        def seg(free):
            L.check(lib.av_ctc_segment(ops.ptr(lp), T * V, V, ops.ptr(tg), Lmax, ops.ptr(il), ops.ptr(tl), ops.ptr(ut), B, T, V, S_max, U, blank,
                                       free, w, *(ops.ptr(x) for x in out), ops.ptr(ws), need.value, ops.stream()))
        fixed = events_ms(lambda: seg(0), repeats, warmup)
        free = events_ms(lambda: seg(3), repeats, warmup)
        dst = torch.empty_like(lp)
        copy = events_ms(lambda: dst.copy_(lp), repeats, warmup)
        del dst
        fm = statistics.median(fixed)
        lines.extend([f"B {B} T {T} V {V}  Lmax {Lmax} (S_max {S_max}), log-probs {lp.numel() * 4 / 1e6:.1f} MB, move workspace {need.value / 1e6:.1f} MB",
                      f"  av_ctc_segment, fixed ends       {fmt(fixed)}   = {1e3 * fm / T:.3f} us per frame",
                      f"  av_ctc_segment, both ends free   {fmt(free)}   = {1e3 * statistics.median(free) / T:.3f} us per frame",
                      f"  device copy of the log-probs     {fmt(copy)}"])
        if against_align:
            need_a = L.ll(0)
            L.check(lib.av_ctc_align_workspace_bytes(B, T, S_max, L.C.byref(need_a)))
            ws_a = torch.empty(((need_a.value + 3) // 4,), dtype=torch.int32, device="cuda")
            al = events_ms(lambda: L.check(lib.av_ctc_align(ops.ptr(lp), T * V, V, ops.ptr(tg), Lmax, ops.ptr(il), ops.ptr(tl), B, T, V, S_max,
                                                            blank, ops.ptr(out[0]), ops.ptr(out[1]), ops.ptr(out[2]), ops.ptr(out[3]),
                                                            ops.ptr(ws_a), need_a.value, ops.stream())), repeats, warmup)
            lines.append(f"  av_ctc_align                     {fmt(al)}   segment (fixed ends) vs align x{fm / statistics.median(al):.2f}")
        if host:
            lp_h, tg_h = lp.cpu(), tg.cpu()
            t0 = time.perf_counter()
            want = S.ctc_segment(lp_h, tg_h, blank=blank, utterances=ut.cpu(), score_window=w)
            hm = (time.perf_counter() - t0) * 1e3
            got = S.ctc_segment(lp, tg, il, tl, blank=blank, utterances=ut, score_window=w)
            same = all(torch.equal(x.cpu().view(torch.int32), y.view(torch.int32)) for x, y in zip(got, want))
            feasible = int(torch.isfinite(want.score).sum())
            lines.append(f"  host path, fixed ends            {hm:12.1f} ms once   device / host results bit-identical: {same}; feasible items {feasible} of {B}; "
                         f"host vs device x{hm / fm:.0f}")
            ok = ok and same and fm < hm

    run(2, 15000, 800, 3000, 5, 1, not args.no_host, False)
    run(2, 90000, 800, 8000, 5, 1, not args.no_host, False)
    run(8, 375, 800, 125, 20, 3, not args.no_host, True)
    lines.append(f"sanity (device bit-identical to and faster than the host path of this run, every shape): {'ok' if ok else 'FAILED'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
