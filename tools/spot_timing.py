"""CTC keyword spotting on one MI355X: device events around av_ctc_spot (its three kernels - row maxima, walk, selection - are launched by
ONE call, so the events bracket all three; the split per kernel comes from a kernel trace of this script, see below), a device-to-device
copy of the same log-probs (the yardstick: one read and one write of the bytes the row-max pass reads once) and the package's host path
(float32 numpy, wall clock) on the same data - the only form there was before the kernels.  Shapes: B 64 / T 100 / V 800 with K 10 and
K 100 keywords of L 4 and L 32 ids, and B 2 / T 90 000 (one hour at 25 frames per second) / K 10 at V 800 and at V 32 (the same dependent
chain per frame with every gather in one or two cache lines: what tells the chain from the gathers).  20 repeats after 3 warm-ups, median
and range.  Writes profiles/ctc_spot_timing.txt and fails only if the device path is not faster than the host path of the same run.

    python tools/spot_timing.py [--out profiles/ctc_spot_timing.txt] [--no-host]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/spot_timing.py --no-host --out <dir>/timing.txt      # time per kernel
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

SHAPES = (  # B, T, V, K, L
    (64, 100, 800, 10, 4), (64, 100, 800, 10, 32), (64, 100, 800, 100, 4), (64, 100, 800, 100, 32),
    (2, 90000, 800, 10, 4), (2, 90000, 800, 10, 32), (2, 90000, 32, 10, 32),
)


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


def keywords(rng, K, L, V, blank):
    """K rows of L ids, none the blank, no two neighbours equal."""
    ids = np.zeros((K, L), np.int32)
    for k in range(K):
        for j in range(L):
            c = int(rng.integers(1, V))
            while c == blank or (j and c == ids[k, j - 1]):
                c = int(rng.integers(1, V))
            ids[k, j] = c
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_spot_timing.txt"))
    ap.add_argument("--no-host", action="store_true", help="skip the host path (and the comparison with it): for a kernel trace of this script")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spot_timing: needs the GPU; there is nothing to time without it")
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops"); S = importlib.import_module(PKG + ".spot")
    torch.set_num_threads(16)
    lib = L.lib()
    blank, N = 0, 4
    lines = [f"# tools/spot_timing.py on {torch.cuda.get_device_name(0)}: float32 log-softmax of seeded normal logits x 3, full input lengths, keywords of",
             "# random ids (no neighbours equal), max_hits 4, no score threshold.  device: events around av_ctc_spot (row maxima + walk + selection,",
             "# one call), 20 repeats after 3 warm-ups.  copy: a device-to-device copy of the log-probs.  host: spot.keyword_spot on the host tensor",
             "# (float32 numpy), wall clock, once."]
    ok = True
    for B, T, V, K, Lk in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1000 * T + V)
        lp = torch.log_softmax(torch.randn((B, T, V), generator=g, device="cuda") * 3.0, -1)
        kw_h = keywords(np.random.default_rng(K * 100 + Lk), K, Lk, V, blank)
        kw, kl = torch.from_numpy(kw_h).cuda(), torch.full((K,), Lk, dtype=torch.int32, device="cuda")
        need = L.ll(0)
        L.check(lib.av_ctc_spot_workspace_bytes(B, T, K, L.C.byref(need)))
        ws = torch.empty((need.value // 4,), dtype=torch.int32, device="cuda")
        hits = torch.empty((B, K, N, 2), dtype=torch.int32, device="cuda")
        scores = torch.empty((B, K, N), dtype=torch.float32, device="cuda")
        counts = torch.empty((B, K), dtype=torch.int32, device="cuda")
        dst = torch.empty_like(lp)
        spot = events_ms(lambda: L.check(lib.av_ctc_spot(ops.ptr(lp), T * V, V, None, ops.ptr(kw), Lk, ops.ptr(kl), B, T, V, K, Lk, blank, N,
                                                         float("-inf"), ops.ptr(hits), ops.ptr(scores), ops.ptr(counts), ops.ptr(ws), need.value,
                                                         ops.stream())))
        copy = events_ms(lambda: dst.copy_(lp))
        sm, cm = statistics.median(spot), statistics.median(copy)
        lines += [f"B {B:2d} T {T:5d} V {V:3d}  K {K:3d} L {Lk:2d} ({2 * Lk - 1} states), log-probs {lp.numel() * 4 / 1e6:.1f} MB, workspace {need.value / 1e6:.2f} MB",
                  f"  av_ctc_spot (three kernels)      {fmt(spot)}   = {1e3 * sm / T:.3f} us per frame",
                  f"  device-to-device copy            {fmt(copy)}   spot / copy x{sm / cm:.2f}"]
        if not args.no_host:
            lp_h = lp.cpu()
            t0 = time.perf_counter()
            want = S.keyword_spot(lp_h, (torch.from_numpy(kw_h), None), blank=blank, max_hits=N)
            hm = (time.perf_counter() - t0) * 1e3
            same = (torch.equal(hits.cpu(), want.hits) and torch.equal(counts.cpu(), want.counts)
                    and torch.equal(scores.cpu().view(torch.int32), want.scores.view(torch.int32)))
            lines.append(f"  host path                        once   {hm:9.1f} ms   host / device x{hm / sm:.0f}, results bit-identical: {same}")
            ok = ok and sm < hm and same
        del lp, dst, ws
    if not args.no_host:
        lines.append(f"sanity (device faster than the host path of this run and bit-identical, every shape): {'ok' if ok else 'FAILED'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
