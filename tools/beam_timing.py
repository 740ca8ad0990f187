"""CTC prefix beam search on one MI355X: device events around the frame pass alone (av_ctc_beam_frame_pass) and around the whole
av_ctc_beam_search (the search pass = whole - frame pass: the two kernels run back to back on one stream), next to av_ctc_greedy on the
same tensor and to the package's host path (float32 numpy, torch / BLAS threads = 16).  B 64, T 199, V 800, W = 5, 16, 64; 20 repeats
after 3 warm-ups, median and range.  Writes profiles/ctc_beam_timing.txt and fails if the device path at W = 5 is not faster than the
host path of the same run.

    python tools/beam_timing.py [--out profiles/ctc_beam_timing.txt] [--host-repeats 1]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_beam_timing.txt"))
    ap.add_argument("--host-repeats", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_timing: needs the GPU; there is nothing to time without it")
    import beam_ref as R
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops"); bs = importlib.import_module(PKG + ".beam_search")
    torch.set_num_threads(16)
    B, T, V, blank = 64, 199, 800, 0
    lp_h = torch.from_numpy(np.stack([R.make_log_probs(31000 + b, T, V, blank) for b in range(B)]))
    lp = lp_h.cuda()
    lib = L.lib()
    lines = [f"# tools/beam_timing.py on {torch.cuda.get_device_name(0)}: B {B}, T {T}, V {V}, float32 log-probs from the tests' generator, full lengths.",
             "# device: events, 20 repeats after 3 warm-ups; search pass = whole call - frame pass (two kernels back to back on one stream);",
             f"# the search pass runs B = {B} workgroups of 256 threads, one per utterance: {B} of the 256 CUs.",
             "# host: beam_search.prefix_beam_search on the host tensor (float32 numpy), wall clock, 16 threads."]
    out_g, cnt_g = torch.empty((B, T), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")
    greedy = events_ms(lambda: L.check(lib.av_ctc_greedy(ops.ptr(lp), None, ops.ptr(out_g), ops.ptr(cnt_g), B, T, V, blank, ops.stream())))
    lines.append(f"av_ctc_greedy                      {fmt(greedy)}")
    ok = True
    for W in (5, 16, 64):
        need = L.ll(0)
        L.check(lib.av_ctc_beam_workspace_bytes(B, T, V, W, L.C.byref(need)))
        ws = torch.empty(((need.value + 7) // 8,), dtype=torch.int64, device="cuda")
        out = torch.empty((B, 1, T), dtype=torch.int32, device="cuda")
        cnt = torch.empty((B, 1), dtype=torch.int32, device="cuda")
        sc = torch.empty((B, 1), dtype=torch.float32, device="cuda")
        frame = events_ms(lambda: L.check(lib.av_ctc_beam_frame_pass(ops.ptr(lp), T * V, V, None, ops.ptr(ws), need.value, B, T, V, blank, W,
                                                                     ops.stream())))
        whole = events_ms(lambda: L.check(lib.av_ctc_beam_search(ops.ptr(lp), T * V, V, None, ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                                                 ops.ptr(ws), need.value, B, T, V, blank, W, 1, ops.stream())))
        host = []
        for _ in range(args.host_repeats):
            t0 = time.perf_counter()
            ids_h = bs.prefix_beam_search(lp_h, W, blank)
            host.append((time.perf_counter() - t0) * 1e3)
        ids_d = bs.prefix_beam_search(lp, W, blank)
        same = sum(a == b for a, b in zip(ids_d, ids_h))
        fm, wm = statistics.median(frame), statistics.median(whole)
        lines += [f"W = {W:2d}  frame pass                 {fmt(frame)}",
                  f"W = {W:2d}  whole av_ctc_beam_search   {fmt(whole)}",
                  f"W = {W:2d}  search pass (whole - frame) median {wm - fm:8.3f} ms = {1e3 * (wm - fm) / T:.2f} us per frame; workspace {need.value} bytes",
                  f"W = {W:2d}  host path                  {fmt(host)}   device / host top-1 ids equal in {same} of {B}",
                  f"W = {W:2d}  whole vs greedy x{wm / statistics.median(greedy):.1f}, host vs device x{statistics.median(host) / wm:.0f}"]
        if W == 5:
            ok = wm < statistics.median(host)
    lines.append(f"sanity (device at W = 5 faster than the host path of this run): {'ok' if ok else 'FAILED'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
