"""The gradient-accumulation launch on one MI355X, on the trainable tensor set of the headline configuration (wav2vec2-large layers 6-9,
fusion, CTC head: the shapes of the parameters with requires_grad, random values), against the only form available before and against a
plain copy:
  (a) av_grad_accum_multi, every tensor in add mode       (acc = acc + grad: read grad, read acc, write acc = 12 B per element),
  (b) av_grad_accum_multi, every tensor in copy mode      (acc = grad: 8 B per element),
  (c) torch._foreach_add_(accs, grads) on the same tensors (12 B per element; it presupposes that somebody cloned the gradients out of the arenas),
  (d) one device-to-device copy of as many bytes as (b) moves (a flat tensor of all the elements).
(a) and (b) are the native call itself, on tables built once; what AvAdam.accumulate() adds on the host is one pointer-table comparison.
Alternating rounds in steady state within one process, device events, median and range; bytes computed from the shapes.  Two passes, as in
tools/adamw_timing.py: "device" queues each side behind a spinning kernel, so the events see its launches back to back, as they run behind
a backward pass; "as called" starts on an idle device, so the launch latency is inside the figure.  Writes profiles/grad_accum_timing.txt;
records, gates nothing.

    python tools/accum_timing.py [--out profiles/grad_accum_timing.txt] [--rounds 30]

AVAMD_LIB=<another build of libavhip.so> times that build instead (one whose accumulate kernel walks with chunk_walk<4>, say).
"""
from __future__ import annotations

import argparse
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = "multimodal-av-model_amd"


def main():
    from adamw_timing import timed_queued
    from clip_timing import fmt, timed, trainable_shapes
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum_timing.txt"))
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("accum_timing: needs the GPU; there is nothing to time without it")
    optim = importlib.import_module(PKG + ".optim"); ops = importlib.import_module(PKG + ".ops"); L = importlib.import_module(PKG + "._lib")
    shapes = trainable_shapes()
    numels = [int(torch.Size(s).numel()) for s in shapes]
    n_el, chunk, dev = sum(numels), optim.AvAdam.CHUNK, torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    grads = [torch.randn(s, device="cuda", generator=g) * 1e-2 for s in shapes]
    accs = [torch.zeros(s, device="cuda") for s in shapes]                       # (a) and (b)
    accs_c = [torch.zeros(s, device="cuda") for s in shapes]                     # (c)
    flat_src, flat_dst = torch.randn(n_el, device="cuda", generator=g), torch.empty(n_el, device="cuda")      # (d)

    ptrs = ops.h2d_async(np.asarray([x for gr, a in zip(grads, accs) for x in (gr.data_ptr(), a.data_ptr())], dtype=np.int64), dev)
    sizes, ct, cs, nch = optim._size_tables(numels, chunk, dev)
    modes = {m: ops.h2d_async(np.full(len(shapes), m, dtype=np.int32), dev) for m in (0, 1)}
    lib = L.lib()

    def accum(mode):
        def fn():
            L.check(lib.av_grad_accum_multi(ops.ptr(ptrs), ops.ptr(modes[mode]), ops.ptr(sizes), ops.ptr(ct), ops.ptr(cs), nch, chunk, ops.stream()),
                    "av_grad_accum_multi")
        return fn

    fns = {"a": accum(1), "b": accum(0), "c": lambda: torch._foreach_add_(accs_c, grads), "d": lambda: flat_dst.copy_(flat_src)}
    for _ in range(5):
        for name in "abcd":
            fns[name]()
    torch.cuda.synchronize()
    gb = n_el * 4 / 1e9
    moved = {"a": 3 * gb, "b": 2 * gb, "c": 3 * gb, "d": 2 * gb}
    label = {"a": "(a) av_grad_accum_multi, add mode   ", "b": "(b) av_grad_accum_multi, copy mode  ", "c": "(c) torch._foreach_add_             ",
             "d": "(d) device-to-device copy, one flat "}
    lines = [f"# tools/accum_timing.py on {torch.cuda.get_device_name(0)}, library {os.path.basename(L.LIB_PATH)}.  {len(shapes)} trainable tensors of "
             f"the headline configuration, {n_el / 1e6:.1f} M elements ({gb:.3f} GB of fp32 gradients), {nch} chunks of {chunk}.",
             f"# {args.rounds} alternating rounds (a, b, c, d) per pass after 5 warm-up rounds, device events around each side."]
    for title, clock in (("device (queued behind a spinning kernel)", timed_queued), ("as called (idle device: launch latency included)", timed)):
        ms = {k: [] for k in "abcd"}
        for _ in range(args.rounds):
            for name in "abcd":
                ms[name].append(clock(fns[name]))
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append(f"# {title}")
        for k in "abcd":
            lines.append(f"  {label[k]} {fmt(ms[k])}   {moved[k]:.3f} GB moved at {moved[k] / med[k] * 1e3:.0f} GB/s")
        wins = sum(a < c for a, c in zip(ms["a"], ms["c"]))
        lines.append(f"  (a) - (c) {med['a'] - med['c']:+.4f} ms, (a) / (c) x{med['a'] / med['c']:.3f}, (a) ahead of (c) in {wins} of {args.rounds} rounds; "
                     f"spread between equal rounds of (c) {max(ms['c']) - min(ms['c']):.4f} ms;  (b) - (d) {med['b'] - med['d']:+.4f} ms")
    fns["b"](); fns["a"]()                                                        # a copy, then an add: g + g, as torch computes it
    assert all(torch.equal(a, gr + gr) for a, gr in zip(accs, grads))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
