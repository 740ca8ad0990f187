"""The fused Adam step with the weight EMA on one MI355X, on the trainable tensor set of the headline configuration (wav2vec2-large layers
6-9, fusion, CTC head: the shapes of the parameters with requires_grad, random values), against the plain step and against the only form
available before:
  (a) the plain step                                      (AvAdam, everything off),
  (b) the step with the EMA                               (AvAdam(ema_decay=0.999): the average moves inside the Adam launch),
  (c) (a) followed by torch._foreach_lerp_ over cloned EMA tensors (what torch.optim.swa_utils.AveragedModel runs after the step; blind to
      skipped steps and to the 16-bit shadows).
(a) and (b) are the same native call, av_adam_multi_wd, with and without an EMA decay.  Also (d), av_param_swap_multi: one exchange of parameters and averages, as evaluate() with eval_ema pays twice per call.
Alternating rounds in steady state within one process, device events, median and range; bytes computed from the shapes.  Writes
profiles/adam_ema_timing.txt; records, gates nothing.

    python tools/ema_timing.py [--out profiles/adam_ema_timing.txt] [--rounds 30]
"""
from __future__ import annotations

import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "multimodal-av-model_amd"

from clip_timing import fmt, timed, trainable_shapes  # noqa: E402  (the same shapes and the same clock as the clipping measurement)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_ema_timing.txt"))
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_timing: needs the GPU; there is nothing to time without it")
    optim = importlib.import_module(PKG + ".optim")
    shapes = trainable_shapes()
    n_el = sum(int(torch.Size(s).numel()) for s in shapes)
    g = torch.Generator(device="cuda").manual_seed(7)
    grads = [torch.randn(s, device="cuda", generator=g) * 1e-2 for s in shapes]

    def make(**kw):
        ps = [torch.randn(s, device="cuda", generator=g).requires_grad_(True) for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr
        return ps, optim.AvAdam(ps, lr=2e-5, **kw)

    pa, oa = make()
    pb, ob = make(ema_decay=0.999)
    pc, oc = make()
    ec = [p.detach().clone() for p in pc]
    pcd = [p.detach() for p in pc]

    def side_c():
        oc.step()
        torch._foreach_lerp_(ec, pcd, 1.0 - 0.999)

    for _ in range(5):
        oa.step(); ob.step(); side_c()
    torch.cuda.synchronize()
    a_ms, b_ms, c_ms, d_ms = [], [], [], []
    for _ in range(args.rounds):
        a_ms.append(timed(oa.step))
        b_ms.append(timed(ob.step))
        c_ms.append(timed(side_c))
    for _ in range(args.rounds // 2 * 2):                           # an even count: the parameters end where they were
        d_ms.append(timed(ob.swap_averaged))
    am, bm, cm, dm = (statistics.median(x) for x in (a_ms, b_ms, c_ms, d_ms))
    between = sum(a < b < c for a, b, c in zip(a_ms, b_ms, c_ms))
    gb = n_el * 4 / 1e9
    lines = [f"# tools/ema_timing.py on {torch.cuda.get_device_name(0)}.  {len(shapes)} trainable tensors of the headline configuration, "
             f"{n_el / 1e6:.1f} M elements ({gb:.3f} GB per fp32 copy), {sum(-(-torch.Size(s).numel() // oa.CHUNK) for s in shapes)} chunks.",
             f"# {args.rounds} alternating rounds (a, b, c) after 5 warm-up rounds, device events around each side, no bf16 shadows.",
             f"  (a) plain step                                  {fmt(a_ms)}   28 B/element = {7 * gb:.2f} GB moved (read p g m v, write p m v; "
             f"30 B with a 16-bit shadow)",
             f"  (b) step with the EMA, decay 0.999              {fmt(b_ms)}   36 B/element = {9 * gb:.2f} GB moved ((a) + read and write ema; "
             f"38 B with a shadow)",
             f"  (c) (a) then torch._foreach_lerp_               {fmt(c_ms)}   40 B/element = {10 * gb:.2f} GB moved ((a) + read p, read and write ema; "
             f"42 B with a shadow)",
             f"  (d) av_param_swap_multi (one exchange)          {fmt(d_ms)}   16 B/element = {4 * gb:.2f} GB moved (read and write p and ema) "
             f"at {4 * gb / max(dm, 1e-9) * 1e3:.0f} GB/s",
             f"  (b) - (a) {bm - am:.3f} ms = {2 * gb:.2f} GB more at {2 * gb / max(bm - am, 1e-9) * 1e3:.0f} GB/s plus one one-thread launch;  "
             f"(c) - (a) {cm - am:.3f} ms;  (b) / (c) x{bm / cm:.3f};  (a) < (b) < (c) in {between} of {args.rounds} rounds",
             f"  (a) {7 * gb / am * 1e3:.0f} GB/s, (b) {9 * gb / bm * 1e3:.0f} GB/s, (c) {10 * gb / cm * 1e3:.0f} GB/s;  "
             f"last EMA decay {float(ob.last_ema_decay):.6f}  EMA updates {ob.ema_step()}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
