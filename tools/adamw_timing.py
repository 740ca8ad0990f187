"""The fused Adam step with decoupled weight decay on one MI355X, on the trainable tensor set of the headline configuration (wav2vec2-large
layers 6-9, fusion, CTC head: the shapes of the parameters with requires_grad, random values), against the plain step and against the only
form available before:
  (a) the plain step                                      (AvAdam, everything off: the kernels of av_adam_multi),
  (b) the step with weight decay                          (AvAdam(weight_decay=0.01): av_adam_multi_wd with a decay table),
  (c) torch._foreach_mul_ over the decayed tensors, then (a).
Tensors with ndim <= 1 are not decayed on either side (AvAdam's default rule).  Alternating triples in steady state within one process, device
events, median and range; bytes computed from the shapes.  Two passes: "as called" has the events around the call on an idle device, so it
includes the host's preparation of the step, during which the device waits (and during which (c)'s _foreach_mul_ already runs); "device"
queues the call behind a spinning kernel, so the events see the launches back to back.  Writes profiles/adam_wd_timing.txt; records, gates
nothing.

    python tools/adamw_timing.py [--out profiles/adam_wd_timing.txt] [--rounds 30] [--order abc]

--order: the order of the three sides within a round (a side's time depends a little on what ran before it).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = "multimodal-av-model_amd"
LR, WD = 2e-5, 0.01


def timed_queued(fn):
    """Device time of fn's launches alone: they are queued while a spinning kernel keeps the device busy."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(4_000_000)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    from clip_timing import fmt, timed, trainable_shapes
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_wd_timing.txt"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--order", default="abc", choices=["abc", "acb", "bac", "bca", "cab", "cba"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw_timing: needs the GPU; there is nothing to time without it")
    optim = importlib.import_module(PKG + ".optim")
    shapes = trainable_shapes()
    n_el = sum(int(torch.Size(s).numel()) for s in shapes)
    n_dec = sum(int(torch.Size(s).numel()) for s in shapes if len(s) > 1)
    g = torch.Generator(device="cuda").manual_seed(7)
    grads = [torch.randn(s, device="cuda", generator=g) * 1e-2 for s in shapes]

    def make(**kw):
        ps = [torch.randn(s, device="cuda", generator=g).requires_grad_(True) for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr
        return ps, optim.AvAdam(ps, lr=LR, **kw)

    pa, oa = make()
    pb, ob = make(weight_decay=WD)
    pc, oc = make()
    decayed = [p.data for p in pc if p.ndim > 1]

    def side_c():
        torch._foreach_mul_(decayed, 1.0 - LR * WD)
        oc.step()

    for _ in range(5):
        oa.step(); ob.step(); side_c()
    torch.cuda.synchronize()
    fns = {"a": oa.step, "b": ob.step, "c": side_c}
    gb, gb_dec = n_el * 4 / 1e9, n_dec * 4 / 1e9
    assert all(pl.wd is not None for pl in ob._plans.values()) and all(pl.wd is None for pl in oa._plans.values())
    lines = [f"# tools/adamw_timing.py on {torch.cuda.get_device_name(0)}.  {len(shapes)} trainable tensors of the headline configuration, "
             f"{n_el / 1e6:.1f} M elements ({gb:.3f} GB of fp32 parameters), {n_dec / 1e6:.1f} M of them in tensors with ndim > 1 (decayed), "
             f"{sum(-(-torch.Size(s).numel() // oa.CHUNK) for s in shapes)} chunks.",
             f"# {args.rounds} alternating rounds ({', '.join(args.order)}) per pass after 5 warm-up rounds, device events around each side, no bf16 "
             f"shadows, lr {LR}, weight_decay {WD}."]
    for title, clock in (("as called (idle device: host preparation included)", timed), ("device (queued behind a spinning kernel)", timed_queued)):
        ms = {"a": [], "b": [], "c": []}
        for _ in range(args.rounds):
            for name in args.order:
                ms[name].append(clock(fns[name]))
        am, bm, cm = (statistics.median(ms[k]) for k in "abc")
        wins = sum(b < c for b, c in zip(ms["b"], ms["c"]))
        lines += [f"# {title}",
                  f"  (a) plain step (kernels of av_adam_multi)       {fmt(ms['a'])}   ~{7 * gb:.2f} GB moved (read p g m v, write p m v)",
                  f"  (b) av_adam_multi_wd with the decay table       {fmt(ms['b'])}   ~{7 * gb:.2f} GB moved (the same bytes, + {len(shapes) * 4} B of table)",
                  f"  (c) _foreach_mul_ then (a)                      {fmt(ms['c'])}   ~{7 * gb + 2 * gb_dec:.2f} GB moved ((a) + read p, write p of the decayed)",
                  f"  (b) - (a) {bm - am:+.3f} ms ({(bm / am - 1) * 100:+.2f} %);  (c) - (a) {cm - am:+.3f} ms for 8 B per decayed element "
                  f"({2 * gb_dec:.2f} GB) and the launches of _foreach_mul_;  (b) / (c) x{bm / cm:.3f};  (b) ahead of (c) in {wins} of {args.rounds} rounds"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
