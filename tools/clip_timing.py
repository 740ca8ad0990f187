"""The fused Adam step with global-norm clipping and the learning-rate schedule on one MI355X, on the trainable tensor set of the headline
configuration (wav2vec2-large layers 6-9, fusion, CTC head: the shapes of the parameters with requires_grad, random values), against the
plain step and against the only form available before:
  (a) the plain step                                      (AvAdam, everything off),
  (b) the step with clipping and schedule                 (AvAdam(max_grad_norm=1.0, warmup_steps=10, total_steps=1000)),
  (c) torch.nn.utils.clip_grad_norm_ followed by (a).
Every side is one av_adam_multi_wd call, with zeros for what is off.  Alternating triples in steady state within one process, device events, median and range; bytes computed from the shapes.  Writes
profiles/adam_clip_timing.txt; records, gates nothing.

    python tools/clip_timing.py [--out profiles/adam_clip_timing.txt] [--rounds 30]
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
PKG = "multimodal-av-model_amd"


def fmt(ms):
    return f"median {statistics.median(ms):8.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def trainable_shapes():
    """Shapes of the parameters the headline configuration trains (bench.py: build_trainer's freeze policy), built on the host."""
    init = importlib.import_module(PKG + ".utils.init"); enc = importlib.import_module(PKG + ".model.encoder")
    fm = importlib.import_module(PKG + ".model.fusion_module"); dm = importlib.import_module(PKG + ".model.decoder")
    cfg = dict(init.W2V2_LARGE)
    ae = enc.AudioEncoder(dict(cfg), freeze=True)
    for n, p in ae.model.named_parameters():
        p.requires_grad = any(f"encoder.layers.{i}." in n for i in range(6, 10))
    fu = fm.CrossAttentionFusion(512, cfg["hidden_size"], 512)
    de = dm.CTCDecoder(1024, 800, 3)
    return [tuple(p.shape) for m in (ae, fu, de) for p in m.parameters() if p.requires_grad]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_clip_timing.txt"))
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_timing: needs the GPU; there is nothing to time without it")
    optim = importlib.import_module(PKG + ".optim")
    shapes = trainable_shapes()
    n_el = sum(int(torch.Size(s).numel()) for s in shapes)
    g = torch.Generator(device="cuda").manual_seed(7)
    grads = [torch.randn(s, device="cuda", generator=g) * 1e-2 for s in shapes]

    def make(**kw):
        ps = [torch.randn(s, device="cuda", generator=g).requires_grad_(True) for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()                                     # (c) rescales its gradients in place: every side owns a copy
        return ps, optim.AvAdam(ps, lr=2e-5, **kw)

    pa, oa = make()
    pb, ob = make(max_grad_norm=1.0, warmup_steps=10, total_steps=1000)
    pc, oc = make()

    def side_c():
        torch.nn.utils.clip_grad_norm_(pc, 1.0)
        oc.step()

    def refill():                                                   # untimed: (c)'s gradients shrink with every clip, put them back
        for p, gr in zip(pc, grads):
            p.grad.copy_(gr)

    for _ in range(5):
        oa.step(); ob.step(); refill(); side_c()
    torch.cuda.synchronize()
    a_ms, b_ms, c_ms = [], [], []
    for _ in range(args.rounds):
        refill()
        a_ms.append(timed(oa.step))
        b_ms.append(timed(ob.step))
        c_ms.append(timed(side_c))
    wins = sum(b < c for b, c in zip(b_ms, c_ms))
    am, bm, cm = statistics.median(a_ms), statistics.median(b_ms), statistics.median(c_ms)
    gb = n_el * 4 / 1e9
    lines = [f"# tools/clip_timing.py on {torch.cuda.get_device_name(0)}.  {len(shapes)} trainable tensors of the headline configuration, "
             f"{n_el / 1e6:.1f} M elements ({gb:.3f} GB of fp32 gradients), {sum(-(-torch.Size(s).numel() // oa.CHUNK) for s in shapes)} chunks.",
             f"# {args.rounds} alternating rounds (a, b, c) after 5 warm-up rounds, device events around each side, no bf16 shadows.",
             f"  (a) plain step                                  {fmt(a_ms)}   ~{7 * gb:.2f} GB moved (read p g m v, write p m v)",
             f"  (b) step with clipping + schedule               {fmt(b_ms)}   ~{8 * gb:.2f} GB moved ((a) + one read of g)",
             f"  (c) clip_grad_norm_ then (a)                    {fmt(c_ms)}   ~{10 * gb:.2f} GB moved ((a) + read g, read g, write g)",
             f"  (b) - (a) {bm - am:.3f} ms = one read of the gradients at {gb / max(bm - am, 1e-9) * 1e3:.0f} GB/s plus two small launches;  "
             f"(b) / (c) x{bm / cm:.3f};  (b) ahead of (c) in {wins} of {args.rounds} rounds",
             f"  last norm {float(ob.last_grad_norm):.6f}  clip coefficient {float(ob.last_clip_coef):.6f}  lr multiplier {float(ob.last_lr_mult):.6f}  "
             f"schedule step {ob.schedule_step()}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
