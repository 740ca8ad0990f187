"""CTC confidences on one MI355X at B 128 / T 100 / V 800, device events, reported and not gated:
  the frame pass (av_ctc_frame_conf, every method) against a device-to-device copy of the same bytes (the floor of a pass that reads the
    block once) and against the torch composition of the same law (max, sub, exp, pow, sum, log, ...);
  av_ctc_greedy_timed against what it fuses: av_ctc_greedy + av_ctc_align on its ids + av_ctc_frame_conf + av_ctc_span_conf.
The candidates of a group run in alternating rounds (one call each per round, 20 rounds after 3 warm-up rounds): whatever drifts on the
device drifts for all of them.  Writes profiles/confidence_timing.txt.

    python tools/confidence_timing.py [--out profiles/confidence_timing.txt]
"""
from __future__ import annotations

import argparse
import importlib
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "multimodal-av-model_amd"


def rounds_ms(fns, rounds=20, warmup=3):
    """{name: fn} -> {name: [ms]}: every round times each candidate once, in turn."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def fmt(ms):
    return f"median {statistics.median(ms) * 1e3:8.1f} us  (min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f})"


def torch_law(lp, method, alpha):
    """The frame law as a composition of torch kernels (what a user without the kernel would write)."""
    V = lp.shape[-1]
    d = lp - lp.amax(-1, keepdim=True)
    e = d.exp()
    s = e.sum(-1)
    if method == "max_prob":
        c = (V / s - 1) / (V - 1)
    elif method == "entropy":
        c = 1 + ((e * d).sum(-1) / s - s.log()) / math.log(V)
    else:
        u = V ** (1 - alpha)
        c = ((alpha * d).exp().sum(-1) / s.pow(alpha) - u) / (1 - u)
    return c.clamp(0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "confidence_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("confidence_timing: needs the GPU; there is nothing to time without it")
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops")
    C = importlib.import_module(PKG + ".confidence"); A = importlib.import_module(PKG + ".align"); lib = L.lib()
    B, T, V, blank = 128, 100, 800, 0
    g = torch.Generator().manual_seed(0)
    logits = 3 * torch.randn(B, T, V, generator=g)
    logits[:, :, blank] += 5.0                                      # the blank wins most frames, as in a trained CTC head
    lp = torch.log_softmax(logits, -1).cuda()
    dst = torch.empty_like(lp)
    mb = lp.numel() * 4 / 1e6
    lines = [f"# tools/confidence_timing.py on {torch.cuda.get_device_name(0)}: float32 log-probs [B {B}][T {T}][V {V}] = {mb:.1f} MB, full lengths;",
             "# device events, alternating rounds (one call of each candidate per round), 20 rounds after 3 warm-up rounds.  Reported, not gated."]
    conf = torch.empty((B, T), dtype=torch.float32, device="cuda")
    for method in ("tsallis", "entropy", "max_prob"):
        m = L.CONF_METHODS[method]
        r = rounds_ms({
            "copy": lambda: dst.copy_(lp),
            "kernel": lambda: L.check(lib.av_ctc_frame_conf(ops.ptr(lp), T * V, V, None, B, T, V, m, 0.33, ops.ptr(conf), ops.stream())),
            "torch": lambda: torch_law(lp, method, 0.33)})
        k, c, t = (statistics.median(r[x]) for x in ("kernel", "copy", "torch"))
        dev = float((conf - torch_law(lp, method, 0.33)).abs().max())
        lines += [f"frame pass, {method}" + (" alpha 0.33" if method == "tsallis" else ""),
                  f"  device-to-device copy (floor)    {fmt(r['copy'])}",
                  f"  av_ctc_frame_conf                {fmt(r['kernel'])}   = {mb / k / 1e3:.2f} TB/s read, x{k / c:.2f} of the copy",
                  f"  torch composition                {fmt(r['torch'])}   x{t / k:.1f} of the kernel; max |kernel - torch| {dev:.1e}"]
    ids = torch.empty((B, T), dtype=torch.int32, device="cuda")
    cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    spans = torch.empty((B, T, 2), dtype=torch.int32, device="cuda")
    tok = torch.empty((B, T), dtype=torch.float32, device="cuda")
    m, a = L.CONF_METHODS["tsallis"], L.CONF_AGGREGATIONS["min"]
    il = torch.full((B,), T, dtype=torch.long, device="cuda")

    def fused():
        L.check(lib.av_ctc_greedy_timed(ops.ptr(lp), T * V, V, None, B, T, V, blank, m, 0.33, a, ops.ptr(ids), ops.ptr(cnt), ops.ptr(spans),
                                        ops.ptr(tok), ops.ptr(conf), ops.stream()))
    fused()
    Lmax = int(cnt.max())                                           # the separate path sizes its lattice for the longest hypothesis
    S_max = 2 * Lmax + 1
    need = L.ll(0)
    L.check(lib.av_ctc_align_workspace_bytes(B, T, S_max, L.C.byref(need)))
    ws = torch.empty(((need.value + 3) // 4,), dtype=torch.int32, device="cuda")
    ids2, cnt2 = torch.empty_like(ids), torch.empty_like(cnt)
    states = torch.empty((B, T), dtype=torch.int32, device="cuda")
    spans2 = torch.empty((B, Lmax, 2), dtype=torch.int32, device="cuda")
    tok2 = torch.empty((B, Lmax), dtype=torch.float32, device="cuda")
    tsc = torch.empty((B, Lmax), dtype=torch.float32, device="cuda")
    score = torch.empty((B,), dtype=torch.float32, device="cuda")
    conf2 = torch.empty_like(conf)

    def greedy():
        L.check(lib.av_ctc_greedy(ops.ptr(lp), None, ops.ptr(ids2), ops.ptr(cnt2), B, T, V, blank, ops.stream()))

    def align():
        tg = ids2[:, :Lmax].long()                                  # the glue the separate path needs: int64 labels and lengths
        L.check(lib.av_ctc_align(ops.ptr(lp), T * V, V, ops.ptr(tg), Lmax, ops.ptr(il), ops.ptr(cnt2.long()), B, T, V, S_max, blank,
                                 ops.ptr(states), ops.ptr(spans2), ops.ptr(tsc), ops.ptr(score), ops.ptr(ws), need.value, ops.stream()))

    def frame():
        L.check(lib.av_ctc_frame_conf(ops.ptr(lp), T * V, V, None, B, T, V, m, 0.33, ops.ptr(conf2), ops.stream()))

    def span():
        L.check(lib.av_ctc_span_conf(ops.ptr(conf2), ops.ptr(spans2), None, B, T, Lmax, a, ops.ptr(tok2), ops.stream()))

    def separate():
        greedy(); align(); frame(); span()
    r = rounds_ms({"fused": fused, "separate": separate, "greedy": greedy, "align": align, "frame": frame, "span": span})
    fused(); separate(); torch.cuda.synchronize()
    same = (torch.equal(ids, ids2) and torch.equal(cnt, cnt2) and torch.equal(spans[:, :Lmax], spans2)
            and torch.equal(tok[:, :Lmax].view(torch.int32), tok2.view(torch.int32)) and torch.equal(conf.view(torch.int32), conf2.view(torch.int32)))
    f, s = statistics.median(r["fused"]), statistics.median(r["separate"])
    lines += [f"greedy decode with times and confidences (tsallis 0.33, min), longest hypothesis {Lmax} tokens",
              f"  av_ctc_greedy_timed              {fmt(r['fused'])}",
              f"  the four separate calls          {fmt(r['separate'])}   x{s / f:.2f} of the fused kernel",
              f"    av_ctc_greedy                  {fmt(r['greedy'])}",
              f"    av_ctc_align (+ label casts)   {fmt(r['align'])}",
              f"    av_ctc_frame_conf              {fmt(r['frame'])}",
              f"    av_ctc_span_conf               {fmt(r['span'])}",
              f"  ids, lengths, spans, token and frame confidences bit-identical between the two: {same}"]
    g2 = C.greedy_timed(lp, blank)
    al = A.forced_align(lp, g2.ids.clamp_min(0), None, g2.lengths, blank=blank)
    lines.append(f"  spans equal forced_align's on all {B} utterances: {bool(torch.equal(al.spans, g2.spans))}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
