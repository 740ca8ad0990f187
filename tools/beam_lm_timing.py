"""CTC prefix beam search with n-gram shallow fusion on one MI355X: device events around av_ctc_beam_search_lm at B 64, T 199, V 800, W 8
for tokens K = 9 and K = 32 and two trigram tables (a small one that fits L2 and one of tens of MB), in alternation with
av_ctc_beam_search at the same shape (both are instantiations of one kernel, csrc/ctc_beam.hip: template <int F>)
and next to the package's host path.  20 repeats after 3 warm-ups, median and range, profiler off.  There is no gate: the file records
the ratio and the per-frame cost.  Writes profiles/ctc_beam_lm_timing.txt.

    python tools/beam_lm_timing.py [--out profiles/ctc_beam_lm_timing.txt] [--big-sentences 60000]
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


def one_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def fmt(ms):
    return f"median {statistics.median(ms):8.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_beam_lm_timing.txt"))
    ap.add_argument("--big-sentences", type=int, default=60000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_lm_timing: needs the GPU; there is nothing to time without it")
    import beam_ref as R
    import lm_ref as LR
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops"); bs = importlib.import_module(PKG + ".beam_search")
    LM = importlib.import_module(PKG + ".lm")
    torch.set_num_threads(16)
    B, T, V, W, blank = 64, 199, 800, 8, 0
    lp_h = torch.from_numpy(np.stack([R.make_log_probs(31000 + b, T, V, blank) for b in range(B)]))
    lp = lp_h.cuda()
    lib = L.lib()
    lines = [f"# tools/beam_lm_timing.py on {torch.cuda.get_device_name(0)}: B {B}, T {T}, V {V}, W {W}, float32 log-probs from the tests' generator, full lengths,",
             "# alpha 0.5, beta 0; events, 20 repeats after 3 warm-ups, the fused and the plain search timed in alternation; whole calls (frame pass + search pass)."]
    need = L.ll(0)
    L.check(lib.av_ctc_beam_workspace_bytes(B, T, V, W, L.C.byref(need)))
    ws0 = torch.empty(((need.value + 7) // 8,), dtype=torch.int64, device="cuda")
    out = torch.empty((B, 1, T), dtype=torch.int32, device="cuda")
    cnt = torch.empty((B, 1), dtype=torch.int32, device="cuda")
    sc, gl = torch.empty((B, 1), dtype=torch.float32, device="cuda"), torch.empty((B, 1), dtype=torch.float32, device="cuda")
    plain = lambda: L.check(lib.av_ctc_beam_search(ops.ptr(lp), T * V, V, None, ops.ptr(out), ops.ptr(cnt), ops.ptr(sc), ops.ptr(ws0), need.value,
                                                   B, T, V, blank, W, 1, ops.stream()))
    for name, sentences in (("small", 400), ("large", args.big_sentences)):
        lm = LM.NGramLM.from_corpus(LR.make_corpus(7, sentences, V, blank, lo=8, hi=30), V, blank, order=3)
        d = lm.to_device("cuda")
        lines.append(f"table {name}: trigram from {sentences} sentences, {len(lm.table)} n-grams of order >= 2, {d.slots} slots = {d.slots * 16 / 2**20:.1f} MiB, "
                     f"probe bound {d.probe_bound}")
        for K in (9, 32):
            nb = L.ll(0)
            L.check(lib.av_ctc_beam_lm_workspace_bytes(B, T, V, W, K, L.C.byref(nb)))
            ws = torch.empty(((nb.value + 7) // 8,), dtype=torch.int64, device="cuda")
            fused = lambda: L.check(lib.av_ctc_beam_search_lm(ops.ptr(lp), T * V, V, None, ops.ptr(out), ops.ptr(cnt), ops.ptr(sc), ops.ptr(gl),
                                                              ops.ptr(ws), nb.value, B, T, V, blank, W, 1, K, ops.ptr(d.unigrams), ops.ptr(d.table),
                                                              d.slots, d.order, d.vocab_size, d.bos, d.probe_bound, 0.5, 0.0, ops.stream()))
            for _ in range(3):
                fused(); plain()
            torch.cuda.synchronize()
            tf, tp = [], []
            for _ in range(20):
                tf.append(one_ms(fused)); tp.append(one_ms(plain))
            mf, mp = statistics.median(tf), statistics.median(tp)
            lines += [f"  K = {K:2d}  av_ctc_beam_search_lm  {fmt(tf)}",
                      f"  K = {K:2d}  av_ctc_beam_search     {fmt(tp)}   (tokens = W + 1 = {W + 1}, no language model)",
                      f"  K = {K:2d}  fused / plain x{mf / mp:.2f}; fused - plain = {1e3 * (mf - mp) / T:.2f} us per frame"]
            if name == "small" and K == 9:
                t0 = time.perf_counter()
                ids_h = bs.prefix_beam_search(lp_h, W, blank, lm=lm, tokens=K)
                host = (time.perf_counter() - t0) * 1e3
                ids_d = bs.prefix_beam_search(lp, W, blank, lm=lm, tokens=K)
                lines.append(f"  K = {K:2d}  host path {host:.0f} ms = x{host / mf:.0f} the device; device / host top-1 ids equal in "
                             f"{sum(a == b for a, b in zip(ids_d, ids_h))} of {B}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
