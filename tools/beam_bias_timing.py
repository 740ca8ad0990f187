"""CTC prefix beam search with contextual phrase biasing on one MI355X: device events around whole calls (frame pass + search pass) at
B 64, T 199, V 800, W 8, tokens 9, in ONE run: av_ctc_beam_search, av_ctc_beam_search_lm (trigram), and av_ctc_beam_search_bias with and
without that language model for phrase sets of 10 and of 1000 phrases (all three are instantiations of one kernel, csrc/ctc_beam.hip:
template <int F>).  20 repeats after 3 warm-ups, median and range, profiler off; the entry points are timed in alternation, round robin,
and the whole round robin is run twice: the difference between the two medians of one entry point is the spread between equal runs.
With --parent-lib (a libavhip.so built from the commit before this feature) that library's av_ctc_beam_search and av_ctc_beam_search_lm
take part in the same round robin, so that today's two entry points are compared with their own earlier times on the same box in the same
minute.  There is no gate: the file records the ratios.  Writes profiles/ctc_beam_bias_timing.txt.

    python tools/beam_bias_timing.py [--out profiles/ctc_beam_bias_timing.txt] [--parent-lib PATH]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import os
import statistics
import sys

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


def phrase_set(n, V, blank, seed):
    """n distinct random phrases of 2..8 non-blank ids."""
    rng = np.random.default_rng(seed)
    nb = [c for c in range(V) if c != blank]
    out = set()
    while len(out) < n:
        out.add(tuple(nb[int(x)] for x in rng.integers(len(nb), size=int(rng.integers(2, 9)))))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_beam_bias_timing.txt"))
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_bias_timing: needs the GPU; there is nothing to time without it")
    import beam_ref as R
    import lm_ref as LR
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops"); bs = importlib.import_module(PKG + ".beam_search")
    LM = importlib.import_module(PKG + ".lm"); BIAS = importlib.import_module(PKG + ".bias")
    torch.set_num_threads(16)
    B, T, V, W, K, blank = 64, 199, 800, 8, 9, 0
    lp = torch.from_numpy(np.stack([R.make_log_probs(31000 + b, T, V, blank) for b in range(B)])).cuda()
    lib = L.lib()
    libs = {"this tree": lib}
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("av_ctc_beam_search", "av_ctc_beam_search_lm"):
            getattr(parent, name).argtypes = L.SIGNATURES[name]
            getattr(parent, name).restype = ctypes.c_int
        libs["parent"] = parent
    lm = LM.NGramLM.from_corpus(LR.make_corpus(7, 400, V, blank, lo=8, hi=30), V, blank, order=3)
    d = lm.to_device("cuda")
    need, nb = L.ll(0), L.ll(0)
    L.check(lib.av_ctc_beam_workspace_bytes(B, T, V, W, L.C.byref(need)))
    L.check(lib.av_ctc_beam_lm_workspace_bytes(B, T, V, W, K, L.C.byref(nb)))
    ws = torch.empty(((max(need.value, nb.value) + 7) // 8,), dtype=torch.int64, device="cuda")
    out = torch.empty((B, 1, T), dtype=torch.int32, device="cuda")
    cnt, kb = torch.empty((B, 1), dtype=torch.int32, device="cuda"), torch.empty((B, 1), dtype=torch.int32, device="cuda")
    sc, gl = torch.empty((B, 1), dtype=torch.float32, device="cuda"), torch.empty((B, 1), dtype=torch.float32, device="cuda")
    head = (ops.ptr(lp), T * V, V, None, ops.ptr(out), ops.ptr(cnt), ops.ptr(sc))
    lm_args = (ops.ptr(d.unigrams), ops.ptr(d.table), d.slots, d.order, d.vocab_size, d.bos, d.probe_bound, 0.5, 0.0)
    no_lm = (None, None, 0, 0, 0, -1, 0, 0.0, 0.0)

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"status {rc}: {lib.av_last_error().decode('utf-8', 'replace')}")
    runs = {}
    for who, l in libs.items():
        runs[f"av_ctc_beam_search ({who})"] = (lambda l=l: ok(l.av_ctc_beam_search(*head, ops.ptr(ws), need.value, B, T, V, blank, W, 1, ops.stream())))
        runs[f"av_ctc_beam_search_lm ({who})"] = (lambda l=l: ok(l.av_ctc_beam_search_lm(*head, ops.ptr(gl), ops.ptr(ws), nb.value, B, T, V, blank, W, 1,
                                                                                        K, *lm_args, ops.stream())))
    lines = [f"# tools/beam_bias_timing.py on {torch.cuda.get_device_name(0)}: B {B}, T {T}, V {V}, W {W}, tokens {K}, float32 log-probs from the tests' generator,",
             "# full lengths, trigram from 400 sentences (alpha 0.5, beta 0), bias weight 2.0; events, 20 repeats after 3 warm-ups, all entry points",
             "# in alternation (round robin), whole calls (frame pass + search pass); the round robin runs twice: pass 1 / pass 2 of one entry point",
             "# are equal runs, their difference is the spread.",
             f"language model: {len(lm.table)} n-grams of order >= 2, {d.slots} slots = {d.slots * 16 / 2**20:.1f} MiB, probe bound {d.probe_bound}"]
    for n in (10, 1000):
        cb = BIAS.ContextBias.from_phrases(phrase_set(n, V, blank, n), vocab_size=V, blank=blank)
        db = cb.to_device("cuda")
        lines.append(f"phrase set {n}: {db.node_count} nodes, {db.slots} edge slots = {db.slots * 16 / 2**10:.1f} KiB, probe bound {db.probe_bound}")
        tail = (ops.ptr(db.nodes), ops.ptr(db.edges), db.node_count, db.slots, db.probe_bound, 2.0, ops.stream())
        for what, la in (("no lm", no_lm), ("with lm", lm_args)):
            runs[f"av_ctc_beam_search_bias {n} phrases, {what}"] = (lambda la=la, tail=tail: ok(lib.av_ctc_beam_search_bias(
                *head, ops.ptr(gl), ops.ptr(kb), ops.ptr(ws), nb.value, B, T, V, blank, W, 1, K, *la, *tail)))
    med = {}
    for rep in (1, 2):
        for _ in range(3):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(20):
            for k, fn in runs.items():
                times[k].append(one_ms(fn))
        lines.append(f"pass {rep}")
        for k, ms in times.items():
            med.setdefault(k, []).append(statistics.median(ms))
            lines.append(f"  {k:52s} {fmt(ms)}")
    spread = max(abs(a - b) / min(a, b) for a, b in med.values())
    m = {k: min(v) for k, v in med.items()}
    lines.append(f"largest spread between the two passes of one entry point: {100 * spread:.1f} %")
    plain, fused = m["av_ctc_beam_search (this tree)"], m["av_ctc_beam_search_lm (this tree)"]
    for n in (10, 1000):
        lines.append(f"biased with lm / av_ctc_beam_search_lm, {n:4d} phrases: x{m[f'av_ctc_beam_search_bias {n} phrases, with lm'] / fused:.2f};  "
                     f"biased without lm / av_ctc_beam_search: x{m[f'av_ctc_beam_search_bias {n} phrases, no lm'] / plain:.2f}")
    if args.parent_lib:
        lines.append(f"this tree / parent: av_ctc_beam_search x{plain / m['av_ctc_beam_search (parent)']:.3f}, "
                     f"av_ctc_beam_search_lm x{fused / m['av_ctc_beam_search_lm (parent)']:.3f}")
    cb = BIAS.ContextBias.from_phrases(phrase_set(1000, V, blank, 1000), vocab_size=V, blank=blank)
    ids_b = bs.prefix_beam_search(lp, W, blank, tokens=K, bias=cb, bias_weight=2.0)
    ids_p = bs.prefix_beam_search(lp, W, blank)
    lines.append(f"1000 random phrases at weight 2.0 change the top hypothesis of {sum(a != b for a, b in zip(ids_b, ids_p))} of {B} utterances")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
