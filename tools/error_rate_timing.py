"""Word / character / token error counts on one MI355X: device events around av_error_counts (both launches; and around the same call
with every hypothesis marked absent, whose distance launch only writes -1: the expansion's share), the package's host path (numpy, wall
clock) and the plain Python loop of trainer.word_error_rate on the decoded strings of the same inputs (word level only: the yardstick
evaluate() uses today), in the same run.  Shapes: B 64, N 1 and B 64, N 8 with transcripts of about 80 characters through
tests/golden/tokenizer800.vocab, and one 4096 x 4096 pair at token level.  20 repeats after 3 warm-ups, median and range.  Writes
profiles/error_rate_timing.txt; records, gates nothing.

    python tools/error_rate_timing.py [--out profiles/error_rate_timing.txt] [--host-repeats 3]
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


def wall_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def fmt(ms):
    return f"median {statistics.median(ms):9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})"


def transcripts(tok, B, N, seed):
    """B references of about 80 characters (words of 1-4 pieces, the way the vocabulary spells text) and N noisy copies of each."""
    rng = np.random.default_rng(seed)
    V, sp = tok.vocab_size, tok.token_to_id["▁"]
    word_start = [i for i, p in enumerate(tok.id_to_token) if p.startswith("▁") and len(p) > 1]
    inner = [i for i, p in enumerate(tok.id_to_token) if i > sp and not p.startswith("▁") and not p.startswith("<")]
    refs, hyps = [], []
    for _ in range(B):
        r, n = [], 0
        while n < 80:
            w = [int(rng.choice(word_start))] + [int(rng.choice(inner)) for _ in range(int(rng.integers(0, 4)))]
            r += w
            n += sum(len(tok.id_to_token[i]) for i in w)
        refs.append(r)
        row = []
        for _ in range(N):
            h = [int(rng.choice(inner)) if rng.random() < 0.15 else i for i in r if rng.random() > 0.05]
            row.append(h)
        hyps.append(row)
    return refs, hyps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_rate_timing.txt"))
    ap.add_argument("--host-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("error_rate_timing: needs the GPU; there is nothing to time without it")
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops"); E = importlib.import_module(PKG + ".error_rate")
    T = importlib.import_module(PKG + ".utils.tokenizer"); bs = importlib.import_module(PKG + ".beam_search")
    wer = importlib.import_module(PKG + ".model.trainer").word_error_rate
    torch.set_num_threads(16)
    lib = L.lib()
    tok = T.Tokenizer(os.path.join(ROOT, "tests", "golden", "tokenizer800.vocab"))
    table = E.PieceTable.from_tokenizer(tok)
    off, chars = table.on("cuda")
    lines = [f"# tools/error_rate_timing.py on {torch.cuda.get_device_name(0)}.  device: events around av_error_counts (expansion + distance, inputs",
             "# and workspace resident), 20 repeats after 3 warm-ups; 'expansion' = the same call with every hypothesis marked absent, whose",
             "# distance launch only writes -1.  host path: error_rate.error_counts on host tensors (numpy; all three levels).  python loop:",
             "# trainer.word_error_rate on the decoded strings (word level only; the decode is not in the time).  wall clock, same run."]

    def device_case(ref, rl, hyp, hl, with_table, hyp_skip):
        B, Lr = ref.shape
        _, N, Lh = hyp.shape
        need = L.ll(0)
        mp = table.max_piece if with_table else 0
        L.check(lib.av_error_counts_workspace_bytes(B, N, Lr, Lh, mp, L.C.byref(need)))
        ws = torch.empty((need.value // 4 + 4,), dtype=torch.int32, device="cuda")
        out = torch.empty((B, N, 3, 4), dtype=torch.int32, device="cuda")
        rd, hd, rld, hld = ref.int().cuda(), hyp.int().cuda(), rl.long().cuda(), hl.long().cuda()
        absent = torch.full_like(hld, -1)
        o, c = (ops.ptr(off), ops.ptr(chars)) if with_table else (None, None)

        def run(lens):
            L.check(lib.av_error_counts(ops.ptr(rd), Lr, ops.ptr(rld), ops.ptr(hd), N * Lh, Lh, ops.ptr(lens), B, N, Lr, Lh, -1, hyp_skip, o, c,
                                        table.vocab_size if with_table else 0, mp, ops.ptr(out), ops.ptr(ws), need.value, ops.stream()))
        full = events_ms(lambda: run(hld))
        expand = events_ms(lambda: run(absent))
        run(hld)
        torch.cuda.synchronize()
        return full, expand, out.cpu(), need.value

    for B, N in ((64, 1), (64, 8)):
        refs, hyps = transcripts(tok, B, N, seed=80 + N)
        rt, rl = E._pad_rows(refs)
        flat, hl = E._pad_rows([h for row in hyps for h in row])
        ht, hl = flat.reshape(B, N, -1), torch.tensor(hl).reshape(B, N)
        rl = torch.tensor(rl)
        full, expand, got, need = device_case(rt, rl, ht, hl, True, tok.blank_id)
        want = None

        def host():
            nonlocal want
            want = E.error_counts(rt, ht, rl, hl, table=table, hyp_skip=tok.blank_id)
        host_ms = wall_ms(host, args.host_repeats)
        ref_s = [tok.decode(r) for r in refs]
        hyp_s = [[bs.fast_decode(h, tok) for h in row] for row in hyps]
        py_ms = wall_ms(lambda: [wer(ref_s, [row[n] for row in hyp_s]) for n in range(N)], args.host_repeats)
        w0 = wer(ref_s, [row[0] for row in hyp_s])
        rate = E.rates(got)
        fm, em, hm, pm = (statistics.median(x) for x in (full, expand, host_ms, py_ms))
        lines += [f"B {B} N {N}: references of {np.mean([len(s) for s in ref_s]):.0f} characters / {np.mean([len(s.split()) for s in ref_s]):.1f} words "
                  f"/ {np.mean([len(r) for r in refs]):.0f} ids on average, workspace {need} bytes",
                  f"  av_error_counts (3 levels)       {fmt(full)}",
                  f"  expansion (hypotheses absent)    {fmt(expand)}   distance by difference: {fm - em:.3f} ms",
                  f"  host path (3 levels)             {fmt(host_ms)}   device / host results equal: {bool(torch.equal(got, want))}",
                  f"  python loop (word level only)    {fmt(py_ms)}   WER {w0:.4f} == device {rate['word']['rate']:.4f}: {w0 == rate['word']['rate']}",
                  f"  host path vs device x{hm / fm:.0f}, python word loop vs device x{pm / fm:.1f}"]
    rng = np.random.default_rng(4096)
    ref = torch.from_numpy(rng.integers(0, 6, size=(1, 4096)))
    hyp = ref.clone()[:, None, :]
    noise = torch.from_numpy(rng.random(hyp.shape) < 0.3)
    hyp[noise] = torch.from_numpy(rng.integers(0, 6, size=int(noise.sum())))
    rl, hl = torch.tensor([4096]), torch.tensor([[4096]])
    full, expand, got, need = device_case(ref, rl, hyp, hl, False, -1)
    want = None

    def host_big():
        nonlocal want
        want = E.error_counts(ref, hyp, rl, hl)
    host_ms = wall_ms(host_big, args.host_repeats)
    r_s, h_s = " ".join(map(str, ref[0].tolist())), " ".join(map(str, hyp[0, 0].tolist()))
    py_ms = wall_ms(lambda: wer([r_s], [h_s]), 1)
    fm = statistics.median(full)
    lines += [f"one 4096 x 4096 pair, token level (no table), workspace {need} bytes",
              f"  av_error_counts                  {fmt(full)}   = {1e3 * fm / 4096:.2f} us per row of 4097 columns (one wave)",
              f"  expansion (hypothesis absent)    {fmt(expand)}",
              f"  host path                        {fmt(host_ms)}   device / host results equal: {bool(torch.equal(got, want))}",
              f"  python loop                      {fmt(py_ms)}   (one run)",
              f"  host path vs device x{statistics.median(host_ms) / fm:.2f}, python loop vs device x{statistics.median(py_ms) / fm:.0f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
