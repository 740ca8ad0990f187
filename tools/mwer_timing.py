"""The n-best CTC kernels on one MI355X against the only form available before them: av_ctc_nbest_fwd + _bwd on [B, T, V] log-probs against
av_ctc_loss_fwd + _bwd on log_probs.repeat_interleave(N, 0), INCLUDING the expanding copy and the sum of the [B N, T, V] gradient over N
(every hypothesis weighted by its g in the kernel, as the n-best form does).  Shape: B = 128 utterances (the step's 2B), T = 100, V = 800,
N = 4 and 8 hypotheses of about 20 tokens in rows of width T (the beam kernel's block).  Alternating pairs in steady state, device events,
median and range; bytes moved computed from the shapes; the two workspaces' sizes.  Writes profiles/ctc_mwer_timing.txt; records, gates
nothing.

    python tools/mwer_timing.py [--out profiles/ctc_mwer_timing.txt] [--pairs 30]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_mwer_timing.txt"))
    ap.add_argument("--pairs", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mwer_timing: needs the GPU; there is nothing to time without it")
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops")
    lib = L.lib()
    B, T, V, blank = 128, 100, 800, 3
    S_max = 2 * T + 1
    lines = [f"# tools/mwer_timing.py on {torch.cuda.get_device_name(0)}.  B {B} T {T} V {V}, hypotheses of 15-25 tokens in rows of width T (S_max {S_max}).",
             f"# n-best: av_ctc_nbest_fwd + av_ctc_nbest_bwd.  composition: repeat_interleave(N, 0) of the log-probs, av_ctc_loss_fwd + _bwd on B N",
             f"# items, sum of the [B, N, T, V] gradient over N.  {args.pairs} alternating pairs after 5 warm-up pairs, device events around each side."]
    for N in (4, 8):
        g = torch.Generator().manual_seed(900 + N)
        lp = torch.log_softmax(torch.randn(B, T, V, generator=g), -1).cuda()
        lens = torch.randint(15, 26, (B, N), generator=g)
        ids = torch.randint(4, V, (B, N, T), generator=g).to(torch.int32).cuda()
        il = torch.randint(80, T + 1, (B,), generator=g).cuda()
        gn = (torch.rand(B, N, generator=g) * 2 - 1).cuda()
        lens_d = lens.cuda()
        nll = torch.empty((B, N), dtype=torch.float32, device="cuda")
        la = torch.empty((B, N, T, S_max), dtype=torch.float32, device="cuda")
        lb = torch.empty_like(la)
        grad = torch.empty((B, T, V), dtype=torch.float32, device="cuda")
        # the composition's operands: int64 targets [B N, T], lengths per item, workspaces of the same size
        tg = ids.long().reshape(B * N, T)
        tl = lens_d.reshape(B * N)
        il_x = il.repeat_interleave(N)
        nll_x = torch.empty((B * N,), dtype=torch.float32, device="cuda")
        grad_x = torch.empty((B * N, T, V), dtype=torch.float32, device="cuda")
        gn_x = gn.reshape(B * N).contiguous()
        st = ops.stream()

        def nbest():
            L.check(lib.av_ctc_nbest_fwd(ops.ptr(lp), T * V, V, ops.ptr(ids), N * T, T, ops.ptr(lens_d), ops.ptr(il), B, N, T, V, S_max, blank,
                                         ops.ptr(nll), ops.ptr(la), ops.ptr(lb), st), "av_ctc_nbest_fwd")
            L.check(lib.av_ctc_nbest_bwd(ops.ptr(lp), T * V, V, ops.ptr(ids), N * T, T, ops.ptr(lens_d), ops.ptr(il), B, N, T, V, S_max, blank,
                                         ops.ptr(nll), ops.ptr(la), ops.ptr(lb), ops.ptr(gn), ops.ptr(grad), st), "av_ctc_nbest_bwd")
            return grad

        def composition():
            lp_x = lp.repeat_interleave(N, 0)
            L.check(lib.av_ctc_loss_fwd(ops.ptr(lp_x), T * V, V, ops.ptr(tg), T, ops.ptr(il_x), ops.ptr(tl), B * N, T, V, S_max, blank, 0,
                                        ops.ptr(nll_x), ops.ptr(la), ops.ptr(lb), st), "av_ctc_loss_fwd")
            L.check(lib.av_ctc_loss_bwd(ops.ptr(lp_x), T * V, V, ops.ptr(tg), T, ops.ptr(il_x), ops.ptr(tl), B * N, T, V, S_max, blank,
                                        ops.ptr(nll_x), ops.ptr(la), ops.ptr(lb), ops.ptr(gn_x), ops.ptr(grad_x), st), "av_ctc_loss_bwd")
            return grad_x.view(B, N, T, V).sum(1)

        for _ in range(5):
            nbest(); composition()
        torch.cuda.synchronize()
        a_ms, b_ms = [], []
        for _ in range(args.pairs):
            a_ms.append(timed(nbest))
            b_ms.append(timed(composition))
        g_a = nbest().clone()
        nll_a = nll.clone()
        g_b = composition()
        torch.cuda.synchronize()
        same_nll = bool(torch.equal(nll_a.reshape(-1).view(torch.int32), nll_x.view(torch.int32)))
        d_grad = float((g_a - g_b).abs().max())
        # bytes from the shapes (fp32): lattice rows written by the forward and read by the gradient, the log-probs and the gradient rows
        mean_S = float((2 * lens + 1).float().mean())
        rows = float(il.float().sum())                                   # [b, t] rows with t < T_b
        ws_rw = 2 * N * rows * mean_S * 4                                # alpha + beta
        nb_bytes = 2 * ws_rw + B * T * V * 4 * 2 + 2 * N * rows * mean_S * 4
        co_bytes = 2 * ws_rw + 2 * N * rows * mean_S * 4 + B * N * T * V * 4 * 4 + B * T * V * 4 * 2
        am, bm = statistics.median(a_ms), statistics.median(b_ms)
        lines += [f"N {N}: workspaces log_alpha + log_beta 2 x {la.numel() * 4 / 2 ** 20:.1f} MiB (the same for both forms); expanded log-probs "
                  f"{B * N * T * V * 4 / 2 ** 20:.1f} MiB and expanded gradient {B * N * T * V * 4 / 2 ** 20:.1f} MiB (composition only)",
                  f"  n-best  fwd + bwd                          {fmt(a_ms)}   ~{nb_bytes / 2 ** 20:.0f} MiB moved",
                  f"  composition (expand, fwd + bwd, sum over N) {fmt(b_ms)}   ~{co_bytes / 2 ** 20:.0f} MiB moved",
                  f"  composition / n-best x{bm / am:.2f};  nll bit-identical: {same_nll};  max |grad difference| {d_grad:.3e} "
                  f"(max |grad| {float(g_b.abs().max()):.3e})"]
    lines += ["# bytes: gathered emissions + lattice rows written (forward), lattice rows + log-prob rows read and gradient rows written (gradient);",
              "# the composition adds the expanded log-probs (written, read by the gradient kernel), the expanded gradient (written, read by the sum)",
              "# and the sum's output."]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
