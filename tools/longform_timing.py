"""Long-form transcription on one MI355X, device events, reported and not gated:
  the three entries of csrc/ctc_longform.hip (called directly, outputs allocated once) at F 1500 / V 800 / W 100 / S 12 / two speakers (a 60 s recording at 25 frames per second),
    each against a device-to-device copy of the bytes it writes (the floor of a pass that moves them once) and against the torch
    composition of the same law (index_select / logsumexp / argmax);
  MultimodalTrainer.transcribe_long on a 60 s synthetic recording with the tiny model, end to end (host wall clock around a synchronised
    call), at beam width 0 and 4, beside the windows' forward calls alone.
The candidates of a group run in alternating rounds (one call each per round, 20 rounds after 3 warm-up rounds): whatever drifts on the
device drifts for all of them.  Writes profiles/longform_timing.txt.

    python tools/longform_timing.py [--out profiles/longform_timing.txt]
"""
from __future__ import annotations

import argparse
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "multimodal-av-model_amd"


def pkg(name):
    return importlib.import_module(PKG + "." + name)


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


def group(title, r, kernel, nbytes, note=""):
    k, c, t = (statistics.median(r[x]) for x in ("kernel", "copy", "torch"))
    return [title,
            f"  device-to-device copy (floor)    {fmt(r['copy'])}",
            f"  {kernel:<32} {fmt(r['kernel'])}   = {nbytes / 1e6 / k / 1e3:.2f} TB/s written, x{k / c:.2f} of the copy",
            f"  torch composition                {fmt(r['torch'])}   x{t / k:.1f} of the kernel{note}"]


def tiny_trainer(**kw):
    """The seeded tiny model of the test-suite (utils.init.W2V2_TINY) on the GPU in fp32."""
    init = pkg("utils.init"); enc = pkg("model.encoder"); fm = pkg("model.fusion_module"); dm = pkg("model.decoder")
    tr = pkg("model.trainer"); tok = pkg("utils.tokenizer")
    pkg("precision").set_precision("fp32")
    cfg = dict(init.W2V2_TINY)
    ve = enc.VisualEncoder(); ve.load_state_dict(init.visual_state_dict())
    ae = enc.AudioEncoder(dict(cfg), freeze=True); ae.load_state_dict(init.w2v2_state_dict(cfg))
    fu = fm.CrossAttentionFusion(512, cfg["hidden_size"], 512); fu.load_state_dict(init.fusion_state_dict(512, cfg["hidden_size"], 512))
    de = dm.CTCDecoder(1024, 800, 3); de.load_state_dict(init.decoder_state_dict(1024, 800))
    return tr.MultimodalTrainer(ve, ae, fu, de, tok.SyntheticTokenizer(800), device="cuda", **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longform_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("longform_timing: needs the GPU; there is nothing to time without it")
    LF = pkg("longform"); L = pkg("_lib"); ops = pkg("ops"); lib = L.lib()
    Sp, F, V, W, S, blank, segment, radius = 2, 1500, 800, 100, 12, 0, 400, 50
    plan = LF.plan_windows(F, W, S)
    g = torch.Generator().manual_seed(0)
    logits = 3 * torch.randn(Sp, plan.count, W, V, generator=g)
    logits[..., blank] += 5.0                                       # the blank wins most frames, as in a trained CTC head
    win = torch.log_softmax(logits, -1).cuda()
    rows = win.view(Sp, plan.count * W, V)
    out_bytes = Sp * F * V * 4
    lines = [f"# tools/longform_timing.py on {torch.cuda.get_device_name(0)}: float32 window log-probs [S {Sp}][nw {plan.count}][W {W}][V {V}] = "
             f"{win.numel() * 4 / 1e6:.1f} MB -> [S {Sp}][F {F}][V {V}] = {out_bytes / 1e6:.1f} MB (stride {S}, hop {plan.hop}, coverage {plan.coverage});",
             "# device events, alternating rounds (one call of each candidate per round), 20 rounds after 3 warm-up rounds.  Reported, not gated."]
    dst = torch.empty((Sp, F, V), dtype=torch.float32, device="cuda")
    src = torch.empty_like(dst)
    for policy in LF.POLICIES:
        row, wt = plan.table(policy, win.device)
        idx = row.clamp_min(0).long()                               # [F, 4]
        logw = torch.where(row >= 0, wt.log(), torch.full_like(wt, float("-inf")))

        def composition():
            if policy == "centre":
                return rows.index_select(1, idx[:, 0])
            x = rows.index_select(1, idx.reshape(-1)).view(Sp, F, 4, V)
            return torch.logsumexp(x + logw[None, :, :, None], 2)

        def kernel():                                              # the entry itself, outputs allocated once
            L.check(lib.av_ctc_stitch(ops.ptr(win), plan.count * W * V, V, ops.ptr(row), ops.ptr(wt), Sp, plan.count * W, F, V, ops.ptr(dst),
                                      ops.stream()))
        r = rounds_ms({"copy": lambda: dst.copy_(src), "kernel": kernel, "torch": composition})
        dev = float((LF.stitch(win, plan, policy) - composition()).abs().max())
        lines += group(f"stitch, policy {policy}", r, "av_ctc_stitch", out_bytes, f"; max |kernel - torch| {dev:.1e}")
    lp = LF.stitch(win, plan, "centre")
    nb = LF.boundaries(F, segment, radius)
    N = segment - 2 * radius
    zone = (torch.arange(1, nb + 1, device="cuda")[:, None] * N + torch.arange(-radius, radius + 1, device="cuda")[None, :]).clamp(1, F - 1)

    def torch_cuts():
        col = lp[:, :, blank].nan_to_num(nan=float("-inf"), neginf=float("-inf"))
        best = col[:, zone.reshape(-1)].view(Sp, nb, 2 * radius + 1).argmax(-1)
        inner = (zone[None, :, 0] + best).int()
        return torch.cat([torch.zeros((Sp, 1), dtype=torch.int32, device="cuda"), inner,
                          torch.full((Sp, 1), F, dtype=torch.int32, device="cuda")], 1)
    small = torch.empty((Sp, nb + 2), dtype=torch.int32, device="cuda")
    small_src = torch.empty_like(small)
    r = rounds_ms({"copy": lambda: small.copy_(small_src), "torch": torch_cuts, "kernel": lambda: L.check(lib.av_ctc_cut_points(
        ops.ptr(lp), F * V, V, Sp, F, V, blank, segment, radius, ops.ptr(small), ops.stream()))})
    cuts = LF.cut_points(lp, blank, segment, radius)
    lines += group(f"cut points, segment {segment} radius {radius}: {nb} boundaries per speaker", r, "av_ctc_cut_points", small.numel() * 4,
                   f"; equal cuts: {bool(torch.equal(cuts, torch_cuts()))}")
    seg_bytes = Sp * (nb + 1) * segment * V * 4
    seg_dst = torch.empty((Sp * (nb + 1), segment, V), dtype=torch.float32, device="cuda")
    seg_src = torch.empty_like(seg_dst)
    ar = torch.arange(segment, device="cuda")

    def torch_segments():
        c = cuts.long()
        ln = (c[:, 1:] - c[:, :-1]).reshape(-1)
        t = (c[:, :-1].reshape(-1, 1) + ar[None, :]).clamp_max(F - 1)                          # [S (nb + 1), segment]
        sp = torch.arange(Sp, device="cuda").repeat_interleave(nb + 1)[:, None]
        return torch.where((ar[None, :] < ln[:, None])[..., None], lp[sp, t], 0.0), ln
    seg_len = torch.empty((Sp * (nb + 1),), dtype=torch.int64, device="cuda")
    r = rounds_ms({"copy": lambda: seg_dst.copy_(seg_src), "torch": torch_segments, "kernel": lambda: L.check(lib.av_ctc_segment_gather(
        ops.ptr(lp), F * V, V, ops.ptr(cuts), Sp, F, V, nb, segment, ops.ptr(seg_dst), ops.ptr(seg_len), ops.stream()))})
    same = torch.equal(LF.split_segments(lp, cuts, segment)[0], torch_segments()[0])
    lines += group(f"segments: [{Sp * (nb + 1)}][{segment}][{V}] = {seg_bytes / 1e6:.1f} MB", r, "av_ctc_segment_gather", seg_bytes,
                   f"; equal segments: {bool(same)}")
    # end to end on the tiny model: 60 s = 1500 lip frames, the default long_* settings
    synth = pkg("dataset.synthetic")
    clips = [synth.make_batch(1, 4.0, seed=100 + i) for i in range(15)]
    rec = {"audio": torch.cat([c["audio"][0] for c in clips]).cuda(), "lip1": torch.cat([c["lip1"][0] for c in clips]).cuda(),
           "lip2": torch.cat([c["lip2"][0] for c in clips]).cuda()}
    lines.append(f"transcribe_long, tiny model (fp32), a {rec['lip1'].shape[0] / 25:.0f} s recording on the device: {rec['lip1'].shape[0]} lip frames, "
                 f"windows of {W} (stride {S}): {plan.count} windows in {-(-plan.count // 16)} forward calls, segments of at most {segment}")
    for beam in (0, 4):
        t = tiny_trainer(eval_beam_width=beam)
        calls = []
        inner = t.forward_log_probs

        def timed(b):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            o = inner(b)
            torch.cuda.synchronize(); calls.append(time.perf_counter() - t0)
            return o
        wall = []
        for i in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = t.transcribe_long(rec)
            torch.cuda.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
        t.forward_log_probs = timed
        t.transcribe_long(rec)
        t.forward_log_probs = inner
        ns = len(res[0]["segments"])
        lines.append(f"  beam {beam}: end to end median {statistics.median(wall[1:]):8.1f} ms  (min {min(wall[1:]):.1f}, max {max(wall[1:]):.1f}; first call "
                     f"{wall[0]:.1f}); of it the forward calls {sum(calls) * 1e3:.1f} ms; {ns} segments per speaker, "
                     f"{len(res[0]['ids'])} + {len(res[1]['ids'])} tokens")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
