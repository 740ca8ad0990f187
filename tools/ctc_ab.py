"""A/B of the CTC entry points between two builds of the library (the shared-laws refactor, csrc/ctc_common.h), on one MI355X.

    AVAMD_LIB=... AVAMD_LIB_F16=... python tools/ctc_ab.py outputs {fp32|fp16} OUT.pt
        one process per library: the outputs of ops.ctc_loss (nll + gradient: both layouts, a strided view, zero_infinity on and off, a
        repeated label, an infeasible item, T_b = 0), ops.ctc_nbest_nll (N 1 and 3, one absent and one over-long hypothesis), ops.ctc_align,
        ops.ctc_frame_conf (3 methods), ops.ctc_greedy_timed, the three beam searches, NGramLM.score_batch and ContextBias.count_batch for
        seeded inputs (B 3, T 37, V 13 and 16, Lmax 6)
    python tools/ctc_ab.py compare A.pt B.pt
        are two such files byte-identical?  (no GPU)
    python tools/ctc_ab.py timing OUT.txt name=path.so ...
        the entry points of the beam family, whose kernels read lengths through the shared clamp, and the two loss gradients, per library in
        one process: device events around single calls, 5 warm-ups, 30 repeats, the libraries in alternation.  Give the parent's library
        twice (two copies of the file): the difference between its two medians is the spread between equal runs.
profiles/ctc_common_refactor_ab.txt is the record of one such run."""
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


def outputs(mode, out_path):
    P = importlib.import_module(PKG + ".precision"); P.set_precision(mode)
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops")
    bs = importlib.import_module(PKG + ".beam_search"); LM = importlib.import_module(PKG + ".lm"); BIAS = importlib.import_module(PKG + ".bias")
    print("library:", L.lib()._name, flush=True)
    out = {"lib": os.path.basename(L.lib()._name)}
    B, T, Lmax, blank = 3, 37, 6, 0

    def beam(k, res):
        """ids past a hypothesis' length and everything of an absent hypothesis are not written: masked before the comparison"""
        ids, cnt = res[0], res[1]
        pos = torch.arange(ids.shape[2], device=ids.device)[None, None, :]
        keep = [torch.where(pos < cnt[..., None], ids, torch.full_like(ids, -9)), cnt]
        keep += [torch.where(cnt >= 0, x, torch.zeros_like(x)) for x in res[2:] if x is not None]
        put(k, *keep)

    def put(k, *ts):
        torch.cuda.synchronize()
        out[k] = [t.detach().cpu().clone() if isinstance(t, torch.Tensor) else t for t in ts]

    for V in (13, 16):
        g = torch.Generator().manual_seed(1000 + V)
        base = torch.log_softmax(torch.randn(B, T, V, generator=g), -1)
        tg = torch.randint(1, V, (B, Lmax), generator=g)
        tg[0, 1] = tg[0, 0]; tg[0, 3] = tg[0, 0]                     # repeated labels
        il = torch.tensor([T, 3, 0])                                 # item 1: infeasible (3 frames, 5 labels); item 2: T_b = 0
        tl = torch.tensor([Lmax, 5, 2])
        gw = torch.tensor([0.7, -1.3, 0.4])
        wide = torch.log_softmax(torch.randn(B, T, 2 * V + 3, generator=g), -1).cuda()
        views = {"bf": (base.cuda(), True), "tf": (base.transpose(0, 1).contiguous().cuda(), False), "strided": (wide[:, :, 2:2 + V], True)}
        for name, (lp0, bf) in views.items():
            for zi in (False, True):
                lp = lp0.detach().requires_grad_(True)
                nll = ops.ctc_loss(lp, tg.cuda(), il, tl, blank=blank, reduction="none", zero_infinity=zi, batch_first=bf)
                fin = torch.isfinite(nll)
                (torch.where(fin, nll, torch.zeros_like(nll)) * gw.cuda()).sum().backward()
                put(f"loss V{V} {name} zi{zi}", nll, lp.grad)
            st, sp, tok, sc = ops.ctc_align(lp0, tg.cuda(), torch.tensor([T, 20, 0]), tl, blank=blank, batch_first=bf)
            put(f"align V{V} {name}", st, sp, tok, sc)
            if bf:
                for m in ("max_prob", "entropy", "tsallis"):
                    put(f"conf V{V} {name} {m}", ops.ctc_frame_conf(lp0, torch.tensor([T, 20, 0]), m, 0.33, True))
                    put(f"greedy V{V} {name} {m}", *ops.ctc_greedy_timed(lp0, blank, torch.tensor([T, 20, 0]), m, 0.33, "min", True))
                put(f"greedy V{V} {name} nolen", *ops.ctc_greedy_timed(lp0, blank, None, "entropy", 0.33, "mean", True))
        # n-best: N = 1 and N = 3 with one absent (-1) and one over-long hypothesis (max_len 5 < 6)
        for N in (1, 3):
            hyp = torch.randint(1, V, (B, N, Lmax), generator=g).to(torch.int32)
            hl = torch.randint(1, 5, (B, N), generator=g)
            if N == 3:
                hl[0, 1] = -1; hl[1, 2] = 6
            for name, (lp0, bf) in views.items():
                lp = lp0.detach().requires_grad_(True)
                nll = ops.ctc_nbest_nll(lp, hyp.cuda(), hl, torch.tensor([T, 20, 0]), blank=blank, batch_first=bf, max_len=5)
                w = torch.randn(B, N, generator=torch.Generator().manual_seed(5)).cuda()
                torch.where(torch.isfinite(nll), nll * w, torch.zeros_like(nll)).sum().backward()
                put(f"nbest V{V} N{N} {name}", nll, lp.grad)
        # beam search family (its kernels read lengths through the shared clamp)
        lens = torch.tensor([T, 20, 0]).cuda()
        lpb = base.cuda()
        import lm_ref as LR
        lm = LM.NGramLM.from_corpus(LR.make_corpus(7, 60, V, blank, lo=3, hi=9), V, blank, order=3)
        cb = BIAS.ContextBias.from_phrases([(1, 2), (3, 4, 5), (2, 2, 7)], vocab_size=V, blank=blank)
        beam(f"beam V{V} plain", bs._device_beam_launch(lpb, lens, 4, blank, 2, None, 0.0, 0.0, 5))
        beam(f"beam V{V} lm", bs._device_beam_launch(lpb, lens, 4, blank, 2, lm, 0.5, 0.1, 5))
        beam(f"beam V{V} bias", bs._device_beam_launch(lpb, lens, 4, blank, 2, lm, 0.5, 0.1, 5, cb, 2.0))
        ids = torch.randint(1, V, (B, 9), generator=g).to(torch.int32).cuda()
        put(f"ngram V{V}", lm.score_batch(ids, torch.tensor([9, 4, 0])), lm.score_batch(ids))
        put(f"biascount V{V}", cb.count_batch(ids, torch.tensor([9, 4, 0])), cb.count_batch(ids))

    torch.cuda.synchronize()
    torch.save(out, out_path)
    print("wrote", out_path, len(out), "entries", flush=True)


def compare(path_a, path_b):
    a, b = torch.load(path_a), torch.load(path_b)
    bad = 0
    assert sorted(a) == sorted(b), "different keys"
    for k in sorted(a):
        if k == "lib":
            continue
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            same = x.shape == y.shape and x.dtype == y.dtype and x.contiguous().reshape(-1).view(torch.uint8).equal(y.contiguous().reshape(-1).view(torch.uint8))
            if not same:
                bad += 1
                print("DIFFERS", k, i, x.dtype, tuple(x.shape))
    n = sum(len(v) for k, v in a.items() if k != "lib")
    print(f"{path_a} ({a['lib']}) vs {path_b} ({b['lib']}): {n} tensors in {len(a) - 1} entries, {bad} differ", flush=True)
    return 1 if bad else 0


def timing(out_path, specs):
    L = importlib.import_module(PKG + "._lib"); ops = importlib.import_module(PKG + ".ops")
    LM = importlib.import_module(PKG + ".lm"); BIAS = importlib.import_module(PKG + ".bias")
    import lm_ref as LR
    NAMES = ("av_ctc_loss_fwd", "av_ctc_loss_bwd", "av_ctc_nbest_fwd", "av_ctc_nbest_bwd", "av_ctc_beam_frame_pass", "av_ctc_beam_search",
             "av_ctc_beam_search_lm", "av_ctc_beam_search_bias", "av_ngram_score", "av_context_bias_count", "av_ctc_beam_lm_workspace_bytes",
             "av_ctc_beam_workspace_bytes")
    libs = {}
    for spec in specs:
        name, path = spec.split("=")
        lib = ctypes.CDLL(os.path.abspath(path))
        for n in NAMES:
            if n in L.SIGNATURES:
                getattr(lib, n).argtypes = L.SIGNATURES[n]
                getattr(lib, n).restype = ctypes.c_int
        lib.av_last_error.restype = ctypes.c_char_p
        libs[name] = lib
    first = next(iter(libs.values()))
    st = ops.stream()
    p = ops.ptr

    def ok(lib, rc):
        if rc != 0:
            raise RuntimeError(f"status {rc}: {lib.av_last_error().decode('utf-8', 'replace')}")

    # ---- the loss gradient kernels: the shapes of tools/mwer_timing.py (B 128, T 100, V 800, hypotheses of 15-25 tokens in rows of width T) ----
    B, T, V, N, blank = 128, 100, 800, 4, 3
    S_max = 2 * T + 1
    g = torch.Generator().manual_seed(904)
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g), -1).cuda()
    lens = torch.randint(15, 26, (B, N), generator=g).cuda()
    ids = torch.randint(4, V, (B, N, T), generator=g).to(torch.int32).cuda()
    il = torch.randint(80, T + 1, (B,), generator=g).cuda()
    gn = (torch.rand(B, N, generator=g) * 2 - 1).cuda()
    nll = torch.empty((B, N), dtype=torch.float32, device="cuda")
    la = torch.empty((B, N, T, S_max), dtype=torch.float32, device="cuda"); lb = torch.empty_like(la)
    grad = torch.empty((B, T, V), dtype=torch.float32, device="cuda")
    tg1 = ids[:, 0].long().contiguous(); tl1 = lens[:, 0].contiguous(); g1 = gn[:, 0].contiguous()
    nll1 = torch.empty((B,), dtype=torch.float32, device="cuda")
    la1 = torch.empty((B, T, S_max), dtype=torch.float32, device="cuda"); lb1 = torch.empty_like(la1)
    ok(first, first.av_ctc_nbest_fwd(p(lp), T * V, V, p(ids), N * T, T, p(lens), p(il), B, N, T, V, S_max, blank, p(nll), p(la), p(lb), st))
    ok(first, first.av_ctc_loss_fwd(p(lp), T * V, V, p(tg1), T, p(il), p(tl1), B, T, V, S_max, blank, 0, p(nll1), p(la1), p(lb1), st))

    # ---- the beam family: the shapes of tools/beam_bias_timing.py (B 64, T 199, V 800, W 8, tokens 9) ----
    Bb, Tb, Vb, W, K = 64, 199, 800, 8, 9
    gb = torch.Generator().manual_seed(31000)
    lpb = torch.log_softmax(3 * torch.randn(Bb, Tb, Vb, generator=gb), -1).cuda()
    lnb = torch.randint(150, Tb + 1, (Bb,), generator=gb).cuda()
    lm = LM.NGramLM.from_corpus(LR.make_corpus(7, 400, Vb, 0, lo=8, hi=30), Vb, 0, order=3)
    d = lm.to_device("cuda")
    cb = BIAS.ContextBias.from_phrases([tuple(int(x) for x in np.random.default_rng(i).integers(1, Vb, size=4)) for i in range(100)], vocab_size=Vb, blank=0)
    db = cb.to_device("cuda")
    need, nb = L.ll(0), L.ll(0)
    ok(first, first.av_ctc_beam_workspace_bytes(Bb, Tb, Vb, W, ctypes.byref(need)))
    ok(first, first.av_ctc_beam_lm_workspace_bytes(Bb, Tb, Vb, W, K, ctypes.byref(nb)))
    ws = torch.empty(((max(need.value, nb.value) + 7) // 8,), dtype=torch.int64, device="cuda")
    out = torch.empty((Bb, 1, Tb), dtype=torch.int32, device="cuda")
    cnt, kb = torch.empty((Bb, 1), dtype=torch.int32, device="cuda"), torch.empty((Bb, 1), dtype=torch.int32, device="cuda")
    sc, gl = torch.empty((Bb, 1), dtype=torch.float32, device="cuda"), torch.empty((Bb, 1), dtype=torch.float32, device="cuda")
    head = (p(lpb), Tb * Vb, Vb, p(lnb), p(out), p(cnt), p(sc))
    lm_args = (p(d.unigrams), p(d.table), d.slots, d.order, d.vocab_size, d.bos, d.probe_bound, 0.5, 0.0)
    tail = (p(db.nodes), p(db.edges), db.node_count, db.slots, db.probe_bound, 2.0, st)
    sid = torch.randint(1, Vb, (4096, 64), generator=gb).to(torch.int32).cuda()
    sln = torch.randint(0, 65, (4096,), generator=gb).cuda()
    sout = torch.empty((4096, 64), dtype=torch.float32, device="cuda")
    cout = torch.empty((4096, 64, 2), dtype=torch.int32, device="cuda")

    CALLS = {
        "av_ctc_loss_bwd": lambda l: l.av_ctc_loss_bwd(p(lp), T * V, V, p(tg1), T, p(il), p(tl1), B, T, V, S_max, blank, p(nll1), p(la1), p(lb1), p(g1), p(grad), st),
        "av_ctc_nbest_bwd N=4": lambda l: l.av_ctc_nbest_bwd(p(lp), T * V, V, p(ids), N * T, T, p(lens), p(il), B, N, T, V, S_max, blank, p(nll), p(la), p(lb),
                                                             p(gn), p(grad), st),
        "av_ctc_beam_frame_pass": lambda l: l.av_ctc_beam_frame_pass(p(lpb), Tb * Vb, Vb, p(lnb), p(ws), need.value, Bb, Tb, Vb, 0, W, st),
        "av_ctc_beam_search": lambda l: l.av_ctc_beam_search(*head, p(ws), need.value, Bb, Tb, Vb, 0, W, 1, st),
        "av_ctc_beam_search_lm": lambda l: l.av_ctc_beam_search_lm(*head, p(gl), p(ws), nb.value, Bb, Tb, Vb, 0, W, 1, K, *lm_args, st),
        "av_ctc_beam_search_bias": lambda l: l.av_ctc_beam_search_bias(*head, p(gl), p(kb), p(ws), nb.value, Bb, Tb, Vb, 0, W, 1, K, *lm_args, *tail),
        "av_ngram_score": lambda l: l.av_ngram_score(p(sid), p(sln), p(sout), 4096, 64, p(d.unigrams), p(d.table), d.slots, d.order, d.vocab_size, d.bos,
                                                     d.probe_bound, st),
        "av_context_bias_count": lambda l: l.av_context_bias_count(p(sid), p(sln), p(cout), 4096, 64, Vb, 0, p(db.nodes), p(db.edges), db.node_count, db.slots,
                                                                   db.probe_bound, st),
    }

    def one_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        return a.elapsed_time(b)

    lines = [f"# {torch.cuda.get_device_name(0)}; loss: B {B} T {T} V {V} S_max {S_max} N {N}; beam: B {Bb} T {Tb} V {Vb} W {W} tokens {K}; scoring: 4096 x 64 ids",
             "# median ms of 30 (min, max), libraries in alternation after 5 warm-ups each"]
    for what, call in CALLS.items():
        for _ in range(5):
            for lib in libs.values():
                ok(lib, call(lib))
        torch.cuda.synchronize()
        times = {k: [] for k in libs}
        for _ in range(30):
            for k, lib in libs.items():
                times[k].append(one_ms(lambda: ok(lib, call(lib))))
        lines.append(what)
        for k, ms in times.items():
            lines.append(f"    {k:12s} median {statistics.median(ms):8.4f}  (min {min(ms):.4f}, max {max(ms):.4f})")
        print("\n".join(lines[-1 - len(libs):]), flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(text)


if __name__ == "__main__":
    what = sys.argv[1]
    if what == "outputs":
        outputs(sys.argv[2], sys.argv[3])
    elif what == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        timing(sys.argv[2], sys.argv[3:])
