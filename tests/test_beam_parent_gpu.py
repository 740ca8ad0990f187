"""GPU: both instantiations of the search kernel of csrc/ctc_beam.hip against a recording of the two separate kernels they replaced
(tests/golden/beam_parent.npz, written by tests/golden/make_beam_parent.py on the commit and the device named inside the file), in both
libraries: ids, lengths, score bits and g bits are equal exactly.  The search is a fixed sequence of individually rounded float32
operations (the build has -ffp-contract=off) plus expf / log1pf of the device library, so the recording is tied to the toolchain that
made it: after a compiler or device-library update that changes those two functions, record again on the commit before the update's first
change to the search and compare."""
import os

import numpy as np
import pytest
import torch

from conftest import pkg
import beam_ref as R
import lm_ref as LR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_parent.npz")
B, T, PAD = 6, 40, 24
LENGTHS = [T, 0, T // 2, 1, T - 1, T]
# (V, W): every token expanded at (9, 16); the candidate buffer full at (800, 64); the frame pass's long-row path at V = 1500
PLAIN = [(40, 5), (9, 16), (800, 64), (1500, 4)]
# (V, W, tokens, order, bos, alpha, beta): wf = tokens - 1 > W puts the arena at the other offset; tokens = 1 gives wf = 1 < W
FUSED = [(40, 5, 6, 3, True, 0.5, 0.0), (40, 8, 40, 4, False, 0.8, 1.0), (800, 6, 1, 3, True, 0.8, 1.0), (800, 64, 65, 2, True, 0.5, 0.25),
         (9, 16, 17, 2, True, 0.5, 0.0)]


def name(case):
    return ("plain" if len(case) == 2 else "fused") + "_" + "_".join(str(int(x) if isinstance(x, bool) else x) for x in case)


@pytest.fixture(params=["fp32", "fp16"])
def library(request):
    """libavhip.so and libavhip_f16.so (decoding is float32 in both)."""
    P = pkg("precision")
    old = P.get_precision()
    P.set_precision(request.param)
    yield request.param
    P.set_precision(old)


def run(case):
    """One case through the C entry points on pre-filled outputs and strided input -> {suffix: host array}."""
    L = pkg("_lib"); ops = pkg("ops")
    V, W = case[:2]
    block = torch.full((B, T, V + PAD), float("nan"), dtype=torch.float32, device="cuda")
    block[:, :, :V] = torch.from_numpy(np.stack([R.make_log_probs(9000 + 10 * V + b, T, V) for b in range(B)])).cuda()
    lp = block[:, :, :V]
    lens = torch.tensor(LENGTHS, dtype=torch.long, device="cuda")
    need = L.ll(0)
    if len(case) == 2:
        L.check(L.lib().av_ctc_beam_workspace_bytes(B, T, V, W, L.C.byref(need)))
    else:
        L.check(L.lib().av_ctc_beam_lm_workspace_bytes(B, T, V, W, case[2], L.C.byref(need)))
    ws = torch.empty(((need.value + 7) // 8,), dtype=torch.int64, device="cuda")
    out = torch.full((B, W, T), 12345, dtype=torch.int32, device="cuda")
    cnt = torch.full((B, W), 12345, dtype=torch.int32, device="cuda")
    sc = torch.full((B, W), float("nan"), dtype=torch.float32, device="cuda")
    gl = torch.full((B, W), float("nan"), dtype=torch.float32, device="cuda")
    if len(case) == 2:
        L.check(L.lib().av_ctc_beam_search(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(lens), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                           ops.ptr(ws), need.value, B, T, V, 0, W, W, ops.stream()), "av_ctc_beam_search")
    else:
        _, _, tokens, order, bos, alpha, beta = case
        d = pkg("lm").NGramLM.from_corpus(LR.make_corpus(V + order, 400, V), V, 0, order=order, bos=bos).to_device("cuda")
        L.check(L.lib().av_ctc_beam_search_lm(ops.ptr(lp), lp.stride(0), lp.stride(1), ops.ptr(lens), ops.ptr(out), ops.ptr(cnt), ops.ptr(sc),
                                              ops.ptr(gl), ops.ptr(ws), need.value, B, T, V, 0, W, W, tokens, ops.ptr(d.unigrams),
                                              ops.ptr(d.table), d.slots, d.order, d.vocab_size, d.bos, d.probe_bound, alpha, beta,
                                              ops.stream()), "av_ctc_beam_search_lm")
    torch.cuda.synchronize()
    res = {"ids": out.cpu().numpy(), "len": cnt.cpu().numpy(), "score": sc.cpu().numpy().view(np.uint32)}
    if len(case) > 2:
        res["g"] = gl.cpu().numpy().view(np.uint32)
    return res


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", PLAIN + FUSED, ids=name)
def test_outputs_equal_the_recorded_ones_bit_for_bit(library, recorded, case):
    got = run(case)
    assert sorted(k for k in recorded if k.startswith(name(case) + ".")) == sorted(f"{name(case)}.{k}" for k in got)
    for k, x in got.items():
        want = recorded[f"{name(case)}.{k}"]
        assert x.dtype == want.dtype and x.shape == want.shape
        bad = np.argwhere(x != want)
        assert len(bad) == 0, (k, len(bad), bad[:5].tolist())
    assert (got["len"][1] == [0] + [-1] * (case[1] - 1)).all()               # length 0: the empty hypothesis alone
