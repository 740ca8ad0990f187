"""GPU: training steps, evaluate() and align() of MultimodalTrainer against a recording of the commit before its body was split into an options
table and named stages (tests/golden/trainer_parent.npz, written by tests/golden/make_trainer_parent.py on the commit, the device and the
toolchain named inside the file): every branch of the step, in fp32 and bf16, is equal to the recording bit for bit - loss scalars, a checksum
of every trainable parameter and BatchNorm buffer after two steps, evaluate()'s loss, WER, decoded strings and report, align()'s segments.

Only the constructor, train_step, evaluate, align, last_decoded and last_report are used, so ``run`` works on any commit that has those options.
The recorder runs every case twice in fresh trainers and keeps what is bit-equal between the two runs; what it had to leave out (only
``k_proj.bias`` tensors may be: in bf16 their rounding-noise gradient depends on the order of the atomics in the column sums, see
test_step_gpu.py) is listed in the file, and the test skips exactly that list.

The recording is tied to the toolchain (compiler, device libraries, torch's own kernels for nn.CTCLoss and the concatenations).  After an
update of those, or after a change that is MEANT to alter the arithmetic of the step, record again on the commit before that change: copy this
file, trainer_util.py and golden/make_trainer_parent.py next to a build of that commit and run the recorder there, as make_beam_parent.py does."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import pkg
from trainer_util import gpu_trainer
import lm_ref as LR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_parent.npz")
SCALARS = ("total", "loss1", "loss2", "contrast1", "contrast2", "mwer1", "mwer2", "grad_norm")
STOCHASTIC = dict(hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, layerdrop=0.1, mask_time_prob=0.05)
# name -> (constructor keywords, what else the case changes)
CASES = {
    "defaults": ({}, ()),
    "per_speaker": (dict(pair_batched=False), ()),
    "no_side_stream": (dict(visual_side_stream=False), ()),
    "two_passes": (dict(audio_passes=2), ()),
    "stochastic": ({}, ("stochastic",)),
    "native_ctc": (dict(native_ctc=True), ()),
    "native_ctc_per_speaker": (dict(native_ctc=True, pair_batched=False), ()),
    "loss_scaling": (dict(loss_scaling=True), ()),
    "reducer": ({}, ("reducer",)),
    "reducer_per_speaker": (dict(pair_batched=False), ("reducer",)),
    "mwer": (dict(mwer_weight=0.25, mwer_nbest=2, mwer_beam=4), ()),
    "augment": ({}, ("augment",)),
    "clip_schedule_ema": (dict(max_grad_norm=1.0, warmup_steps=2, total_steps=8, ema_decay=0.5, eval_ema=True), ()),
    "lip2_longer": ({}, ("lip2_longer",)),
    "beam": (dict(eval_beam_width=4), ()),
    "beam_lm": (dict(eval_beam_width=4), ("lm",)),
    "beam_bias": (dict(eval_beam_width=4), ("bias",)),
    "beam_lm_bias": (dict(eval_beam_width=4), ("lm", "bias")),
    "report": (dict(eval_report=True), ()),
    "align": ({}, ("align",)),
}
RUNS = [(c, p) for c in CASES for p in ("fp32", "bf16")] + [("loss_scaling", "fp16")]


def bits(x) -> np.ndarray:
    """The float32 bit pattern of a scalar tensor."""
    return x.detach().float().reshape(1).cpu().numpy().view(np.uint32)


def checksum(x: torch.Tensor) -> int:
    """Sum of the elements' bit patterns as integers: exact and independent of the order of the sum."""
    ints = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]
    return int(x.detach().contiguous().view(ints).to(torch.int64).sum())


def state(t) -> dict:
    """name -> checksum of every trainable parameter and of every BatchNorm buffer."""
    mods = (("visual", t.visual_encoder), ("audio", t.audio_encoder), ("fusion", t.fusion_module), ("decoder", t.decoder1))
    out = {f"{m}.{n}": checksum(p) for m, mod in mods for n, p in mod.named_parameters() if p.requires_grad}
    out.update({f"visual.{n}": checksum(b) for n, b in t.visual_encoder.named_buffers()})
    return out


def run(case: str, precision: str) -> dict:
    """One case in a fresh trainer -> {quantity: host array or JSON text}; two train_step calls, evaluate([batch]), for "align" an align(batch)."""
    init = pkg("utils.init"); synth = pkg("dataset.synthetic")
    kw, extra = CASES[case]
    kw = dict(kw)
    cfg = dict(init.W2V2_TINY)
    if "stochastic" in extra:
        cfg.update(STOCHASTIC)
    torch.manual_seed(1234)
    np.random.seed(1234)                                   # the SpecAugment masks of wav2vec2 come from numpy's global generator, as in HF
    if "reducer" in extra:
        kw["reducer"] = pkg("parallel.dp").GradBucketReducer()
    if "augment" in extra:
        kw["augment"] = pkg("augment").Augment(max_shift=3, flip=0.5, mask_max=2, mask_every=10, snr=(5.0, 25.0), seed=11)
    tok = pkg("utils.tokenizer").SyntheticTokenizer(800)
    if "lm" in extra:
        kw.update(eval_lm=pkg("lm").NGramLM.from_corpus(LR.make_corpus(3, 200, tok.vocab_size, blank=tok.blank_id), tok.vocab_size, tok.blank_id,
                                                        order=3), eval_lm_weight=0.8, eval_token_bonus=1.0)
    if "bias" in extra:
        kw.update(eval_bias=pkg("bias").ContextBias.from_phrases([(5, 6, 7), (40, 41)], vocab_size=tok.vocab_size, blank=tok.blank_id),
                  eval_bias_weight=2.5)
    t = gpu_trainer(cfg, precision, **kw)
    t.audio_encoder.model.layerdrop_generator = torch.Generator().manual_seed(21)
    t.audio_encoder.model.dropout_generator = torch.Generator().manual_seed(22)
    batch = synth.make_batch(2, 1.0, seed=5, ragged=True)
    if "lip2_longer" in extra:
        batch["lip2"] = F.pad(batch["lip2"], (0, 0, 0, 0, 0, 0, 0, 1))        # one more frame: one fusion / decoder / CTC call per speaker
    for m in (t.visual_encoder, t.audio_encoder, t.fusion_module, t.decoder1):
        m.train()
    res = {}
    for step in (1, 2):
        out = t.train_step(batch)
        for k in SCALARS:
            if k in out:
                res[f"step{step}.{k}"] = bits(out[k])
    st = state(t)
    res["state.names"] = np.array(json.dumps(sorted(st)))
    res["state.sums"] = np.array([st[n] for n in sorted(st)], dtype=np.int64)
    loss, wer = t.evaluate([batch])
    res["eval.loss"] = np.array([loss], dtype=np.float64).view(np.uint64)
    res["eval.wer"] = np.array([wer], dtype=np.float64).view(np.uint64)
    res["eval.decoded"] = np.array(json.dumps(t.last_decoded, ensure_ascii=True))
    res["eval.report"] = np.array(json.dumps(t.last_report, sort_keys=True))
    if "align" in extra:
        res["align.segments"] = np.array(json.dumps(t.align(batch), sort_keys=True))      # floats are written with repr: exact
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(autouse=True)
def _precision_restored():
    P = pkg("precision")
    old = P.get_precision()
    yield
    P.set_precision(old)


@pytest.mark.parametrize("case,precision", RUNS, ids=[f"{c}-{p}" for c, p in RUNS])
def test_steps_evaluate_and_align_equal_the_recorded_ones_bit_for_bit(recorded, case, precision):
    pre = f"{case}.{precision}."
    want = {k[len(pre):]: v for k, v in recorded.items() if k.startswith(pre)}
    assert want, f"{case} in {precision} is not in the recording"
    got = run(case, precision)
    left_out = json.loads(str(want.pop("left_out")))
    assert all(n.endswith("k_proj.bias") for n in left_out["state"]), left_out                # the one tolerated hole, and it cannot grow
    names = json.loads(str(got["state.names"]))
    assert names == json.loads(str(want["state.names"]))
    keep = np.array([n not in left_out["state"] for n in names])
    assert sorted(set(got) - set(want)) == sorted(left_out["quantities"]), (sorted(got), sorted(want))
    assert all(k.startswith("step2.") for k in left_out["quantities"]), left_out              # step 1, evaluate() and align() are always compared
    for k, x in want.items():
        y = got[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if k == "state.sums":
            bad = [n for n, a, b, on in zip(names, x, y, keep) if on and a != b]
            assert not bad, (len(bad), bad[:5])
        else:
            assert np.array_equal(x, y), (k, x, y)
