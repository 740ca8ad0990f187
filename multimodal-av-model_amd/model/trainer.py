"""MultimodalTrainer with the reference's surface (model/trainer.py:12-252) on the HIP path.

Same constructor arguments and attributes (.visual_encoder .audio_encoder .fusion_module .decoder1 .optimizer
.device .tokenizer), ``train_epoch(loader) -> float``, ``evaluate(loader) -> (loss, wer)``, ``ctc_decode(ids)``.
Differences that do not change results:
  * compute runs in the package precision mode (bf16 perf / fp32 parity) instead of fp16 autocast + GradScaler;
  * attn_mask1 == attn_mask2 always, so with every stochastic regulariser of wav2vec2 at 0 the two audio
    passes of the reference are bit-identical and the encoder runs ONCE; as soon as dropout / LayerDrop / SpecAugment
    are active in train mode it runs twice with independent masks, as the reference does (``audio_passes`` forces it);
  * the class counts of the contrastive loss are taken from the CPU masks (no host sync);
  * optional data parallelism: bucketed gradient all-reduce over RCCL overlapped with the audio backward.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .. import _lib as L
from ..align import forced_align, word_segments
from ..augment import Augment
from ..beam_search import fast_decode, greedy_batch, prefix_beam_search
from ..bias import ContextBias
from ..lm import NGramLM
from ..contrastive import contrastive_loss_with_mask
from ..optim import AvAdam, AvGradScaler
from ..parallel.dp import GradArena, GradBucketReducer


def word_error_rate(refs, hyps) -> float:
    """jiwer.wer stand-in (jiwer is not installed): total word-level edit distance / total reference words."""
    errs = words = 0
    for r, h in zip(refs, hyps):
        r, h = r.split(), h.split()
        prev = list(range(len(h) + 1))
        for i in range(1, len(r) + 1):
            cur = [i] + [0] * len(h)
            for j in range(1, len(h) + 1):
                cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (r[i - 1] != h[j - 1]))
            prev = cur
        errs += prev[-1]
        words += len(r)
    return errs / max(1, words)


_FUSED_LOSS = os.environ.get("AVAMD_FUSED_LOSS", "1") != "0"
_VIS_STREAMS = int(os.environ.get("AVAMD_VISUAL_STREAMS", "2"))          # 1: both speakers' lip streams on one side stream


class _CombineFn(torch.autograd.Function):
    """total = mean-reduced CTC of both speakers / 2 + lambda (c1 + c2) / 2 (model/trainer.py:111-119) in one kernel."""

    @staticmethod
    def forward(fctx, nll, w, c1, c2, lam):
        out = torch.empty(3, dtype=torch.float32, device=nll.device)
        c1f = c1.detach().reshape(1).float() if c1.is_cuda else None
        c2f = c2.detach().reshape(1).float() if c2.is_cuda else None
        L.check(L.lib().av_loss_combine(ops.ptr(nll.detach().contiguous()), ops.ptr(w.contiguous()), ops.ptr(c1f), ops.ptr(c2f), 0.5 * lam,
                                        nll.numel(), ops.ptr(out), ops.stream()), "av_loss_combine")
        fctx.save_for_backward(w)
        fctx.lam = lam
        total, l1, l2 = out[0].clone(), out[1].clone(), out[2].clone()
        fctx.mark_non_differentiable(l1, l2)
        return total, l1, l2

    @staticmethod
    def backward(fctx, g, _g1, _g2):
        (w,) = fctx.saved_tensors
        gc = g * (0.5 * fctx.lam)
        return g * w, None, gc, gc, None


class MultimodalTrainer:
    def __init__(self, visual_encoder, audio_encoder, fusion_module, decoder1, tokenizer, learning_rate=1e-4, device="cuda",
                 lambda_=0.1, audio_passes: Optional[int] = None, reducer: Optional[GradBucketReducer] = None, pair_batched: bool = True,
                 visual_side_stream: bool = True, loss_scaling: bool = False, native_ctc: Optional[bool] = None,
                 eval_beam_width: Optional[int] = None, eval_lm=None, eval_lm_weight: Optional[float] = None,
                 eval_token_bonus: Optional[float] = None, eval_report: Optional[bool] = None, eval_bias=None,
                 eval_bias_weight: Optional[float] = None, mwer_weight: Optional[float] = None, mwer_nbest: Optional[int] = None,
                 mwer_beam: Optional[int] = None, mwer_level: str = "word", max_grad_norm: Optional[float] = None,
                 warmup_steps: Optional[int] = None, total_steps: Optional[int] = None, ema_decay: Optional[float] = None,
                 ema_warmup: Optional[bool] = None, eval_ema: Optional[bool] = None, augment=None):
        self.visual_encoder = visual_encoder.to(device)
        self.audio_encoder = audio_encoder.to(device)
        self.fusion_module = fusion_module.to(device)
        self.decoder1 = decoder1.to(device)
        self.tokenizer = tokenizer
        self.device = device
        self.lambda_ = lambda_
        self.audio_passes = audio_passes
        # both speakers go through fusion / BiLSTM / CTC head as ONE 2B batch (items are independent there, so results are
        # identical; it halves the number of latency-bound LSTM step launches), and the frozen visual encoder runs on a
        # side stream concurrently with the wav2vec2 forward
        self.pair_batched = pair_batched
        self.visual_side_stream = visual_side_stream
        self._vstream = None
        self.ctc_loss = nn.CTCLoss(blank=tokenizer.blank_id, zero_infinity=True)       # stays on PyTorch-ROCm (the default)
        # opt-in: the CTC loss of both branches of forward_losses (and so of evaluate()) on the device kernels of ops.ctc_loss.  None reads
        # AVAMD_NATIVE_CTC (default "0") here.  Lengths and targets stay on the device: the step then holds no synchronising call and
        # ignores the host copies ``_ctc_input_lengths`` / ``_ctc_target_lengths`` of host_metadata()
        self.native_ctc = ops.native_ctc_default() if native_ctc is None else bool(native_ctc)
        # opt-in: evaluate() decodes with CTC prefix beam search of this width (beam_search.prefix_beam_search, csrc/ctc_beam.hip).  None reads
        # AVAMD_EVAL_BEAM (default "0") here; 0 = the greedy decode, which is what the reference's simple_beam_search computes
        self.eval_beam_width = int(os.environ.get("AVAMD_EVAL_BEAM", "0")) if eval_beam_width is None else int(eval_beam_width)
        if self.eval_beam_width < 0:
            raise ValueError(f"eval_beam_width must be >= 0, got {self.eval_beam_width}")
        # opt-in: the beam search of evaluate() with n-gram shallow fusion (lm.NGramLM over the tokenizer's ids, csrc/ctc_beam_lm.hip).  eval_lm:
        # an NGramLM or the path of an ARPA file whose tokens are the tokenizer's pieces; None reads AVAMD_EVAL_LM (default: none),
        # AVAMD_EVAL_LM_WEIGHT (0.5) and AVAMD_EVAL_TOKEN_BONUS (0.0).  Used only with eval_beam_width > 0
        eval_lm = os.environ.get("AVAMD_EVAL_LM") or None if eval_lm is None else eval_lm
        if isinstance(eval_lm, (str, os.PathLike)):
            eval_lm = NGramLM.from_arpa(os.fspath(eval_lm), tokenizer.token_to_id, vocab_size=tokenizer.vocab_size, blank=tokenizer.blank_id)
        self.eval_lm = eval_lm
        self.eval_lm_weight = float(os.environ.get("AVAMD_EVAL_LM_WEIGHT", "0.5")) if eval_lm_weight is None else float(eval_lm_weight)
        self.eval_token_bonus = float(os.environ.get("AVAMD_EVAL_TOKEN_BONUS", "0.0")) if eval_token_bonus is None else float(eval_token_bonus)
        if self.eval_lm is not None and self.eval_beam_width == 0:
            raise ValueError("eval_lm needs eval_beam_width > 0: the greedy decode has no language model")
        # opt-in: the beam search of evaluate() with contextual phrase biasing (bias.ContextBias over the tokenizer's ids), with or without
        # eval_lm.  eval_bias: a ContextBias or the path of a phrase file (UTF-8, one phrase per line); None reads AVAMD_EVAL_BIAS (default:
        # none) and AVAMD_EVAL_BIAS_WEIGHT (1.0: a setting, not a tuned value).  Used only with eval_beam_width > 0; unset: none of that code runs
        eval_bias = os.environ.get("AVAMD_EVAL_BIAS") or None if eval_bias is None else eval_bias
        if isinstance(eval_bias, (str, os.PathLike)):
            eval_bias = ContextBias.from_file(os.fspath(eval_bias), tokenizer)
        self.eval_bias = eval_bias
        self.eval_bias_weight = float(os.environ.get("AVAMD_EVAL_BIAS_WEIGHT", "1.0")) if eval_bias_weight is None else float(eval_bias_weight)
        if self.eval_bias is not None and self.eval_beam_width == 0:
            raise ValueError("eval_bias needs eval_beam_width > 0: the greedy decode has no phrase biasing")
        # opt-in: evaluate() also counts token / character / word errors with their S / D / I split on the device (error_rate.error_counts,
        # csrc/error_counts.hip), leaves the rates in ``last_report`` and takes its WER from those counts.  None reads AVAMD_EVAL_REPORT
        # (default "0"); off: none of that code runs
        self.eval_report = os.environ.get("AVAMD_EVAL_REPORT", "0") == "1" if eval_report is None else bool(eval_report)
        self.last_report = None
        # opt-in: minimum word error rate training (mwer.mwer_loss: n-best beam search, error counts and the n-best CTC loss of
        # csrc/ctc_loss.hip, all on the device).  With mwer_weight > 0 and gradients enabled forward_losses adds
        # mwer_weight * (mwer1 + mwer2) / 2 to ``total``; evaluate()'s loss stays the CTC loss.  None reads AVAMD_MWER_WEIGHT (default "0"),
        # AVAMD_MWER_NBEST (4) and AVAMD_MWER_BEAM (8); weight 0: none of that code runs
        self.mwer_weight = float(os.environ.get("AVAMD_MWER_WEIGHT", "0")) if mwer_weight is None else float(mwer_weight)
        self.mwer_nbest = int(os.environ.get("AVAMD_MWER_NBEST", "4")) if mwer_nbest is None else int(mwer_nbest)
        self.mwer_beam = int(os.environ.get("AVAMD_MWER_BEAM", "8")) if mwer_beam is None else int(mwer_beam)
        self.mwer_level = mwer_level
        if not 0.0 <= self.mwer_weight < float("inf"):         # NaN fails both comparisons
            raise ValueError(f"mwer_weight must be finite and >= 0, got {self.mwer_weight}")
        if not 1 <= self.mwer_nbest <= self.mwer_beam <= 64:
            raise ValueError(f"need 1 <= mwer_nbest <= mwer_beam <= 64, got mwer_nbest={self.mwer_nbest} mwer_beam={self.mwer_beam}")
        if mwer_level not in ("word", "char", "token"):
            raise ValueError(f"mwer_level must be 'word', 'char' or 'token', got {mwer_level!r}")
        self._mwer_table = None                                # the tokenizer's PieceTable, built once when the term first runs
        # opt-in: data augmentation on the device (augment.Augment, csrc/augment.hip): in a training step forward_losses feeds the encoders
        # shifted / mirrored / frame-frozen lip clips and the mixture with noise at a drawn SNR, written into buffers this trainer owns (the
        # batch's tensors are never written).  augment: an Augment; None reads AVAMD_AUG_SHIFT / _FLIP / _TMASK / _TMASK_EVERY / _SNR / _SEED
        # (augment.Augment.from_env: nothing set = off).  evaluate() and align() never augment.  Off: none of that code runs and no buffer
        # exists.  Data parallel: each rank adds its rank to the seed, as the dropout generator does
        if augment is not None and not isinstance(augment, Augment):
            raise TypeError(f"augment must be an augment.Augment or None, got {type(augment).__name__}")
        self.augment = Augment.from_env() if augment is None else augment
        self._aug_buf = {}
        self.last_aug_sigma = None                             # noise level per item of the last augmented step, device float32 [B]
        self.parameters = (list(self.visual_encoder.parameters()) + list(self.audio_encoder.parameters())
                           + list(self.fusion_module.parameters()) + list(self.decoder1.parameters()))
        # opt-in: global-norm gradient clipping and a linear warmup / decay of the learning rate inside the fused Adam step (optim.AvAdam,
        # av_adam_multi_ex: norm, clip coefficient and schedule step live on the device, the step still holds no synchronising call).
        # max_grad_norm: torch.nn.utils.clip_grad_norm_'s law; None reads AVAMD_CLIP_NORM (default "0" = off).  warmup_steps / total_steps:
        # optim.lr_multiplier, one multiplier for all four groups (with a warmup the first step runs at multiplier 0, as torch's LambdaLR
        # does); None reads AVAMD_WARMUP_STEPS / AVAMD_TOTAL_STEPS (default "0").  All off: none of that code runs.  Data parallel: the norm
        # is taken after the all-reduce, over grad * grad_scale, so every rank computes the same bits from the same bytes
        max_grad_norm = float(os.environ.get("AVAMD_CLIP_NORM", "0")) if max_grad_norm is None else float(max_grad_norm)
        warmup_steps = int(os.environ.get("AVAMD_WARMUP_STEPS", "0")) if warmup_steps is None else int(warmup_steps)
        total_steps = int(os.environ.get("AVAMD_TOTAL_STEPS", "0")) if total_steps is None else int(total_steps)
        # opt-in: an exponential moving average of the trainable weights kept inside the same fused step (optim.AvAdam(ema_decay=...),
        # av_adam_multi_ema: skipped with an overflowing step on the device, moved for LayerDrop-ped layers too, no synchronising call).
        # ema_decay: None reads AVAMD_EMA_DECAY (default "0" = off); ema_warmup: optim.ema_decay's warmup, None reads AVAMD_EMA_WARMUP
        # ("0").  eval_ema: evaluate() and align() run with the averaged weights (optimizer.averaged(): swapped in and back in place;
        # BatchNorm buffers are not averaged, torch.optim.swa_utils.AveragedModel's default); None reads AVAMD_EVAL_EMA ("0").  Off: none of
        # that code runs.  Data parallel: every rank computes the same averages from the same bytes, nothing is communicated
        ema_decay = float(os.environ.get("AVAMD_EMA_DECAY", "0")) if ema_decay is None else float(ema_decay)
        ema_warmup = os.environ.get("AVAMD_EMA_WARMUP", "0") == "1" if ema_warmup is None else bool(ema_warmup)
        self.eval_ema = os.environ.get("AVAMD_EVAL_EMA", "0") == "1" if eval_ema is None else bool(eval_ema)
        if self.eval_ema and not ema_decay > 0:
            raise ValueError("eval_ema needs ema_decay > 0: there is no averaged model to evaluate")
        self.optimizer = AvAdam([
            {"params": list(self.visual_encoder.parameters()), "lr": learning_rate},
            {"params": list(self.audio_encoder.parameters()), "lr": 2e-5},
            {"params": list(self.fusion_module.parameters()), "lr": learning_rate},
            {"params": list(self.decoder1.parameters()), "lr": learning_rate},
        ], max_grad_norm=max_grad_norm, warmup_steps=warmup_steps, total_steps=total_steps, ema_decay=ema_decay,
            ema_warmup=ema_warmup)                                                          # ValueError on bad values
        self.max_grad_norm, self.warmup_steps, self.total_steps = max_grad_norm, warmup_steps, total_steps
        self.ema_decay, self.ema_warmup = ema_decay, ema_warmup
        # model/trainer.py:40 (GradScaler); off by default: bf16 operands need no loss scaling.  On = the reference's overflow-skip /
        # growth / backoff law, evaluated on the device
        self.scaler = AvGradScaler(device=device, enabled=loss_scaling)
        self.projection_layer = None
        self.fixed_projection = None        # (weight, bias) to inject instead of a fresh random layer (parity tests)
        # decoder + fusion gradients are produced straight into ONE flat buffer (no packing copy before their all-reduce, no per-step
        # allocations, a pointer table of the fused Adam that never changes); the wav2vec2 layers keep one such buffer each
        self._head_arena = GradArena()
        self.fusion_module.grad_arena = self.decoder1.grad_arena = self._head_arena
        self.reducer = reducer
        if reducer is not None:
            self.optimizer.grad_scale = 1.0 / reducer.world
            if reducer.world > 1:
                # the collective schedule must not depend on the rank: LayerDrop decisions come from a generator seeded identically
                # everywhere (every rank draws once per layer and pass), dropout masks from one seeded per rank
                import torch.distributed as dist
                m = self.audio_encoder.model
                m.layerdrop_generator = torch.Generator().manual_seed(0x5EED1A7E)
                m.dropout_generator = torch.Generator().manual_seed(0xD120 + 7919 * dist.get_rank(reducer.group))
                if self.augment is not None:
                    self.augment.rank_offset = dist.get_rank(reducer.group)
            self.audio_encoder.model.grad_ready = reducer.reduce_async
            self.audio_encoder.model.grad_flat_ready = reducer.reduce_flat
            self.audio_encoder.model.grad_wait = reducer.wait
            self._head_params = [p for m in (self.decoder1, self.fusion_module) for n, p in m.named_parameters()
                                 if not n.startswith("cross_attn_visual.")]
            # decoder + fusion gradients are complete when the wav2vec2 backward starts (their AccumulateGrad nodes run with top
            # priority right after the fusion backward): start their all-reduce there, under the whole audio backward
            self._head_done = False
            if pair_batched:                                   # one fusion / decoder call per step: no later accumulation into these grads
                self.audio_encoder.model.grad_pre = self._reduce_head_early

    # ------------------------------------------------------------------------------------------------------------
    def _to_dev(self, batch):
        dev = self.device
        nb = lambda t: t.to(dev, non_blocking=True)
        d = {k: nb(batch[k]) for k in ("audio", "mask1", "mask2", "text1", "text2", "text1_lengths", "text2_lengths")}
        # [B,T,1,H,W] -> [B,1,T,H,W]: with one channel the two layouts are byte-identical => a view
        d["lip1"] = nb(batch["lip1"]).permute(0, 2, 1, 3, 4)
        d["lip2"] = nb(batch["lip2"]).permute(0, 2, 1, 3, 4)
        return d

    def _mask_ds(self, mask, T_enc):
        B, Tin = mask.shape
        out = torch.empty((B, T_enc), dtype=torch.long, device=mask.device)
        L.check(L.lib().av_mask_downsample(ops.ptr(mask.contiguous()), ops.ptr(out), B, Tin, T_enc, ops.stream()), "av_mask_downsample")
        return out

    @staticmethod
    def _mask_ds_host(mask_cpu: torch.Tensor, T_enc: int) -> torch.Tensor:
        """Host restatement of av_mask_downsample (nearest index floor(i * Tin / T_enc), fp32 as on the device)."""
        mask_cpu = mask_cpu.cpu()
        Tin = mask_cpu.shape[1]
        scale = torch.tensor(Tin / T_enc, dtype=torch.float32)
        idx = torch.floor(torch.arange(T_enc, dtype=torch.float32) * scale).long().clamp_(max=Tin - 1)
        return mask_cpu[:, idx]

    @staticmethod
    def _class_counts(mask_cpu: torch.Tensor, T_enc: int):
        """(#1, #2, #0) of the down-sampled mask, computed on the host copy of the batch (no device sync when the
        batch arrives from a DataLoader; a device-resident batch should carry precomputed ``_counts1/_counts2``)."""
        c = torch.bincount(MultimodalTrainer._mask_ds_host(mask_cpu, T_enc).reshape(-1).clamp(0, 3), minlength=4).tolist()
        return (c[1], c[2], c[0])

    @staticmethod
    def _fusion_lengths_host(mask_cpu: torch.Tensor, T_enc: int, Tv: int) -> torch.Tensor:
        """Host restatement of the ``input_lengths`` CrossAttentionFusion returns for ONE call (model/fusion_module.py:41-59 of the
        reference; av_fusion_gather_lerp_fwd here): n_b speech frames (mask 1/2) are kept per item and padded to the call's
        maximum Tm, the mask is resampled to Tv frames with nearest index floor(i * Tm / Tv), and the length is the number
        of resampled positions that fall on a kept frame."""
        import numpy as np
        m = MultimodalTrainer._mask_ds_host(mask_cpu, T_enc)
        n = ((m == 1) | (m == 2)).sum(1).numpy().astype(np.int64)
        Tm = int(n.max()) if n.size else 0
        i = np.arange(Tv, dtype=np.float32)
        if Tm == Tv:
            j = np.arange(Tv, dtype=np.int64)
        else:
            j = np.floor(i * (np.float32(Tm) / np.float32(Tv))).astype(np.int64)
            j = np.minimum(j, max(Tm - 1, 0))
        return torch.from_numpy((j[None, :] < n[:, None]).sum(1).astype(np.int64))

    def host_metadata(self, cpu_batch: Dict[str, torch.Tensor], T_enc: int) -> Dict[str, object]:
        """Everything the step would otherwise read back from the device, computed from the HOST copy of a collated batch:
        contrastive class counts and the CTC length vectors (nn.functional.ctc_loss wants its lengths on the host; handing
        it device tensors costs a full device synchronisation per call).  Keys start with ``_``; merge into the batch."""
        Tv = cpu_batch["lip1"].shape[1]
        il = torch.cat([self._fusion_lengths_host(cpu_batch["mask1"], T_enc, Tv), self._fusion_lengths_host(cpu_batch["mask2"], T_enc, Tv)])
        tl = torch.cat([cpu_batch["text1_lengths"].cpu().long(), cpu_batch["text2_lengths"].cpu().long()])
        return {"_counts1": self._class_counts(cpu_batch["mask1"], T_enc), "_counts2": self._class_counts(cpu_batch["mask2"], T_enc),
                "_ctc_input_lengths": il, "_ctc_target_lengths": tl,
                "_same_padding": bool(torch.equal(cpu_batch["mask1"] != 3, cpu_batch["mask2"] != 3)),
                "_audio_valid1": (cpu_batch["mask1"] != 3).sum(1).tolist(), "_audio_valid2": (cpu_batch["mask2"] != 3).sum(1).tolist()}

    def forward_losses(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """model/trainer.py:66-119 for one batch; everything stays on the device.

        With ``native_ctc`` nothing in here synchronises, so the BiLSTM timeout words staged by a step are normally evaluated at the
        start of the NEXT call (or at the end of train_epoch / evaluate()): the RuntimeError of a timed-out persistent LSTM launch then
        names the previous step, not the one that is being enqueued."""
        if self.native_ctc:
            self.fusion_module.finish_flag_check(wait=True)        # staged one step ago: its event has completed unless the host runs far ahead
        d = self._to_dev(batch)
        if self.augment is not None and torch.is_grad_enabled() and self.decoder1.training and self.audio_encoder.training:
            self._augment_inputs(d, batch)                         # on the main stream, before the lip streams fork
        use_side = self.visual_side_stream and d["audio"].is_cuda
        if use_side:
            # the frozen visual encoder runs beside the wav2vec2 forward, one stream per speaker: its HBM-bound BatchNorm / pooling passes overlap
            # the other streams' MFMA-bound kernels
            dev_ = d["audio"].device
            if self._vstream is None:
                self._vstream = torch.cuda.Stream(device=dev_)
                self._vstream2 = torch.cuda.Stream(device=dev_) if _VIS_STREAMS >= 2 else self._vstream
            main = torch.cuda.current_stream(dev_)
            two = self._vstream2 is not self._vstream
            evs = []
            from ..precision import compute_dtype
            self.visual_encoder.warm_caches(compute_dtype())       # weight re-layouts are built on main, before the lip streams fork
            self._vstream.wait_stream(main)
            with torch.cuda.stream(self._vstream):
                if two:
                    self.visual_encoder._bn_sync, self.visual_encoder._bn_idx = ("lead", evs), 0
                vf1 = self.visual_encoder(d["lip1"])
            if two:
                self._vstream2.wait_stream(main)
                self.visual_encoder._bn_sync, self.visual_encoder._bn_idx = ("follow", evs), 0
            try:
                with torch.cuda.stream(self._vstream2):
                    vf2 = self.visual_encoder(d["lip2"])
            finally:
                self.visual_encoder._bn_sync = None
        else:
            vf1 = self.visual_encoder(d["lip1"])
            vf2 = self.visual_encoder(d["lip2"])
        attn1 = d["mask1"] != 3
        passes = self.audio_passes
        if passes is None:      # auto: the duplicate pass only differs when a stochastic regulariser is active in train mode
            cfg = getattr(self.audio_encoder.model, "cfg", {})
            knobs = ("hidden_dropout", "attention_dropout", "activation_dropout", "feat_proj_dropout", "layerdrop", "mask_time_prob")
            passes = 2 if (self.audio_encoder.training and any(cfg.get(k, 0) > 0 for k in knobs)) else 1
        if passes == 1:
            # one pass stands for both only if the two padding patterns are the same (they are for the reference's dataset, SURVEY
            # §0.3; a batch from elsewhere falls back to two passes).  Host copy when available, otherwise one device comparison
            same = batch.get("_same_padding")
            if same is None:
                same = bool(torch.equal(batch["mask1"] != 3, batch["mask2"] != 3))
            if not same:
                passes = 2
        if passes == 2:
            self.audio_encoder.model._feat_cache = {}              # both passes read the same waveform: one conv feature-extractor run
        try:
            v1, v2 = batch.get("_audio_valid1"), batch.get("_audio_valid2")      # host copies of the valid lengths (host_metadata)
            if v1 is None and not batch["mask1"].is_cuda:                        # batch straight from a DataLoader: the masks ARE on the host
                v1, v2 = (batch["mask1"] != 3).sum(1).tolist(), (batch["mask2"] != 3).sum(1).tolist()
            if passes == 2:
                a1, mid1, a2, mid2 = self.audio_encoder.forward_pair(d["audio"], attn1, d["mask2"] != 3, v1, v2)
            else:
                a1, mid1 = self.audio_encoder(d["audio"], attention_mask=attn1, valid_lengths=v1)
                a2, mid2 = a1, mid1
        finally:
            self.audio_encoder.model._feat_cache = None
        T_enc, D = a1.shape[1], a1.shape[2]
        m1 = self._mask_ds(d["mask1"], T_enc)
        m2 = self._mask_ds(d["mask2"], T_enc)
        out = {}
        if self.lambda_ != 0:
            if self.projection_layer is None:
                self.projection_layer = nn.Linear(D, 128).to(self.device)          # model/trainer.py:105-106
                if self.fixed_projection is not None:
                    with torch.no_grad():
                        self.projection_layer.weight.copy_(self.fixed_projection[0]); self.projection_layer.bias.copy_(self.fixed_projection[1])
            k1 = batch.get("_counts1") or self._class_counts(batch["mask1"], T_enc)
            k2 = batch.get("_counts2") or self._class_counts(batch["mask2"], T_enc)
            c1 = contrastive_loss_with_mask(mid1, m1.reshape(-1), self.projection_layer, counts=k1)
            c2 = contrastive_loss_with_mask(mid2, m2.reshape(-1), self.projection_layer, counts=k2)
        else:
            c1 = c2 = torch.zeros((), device=a1.device)
        if use_side:
            main.wait_stream(self._vstream)
            if self._vstream2 is not self._vstream:
                main.wait_stream(self._vstream2)
            vf1.record_stream(main); vf2.record_stream(main)
        B = a1.shape[0]
        # the two speakers go through fusion / decoder / CTC as one stacked call only if their lip clips were padded to the same length;
        # the reference's collate pads lip1 and lip2 separately (dataset/collate_fn.py:8-13,27-31), so a real batch can differ - then one
        # call per speaker, as the reference does (found by tests/test_dataset_gpu.py::test_dataset_feeds_the_training_step)
        pair = self.pair_batched and vf1.shape[1] == vf2.shape[1]
        self._pair_step = pair
        if pair:
            f12, il12 = self.fusion_module(torch.cat([vf1, vf2], 0), torch.cat([a1, a2], 0), mask=torch.cat([m1, m2], 0), groups=2)
            lp12 = self.decoder1(f12)
            f1, f2, il1, il2, lp1, lp2 = f12[:B], f12[B:], il12[:B], il12[B:], lp12[:B], lp12[B:]
        else:
            f1, il1 = self.fusion_module(vf1, a1, mask=m1)
            f2, il2 = self.fusion_module(vf2, a2, mask=m2)
            lp1 = self.decoder1(f1)
            lp2 = self.decoder1(f2)
        if pair:
            # one nn.functional.ctc_loss call (PyTorch-ROCm, as north_star prescribes) over the 2B items; 'mean' reduction
            # of nn.CTCLoss = mean_i(nll_i / clamp(target_len_i, 1)) is re-applied per speaker half
            t1, t2 = d["text1"], d["text2"]
            Lm = max(t1.shape[1], t2.shape[1])
            tg = torch.cat([F.pad(t1, (0, Lm - t1.shape[1])), F.pad(t2, (0, Lm - t2.shape[1]))], 0)
            tl = torch.cat([d["text1_lengths"], d["text2_lengths"]], 0)
            il_h, tl_h = batch.get("_ctc_input_lengths"), batch.get("_ctc_target_lengths")     # host copies: no device sync in ctc_loss
            w_ctc = (0.5 / B) / tl.clamp_min(1).to(torch.float32)        # weights of the per-speaker means (before the CTC call: off the sync)
            self.fusion_module.stage_flag_check()                  # BiLSTM timeout words -> pinned memory, visible after ctc_loss's own sync
            if self.native_ctc:
                # device CTC: lengths and targets are read from device memory, nothing blocks (the staged words are looked at below if
                # their copy happens to be complete, otherwise by the next forward_losses / train_epoch / evaluate())
                nll = ops.ctc_loss(lp12, tg, il12, tl, blank=self.tokenizer.blank_id, reduction="none", zero_infinity=True, batch_first=True)
            else:
                nll = F.ctc_loss(lp12.transpose(0, 1), tg, il12 if il_h is None else il_h, tl if tl_h is None else tl_h,
                                 blank=self.tokenizer.blank_id, reduction="none", zero_infinity=True)
            self.fusion_module.finish_flag_check()                 # raises if a persistent BiLSTM launch timed out (event query, no sync)
            if nll.is_cuda and nll.dtype == torch.float32 and _FUSED_LOSS:
                total, l1, l2 = _CombineFn.apply(nll, w_ctc, c1, c2, float(self.lambda_))    # one kernel forward, one backward
            else:
                per = nll / tl.clamp_min(1).to(nll.dtype)
                l1, l2 = per[:B].mean(), per[B:].mean()
                total = None
        else:
            total = None
            if self.native_ctc:
                kw = dict(blank=self.tokenizer.blank_id, reduction="mean", zero_infinity=True, batch_first=True)
                self.fusion_module.stage_flag_check()
                l1 = ops.ctc_loss(lp1, d["text1"], il1, d["text1_lengths"], **kw)
                l2 = ops.ctc_loss(lp2, d["text2"], il2, d["text2_lengths"], **kw)
                self.fusion_module.finish_flag_check()
            else:
                l1 = self.ctc_loss(lp1.transpose(0, 1), d["text1"], il1, d["text1_lengths"])
                l2 = self.ctc_loss(lp2.transpose(0, 1), d["text2"], il2, d["text2_lengths"])
        if total is None:
            total = (l1 + l2) / 2 + self.lambda_ * (c1 + c2) / 2
        if self.mwer_weight > 0 and torch.is_grad_enabled():
            # the MWER term meets the CTC term at the log-probs through autograd, as the contrastive and CTC terms meet further down
            if pair:
                per = self._mwer(lp12, tg, tl, il12)
                mw1, mw2 = per[:B].mean(), per[B:].mean()
            else:
                mw1 = self._mwer(lp1, d["text1"], d["text1_lengths"], il1).mean()
                mw2 = self._mwer(lp2, d["text2"], d["text2_lengths"], il2).mean()
            total = total + self.mwer_weight * (mw1 + mw2) / 2
            out.update(mwer1=mw1, mwer2=mw2)
        out.update(visual_feat1=vf1, visual_feat2=vf2, audio_last=a1, audio_mid=mid1, fused1=f1, fused2=f2, input_lengths1=il1,
                   input_lengths2=il2, log_probs1=lp1, log_probs2=lp2, loss1=l1, loss2=l2, contrast1=c1, contrast2=c2, total=total)
        return out

    def _aug_buffer(self, name: str, like: torch.Tensor) -> torch.Tensor:
        buf = self._aug_buf.get(name)
        if buf is None or buf.shape != like.shape or buf.device != like.device:
            buf = self._aug_buf[name] = torch.empty(like.shape, dtype=torch.float32, device=like.device)
        return buf

    def _augment_inputs(self, d, batch) -> None:
        """Replaces d["lip1"], d["lip2"] and d["audio"] by their augmented versions of step ``augment.step``, in buffers reused from step to
        step (the previous step's readers have finished in stream order: the lip streams are joined before the fusion).  Valid lengths stay
        on the device; nothing synchronises."""
        aug = self.augment
        if aug.lips_on:
            for spk in (1, 2):
                key = f"lip{spk}"
                d[key] = aug.lips(d[key], batch.get(key + "_lengths"), aug.step, spk, out=self._aug_buffer(key, d[key]))
        if aug.noise_on:
            B = d["audio"].shape[0]
            sg = self._aug_buf.get("sigma")
            if sg is None or sg.shape[0] != B or sg.device != d["audio"].device:
                sg = self._aug_buf["sigma"] = torch.empty((B,), dtype=torch.float32, device=d["audio"].device)
            d["audio"], self.last_aug_sigma = aug.noise(d["audio"], (d["mask1"] != 3).sum(1), aug.step,
                                                        out=self._aug_buffer("audio", d["audio"]), sigma=sg)

    def _mwer(self, lp, refs, ref_lengths, input_lengths):
        """Per-utterance MWER risk [B] of one decoder call (mwer.mwer_loss, reduction "none"); float32 log-probs as the CTC loss reads them."""
        from ..mwer import mwer_loss
        if self.mwer_level != "token" and self._mwer_table is None:
            from ..error_rate import PieceTable
            self._mwer_table = PieceTable.from_tokenizer(self.tokenizer)
        return mwer_loss(lp.float(), refs, ref_lengths, input_lengths, self.tokenizer.blank_id, nbest=self.mwer_nbest,
                         beam_width=self.mwer_beam, table=self._mwer_table, level=self.mwer_level, reduction="none")

    def train_step(self, batch) -> Dict[str, torch.Tensor]:
        """zero_grad -> forward -> backward (-> bucketed all-reduce) -> Adam; no host sync.  With max_grad_norm > 0 the result also has
        ``grad_norm``: the global gradient norm before clipping, a device scalar."""
        self.optimizer.zero_grad(set_to_none=True)
        self._head_arena.begin_step()
        begin = getattr(self.audio_encoder.model, "begin_grad_step", None)
        if begin is not None:
            begin()
        if self.reducer is not None:
            self._head_done = False
        out = self.forward_losses(batch)
        if self.augment is not None:
            self.augment.step += 1                                 # once per training step: the next step draws a new plan
        self.scaler.scale(out["total"]).backward()                 # model/trainer.py:121
        self._head_arena.finalize()
        if self.reducer is not None:
            # wav2vec2 layer buckets were reduced inside its backward (overlapped), the decoder + fusion bucket at its start; if that
            # backward did not run (nothing trainable below the fusion) the bucket goes now
            if not self._head_done:
                self._reduce_head()
            self.reducer.wait()
            self._head_done = False
        self.scaler.step(self.optimizer)                           # model/trainer.py:122-123 (update() is part of the device-side step)
        self.scaler.update()
        if self.optimizer.clipping:
            out["grad_norm"] = self.optimizer.last_grad_norm
        return out

    def _reduce_head_early(self):
        # hook at the start of the wav2vec2 backward: valid only when this step made ONE fusion / decoder call (a batch whose two lip
        # clips were padded differently falls back to one call per speaker: its head bucket goes after the backward, in train_step)
        if getattr(self, "_pair_step", True):
            self._reduce_head()

    def _reduce_head(self):
        # once per step: with two audio passes the wav2vec2 backward (and this hook) runs twice, and p.grad are by then views of the
        # already reduced bucket (a second all-reduce would sum them world_size times)
        if self._head_done:
            return
        hp = [p for p in self._head_params if p.grad is not None]
        ar = self._head_arena
        if hp and ar.flat is not None and all(ar.owns(p.grad) for p in hp):
            self.reducer.reduce_flat(ar)                           # the gradients ARE the bucket: all-reduced in place, nothing is packed
        else:                                                      # first step (layout still being discovered) / two fusion calls per step
            for p, v in zip(hp, self.reducer.reduce_async([p.grad for p in hp])):
                p.grad = v
        self._head_done = True

    def train_epoch(self, dataloader):
        self.visual_encoder.train(); self.audio_encoder.train(); self.fusion_module.train(); self.decoder1.train()
        self.projection_layer = None
        total_loss = 0.0
        for batch_idx, batch in enumerate(dataloader):
            try:
                out = self.train_step(batch)
                total_loss += out["total"].item()
                if batch_idx % 100 == 0:
                    print(f"[Batch {batch_idx}] CTC1: {out['loss1'].item():.4f}, CTC2: {out['loss2'].item():.4f}, "
                          f"Contrast1: {float(out['contrast1']):.4f}, Contrast2: {float(out['contrast2']):.4f}, "
                          f"Total: {out['total'].item():.4f}", flush=True)
                    if self.optimizer.clipping or self.optimizer.scheduled:
                        print(f"[Batch {batch_idx}] grad norm: {float(self.optimizer.last_grad_norm):.4f}, "
                              f"LR multiplier: {float(self.optimizer.last_lr_mult):.4f}", flush=True)
            except NotImplementedError:  # a configuration this build does not cover: every later batch would fail the same way
                raise
            except Exception as e:       # model/trainer.py:162-164: skip the batch, keep going
                print(f"Error at batch {batch_idx}: {e}", flush=True)
                if self.reducer is not None and self.reducer.world > 1:
                    # data parallel: a rank that skips a batch no longer issues the collectives its peers are waiting in
                    raise
                continue
        if self.native_ctc:
            self.fusion_module.drain_flag_check()                  # the last step's timeout words: nothing stays pending past the epoch
        return total_loss / max(1, len(dataloader))

    def ctc_decode(self, pred_ids):
        """model/trainer.py:168-177 (prev is NOT reset on blank — kept as in the reference's debug helper)."""
        result, prev = [], None
        for idx in pred_ids:
            if idx == self.tokenizer.blank_id:
                continue
            if idx != prev:
                result.append(idx)
            prev = idx
        return result

    def evaluate(self, dataloader):
        """(loss, WER) over the loader.  With ``eval_ema`` the loop runs on the averaged weights and the trained ones are back afterwards."""
        if self.eval_ema:
            with self.optimizer.averaged():
                return self._evaluate(dataloader)
        return self._evaluate(dataloader)

    @torch.no_grad()
    def _evaluate(self, dataloader):
        self.visual_encoder.eval(); self.audio_encoder.eval(); self.fusion_module.eval(); self.decoder1.eval()
        refs1, hyps1, refs2, hyps2 = [], [], [], []
        total_loss = 0.0
        lam, self.lambda_ = self.lambda_, 0.0
        self.last_report = None
        report = self._report_begin() if self.eval_report else None
        try:
            for batch in dataloader:
                out = self.forward_losses(batch)
                total_loss += (out["loss1"].item() + out["loss2"].item()) / 2
                for spk, lp, refs, hyps in (("1", out["log_probs1"], refs1, hyps1), ("2", out["log_probs2"], refs2, hyps2)):
                    if self.eval_beam_width > 0 and self.eval_bias is not None:
                        fusion = {} if self.eval_lm is None else dict(lm=self.eval_lm, lm_weight=self.eval_lm_weight,
                                                                      token_bonus=self.eval_token_bonus)
                        ids = prefix_beam_search(lp, self.eval_beam_width, self.tokenizer.blank_id, bias=self.eval_bias,
                                                 bias_weight=self.eval_bias_weight, **fusion)
                    elif self.eval_beam_width > 0 and self.eval_lm is not None:
                        ids = prefix_beam_search(lp, self.eval_beam_width, self.tokenizer.blank_id, lm=self.eval_lm,
                                                 lm_weight=self.eval_lm_weight, token_bonus=self.eval_token_bonus)
                    elif self.eval_beam_width > 0:
                        ids = prefix_beam_search(lp, self.eval_beam_width, self.tokenizer.blank_id)
                    else:
                        ids = greedy_batch(lp, self.tokenizer.blank_id)   # == simple_beam_search best beam
                    txt, tl = batch["text" + spk], batch["text" + spk + "_lengths"]
                    for i, seq in enumerate(ids):
                        hyps.append(fast_decode(seq, self.tokenizer))
                        refs.append(self.tokenizer.decode(txt[i][: int(tl[i])].tolist()))
                    if report is not None:
                        self._report_add(report, spk, txt, tl, ids)
            if self.native_ctc:
                self.fusion_module.drain_flag_check()
        finally:
            self.lambda_ = lam
        if report is not None:
            wer1, wer2 = self._report_finish(report)
        else:
            wer1, wer2 = word_error_rate(refs1, hyps1), word_error_rate(refs2, hyps2)
        avg_wer = (wer1 + wer2) / 2
        avg_loss = total_loss / max(1, len(dataloader))
        print(f"[Eval] WER1: {wer1:.3f}, WER2: {wer2:.3f}, Avg: {avg_wer:.3f}, Loss: {avg_loss:.4f}")
        self.last_decoded = (hyps1, hyps2)
        return avg_loss, avg_wer

    # evaluate()'s opt-in report: error counts of both speakers on the device, one accumulator, one transfer after the loop
    def _report_begin(self):
        from ..error_rate import PieceTable
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("MultimodalTrainer.evaluate: eval_report counts errors on the GPU; there is no CPU fallback")
        return {"table": PieceTable.from_tokenizer(self.tokenizer), "acc": torch.zeros((2, 3, 4), dtype=torch.int64, device=self.device)}

    def _report_add(self, report, spk, txt, tl, ids):
        from ..error_rate import error_counts
        # references as evaluate() decodes them (nothing skipped), hypotheses as fast_decode does (the blank skipped)
        counts = error_counts(txt.to(self.device, non_blocking=True), ids, ref_lengths=tl, table=report["table"], ref_skip=-1,
                              hyp_skip=self.tokenizer.blank_id)
        best = counts[:, 0].long()
        report["acc"][int(spk) - 1] += (best * (best[:, :, 3:4] >= 0)).sum(0)          # a level of -1 (a text beyond the limit) adds nothing

    def _report_finish(self, report):
        from ..error_rate import rates
        acc = report["acc"].cpu()
        self.last_report = {"speaker1": rates(acc[0]), "speaker2": rates(acc[1])}
        return self.last_report["speaker1"]["word"]["rate"], self.last_report["speaker2"]["word"]["rate"]

    def align(self, batch, frame_rate: float = 25.0):
        """``_align`` - on the averaged weights with ``eval_ema``."""
        if self.eval_ema:
            with self.optimizer.averaged():
                return self._align(batch, frame_rate)
        return self._align(batch, frame_rate)

    @torch.no_grad()
    def _align(self, batch, frame_rate: float = 25.0):
        """Word times of both speakers' transcripts in one batch: CTC forced alignment (align.forced_align, csrc/ctc_align.hip) of
        ``text*`` against the log-probs of ONE forward_losses call in eval mode.  Returns (segments1, segments2): per utterance the
        ``align.word_segments`` list ([] for a transcript that cannot be aligned).  The CTC head runs at the lip-frame rate, so
        ``frame_rate`` is the video's.  One device-to-host transfer per speaker; every module's train / eval mode is restored."""
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("MultimodalTrainer.align: the model runs on the GPU; there is no CPU fallback")
        mods = (self.visual_encoder, self.audio_encoder, self.fusion_module, self.decoder1)
        modes = [(sm, sm.training) for m in mods for sm in m.modules()]      # per sub-module: a frozen part may sit in eval mode
        for m in mods:
            m.eval()
        lam, self.lambda_ = self.lambda_, 0.0              # as evaluate(): no contrastive term (and no projection layer is created)
        try:
            out = self.forward_losses(batch)
            if self.native_ctc:
                self.fusion_module.drain_flag_check()
            res = []
            for spk in ("1", "2"):
                txt, tl = batch["text" + spk], batch["text" + spk + "_lengths"]
                al = forced_align(out["log_probs" + spk], txt, out["input_lengths" + spk], tl, blank=self.tokenizer.blank_id)
                # spans and the token scores' bits in one int32 block [B][Lmax][3]: a single transfer
                packed = torch.cat([al.spans, al.token_scores.view(torch.int32)[..., None]], dim=2).cpu()
                spans, tok = packed[..., :2], packed[..., 2].contiguous().view(torch.float32)
                txt_h, tl_h = txt.cpu(), tl.cpu().tolist()
                res.append([word_segments(self.tokenizer, txt_h[i, :max(0, int(tl_h[i]))], spans[i], tok[i], frame_rate)
                            for i in range(txt_h.shape[0])])
        finally:
            self.lambda_ = lam
            for sm, was in modes:
                sm.training = was
        return tuple(res)
