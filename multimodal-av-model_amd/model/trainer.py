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

import contextlib
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
from ..error_rate import PieceTable, error_counts, rates, word_error_rate
from ..optim import AvAdam, AvGradScaler
from ..parallel.dp import GradArena, GradBucketReducer
from . import host_meta, options


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
                 ema_warmup: Optional[bool] = None, eval_ema: Optional[bool] = None, augment=None, conf_method: Optional[str] = None,
                 conf_alpha: Optional[float] = None, conf_aggregation: Optional[str] = None, weight_decay: Optional[float] = None,
                 lr_schedule: Optional[str] = None, accum_steps: Optional[int] = None, long_window: Optional[int] = None,
                 long_stride: Optional[int] = None, long_policy: Optional[str] = None, long_batch: Optional[int] = None,
                 long_segment: Optional[int] = None, long_radius: Optional[int] = None, spot_min_score: Optional[float] = None,
                 spot_max_hits: Optional[int] = None, segment_window: Optional[int] = None, segment_free: Optional[int] = None):
        """The opt-in settings (a None argument reads its AVAMD_* variable here) are the rows of model/options.py."""
        self.visual_encoder = visual_encoder.to(device)
        self.audio_encoder = audio_encoder.to(device)
        self.fusion_module = fusion_module.to(device)
        self.decoder1 = decoder1.to(device)
        self.tokenizer = tokenizer
        self.device = device
        self.lambda_ = lambda_
        self.audio_passes = audio_passes
        # both speakers go through fusion / BiLSTM / CTC head as ONE 2B batch (items are independent there, so results are identical; it halves the
        # number of latency-bound LSTM step launches), and the frozen visual encoder runs on side streams concurrently with the wav2vec2 forward
        self.pair_batched = pair_batched
        self.visual_side_stream = visual_side_stream
        self._vstream = None
        self.ctc_loss = nn.CTCLoss(blank=tokenizer.blank_id, zero_infinity=True)       # stays on PyTorch-ROCm (the default)
        opt = options.resolve
        self.native_ctc = opt("native_ctc", native_ctc)
        self._resolve_decode(eval_beam_width, eval_lm, eval_lm_weight, eval_token_bonus, eval_bias, eval_bias_weight)
        self.eval_report, self.last_report = opt("eval_report", eval_report), None
        self.conf_method, self.conf_alpha = opt("conf_method", conf_method), opt("conf_alpha", conf_alpha)
        self.conf_aggregation = opt("conf_aggregation", conf_aggregation)
        options.check_confidence(self.conf_method, self.conf_alpha, self.conf_aggregation)
        self.long_window, self.long_stride = opt("long_window", long_window), opt("long_stride", long_stride)
        self.long_policy, self.long_batch = opt("long_policy", long_policy), opt("long_batch", long_batch)
        self.long_segment, self.long_radius = opt("long_segment", long_segment), opt("long_radius", long_radius)
        options.check_longform(self.long_window, self.long_stride, self.long_policy, self.long_batch, self.long_segment, self.long_radius)
        self.spot_min_score, self.spot_max_hits = opt("spot_min_score", spot_min_score), opt("spot_max_hits", spot_max_hits)
        options.check_spot(self.spot_min_score, self.spot_max_hits)
        self.segment_window, self.segment_free = opt("segment_window", segment_window), opt("segment_free", segment_free)
        options.check_segmentation(self.segment_window, self.segment_free)
        self.mwer_weight, self.mwer_nbest = opt("mwer_weight", mwer_weight), opt("mwer_nbest", mwer_nbest)
        self.mwer_beam, self.mwer_level = opt("mwer_beam", mwer_beam), mwer_level
        options.check_mwer(self.mwer_weight, self.mwer_nbest, self.mwer_beam, mwer_level)
        self._mwer_table = None                                # the tokenizer's PieceTable, built once when the term first runs
        # augmentation on the device (augment.Augment: None reads AVAMD_AUG_*, nothing set = off): in a training step forward_losses feeds the
        # encoders augmented lip clips and mixture, written into buffers this trainer owns; evaluate() and align() never augment
        if augment is not None and not isinstance(augment, Augment):
            raise TypeError(f"augment must be an augment.Augment or None, got {type(augment).__name__}")
        self.augment = Augment.from_env() if augment is None else augment
        self._aug_buf = {}
        self.last_aug_sigma = None                             # noise level per item of the last augmented step, device float32 [B]
        self.parameters = (list(self.visual_encoder.parameters()) + list(self.audio_encoder.parameters())
                           + list(self.fusion_module.parameters()) + list(self.decoder1.parameters()))
        self.max_grad_norm, self.warmup_steps = opt("max_grad_norm", max_grad_norm), opt("warmup_steps", warmup_steps)
        self.total_steps = opt("total_steps", total_steps)
        self.weight_decay, self.lr_schedule = opt("weight_decay", weight_decay), opt("lr_schedule", lr_schedule)
        options.check_schedule(self.lr_schedule, self.total_steps)
        self.ema_decay, self.ema_warmup = opt("ema_decay", ema_decay), opt("ema_warmup", ema_warmup)
        self.eval_ema = opt("eval_ema", eval_ema)
        options.check_ema(self.eval_ema, self.ema_decay)
        self.accum_steps = opt("accum_steps", accum_steps)
        options.check_accum(self.accum_steps)
        self.optimizer = AvAdam([
            {"params": list(self.visual_encoder.parameters()), "lr": learning_rate},
            {"params": list(self.audio_encoder.parameters()), "lr": 2e-5},
            {"params": list(self.fusion_module.parameters()), "lr": learning_rate},
            {"params": list(self.decoder1.parameters()), "lr": learning_rate},
        ], max_grad_norm=self.max_grad_norm, warmup_steps=self.warmup_steps, total_steps=self.total_steps, ema_decay=self.ema_decay,
            ema_warmup=self.ema_warmup, weight_decay=self.weight_decay, lr_schedule=self.lr_schedule)    # ValueError on bad values
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
            self._attach_reducer(reducer)

    def _resolve_decode(self, beam, lm, lm_weight, token_bonus, bias, bias_weight):
        """evaluate()'s decoder settings; a path is loaded here.  The language model and the phrases are used only by the beam search."""
        opt, tok = options.resolve, self.tokenizer
        self.eval_beam_width = opt("eval_beam_width", beam)
        if self.eval_beam_width < 0:
            raise ValueError(f"eval_beam_width must be >= 0, got {self.eval_beam_width}")
        lm = opt("eval_lm", lm)
        if isinstance(lm, (str, os.PathLike)):
            lm = NGramLM.from_arpa(os.fspath(lm), tok.token_to_id, vocab_size=tok.vocab_size, blank=tok.blank_id)
        self.eval_lm, self.eval_lm_weight = lm, opt("eval_lm_weight", lm_weight)
        self.eval_token_bonus = opt("eval_token_bonus", token_bonus)
        options.check_decode(self.eval_beam_width, "eval_lm", lm, "language model")
        bias = opt("eval_bias", bias)
        if isinstance(bias, (str, os.PathLike)):
            bias = ContextBias.from_file(os.fspath(bias), tok)
        self.eval_bias, self.eval_bias_weight = bias, opt("eval_bias_weight", bias_weight)
        options.check_decode(self.eval_beam_width, "eval_bias", bias, "phrase biasing")

    def _attach_reducer(self, reducer):
        """Data parallelism: gradient buckets go to ``reducer`` as the backward produces them, the fused Adam averages over the ranks."""
        self.optimizer.grad_scale = 1.0 / reducer.world
        if reducer.world > 1:
            # the collective schedule must not depend on the rank: LayerDrop decisions come from a generator seeded identically
            # everywhere (every rank draws once per layer and pass), dropout masks and augmentation plans from ones seeded per rank
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
        if self.pair_batched:                              # one fusion / decoder call per step: no later accumulation into these grads
            self.audio_encoder.model.grad_pre = self._reduce_head_early

    def _to_dev(self, batch):
        dev = self.device
        nb = lambda t: t.to(dev, non_blocking=True)
        d = {k: nb(batch[k]) for k in ("audio", "mask1", "mask2")}
        d.update((k, nb(batch[k])) for k in ("text1", "text2", "text1_lengths", "text2_lengths") if k in batch)    # an unlabeled batch has none
        # [B,T,1,H,W] -> [B,1,T,H,W]: with one channel the two layouts are byte-identical => a view
        d["lip1"] = nb(batch["lip1"]).permute(0, 2, 1, 3, 4)
        d["lip2"] = nb(batch["lip2"]).permute(0, 2, 1, 3, 4)
        return d

    def _mask_ds(self, mask, T_enc):
        B, Tin = mask.shape
        out = torch.empty((B, T_enc), dtype=torch.long, device=mask.device)
        L.check(L.lib().av_mask_downsample(ops.ptr(mask.contiguous()), ops.ptr(out), B, Tin, T_enc, ops.stream()), "av_mask_downsample")
        return out

    # host restatements of what the step would otherwise read back from the device (model/host_meta.py)
    _mask_ds_host = staticmethod(host_meta.mask_ds_host)
    _class_counts = staticmethod(host_meta.class_counts)
    _fusion_lengths_host = staticmethod(host_meta.fusion_lengths_host)

    def host_metadata(self, cpu_batch: Dict[str, torch.Tensor], T_enc: int) -> Dict[str, object]:
        return host_meta.host_metadata(cpu_batch, T_enc)

    def forward_losses(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """model/trainer.py:66-119 for one batch; everything stays on the device.  The stages below enqueue in the order they are called in.
        With ``native_ctc`` nothing in here synchronises, so the BiLSTM timeout words staged by a step are normally evaluated at the
        start of the NEXT call (or at the end of train_epoch / evaluate()): the RuntimeError of a timed-out persistent LSTM launch then
        names the previous step, not the one that is being enqueued."""
        d = self._inputs(batch)
        vf1, vf2, join = self._lips(d)
        a1, mid1, a2, mid2 = self._audio(d, batch)
        T_enc = a1.shape[1]
        m1, m2 = self._mask_ds(d["mask1"], T_enc), self._mask_ds(d["mask2"], T_enc)
        c1, c2 = self._contrastive(batch, mid1, mid2, m1, m2, T_enc)
        join()
        f1, f2, il1, il2, lp1, lp2, lp12, il12 = self._heads(vf1, vf2, a1, a2, m1, m2)
        if lp12 is not None:
            total, l1, l2, tg, tl = self._ctc_stacked(d, batch, lp12, il12, c1, c2)
        else:
            total, tg, tl = None, None, None
            l1, l2 = self._ctc_per_speaker(d, lp1, lp2, il1, il2)
        if total is None:
            total = (l1 + l2) / 2 + self.lambda_ * (c1 + c2) / 2
        out = {}
        if self.mwer_weight > 0 and torch.is_grad_enabled():
            mw1, mw2 = self._mwer_term(d, lp1, lp2, il1, il2, lp12, il12, tg, tl)
            total = total + self.mwer_weight * (mw1 + mw2) / 2
            out.update(mwer1=mw1, mwer2=mw2)
        out.update(visual_feat1=vf1, visual_feat2=vf2, audio_last=a1, audio_mid=mid1, fused1=f1, fused2=f2, input_lengths1=il1,
                   input_lengths2=il2, log_probs1=lp1, log_probs2=lp2, loss1=l1, loss2=l2, contrast1=c1, contrast2=c2, total=total)
        return out

    def forward_log_probs(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """forward_losses without a transcript: the same stages up to the CTC head, no loss and no contrastive term.  ``batch`` needs
        ``audio``, ``lip1`` and ``lip2``; the ``text*`` keys are not read, and where ``mask1`` / ``mask2`` are missing they are built on the
        host from the optional ``audio_lengths`` / ``lip*_lengths`` (host_meta.batch_inference_masks)."""
        if "mask1" not in batch or "mask2" not in batch:
            m1, m2 = host_meta.batch_inference_masks(batch)
            batch = {**batch, "mask1": m1, "mask2": m2}
        d = self._inputs(batch)
        vf1, vf2, join = self._lips(d)
        a1, _, a2, _ = self._audio(d, batch)
        T_enc = a1.shape[1]
        m1, m2 = self._mask_ds(d["mask1"], T_enc), self._mask_ds(d["mask2"], T_enc)
        join()
        _, _, il1, il2, lp1, lp2, _, _ = self._heads(vf1, vf2, a1, a2, m1, m2)
        return dict(log_probs1=lp1, log_probs2=lp2, input_lengths1=il1, input_lengths2=il2)

    def _inputs(self, batch):
        """Main stream: the batch's device copy and, in a training step with ``augment``, its augmented lips and mixture.  Before that the
        timeout words the previous step staged are looked at (``native_ctc``: their event has completed unless the host runs far ahead)."""
        if self.native_ctc:
            self.fusion_module.finish_flag_check(wait=True)
        d = self._to_dev(batch)
        if self.augment is not None and torch.is_grad_enabled() and self.decoder1.training and self.audio_encoder.training:
            self._augment_inputs(d, batch)                         # before the lip streams fork
        return d

    def _lips(self, d):
        """The frozen visual encoder for both speakers -> (feat1, feat2, join).  With ``visual_side_stream`` it runs beside the wav2vec2 forward
        on side streams forked from main, one per speaker (AVAMD_VISUAL_STREAMS=1: both on one): its HBM-bound BatchNorm / pooling passes overlap
        the other streams' MFMA-bound kernels.  ``join()`` makes main wait for them; otherwise two calls on main and ``join`` does nothing."""
        if not (self.visual_side_stream and d["audio"].is_cuda):
            return self.visual_encoder(d["lip1"]), self.visual_encoder(d["lip2"]), lambda: None
        dev = d["audio"].device
        if self._vstream is None:
            self._vstream = torch.cuda.Stream(device=dev)
            self._vstream2 = torch.cuda.Stream(device=dev) if _VIS_STREAMS >= 2 else self._vstream
        main = torch.cuda.current_stream(dev)
        vf1, vf2 = self.visual_encoder.forward_pair(d["lip1"], d["lip2"], (self._vstream, self._vstream2))

        def join():
            main.wait_stream(self._vstream)
            if self._vstream2 is not self._vstream:
                main.wait_stream(self._vstream2)
            vf1.record_stream(main); vf2.record_stream(main)
        return vf1, vf2, join

    def _audio(self, d, batch):
        """Main stream: wav2vec2 -> (last1, mid1, last2, mid2).  One pass stands for both speakers unless a stochastic regulariser is active in
        train mode (``audio_passes`` forces either); two passes are one forward_pair call over one conv feature-extractor run."""
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
                return self.audio_encoder.forward_pair(d["audio"], attn1, d["mask2"] != 3, v1, v2)
            a1, mid1 = self.audio_encoder(d["audio"], attention_mask=attn1, valid_lengths=v1)
            return a1, mid1, a1, mid1
        finally:
            self.audio_encoder.model._feat_cache = None

    def _contrastive(self, batch, mid1, mid2, m1, m2, T_enc):
        """Main stream: the contrastive terms (c1, c2) of the mid-layer features; zeros at ``lambda_`` 0.  The projection layer is made on first use."""
        if self.lambda_ == 0:
            return (torch.zeros((), device=mid1.device),) * 2
        if self.projection_layer is None:
            self.projection_layer = nn.Linear(mid1.shape[2], 128).to(self.device)          # model/trainer.py:105-106
            if self.fixed_projection is not None:
                with torch.no_grad():
                    self.projection_layer.weight.copy_(self.fixed_projection[0]); self.projection_layer.bias.copy_(self.fixed_projection[1])
        k1 = batch.get("_counts1") or self._class_counts(batch["mask1"], T_enc)
        k2 = batch.get("_counts2") or self._class_counts(batch["mask2"], T_enc)
        return (contrastive_loss_with_mask(mid1, m1.reshape(-1), self.projection_layer, counts=k1),
                contrastive_loss_with_mask(mid2, m2.reshape(-1), self.projection_layer, counts=k2))

    def _heads(self, vf1, vf2, a1, a2, m1, m2):
        """Main stream: fusion and decoder -> (fused1, fused2, lengths1, lengths2, log_probs1, log_probs2, log_probs12, lengths12).  One stacked
        call (the last two are its results, else None) only if the lip clips were padded to the same length: the reference's collate pads lip1
        and lip2 separately (dataset/collate_fn.py:8-13,27-31), so a real batch can differ - then one call per speaker, as the reference does
        (found by tests/test_dataset_gpu.py::test_dataset_feeds_the_training_step).  Sets ``_pair_step`` for the head bucket's early reduce."""
        B = a1.shape[0]
        pair = self._pair_step = self.pair_batched and vf1.shape[1] == vf2.shape[1]
        if pair:
            f12, il12 = self.fusion_module(torch.cat([vf1, vf2], 0), torch.cat([a1, a2], 0), mask=torch.cat([m1, m2], 0), groups=2)
            lp12 = self.decoder1(f12)
            return f12[:B], f12[B:], il12[:B], il12[B:], lp12[:B], lp12[B:], lp12, il12
        f1, il1 = self.fusion_module(vf1, a1, mask=m1)
        f2, il2 = self.fusion_module(vf2, a2, mask=m2)
        return f1, f2, il1, il2, self.decoder1(f1), self.decoder1(f2), None, None

    def _ctc_stacked(self, d, batch, lp12, il12, c1, c2):
        """Main stream: ONE CTC call over the 2B items -> (total or None, loss1, loss2, targets, target lengths); the 'mean' reduction of
        nn.CTCLoss = mean_i(nll_i / clamp(target_len_i, 1)) is re-applied per speaker half, with the contrastive terms in one kernel
        (_CombineFn) where that applies.  nn.functional.ctc_loss (PyTorch-ROCm, as north_star prescribes) synchronises unless the batch
        carries host_metadata()'s lengths; ops.ctc_loss reads lengths and targets from device memory and nothing blocks (the staged timeout
        words are then looked at only if their copy happens to be complete, otherwise by the next forward_losses / train_epoch / evaluate())."""
        B = lp12.shape[0] // 2
        t1, t2 = d["text1"], d["text2"]
        Lm = max(t1.shape[1], t2.shape[1])
        tg = torch.cat([F.pad(t1, (0, Lm - t1.shape[1])), F.pad(t2, (0, Lm - t2.shape[1]))], 0)
        tl = torch.cat([d["text1_lengths"], d["text2_lengths"]], 0)
        il_h, tl_h = batch.get("_ctc_input_lengths"), batch.get("_ctc_target_lengths")     # host copies: no device sync in ctc_loss
        w_ctc = (0.5 / B) / tl.clamp_min(1).to(torch.float32)        # weights of the per-speaker means (before the CTC call: off the sync)
        self.fusion_module.stage_flag_check()                  # BiLSTM timeout words -> pinned memory, visible after ctc_loss's own sync
        if self.native_ctc:
            nll = ops.ctc_loss(lp12, tg, il12, tl, blank=self.tokenizer.blank_id, reduction="none", zero_infinity=True, batch_first=True)
        else:
            nll = F.ctc_loss(lp12.transpose(0, 1), tg, il12 if il_h is None else il_h, tl if tl_h is None else tl_h,
                             blank=self.tokenizer.blank_id, reduction="none", zero_infinity=True)
        self.fusion_module.finish_flag_check()                 # raises if a persistent BiLSTM launch timed out (event query, no sync)
        if nll.is_cuda and nll.dtype == torch.float32 and _FUSED_LOSS:
            return (*_CombineFn.apply(nll, w_ctc, c1, c2, float(self.lambda_)), tg, tl)      # one kernel forward, one backward
        per = nll / tl.clamp_min(1).to(nll.dtype)
        return None, per[:B].mean(), per[B:].mean(), tg, tl

    def _ctc_per_speaker(self, d, lp1, lp2, il1, il2):
        """Main stream: one mean-reduced CTC call per speaker -> (loss1, loss2), as the reference does; nn.CTCLoss synchronises in each."""
        if not self.native_ctc:
            return (self.ctc_loss(lp1.transpose(0, 1), d["text1"], il1, d["text1_lengths"]),
                    self.ctc_loss(lp2.transpose(0, 1), d["text2"], il2, d["text2_lengths"]))
        kw = dict(blank=self.tokenizer.blank_id, reduction="mean", zero_infinity=True, batch_first=True)
        self.fusion_module.stage_flag_check()
        l1 = ops.ctc_loss(lp1, d["text1"], il1, d["text1_lengths"], **kw)
        l2 = ops.ctc_loss(lp2, d["text2"], il2, d["text2_lengths"], **kw)
        self.fusion_module.finish_flag_check()
        return l1, l2

    def _mwer_term(self, d, lp1, lp2, il1, il2, lp12, il12, tg, tl):
        """Main stream: the mean MWER risk per speaker (mwer1, mwer2), from one ``_mwer`` call on the stacked log-probs or one per speaker.  The
        term meets the CTC term at the log-probs through autograd, as the contrastive and CTC terms meet further down."""
        if lp12 is not None:
            B = lp12.shape[0] // 2
            per = self._mwer(lp12, tg, tl, il12)
            return per[:B].mean(), per[B:].mean()
        return (self._mwer(lp1, d["text1"], d["text1_lengths"], il1).mean(),
                self._mwer(lp2, d["text2"], d["text2_lengths"], il2).mean())

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
            d["audio"], self.last_aug_sigma = aug.noise(d["audio"], (d["mask1"] != 3).sum(1), aug.step, out=self._aug_buffer("audio", d["audio"]),
                                                        sigma=self._aug_buffer("sigma", d["audio"][:, 0]))

    def _mwer(self, lp, refs, ref_lengths, input_lengths):
        """Per-utterance MWER risk [B] of one decoder call (mwer.mwer_loss, reduction "none"); float32 log-probs as the CTC loss reads them."""
        from ..mwer import mwer_loss
        if self.mwer_level != "token" and self._mwer_table is None:
            self._mwer_table = PieceTable.from_tokenizer(self.tokenizer)
        return mwer_loss(lp.float(), refs, ref_lengths, input_lengths, self.tokenizer.blank_id, nbest=self.mwer_nbest,
                         beam_width=self.mwer_beam, table=self._mwer_table, level=self.mwer_level, reduction="none")

    def train_step(self, batch) -> Dict[str, torch.Tensor]:
        """zero_grad -> forward -> backward (-> bucketed all-reduce) -> Adam; no host sync.  With max_grad_norm > 0 the result also has
        ``grad_norm``: the global gradient norm before clipping, a device scalar.  With accum_steps > 1 every call is one micro-step: its
        gradients go into the optimizer's accumulators, and the call that completes the cycle ends with the Adam step on their mean;
        ``stepped`` (a bool) says which, and ``grad_norm`` is there only on those calls."""
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
        if self.accum_steps > 1:
            self.optimizer.accumulate()                            # the arenas are free for the next backward (stream order)
            out["stepped"] = self.optimizer.accum_pending >= self.accum_steps
            if not out["stepped"]:
                return out
        self.scaler.step(self.optimizer)                           # model/trainer.py:122-123 (update() is part of the device-side step)
        self.scaler.update()
        if self.optimizer.clipping:
            out["grad_norm"] = self.optimizer.last_grad_norm
        return out

    def flush_accumulated(self) -> bool:
        """Step an open accumulation cycle now, on the mean of the micro-steps it holds (the end of an epoch whose length is no multiple of
        accum_steps; before a checkpoint).  False when no cycle is open."""
        if self.optimizer.accum_pending == 0:
            return False
        self.scaler.step(self.optimizer)
        self.scaler.update()
        return True

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
                    # the last optimizer step's; with accum_steps > 1 none may have been taken yet (the state block is made by the first)
                    if (self.optimizer.clipping or self.optimizer.scheduled) and self.optimizer.last_grad_norm is not None:
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
        if self.accum_steps > 1:
            self.flush_accumulated()                               # a loader whose length is no multiple of accum_steps: no cycle spans two epochs
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

    @contextlib.contextmanager
    def _inference(self):
        """What evaluate() and align() share: no autograd; with ``eval_ema`` the averaged weights inside the block and the trained ones after
        it; no contrastive term (so no projection layer is created); with ``native_ctc`` every pending timeout word is looked at on the way out."""
        with self.optimizer.averaged() if self.eval_ema else contextlib.nullcontext(), torch.no_grad():
            lam, self.lambda_ = self.lambda_, 0.0
            try:
                yield
                if self.native_ctc:
                    self.fusion_module.drain_flag_check()
            finally:
                self.lambda_ = lam

    def _decode(self, lp):
        """Token ids per utterance: greedy (== the reference's simple_beam_search best beam) at ``eval_beam_width`` 0, otherwise the
        prefix beam search, with shallow fusion and / or phrase biasing where set (it rejects their weights without ``lm=`` / ``bias=``)."""
        if self.eval_beam_width == 0:
            return greedy_batch(lp, self.tokenizer.blank_id)
        kw = {}
        if self.eval_lm is not None:
            kw.update(lm=self.eval_lm, lm_weight=self.eval_lm_weight, token_bonus=self.eval_token_bonus)
        if self.eval_bias is not None:
            kw.update(bias=self.eval_bias, bias_weight=self.eval_bias_weight)
        return prefix_beam_search(lp, self.eval_beam_width, self.tokenizer.blank_id, **kw)

    def evaluate(self, dataloader):
        """(loss, WER) over the loader, decoded by ``_decode``; the modules are left in eval mode."""
        refs1, hyps1, refs2, hyps2 = [], [], [], []
        total_loss = 0.0
        self.last_report = None
        with self._inference():
            self.visual_encoder.eval(); self.audio_encoder.eval(); self.fusion_module.eval(); self.decoder1.eval()
            report = self._report_begin() if self.eval_report else None
            for batch in dataloader:
                out = self.forward_losses(batch)
                total_loss += (out["loss1"].item() + out["loss2"].item()) / 2
                for spk, lp, refs, hyps in (("1", out["log_probs1"], refs1, hyps1), ("2", out["log_probs2"], refs2, hyps2)):
                    ids = self._decode(lp)
                    txt, tl = batch["text" + spk], batch["text" + spk + "_lengths"]
                    for i, seq in enumerate(ids):
                        hyps.append(fast_decode(seq, self.tokenizer))
                        refs.append(self.tokenizer.decode(txt[i][: int(tl[i])].tolist()))
                    if report is not None:
                        self._report_add(report, spk, txt, tl, ids)
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
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("MultimodalTrainer.evaluate: eval_report counts errors on the GPU; there is no CPU fallback")
        return {"table": PieceTable.from_tokenizer(self.tokenizer), "acc": torch.zeros((2, 3, 4), dtype=torch.int64, device=self.device)}

    def _report_add(self, report, spk, txt, tl, ids):
        # references as evaluate() decodes them (nothing skipped), hypotheses as fast_decode does (the blank skipped)
        counts = error_counts(txt.to(self.device, non_blocking=True), ids, ref_lengths=tl, table=report["table"], ref_skip=-1,
                              hyp_skip=self.tokenizer.blank_id)
        best = counts[:, 0].long()
        report["acc"][int(spk) - 1] += (best * (best[:, :, 3:4] >= 0)).sum(0)          # a level of -1 (a text beyond the limit) adds nothing

    def _report_finish(self, report):
        acc = report["acc"].cpu()
        self.last_report = {"speaker1": rates(acc[0]), "speaker2": rates(acc[1])}
        return self.last_report["speaker1"]["word"]["rate"], self.last_report["speaker2"]["word"]["rate"]

    @torch.no_grad()
    def align(self, batch, frame_rate: float = 25.0):
        """Word times of both speakers' transcripts in one batch: CTC forced alignment (align.forced_align, csrc/ctc_align.hip) of
        ``text*`` against the log-probs of ONE forward_losses call in eval mode.  Returns (segments1, segments2): per utterance the
        ``align.word_segments`` list ([] for a transcript that cannot be aligned).  The CTC head runs at the lip-frame rate, so
        ``frame_rate`` is the video's.  One device-to-host transfer per speaker; every module's train / eval mode is restored."""
        with self._inference():
            if torch.device(self.device).type != "cuda":
                raise RuntimeError("MultimodalTrainer.align: the model runs on the GPU; there is no CPU fallback")
            mods = (self.visual_encoder, self.audio_encoder, self.fusion_module, self.decoder1)
            modes = [(sm, sm.training) for m in mods for sm in m.modules()]      # per sub-module: a frozen part may sit in eval mode
            for m in mods:
                m.eval()
            try:
                out = self.forward_losses(batch)
            finally:
                for sm, was in modes:
                    sm.training = was
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
        return tuple(res)

    # ---- transcription of unlabeled clips: text, word times and confidences, decoded and timed on the device ----
    def transcribe(self, batch, nbest: int = 1, frame_rate: float = 25.0):
        """Both speakers' transcripts of a batch that needs no ``text*`` and no ``mask*`` keys (forward_log_probs), in eval mode, with the
        averaged weights under ``eval_ema``, decoded as evaluate() decodes (all T frames; ``eval_beam_width``, ``eval_lm``, ``eval_bias``).
        Returns (results1, results2): per utterance a dict with ``text``, ``ids``, ``confidence`` (the utterance's: ``conf_aggregation`` of
        its tokens' confidences), ``words`` (``align.word_segments`` with ``confidence``: word, start, end, score, confidence) and, with a
        beam, ``nbest``: up to ``nbest`` (text, score) pairs in descending order.  Beam width 0: one confidence.greedy_timed call per
        speaker.  Otherwise nbest_on_device, forced_align on the best hypothesis (T <= 408: its lattice is sized for T labels), then the
        frame and span passes of confidence.py.  Nothing travels to the host before the end; then ONE transfer per speaker.  Every
        module's train / eval mode is restored; a timed-out persistent BiLSTM launch raises here as it does from evaluate()."""
        nbest, W = int(nbest), self.eval_beam_width
        if not 1 <= nbest <= max(W, 1):
            raise ValueError(f"transcribe: need 1 <= nbest <= max(eval_beam_width, 1), got nbest={nbest} with eval_beam_width={W}")
        with self._inference():
            if torch.device(self.device).type != "cuda":
                raise RuntimeError("MultimodalTrainer.transcribe: the model runs on the GPU; there is no CPU fallback")
            mods = (self.visual_encoder, self.audio_encoder, self.fusion_module, self.decoder1)
            modes = [(sm, sm.training) for m in mods for sm in m.modules()]
            for m in mods:
                m.eval()
            try:
                out = self.forward_log_probs(batch)
            finally:
                for sm, was in modes:
                    sm.training = was
            self.fusion_module.stage_flag_check()
            B, T, _ = out["log_probs1"].shape
            packed = [self._transcribe_device(out["log_probs" + spk].float(), nbest) for spk in ("1", "2")]
            host = [p.cpu() for p in packed]                       # the only transfers: one int32 block per speaker
            self.fusion_module.drain_flag_check()                  # raises if a persistent BiLSTM launch timed out
        return tuple(self._transcribe_host(h, B, T, nbest, frame_rate) for h in host)

    def _transcribe_device(self, lp, nbest, input_lengths=None):
        """One speaker's log-probs [B, T, V] -> flat int32 block on the device: [B][T + 1][5] = per token (id, first frame, end frame, bits of
        its confidence, bits of its path score), the last row (number of tokens, bits of the utterance confidence, 0, 0, 0); with a beam then
        [B][nbest][T + 2] = per hypothesis its ids, its length and the bits of its score.  ``input_lengths`` (transcribe_long's segments):
        int64 [B] on the device, read there by every pass; None decodes all T frames."""
        from ..beam_search import nbest_on_device
        from ..confidence import frame_confidence, greedy_timed, span_confidence, utterance_confidence
        blank, (B, T, _) = self.tokenizer.blank_id, lp.shape
        method, alpha, agg = self.conf_method, self.conf_alpha, self.conf_aggregation
        i32 = lambda x: x.contiguous().view(torch.int32)       # noqa: E731
        if self.eval_beam_width == 0:
            g = greedy_timed(lp, blank, input_lengths, method, alpha, agg)
            ids, n, spans, tc, ts, extra = g.ids, g.lengths, g.spans, g.token_conf, self._greedy_token_scores(lp, g), []
        else:
            kw = {}
            if self.eval_lm is not None:
                kw.update(lm=self.eval_lm, lm_weight=self.eval_lm_weight, token_bonus=self.eval_token_bonus)
            if self.eval_bias is not None:
                kw.update(bias=self.eval_bias, bias_weight=self.eval_bias_weight)
            if input_lengths is not None:
                kw.update(lengths=input_lengths)
            hyp, hl, hs = nbest_on_device(lp, self.eval_beam_width, blank, nbest=nbest, **kw)[:3]
            ids, n = hyp[:, 0], hl[:, 0].clamp_min(0)
            al = forced_align(lp, ids, input_lengths, n, blank=blank)
            tc = span_confidence(frame_confidence(lp, input_lengths, method, alpha), al.spans, input_lengths, agg)
            spans, ts, extra = al.spans, al.token_scores, [torch.cat([hyp, hl[..., None], i32(hs)[..., None]], 2).reshape(-1)]
        utt = utterance_confidence(tc, n, agg)
        tail = torch.zeros((B, 1, 5), dtype=torch.int32, device=lp.device)
        tail[:, 0, 0], tail[:, 0, 1] = n, i32(utt)
        main = torch.cat([ids[..., None], spans, i32(tc)[..., None], i32(ts)[..., None]], 2)
        return torch.cat([torch.cat([main, tail], 1).reshape(-1)] + extra)

    @staticmethod
    def _greedy_token_scores(lp, g):
        """float32 [B, T]: the sum of lp[t][id_j] over the run of greedy token j (forced_align's token score), 0 padded, from T gathered
        elements per utterance: the label of each frame from the runs, the path's emissions, their float64 running sum, its differences."""
        B, T, _ = lp.shape
        t = torch.arange(T, device=lp.device).expand(B, T).contiguous()
        first, end = g.spans[..., 0].long(), g.spans[..., 1].long()
        j = torch.searchsorted(torch.where(first < 0, T, first), t, right=True) - 1       # the last run that starts at or before frame t
        jc = j.clamp_min(0)
        inside = (j >= 0) & (t < end.gather(1, jc))
        label = g.ids.long().gather(1, jc).clamp_min(0)
        em = torch.where(inside, lp.gather(2, label[..., None])[..., 0], 0.0).double()
        cs = F.pad(em.cumsum(1), (1, 0))
        return (cs.gather(1, end.clamp_min(0)) - cs.gather(1, first.clamp_min(0))).float()

    def _transcribe_host(self, flat, B, T, nbest, frame_rate):
        f32 = lambda x: x.contiguous().view(torch.float32)     # noqa: E731
        main = flat[:B * (T + 1) * 5].view(B, T + 1, 5)
        hyps = flat[B * (T + 1) * 5:].view(B, nbest, T + 2) if self.eval_beam_width > 0 else None
        tc, ts, utt = f32(main[:, :T, 3]), f32(main[:, :T, 4]), f32(main[:, T, 1]).tolist()
        res = []
        for i in range(B):
            n = int(main[i, T, 0])
            ids = main[i, :n, 0].tolist()
            r = {"text": fast_decode(ids, self.tokenizer), "ids": ids, "confidence": utt[i],
                 "words": word_segments(self.tokenizer, ids, main[i, :T, 1:3], ts[i], frame_rate, token_conf=tc[i],
                                        aggregation=self.conf_aggregation)}
            if hyps is not None:
                sc = f32(hyps[i, :, T + 1]).tolist()
                r["nbest"] = [(fast_decode(hyps[i, k, :int(hyps[i, k, T])].tolist(), self.tokenizer), sc[k])
                              for k in range(nbest) if int(hyps[i, k, T]) >= 0]
            res.append(r)
        return res

    # ---- transcription of a recording of any length: overlapping windows, stitched and cut on the device (longform.py) ----
    def transcribe_long(self, recording, frame_rate: float = 25.0, nbest: int = 1):
        """Both speakers' transcripts of ONE recording of any length: ``audio`` [n] or [1, n], ``lip1`` / ``lip2`` [F, 1, H, W] or
        [1, F, 1, H, W], on the host or the device; F comes from the lips (which must agree), the audio is cut or zero-padded to 640 F.
        The recording is covered with windows of ``long_window`` lip frames (longform.plan_windows: ``long_stride`` frames per side are
        discarded, no window is padded), they go through forward_log_probs ``long_batch`` at a time in eval mode (the averaged weights
        under ``eval_ema``) into one [2, nw, W, V] device buffer, are stitched by ``long_policy`` into [2, F, V], cut at blank frames into
        segments of at most ``long_segment`` frames (cuts searched within ``long_radius`` frames) and decoded in ONE batch of segments as
        transcribe() decodes (``eval_beam_width``, ``eval_lm``, ``eval_bias``, ``conf_*``); the decoders read the segment lengths on the
        device.  F <= ``long_segment`` is not cut, so F <= ``long_window`` too is what transcribe() computes for that clip.  The cuts ride
        in the decode's int32 block: ONE transfer at the end and no synchronisation before it.
        Returns (result1, result2), a dict per speaker: ``text``, ``ids``, ``confidence`` (``conf_aggregation`` over ALL tokens in order,
        confidence.host_span_law in float32), ``words`` (transcribe()'s, times counted from the start of the recording; a word may span a
        cut) and ``segments``: per segment ``start``, ``end`` (seconds), ``text``, ``confidence`` and, with a beam, ``nbest``.
        A run of equal argmax frames across a cut that is not at an argmax-blank frame may be emitted twice, and a language model or a
        phrase match restarts at every segment (longform.py).  There is no limit on F other than memory."""
        from .. import longform
        from ..confidence import host_span_law
        nbest, Wb = int(nbest), self.eval_beam_width
        if not 1 <= nbest <= max(Wb, 1):
            raise ValueError(f"transcribe_long: need 1 <= nbest <= max(eval_beam_width, 1), got nbest={nbest} with eval_beam_width={Wb}")
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("MultimodalTrainer.transcribe_long: the model runs on the GPU; there is no CPU fallback")
        audio, lip1, lip2 = self._recording(recording)
        F_, seg, rad = lip1.shape[0], self.long_segment, self.long_radius
        plan = longform.plan_windows(F_, self.long_window, self.long_stride)
        plan.sources(self.long_policy)                             # a plan the policy cannot join raises before anything runs
        with self._inference():
            stitched = self._stitched_windows("transcribe_long", plan, audio, lip1, lip2)
            if F_ <= seg:                                          # one segment per speaker: exactly what transcribe() decodes
                cuts = ops.h2d_async(torch.tensor([[0, F_]] * 2, dtype=torch.int32).numpy(), stitched.device)
                flat, T = self._transcribe_device(stitched, nbest), F_
            else:
                cuts = longform.cut_points(stitched, self.tokenizer.blank_id, seg, rad)
                seg_lp, seg_len = longform.split_segments(stitched, cuts, seg)
                flat, T = self._transcribe_device(seg_lp, nbest, seg_len), seg
            host = torch.cat([flat, cuts.reshape(-1)]).cpu()       # the only transfer
            self.fusion_module.drain_flag_check()                  # raises if a persistent BiLSTM launch timed out
        ns = cuts.shape[1] - 1                                     # segments per speaker
        cuts_h = host[-2 * (ns + 1):].view(2, ns + 1).tolist()
        segs = self._transcribe_host(host[:-2 * (ns + 1)], 2 * ns, T, nbest, frame_rate)
        main = host[:2 * ns * (T + 1) * 5].view(2 * ns, T + 1, 5)
        f32 = lambda x: x.contiguous().view(torch.float32)         # noqa: E731
        res = []
        for s in range(2):
            ids, spans, tc, ts, parts = [], [], [], [], []
            for j in range(ns):
                i, c0, c1 = s * ns + j, cuts_h[s][j], cuts_h[s][j + 1]
                n, r = int(main[i, T, 0]), segs[i]
                ids += r["ids"]
                sp = main[i, :n, 1:3]
                spans.append(torch.where(sp < 0, sp, sp + c0))      # a token that could not be aligned keeps its -1
                tc.append(f32(main[i, :n, 3])); ts.append(f32(main[i, :n, 4]))
                parts.append({"start": c0 / frame_rate, "end": c1 / frame_rate, "text": r["text"], "confidence": r["confidence"]})
                if "nbest" in r:
                    parts[-1]["nbest"] = r["nbest"]
            spans, tc, ts = torch.cat(spans), torch.cat(tc), torch.cat(ts)
            conf = float(host_span_law(tc.numpy(), 0, len(ids), len(ids), self.conf_aggregation)) if ids else 0.0
            res.append({"text": fast_decode(ids, self.tokenizer), "ids": ids, "confidence": conf,
                        "words": word_segments(self.tokenizer, ids, spans, ts, frame_rate, token_conf=tc, aggregation=self.conf_aggregation),
                        "segments": parts})
        return tuple(res)

    def _stitched_windows(self, who, plan, audio, lip1, lip2):
        """What transcribe_long() and spot_long() share, inside ``_inference()``: the plan's windows through forward_log_probs ``long_batch``
        at a time in eval mode (every module's train / eval mode restored) into one [2, nw, W, V] device buffer, stitched by ``long_policy``
        -> float32 [2, F, V] on the device."""
        from .. import longform
        Wd, nw, buf = plan.width, plan.count, None
        mods = (self.visual_encoder, self.audio_encoder, self.fusion_module, self.decoder1)
        modes = [(sm, sm.training) for m in mods for sm in m.modules()]
        for m in mods:
            m.eval()
        try:
            for k0 in range(0, nw, self.long_batch):
                ks = range(k0, min(k0 + self.long_batch, nw))
                out = self.forward_log_probs({
                    "audio": torch.stack([audio[slice(*plan.audio_window(k))] for k in ks]),
                    "lip1": torch.stack([lip1[plan.starts[k]:plan.starts[k] + Wd] for k in ks]),
                    "lip2": torch.stack([lip2[plan.starts[k]:plan.starts[k] + Wd] for k in ks])})
                self.fusion_module.stage_flag_check()
                for s, spk in enumerate(("1", "2")):
                    lp = out["log_probs" + spk]
                    if lp.shape[1] != Wd:
                        raise RuntimeError(f"{who}: a window of {Wd} lip frames came back with {lp.shape[1]} CTC frames")
                    if buf is None:
                        buf = torch.empty((2, nw, Wd, lp.shape[2]), dtype=torch.float32, device=lp.device)
                    buf[s, k0:k0 + len(ks)].copy_(lp)
        finally:
            for sm, was in modes:
                sm.training = was
        return longform.stitch(buf, plan, self.long_policy)

    # ---- keyword spotting: was this phrase said, where, and how sure (spot.py, csrc/ctc_spot.hip) ----
    def _spot_keywords(self, who, keywords, max_hits, min_score):
        """-> (ContextBias, the keywords' names, max_hits, min_score): strings go through ``ContextBias.from_phrases`` with the tokenizer, one
        string or path is a phrase file, a ContextBias is taken as it is; None reads ``spot_max_hits`` / ``spot_min_score``."""
        if torch.device(self.device).type != "cuda":
            raise RuntimeError(f"MultimodalTrainer.{who}: the model runs on the GPU; there is no CPU fallback")
        if isinstance(keywords, (str, os.PathLike)):
            keywords = ContextBias.from_file(keywords, self.tokenizer)
        elif not isinstance(keywords, ContextBias):
            keywords = ContextBias.from_phrases(list(keywords), self.tokenizer)
        if not keywords.phrases:
            raise ValueError(f"{who}: no keywords")
        max_hits = self.spot_max_hits if max_hits is None else int(max_hits)
        min_score = self.spot_min_score if min_score is None else float(min_score)
        options.check_spot(min_score, max_hits)
        pieces = self.tokenizer.id_to_token
        names = ["".join(pieces[i] for i in p).replace("▁", " ") for p in keywords.phrases]
        return keywords, names, max_hits, min_score

    def _spot_device(self, lp, bias, max_hits, min_score):
        """One block of log-probs [B, T, V] -> flat int32 block on the device: per (utterance, keyword) ``max_hits`` rows of (first frame, end
        frame, bits of the score), then the counts."""
        from ..spot import keyword_spot
        s = keyword_spot(lp, bias, blank=self.tokenizer.blank_id, max_hits=max_hits, min_score=min_score)
        return torch.cat([torch.cat([s.hits, s.scores.view(torch.int32)[..., None]], 3).reshape(-1), s.counts.reshape(-1)])

    @staticmethod
    def _spot_host(flat, B, K, N, names, frame_rate):
        from ..spot import Spots, hit_segments
        main = flat[:B * K * N * 3].view(B, K, N, 3)
        return hit_segments(Spots(main[..., :2], main[..., 2].contiguous().view(torch.float32), flat[B * K * N * 3:].view(B, K)), names, frame_rate)

    def spot(self, batch, keywords, max_hits: Optional[int] = None, min_score: Optional[float] = None, frame_rate: float = 25.0):
        """Where both speakers of a batch said the ``keywords``: strings (``ContextBias.from_phrases`` with the tokenizer), the path of a phrase
        file, or a ``ContextBias``.  The batch needs no ``text*`` and no ``mask*`` keys (forward_log_probs); eval mode and ``eval_ema`` as
        in transcribe().  ``max_hits`` hits per utterance and keyword (None: ``spot_max_hits``) with a score of at least ``min_score``
        (None: ``spot_min_score``) - spot.keyword_spot over all T frames.  Returns (hits1, hits2): per utterance the ``spot.hit_segments``
        list (keyword, start, end, score, per_frame).  Nothing travels to the host before the end; then ONE int32 block per speaker.
        Every module's train / eval mode is restored; a timed-out persistent BiLSTM launch raises here as it does from evaluate()."""
        bias, names, N, ms = self._spot_keywords("spot", keywords, max_hits, min_score)
        with self._inference():
            mods = (self.visual_encoder, self.audio_encoder, self.fusion_module, self.decoder1)
            modes = [(sm, sm.training) for m in mods for sm in m.modules()]
            for m in mods:
                m.eval()
            try:
                out = self.forward_log_probs(batch)
            finally:
                for sm, was in modes:
                    sm.training = was
            self.fusion_module.stage_flag_check()
            B = out["log_probs1"].shape[0]
            packed = [self._spot_device(out["log_probs" + spk].float(), bias, N, ms) for spk in ("1", "2")]
            host = [p.cpu() for p in packed]                       # the only transfers: one int32 block per speaker
            self.fusion_module.drain_flag_check()                  # raises if a persistent BiLSTM launch timed out
        return tuple(self._spot_host(h, B, len(names), N, names, frame_rate) for h in host)

    def spot_long(self, recording, keywords, max_hits: Optional[int] = None, min_score: Optional[float] = None, frame_rate: float = 25.0):
        """spot() for ONE recording of any length (``recording`` as for transcribe_long): its windows and stitch, then spot.keyword_spot on
        the stitched [2, F, V] - there is no bound on F other than memory, and a hit may lie across any window edge.  Returns (hits1,
        hits2): per speaker the ``spot.hit_segments`` list, times counted from the start of the recording.  ONE transfer at the end."""
        from .. import longform
        bias, names, N, ms = self._spot_keywords("spot_long", keywords, max_hits, min_score)
        audio, lip1, lip2 = self._recording(recording)
        plan = longform.plan_windows(lip1.shape[0], self.long_window, self.long_stride)
        plan.sources(self.long_policy)                             # a plan the policy cannot join raises before anything runs
        with self._inference():
            stitched = self._stitched_windows("spot_long", plan, audio, lip1, lip2)
            host = self._spot_device(stitched, bias, N, ms).cpu()  # the only transfer
            self.fusion_module.drain_flag_check()
        return tuple(self._spot_host(host, 2, len(names), N, names, frame_rate))

    # ---- a recording against its transcript: word and utterance times with scores (segmentation.py, csrc/ctc_segment.hip) ----
    def _segment_targets(self, transcripts):
        """Two transcripts (a string = one utterance, or a list of strings) -> (per speaker the token ids, targets int64 [2, Lmax] padded
        with the blank, their lengths, utterances int32 [2, U, 2] padded with -1, per speaker the utterances' texts).  Every utterance goes
        through ``tokenizer.encode``; a '▁' piece is put between two utterances where the tokenizer has one - it belongs to neither."""
        space = self.tokenizer.token_to_id.get("▁")
        texts = [[t] if isinstance(t, str) else [str(x) for x in t] for t in transcripts]
        ids, ranges = [], []
        for utts in texts:
            row, rng = [], []
            for k, text in enumerate(utts):
                if k and space is not None:
                    row.append(int(space))
                rng.append((len(row), len(row) + len(enc := [int(i) for i in self.tokenizer.encode(text)])))
                row += enc
            ids.append(row)
            ranges.append(rng)
        Lmax, U = max(len(r) for r in ids), max(len(r) for r in ranges)
        tg = torch.full((2, Lmax), int(self.tokenizer.blank_id), dtype=torch.long)
        ut = torch.full((2, U, 2), -1, dtype=torch.int32)
        for i in range(2):
            tg[i, :len(ids[i])] = torch.tensor(ids[i], dtype=torch.long)
            if ranges[i]:
                ut[i, :len(ranges[i])] = torch.tensor(ranges[i], dtype=torch.int32)
        return ids, tg, torch.tensor([len(r) for r in ids]), ut, texts

    def align_long(self, recording, transcript1, transcript2, frame_rate: float = 25.0, free_start: Optional[bool] = None,
                   free_end: Optional[bool] = None):
        """Where in ONE recording of any length (``recording`` as for transcribe_long) each speaker's transcript was said: a transcript is
        a string (one utterance) or a list of strings (utterances, joined by a '▁' piece where the tokenizer has one).  The windows
        and the stitch of transcribe_long, then segmentation.ctc_segment on the stitched [2, F, V]: no bound on F other than memory, up to
        8191 tokens per transcript.  ``free_start`` / ``free_end`` (None: bits 0 / 1 of ``segment_free``) let the transcript begin after
        and end before the recording does; utterance scores use windows of ``segment_window`` frames.  Returns (result1, result2), a dict
        per speaker: ``score`` (the path's; -inf with empty lists for a transcript that cannot be aligned), ``words``
        (``align.word_segments``, times counted from the start of the recording) and ``utterances``
        (``segmentation.utterance_segments``: text, start, end, score, mean).  ONE int32 block goes to the host at the end."""
        from .. import longform
        from ..segmentation import Segmentation, ctc_segment, utterance_segments
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("MultimodalTrainer.align_long: the model runs on the GPU; there is no CPU fallback")
        fs = bool(self.segment_free & 1) if free_start is None else bool(free_start)
        fe = bool(self.segment_free & 2) if free_end is None else bool(free_end)
        ids, tg, tl, ut, texts = self._segment_targets((transcript1, transcript2))
        audio, lip1, lip2 = self._recording(recording)
        plan = longform.plan_windows(lip1.shape[0], self.long_window, self.long_stride)
        plan.sources(self.long_policy)                             # a plan the policy cannot join raises before anything runs
        with self._inference():
            stitched = self._stitched_windows("align_long", plan, audio, lip1, lip2)
            dev = stitched.device                                  # targets, lengths and ranges: pinned copies that do not drain the stream
            seg = ctc_segment(stitched, ops.h2d_async(tg.numpy(), dev), None, ops.h2d_async(tl.numpy(), dev), blank=self.tokenizer.blank_id,
                              utterances=ops.h2d_async(ut.numpy(), dev), free_start=fs, free_end=fe, score_window=self.segment_window)
            parts = [seg.spans, seg.token_scores.view(torch.int32), seg.score.view(torch.int32), seg.utt_spans,
                     seg.utt_means.view(torch.int32), seg.utt_scores.view(torch.int32)]
            host = torch.cat([x.reshape(-1) for x in parts]).cpu()  # the only transfer
            self.fusion_module.drain_flag_check()
        got, at = [], 0
        for x in parts:
            got.append(host[at:at + x.numel()].view(x.shape))
            at += x.numel()
        spans, tok, score, usp, um, us = (x if k in (0, 3) else x.contiguous().view(torch.float32) for k, x in enumerate(got))
        utts = utterance_segments(Segmentation(None, spans, tok, score, None, usp, um, us), texts, frame_rate)
        return tuple({"score": float(score[i]),
                      "words": word_segments(self.tokenizer, ids[i], spans[i], tok[i], frame_rate) if bool(score[i] > float("-inf")) else [],
                      "utterances": utts[i]} for i in range(2))

    @staticmethod
    def _recording(recording):
        """-> (audio [640 F], lip1 [F, 1, H, W], lip2 [F, 1, H, W]), each on the side it came from."""
        audio, lips = recording["audio"], [recording["lip1"], recording["lip2"]]
        if audio.dim() == 2 and audio.shape[0] == 1:
            audio = audio[0]
        lips = [x[0] if x.dim() == 5 and x.shape[0] == 1 else x for x in lips]
        if audio.dim() != 1 or any(x.dim() != 4 or x.shape[1] != 1 for x in lips):
            raise ValueError("transcribe_long: need audio [n] or [1, n] and lip1 / lip2 [F, 1, H, W] or [1, F, 1, H, W], got "
                             f"{tuple(recording['audio'].shape)}, {tuple(recording['lip1'].shape)} and {tuple(recording['lip2'].shape)}")
        if lips[0].shape != lips[1].shape or lips[0].shape[0] < 1:
            raise ValueError(f"transcribe_long: lip1 {tuple(lips[0].shape)} and lip2 {tuple(lips[1].shape)} must agree and hold a frame")
        n = host_meta.AUDIO_PER_LIP_FRAME * lips[0].shape[0]
        audio = audio[:n] if audio.shape[0] >= n else F.pad(audio, (0, n - audio.shape[0]))
        return audio, lips[0], lips[1]
