"""Host restatements of what the training step would otherwise read back from the device, computed from the HOST copy of a collated batch.
MultimodalTrainer carries them as ``_mask_ds_host``, ``_class_counts``, ``_fusion_lengths_host`` and ``host_metadata``."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch


def mask_ds_host(mask_cpu: torch.Tensor, T_enc: int) -> torch.Tensor:
    """Host restatement of av_mask_downsample (nearest index floor(i * Tin / T_enc), fp32 as on the device)."""
    mask_cpu = mask_cpu.cpu()
    Tin = mask_cpu.shape[1]
    scale = torch.tensor(Tin / T_enc, dtype=torch.float32)
    idx = torch.floor(torch.arange(T_enc, dtype=torch.float32) * scale).long().clamp_(max=Tin - 1)
    return mask_cpu[:, idx]


def class_counts(mask_cpu: torch.Tensor, T_enc: int):
    """(#1, #2, #0) of the down-sampled mask, computed on the host copy of the batch (no device sync when the
    batch arrives from a DataLoader; a device-resident batch should carry precomputed ``_counts1/_counts2``)."""
    c = torch.bincount(mask_ds_host(mask_cpu, T_enc).reshape(-1).clamp(0, 3), minlength=4).tolist()
    return (c[1], c[2], c[0])


def fusion_lengths_host(mask_cpu: torch.Tensor, T_enc: int, Tv: int) -> torch.Tensor:
    """Host restatement of the ``input_lengths`` CrossAttentionFusion returns for ONE call (model/fusion_module.py:41-59 of the
    reference; av_fusion_gather_lerp_fwd here): n_b speech frames (mask 1/2) are kept per item and padded to the call's
    maximum Tm, the mask is resampled to Tv frames with nearest index floor(i * Tm / Tv), and the length is the number
    of resampled positions that fall on a kept frame."""
    m = mask_ds_host(mask_cpu, T_enc)
    n = ((m == 1) | (m == 2)).sum(1).numpy().astype(np.int64)
    Tm = int(n.max()) if n.size else 0
    i = np.arange(Tv, dtype=np.float32)
    if Tm == Tv:
        j = np.arange(Tv, dtype=np.int64)
    else:
        j = np.floor(i * (np.float32(Tm) / np.float32(Tv))).astype(np.int64)
        j = np.minimum(j, max(Tm - 1, 0))
    return torch.from_numpy((j[None, :] < n[:, None]).sum(1).astype(np.int64))


AUDIO_PER_LIP_FRAME = 640            # waveform samples per lip frame: 16 kHz / 25 frames per second


def inference_masks(n_audio, n1, n2, width: int):
    """(mask1, mask2), int64 [B, width], for a mixture that comes without the two clean clips the dataset builds its masks from: per item
    the mixture holds ``n_audio`` samples, speaker k speaks during the first ``n_k``.  For speaker k: 1 where t < min(n1, n2) (both
    speak), 2 where min(n1, n2) <= t < n_k (only this speaker), 0 up to n_audio, 3 beyond - the law of the reference's mixing
    (oracle/pipeline_oracle.py mix_pair) plus the collate's pad code.  Lengths are clamped to [0, width] and n_k to n_audio."""
    na = np.clip(np.asarray(n_audio, np.int64).reshape(-1), 0, width)
    a, b = (np.minimum(np.clip(np.asarray(n, np.int64).reshape(-1), 0, width), na) for n in (n1, n2))
    if not na.shape == a.shape == b.shape:
        raise ValueError(f"inference_masks: need one length per item, got {na.shape[0]}, {a.shape[0]} and {b.shape[0]}")
    t = np.arange(width, dtype=np.int64)[None, :]
    both = np.minimum(a, b)[:, None]
    out = []
    for n in (a, b):
        m = np.where(t < both, 1, np.where(t < n[:, None], 2, np.where(t < na[:, None], 0, 3)))
        out.append(torch.from_numpy(m.astype(np.int64)))
    return tuple(out)


def batch_inference_masks(batch: Dict[str, torch.Tensor]):
    """``inference_masks`` from what an unlabeled batch carries: ``audio`` [B, width], optionally ``audio_lengths`` (default: the full width)
    and ``lip{k}_lengths`` in lip frames (x 640 samples, clamped to the audio; default: the audio's length)."""
    B, width = batch["audio"].shape
    host = lambda t: torch.as_tensor(t).cpu().long().numpy()                  # noqa: E731
    na = host(batch["audio_lengths"]) if "audio_lengths" in batch else np.full(B, width, np.int64)
    n1, n2 = (host(batch[k]) * AUDIO_PER_LIP_FRAME if k in batch else na for k in ("lip1_lengths", "lip2_lengths"))
    return inference_masks(na, n1, n2, width)


def host_metadata(cpu_batch: Dict[str, torch.Tensor], T_enc: int) -> Dict[str, object]:
    """Everything the step would otherwise read back from the device: contrastive class counts and the CTC length vectors
    (nn.functional.ctc_loss wants its lengths on the host; handing it device tensors costs a full device synchronisation per call).
    Keys start with ``_``; merge into the batch."""
    Tv = cpu_batch["lip1"].shape[1]
    il = torch.cat([fusion_lengths_host(cpu_batch["mask1"], T_enc, Tv), fusion_lengths_host(cpu_batch["mask2"], T_enc, Tv)])
    tl = torch.cat([cpu_batch["text1_lengths"].cpu().long(), cpu_batch["text2_lengths"].cpu().long()])
    return {"_counts1": class_counts(cpu_batch["mask1"], T_enc), "_counts2": class_counts(cpu_batch["mask2"], T_enc),
            "_ctc_input_lengths": il, "_ctc_target_lengths": tl,
            "_same_padding": bool(torch.equal(cpu_batch["mask1"] != 3, cpu_batch["mask2"] != 3)),
            "_audio_valid1": (cpu_batch["mask1"] != 3).sum(1).tolist(), "_audio_valid2": (cpu_batch["mask2"] != 3).sum(1).tolist()}
