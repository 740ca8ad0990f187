"""Long-form transcription: a recording of any length through a model that takes short clips.

The recording is covered with overlapping windows of the clip length, every window's CTC log-probs are computed on their own, the edge
frames of each window (where the encoders had no context) are discarded, the rest is stitched into ONE sequence of posteriors, and that
sequence is decoded once - the chunk_length_s / stride_length_s scheme of the Hugging Face ASR pipeline.  The decoders here are built for
T <= 408 (forced alignment behind a beam) and T <= 4096, so the stitched sequence is cut at blank frames into segments that are decoded as
one batch.  GPU tensors run on the kernels of csrc/ctc_longform.hip, host tensors on the same laws in float32 numpy.

Window plan for F frames, a window of W frames and S discarded frames per side (W >= 1, S >= 0, hop = W - 2 S >= 1):
  F <= W     one window [0, F), not padded
  otherwise  nw = ceil((F - W) / hop) + 1 windows of W frames at s_k = min(k hop, F - W): the last one is moved back so that it ends with
             the recording.  Every window is full and none is padded, so a window's CTC frames are its lip frames one to one
             (CrossAttentionFusion stretches an item's speech frames to the call's T_v: a padded window would get another time axis)
  ownership  cut_0 = 0, cut_k = (s_{k-1} + s_k + W) // 2, cut_nw = F; window k owns the frames [cut_k, cut_{k+1}), which lie inside it
  coverage   the largest number of windows over one frame
  audio      window k is the samples [640 s_k, 640 (s_k + W))

Stitch of window log-probs [S, nw, W, V] (S = speakers) into float32 [S, F, V]:
  centre     row t is the owner's row t - s_k, copied bit for bit
  average    over the windows k (ascending) that cover t, with w_k = min(t - s_k + 1, s_k + W - t) normalised in float32 to wn_k: per class
             M = max_k x_k, out = M + log(sum_k wn_k exp(x_k - M)), every operation in float32; M = -inf gives -inf, a NaN source gives
             NaN, a frame with a single source is copied bit for bit.  At most 4 sources per frame

Cut points of log-probs [S, F, V] for segments of at most ``segment`` frames, N = segment - 2 radius (N >= 2 radius + 1: the search zones
are disjoint; segment <= 408):
  nb = the number of j >= 1 with j N + radius < F (a function of the shapes alone);  c_0 = 0, c_{nb+1} = F,
  c_j = the frame t of [j N - radius, j N + radius] intersected with [1, F - 1] with the largest log_probs[t, blank]: float32 compare, a NaN
  ranks as -inf, ties go to the smallest t.  Every segment [c_j, c_{j+1}) then has between 1 and ``segment`` frames.

Segments: seg_lp float32 [S (nb + 1), segment, V], row i of segment j = log_probs[c_j + i] for i < c_{j+1} - c_j and exactly 0.0 after it;
seg_len int64 [S (nb + 1)].  Both stay on the input's device; the decoders read the lengths there.

What the cuts do to a decode.  A cut at a frame whose argmax is the blank cannot split a run of equal argmax frames, so where every zone
holds such a frame the greedy decode of the segments, joined, IS the greedy decode of the whole sequence (ids, spans shifted by c_j and
token confidences).  Where a zone holds none, the cut takes the best blank posterior and a run across it may be emitted twice.  A beam search
restarts at every segment: a language model and a phrase match see no context from the segment before.

What stitching does to the word error rate at window edges has not been measured here: there is no trained checkpoint and no data."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np
import torch

from .model.host_meta import AUDIO_PER_LIP_FRAME

MAX_SOURCES = 4                    # AV_LONGFORM_MAX_SOURCES
MAX_SEGMENT = 408                  # AV_LONGFORM_MAX_SEGMENT: forced_align's lattice behind a beam is sized for T <= 408 labels
POLICIES = ("centre", "average")


@dataclass
class WindowPlan:
    frames: int                    # F
    window: int                    # W
    stride: int                    # S, discarded frames per side
    hop: int                       # W - 2 S
    width: int                     # frames per window: W, or F where F <= W
    starts: List[int]              # s_k
    cuts: List[int]                # nw + 1 ownership cuts
    coverage: int
    _tables: dict = field(default_factory=dict, repr=False, compare=False)

    @property
    def count(self) -> int:
        return len(self.starts)

    def audio_window(self, k: int) -> Tuple[int, int]:
        return AUDIO_PER_LIP_FRAME * self.starts[k], AUDIO_PER_LIP_FRAME * (self.starts[k] + self.width)

    def sources(self, policy: str) -> Tuple[np.ndarray, np.ndarray]:
        """(src_row int32 [F, 4], src_weight float32 [F, 4]): per frame the rows of the [nw * width] window rows it is made of, ascending,
        -1 for none, and their normalised weights."""
        if policy not in POLICIES:
            raise ValueError(f"stitch: policy must be one of {POLICIES}, got {policy!r}")
        if policy == "average" and self.coverage > MAX_SOURCES:
            raise ValueError(f"stitch: policy 'average' takes at most {MAX_SOURCES} windows per frame, this plan has {self.coverage}; the "
                             f"smallest hop that is admissible at every length for window {self.window} is {min_average_hop(self.window)} "
                             f"(hop = window - 2 stride = {self.hop})")
        key = ("host", policy)
        if key not in self._tables:
            F, Wd = self.frames, self.width
            row = np.full((F, MAX_SOURCES), -1, np.int32)
            wt = np.zeros((F, MAX_SOURCES), np.float32)
            if policy == "centre":
                for k, s in enumerate(self.starts):
                    t = np.arange(self.cuts[k], self.cuts[k + 1])
                    row[t, 0] = k * Wd + (t - s)
                    wt[t, 0] = 1.0
            else:
                fill = np.zeros(F, np.int64)
                for k, s in enumerate(self.starts):
                    t = np.arange(s, s + Wd)
                    row[t, fill[t]] = k * Wd + (t - s)
                    wt[t, fill[t]] = np.minimum(t - s + 1, s + Wd - t).astype(np.float32)
                    fill[t] += 1
                tot = wt[:, 0].copy()
                for c in range(1, MAX_SOURCES):
                    tot = tot + wt[:, c]                                   # float32, ascending: small integers, exact
                wt = (wt / tot[:, None]).astype(np.float32)
            self._tables[key] = (row, wt)
        return self._tables[key]

    def table(self, policy: str, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """``sources`` on ``device``: uploaded once per plan, policy and device, without draining the stream."""
        key = (str(device), policy)
        if key not in self._tables:
            from . import ops
            row, wt = self.sources(policy)
            self._tables[key] = (ops.h2d_async(row, device), ops.h2d_async(wt, device))
        return self._tables[key]


def min_average_hop(window: int) -> int:
    """The smallest hop at which no frame lies under more than 4 windows of ``window`` frames, whatever the recording's length: the regular
    starts put ceil(window / hop) windows over a frame and the last window, moved back, can add one."""
    return -(-int(window) // (MAX_SOURCES - 1))


def check_plan(window: int, stride: int) -> int:
    window, stride = int(window), int(stride)
    if window < 1 or stride < 0 or window - 2 * stride < 1:
        raise ValueError(f"longform: need window >= 1, stride >= 0 and hop = window - 2 stride >= 1, got window={window} stride={stride}")
    return window - 2 * stride


def check_segment(segment: int, radius: int) -> int:
    segment, radius = int(segment), int(radius)
    if radius < 0 or not 1 <= segment <= MAX_SEGMENT or segment - 2 * radius < 2 * radius + 1:
        raise ValueError(f"longform: need radius >= 0, 1 <= segment <= {MAX_SEGMENT} (the forced-alignment limit behind a beam) and "
                         f"segment - 2 radius >= 2 radius + 1 (disjoint search zones), got segment={segment} radius={radius}")
    return segment - 2 * radius


def plan_windows(F: int, window: int, stride: int) -> WindowPlan:
    """The window plan above for ``F`` lip frames: pure host integers."""
    F, W, S = int(F), int(window), int(stride)
    hop = check_plan(W, S)
    if F < 1:
        raise ValueError(f"plan_windows: need at least one frame, got F={F}")
    if F <= W:
        return WindowPlan(F, W, S, hop, F, [0], [0, F], 1)
    nw = -(-(F - W) // hop) + 1
    starts = [min(k * hop, F - W) for k in range(nw)]
    cuts = [0] + [(starts[k - 1] + starts[k] + W) // 2 for k in range(1, nw)] + [F]
    cover = np.zeros(F + 1, np.int64)
    for s in starts:
        cover[s] += 1
        cover[s + W] -= 1
    return WindowPlan(F, W, S, hop, W, starts, cuts, int(np.cumsum(cover).max()))


def boundaries(F: int, segment: int, radius: int) -> int:
    """nb: the number of j >= 1 with j N + radius < F."""
    N = check_segment(segment, radius)
    return max(0, (int(F) - 1 - int(radius)) // N)


def _f32(x: torch.Tensor) -> torch.Tensor:
    x = x.detach()
    return x if x.dtype == torch.float32 else x.float()


def _block(who: str, x, dims: int) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != dims or not x.dtype.is_floating_point:
        raise ValueError(f"{who}: need a floating-point tensor of {dims} dimensions, got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if x.shape[-1] < 2:
        raise ValueError(f"{who}: need V >= 2, got {x.shape[-1]}")


def host_stitch_law(win: np.ndarray, row: np.ndarray, wt: np.ndarray) -> np.ndarray:
    """The stitch law on window rows [S, R, V] with a source table, in the dtype of ``win`` (float32: the law the device follows)."""
    Z = win.dtype.type
    S, _, V = win.shape
    F = row.shape[0]
    n = (row >= 0).sum(1)
    out = np.empty((S, F, V), win.dtype)
    one = n == 1
    out[:, one] = win[:, row[one, 0]]                                      # bit copies
    with np.errstate(all="ignore"):
        for cnt in range(2, MAX_SOURCES + 1):
            t = np.nonzero(n == cnt)[0]
            if not len(t):
                continue
            x = np.stack([win[:, row[t, k]] for k in range(cnt)])           # [cnt, S, len(t), V]
            M = x.max(0)                                                   # a NaN propagates
            acc = None
            for k in range(cnt):
                term = wt[t, k].astype(win.dtype)[None, :, None] * np.exp(x[k] - M)
                acc = term if acc is None else acc + term
            out[:, t] = np.where(M == Z(-np.inf), Z(-np.inf), M + np.log(acc))
    return out


def stitch(window_log_probs: torch.Tensor, plan: WindowPlan, policy: str = "centre") -> torch.Tensor:
    """``window_log_probs`` [S, nw, W, V] (W = ``plan.width``) -> float32 [S, F, V] on the input's device: the stitch law above.  GPU
    tensor: av_ctc_stitch with the plan's source table, uploaded once per plan.  Host tensor: the same law in float32 numpy."""
    _block("stitch", window_log_probs, 4)
    S, nw, W, V = window_log_probs.shape
    if nw != plan.count or W != plan.width:
        raise ValueError(f"stitch: the plan has {plan.count} windows of {plan.width} frames, the log-probs {nw} of {W}")
    if window_log_probs.is_cuda:
        from . import ops
        row, wt = plan.table(policy, window_log_probs.device)
        return ops.ctc_stitch(_f32(window_log_probs), row, wt, plan.frames)
    row, wt = plan.sources(policy)
    win = _f32(window_log_probs).contiguous().numpy().reshape(S, nw * W, V)
    return torch.from_numpy(host_stitch_law(win, row, wt))


def host_cut_law(col: np.ndarray, segment: int, radius: int) -> np.ndarray:
    """The cut-point law on ONE speaker's blank column [F] (float32) -> int32 [nb + 2]."""
    F = col.shape[0]
    N, nb = segment - 2 * radius, boundaries(F, segment, radius)
    cuts = np.empty(nb + 2, np.int32)
    cuts[0], cuts[nb + 1] = 0, F
    for j in range(1, nb + 1):
        lo, hi = max(j * N - radius, 1), min(j * N + radius, F - 1)
        z = col[lo:hi + 1].astype(np.float32)
        z = np.where(np.isnan(z), np.float32(-np.inf), z)
        cuts[j] = lo + int(np.argmax(z))                                   # the first maximal index
    return cuts


def cut_points(log_probs: torch.Tensor, blank: int, segment: int, radius: int) -> torch.Tensor:
    """``log_probs`` [S, F, V] -> int32 [S, nb + 2] on the input's device: the cut-point law above (GPU: av_ctc_cut_points, strided views with
    contiguous rows are taken as they are, nothing is read back)."""
    _block("cut_points", log_probs, 3)
    S, F, V = log_probs.shape
    blank = int(blank)
    if not 0 <= blank < V or F < 1:
        raise ValueError(f"cut_points: need 0 <= blank < V and F >= 1, got F={F} V={V} blank={blank}")
    nb = boundaries(F, segment, radius)
    if log_probs.is_cuda:
        from . import ops
        return ops.ctc_cut_points(_f32(log_probs), blank, int(segment), int(radius), nb)
    col = _f32(log_probs)[:, :, blank].numpy()
    return torch.from_numpy(np.stack([host_cut_law(col[s], int(segment), int(radius)) for s in range(S)]).reshape(S, nb + 2))


def split_segments(log_probs: torch.Tensor, cuts: torch.Tensor, segment: int):
    """``log_probs`` [S, F, V], ``cuts`` int32 [S, nb + 2] as ``cut_points`` returns them -> (seg_lp float32 [S (nb + 1), segment, V], seg_len
    int64 [S (nb + 1)]) on the input's device, every element written (GPU: av_ctc_segment_gather reads the cuts from device memory).  Cuts
    are clamped to [0, F] and made monotone, a segment longer than ``segment`` is cut there: ``cut_points`` never produces either."""
    _block("split_segments", log_probs, 3)
    S, F, V = log_probs.shape
    segment = int(segment)
    if not 1 <= segment <= MAX_SEGMENT or F < 1:
        raise ValueError(f"split_segments: need 1 <= segment <= {MAX_SEGMENT} and F >= 1, got segment={segment} F={F}")
    if not isinstance(cuts, torch.Tensor) or cuts.dim() != 2 or cuts.shape[0] != S or cuts.shape[1] < 2 or cuts.dtype != torch.int32:
        raise ValueError(f"split_segments: cuts must be int32 [S={S}, nb + 2]")
    if cuts.shape[1] - 2 >= F:
        raise ValueError(f"split_segments: {cuts.shape[1] - 2} boundaries for {F} frames")
    if log_probs.is_cuda:
        from . import ops
        return ops.ctc_segment_gather(_f32(log_probs), cuts.to(log_probs.device, non_blocking=True), segment)
    lp, c = _f32(log_probs).numpy(), cuts.numpy()
    nb = c.shape[1] - 2
    seg = np.zeros((S * (nb + 1), segment, V), np.float32)
    ln = np.zeros((S * (nb + 1),), np.int64)
    for s in range(S):
        for j in range(nb + 1):
            c0 = min(max(int(c[s, j]), 0), F)
            c1 = min(max(int(c[s, j + 1]), c0), F)
            n = min(c1 - c0, segment)
            seg[s * (nb + 1) + j, :n] = lp[s, c0:c0 + n]
            ln[s * (nb + 1) + j] = n
    return torch.from_numpy(seg), torch.from_numpy(ln)
