"""The opt-in settings of MultimodalTrainer in one table: keyword argument -> (environment variable, parser of its text, default text, cast of an
explicit argument).  ``resolve(name, argument)``: an argument that is not None wins, otherwise the variable is parsed,
otherwise the default text is.  The variables are read when the trainer is constructed.  Every feature is off at its default, and off means that
none of its code runs.  Not here: AVAMD_AUG_* (augment.Augment.from_env), AVAMD_FUSED_LOSS / AVAMD_VISUAL_STREAMS (read when trainer.py is imported).
"""
from __future__ import annotations

import os

from .. import ops

_is1 = lambda text: text == "1"         # noqa: E731  the flags that are on only at "1"
_path = lambda text: text or None       # noqa: E731  an empty variable is an unset one
_same = lambda x: x                     # noqa: E731

OPTIONS = {
    # CTC loss of forward_losses (and so of evaluate()) on the device kernels of ops.ctc_loss: lengths and targets stay on the device, the step holds
    # no synchronising call and ignores host_metadata()'s ``_ctc_*_lengths``.  The law (on unless "0") is ops.native_ctc_default's, as for CTCDecoder
    "native_ctc": ("AVAMD_NATIVE_CTC", lambda _text: ops.native_ctc_default(), "0", bool),
    # evaluate() decodes with beam_search.prefix_beam_search of this width; 0 = greedy, what the reference's simple_beam_search computes
    "eval_beam_width": ("AVAMD_EVAL_BEAM", int, "0", int),
    # ... with n-gram shallow fusion: an lm.NGramLM, or the path of an ARPA file whose tokens are the tokenizer's pieces
    "eval_lm": ("AVAMD_EVAL_LM", _path, "", _same),
    "eval_lm_weight": ("AVAMD_EVAL_LM_WEIGHT", float, "0.5", float),
    "eval_token_bonus": ("AVAMD_EVAL_TOKEN_BONUS", float, "0.0", float),
    # ... with contextual phrase biasing, with or without eval_lm: a bias.ContextBias, or the path of a phrase file (UTF-8, one phrase per line);
    # the weight 1.0 is a setting, not a tuned value
    "eval_bias": ("AVAMD_EVAL_BIAS", _path, "", _same),
    "eval_bias_weight": ("AVAMD_EVAL_BIAS_WEIGHT", float, "1.0", float),
    # evaluate() counts token / character / word errors with their S / D / I split on the device (error_rate.error_counts), leaves the rates in
    # ``last_report`` and takes its WER from those counts
    "eval_report": ("AVAMD_EVAL_REPORT", _is1, "0", bool),
    # minimum word error rate training (mwer.mwer_loss, all on the device): with gradients enabled forward_losses adds
    # mwer_weight * (mwer1 + mwer2) / 2 to ``total``; evaluate()'s loss stays the CTC loss
    "mwer_weight": ("AVAMD_MWER_WEIGHT", float, "0", float),
    "mwer_nbest": ("AVAMD_MWER_NBEST", int, "4", int),
    "mwer_beam": ("AVAMD_MWER_BEAM", int, "8", int),
    # global-norm clipping (clip_grad_norm_'s law) and a linear warmup / decay of the learning rate (optim.lr_multiplier, one multiplier for all
    # groups; with a warmup the first step runs at 0, as LambdaLR does) inside the fused Adam step: no synchronising call.  Data parallel: the
    # norm is taken after the all-reduce, over grad * grad_scale, so every rank computes the same bits
    "max_grad_norm": ("AVAMD_CLIP_NORM", float, "0", float),
    "warmup_steps": ("AVAMD_WARMUP_STEPS", int, "0", int),
    "total_steps": ("AVAMD_TOTAL_STEPS", int, "0", int),
    # decoupled weight decay (torch.optim.AdamW's law; the same value for all four groups, tensors with ndim <= 1 - biases, norm weights, PReLU
    # slopes - not decayed) and the schedule after the warmup ("linear", or "cosine": optim.lr_multiplier(..., schedule="cosine"), needs
    # total_steps), both inside the same fused step.  Data parallel: every rank computes the same bytes, nothing is communicated
    "weight_decay": ("AVAMD_WEIGHT_DECAY", float, "0", float),
    "lr_schedule": ("AVAMD_LR_SCHEDULE", str, "linear", str),
    # an exponential moving average of the trainable weights inside the same fused step (skipped with an overflowing step, moved for LayerDrop-ped
    # layers too); ema_warmup: optim.ema_decay's.  eval_ema: evaluate() and align() run on the averages (swapped in and back in place; BatchNorm
    # buffers are not averaged, AveragedModel's default).  Data parallel: every rank computes the same averages, nothing is communicated
    "ema_decay": ("AVAMD_EMA_DECAY", float, "0", float),
    "ema_warmup": ("AVAMD_EMA_WARMUP", _is1, "0", bool),
    "eval_ema": ("AVAMD_EVAL_EMA", _is1, "0", bool),
    # gradient accumulation: every train_step is one micro-step whose gradients are summed on the device (optim.AvAdam.accumulate), and every
    # accum_steps-th ends with ONE fused step on the mean - clipping, schedule, EMA, decay and loss scaling per optimizer step.  1: no accumulation.
    # Data parallel: every micro-step all-reduces its buckets as a step does, so every rank accumulates the same bytes
    "accum_steps": ("AVAMD_ACCUM_STEPS", int, "1", int),
    # transcribe()'s confidences (confidence.py): the frame measure ("tsallis", "entropy", "max_prob"), the Tsallis exponent, and how a token's
    # frames, a word's tokens and an utterance's tokens are aggregated ("min", "mean", "prod"); read by transcribe() alone
    "conf_method": ("AVAMD_CONF_METHOD", str, "tsallis", str),
    "conf_alpha": ("AVAMD_CONF_ALPHA", float, "0.33", float),
    "conf_aggregation": ("AVAMD_CONF_AGG", str, "min", str),
    # transcribe_long() (longform.py), read by it alone: lip frames per window and discarded per window side, how overlapping windows are
    # joined ("centre": the owner's rows; "average": the weighted mean of the posteriors), windows per forward call, and the longest segment
    # of the stitched sequence with the half-width of the zone in which its cut is searched
    "long_window": ("AVAMD_LONG_WINDOW", int, "100", int),
    "long_stride": ("AVAMD_LONG_STRIDE", int, "12", int),
    "long_policy": ("AVAMD_LONG_POLICY", str, "centre", str),
    "long_batch": ("AVAMD_LONG_BATCH", int, "16", int),
    "long_segment": ("AVAMD_LONG_SEGMENT", int, "400", int),
    "long_radius": ("AVAMD_LONG_RADIUS", int, "50", int),
    # spot() and spot_long() (spot.py), read by them alone where the call gives None: the lowest score a hit may have (a log-likelihood ratio,
    # <= 0; "-inf" keeps every hit) and the hits reported per utterance and keyword (1 .. 8)
    "spot_min_score": ("AVAMD_SPOT_MIN_SCORE", float, "-inf", float),
    "spot_max_hits": ("AVAMD_SPOT_MAX_HITS", int, "4", int),
    # align_long() (segmentation.py), read by it alone where the call gives None: the frames per window of an utterance's score (the least
    # window mean) and which ends of the path may float - 0 none, 1 the start, 2 the end, 3 both
    "segment_window": ("AVAMD_SEGMENT_WINDOW", int, "30", int),
    "segment_free": ("AVAMD_SEGMENT_FREE", int, "0", int),
}


def resolve(name: str, argument):
    env, parse, default, cast = OPTIONS[name]
    return parse(os.environ.get(env, default)) if argument is None else cast(argument)


# cross-field checks, one per feature group; the trainer calls each right after it has resolved the group
def check_decode(beam_width: int, what: str, value, lacks: str) -> None:
    if value is not None and beam_width == 0:
        raise ValueError(f"{what} needs eval_beam_width > 0: the greedy decode has no {lacks}")


def check_mwer(weight: float, nbest: int, beam: int, level: str) -> None:
    if not 0.0 <= weight < float("inf"):                   # NaN fails both comparisons
        raise ValueError(f"mwer_weight must be finite and >= 0, got {weight}")
    if not 1 <= nbest <= beam <= 64:
        raise ValueError(f"need 1 <= mwer_nbest <= mwer_beam <= 64, got mwer_nbest={nbest} mwer_beam={beam}")
    if level not in ("word", "char", "token"):
        raise ValueError(f"mwer_level must be 'word', 'char' or 'token', got {level!r}")


def check_confidence(method: str, alpha: float, aggregation: str) -> None:
    from ..confidence import check_aggregation, check_method
    check_method("conf_method / conf_alpha", method, alpha)
    check_aggregation("conf_aggregation", aggregation)


def check_longform(window: int, stride: int, policy: str, batch: int, segment: int, radius: int) -> None:
    from ..longform import MAX_SOURCES, POLICIES, check_plan, check_segment, min_average_hop
    hop = check_plan(window, stride)
    check_segment(segment, radius)
    if policy not in POLICIES:
        raise ValueError(f"long_policy must be one of {POLICIES}, got {policy!r}")
    if policy == "average" and hop < min_average_hop(window):
        raise ValueError(f"long_policy='average' joins at most {MAX_SOURCES} windows per frame: long_window={window} needs a hop of at least "
                         f"{min_average_hop(window)}, long_window - 2 long_stride is {hop}")
    if batch < 1:
        raise ValueError(f"long_batch must be >= 1, got {batch}")


def check_spot(min_score: float, max_hits: int) -> None:
    from ..spot import MAX_HITS
    if min_score != min_score:
        raise ValueError("spot_min_score must not be NaN")
    if not 1 <= max_hits <= MAX_HITS:
        raise ValueError(f"spot_max_hits must be in [1, {MAX_HITS}], got {max_hits}")


def check_segmentation(window: int, free: int) -> None:
    if window < 1:
        raise ValueError(f"segment_window must be >= 1, got {window}")
    if not 0 <= free <= 3:
        raise ValueError(f"segment_free must be 0 (fixed ends), 1 (free start), 2 (free end) or 3 (both), got {free}")


def check_ema(eval_ema: bool, ema_decay: float) -> None:
    if eval_ema and not ema_decay > 0:
        raise ValueError("eval_ema needs ema_decay > 0: there is no averaged model to evaluate")


def check_accum(accum_steps: int) -> None:
    if accum_steps < 1:
        raise ValueError(f"accum_steps must be >= 1 (1 = no accumulation), got {accum_steps}")


def check_schedule(lr_schedule: str, total_steps: int) -> None:
    if lr_schedule not in ("linear", "cosine"):
        raise ValueError(f"lr_schedule must be 'linear' or 'cosine', got {lr_schedule!r}")
    if lr_schedule == "cosine" and not total_steps > 0:
        raise ValueError("lr_schedule='cosine' needs total_steps > 0: the cosine has to know where it ends")
