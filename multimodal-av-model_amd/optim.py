"""Adam with a fused HIP step kernel (torch.optim.Adam defaults: betas (0.9, 0.999), eps 1e-8, no weight decay —
model/trainer.py:34-39).  State keys (step / exp_avg / exp_avg_sq) match torch.optim.Adam, so the reference's
checkpoint dict (main.py:47-55) stays loadable.  ``grad_scale`` folds the data-parallel 1/world_size (or a loss
un-scale) into the step so that no extra pass over the gradients is needed.  Opt-in (``max_grad_norm`` / ``warmup_steps`` /
``total_steps``): global-norm gradient clipping and a linear warmup / decay schedule of the learning rate, decided on the device inside
the same fused step.  Opt-in (``ema_decay``): an exponential moving average of the weights kept by that step, and
``swap_averaged`` / ``averaged`` to evaluate and save with it.  Opt-in (``weight_decay`` / ``lr_schedule="cosine"``):
decoupled weight decay - torch.optim.AdamW's law - and a warmup + cosine schedule, inside the same step.  Opt-in
(``accumulate()``): the gradients of several micro-batches summed on the device into one such step."""
from __future__ import annotations

import contextlib
import math

import numpy as np
import torch

from . import _lib as L
from . import ops
from .utils import shadow

# slots of the device state blocks, as csrc/optim.hip names them: loss scaling (five floats), clipping / schedule (three floats and an int32
# step counter), EMA (a float and an int32 update counter)
GS_SCALE, GS_INV, GS_INF, GS_TRACK, GS_STEP = range(5)
CS_NORM, CS_COEF, CS_LRM, CS_K = range(4)
ES_DECAY, ES_K = range(2)


class AvGradScaler:
    """torch.amp.GradScaler semantics (model/trainer.py:40,121-123 of the reference; torch/amp/grad_scaler.py:126-129 defaults: init
    65536, growth 2x after 2000 clean steps, backoff 0.5x on overflow, overflowing steps skipped) kept ENTIRELY on the device: the
    state is five floats {scale, 1/scale, found_inf, growth tracker, optimizer steps taken}; ``step`` is three launches (non-finite
    check over every gradient, fused Adam that unscales / skips, scale update) and never synchronises with the host (torch's
    ``scaler.step`` calls ``found_inf.item()``).  ``update()`` exists for call-sequence compatibility; the update has already
    happened inside ``step``.  With bf16 MFMA operands (the package's perf mode) the scaling is not needed for range - bf16 has
    fp32's exponent - but the reference's training loop is fp16 autocast + GradScaler, so its step-skipping law is reproduced."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000,
                 device="cuda", enabled: bool = True):
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.enabled = enabled
        self.state = torch.tensor([init_scale, 1.0 / init_scale, 0.0, 0.0, 0.0], dtype=torch.float32, device=device)

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        return loss * self.state[GS_SCALE] if self.enabled else loss

    def step(self, optimizer: "AvAdam"):
        return optimizer.step(scaler=self if self.enabled else None)

    def update(self) -> None:            # folded into step(): the device already applied the growth / backoff law
        return None

    def get_scale(self) -> float:        # host synchronisation (diagnostics / checkpoints only)
        return float(self.state[GS_SCALE])

    def steps_taken(self) -> int:
        return int(self.state[GS_STEP])

    def state_dict(self):
        st = self.state.tolist()
        return {"scale": st[GS_SCALE], "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(st[GS_TRACK]), "_steps_taken": int(st[GS_STEP])}

    def load_state_dict(self, sd):
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        self.state[GS_SCALE] = float(sd["scale"]); self.state[GS_INV] = 1.0 / float(sd["scale"]); self.state[GS_TRACK] = float(sd["_growth_tracker"])
        self.state[GS_STEP] = float(sd.get("_steps_taken", 0))


LR_SCHEDULES = {"linear": 0, "cosine": 1}                          # lr_schedule of av_adam_multi_wd


def lr_multiplier(k: int, warmup_steps: int = 0, total_steps: int = 0, schedule: str = "linear") -> float:
    """Learning-rate multiplier of optimizer step ``k`` (0-based, counting steps actually taken): HF get_linear_schedule_with_warmup under
    torch.optim.lr_scheduler.LambdaLR - k / warmup below the warmup, then max(0, (total - k) / (total - warmup)); ``total_steps == 0``:
    constant 1 after the warmup; both 0: always 1.  ``schedule="cosine"`` (needs total_steps > warmup_steps): after the same warmup
    max(0, 0.5 * (1 + cos(pi * (k - warmup) / (total - warmup)))), HF get_cosine_schedule_with_warmup with num_cycles = 0.5, and 0 from
    k = total on (HF's lambda rises again there).  The host form of the law the fused step evaluates on the device (tests, logging).
    With a warmup step 0 runs at multiplier 0, as in torch: moments and step counts advance, the parameters do not move."""
    k, warmup_steps, total_steps = int(k), int(warmup_steps), int(total_steps)
    check_lr_schedule(schedule, warmup_steps, total_steps)
    if k < warmup_steps:
        return k / warmup_steps
    if schedule == "cosine":
        if k >= total_steps:
            return 0.0
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((k - warmup_steps) / (total_steps - warmup_steps)))))
    if total_steps == 0:
        return 1.0
    return max(0.0, (total_steps - k) / (total_steps - warmup_steps))


def check_clip_schedule(max_grad_norm, warmup_steps, total_steps):
    """Validated (max_grad_norm, warmup_steps, total_steps); ValueError otherwise (the conditions of av_adam_multi_ex)."""
    max_grad_norm, warmup_steps, total_steps = float(max_grad_norm), int(warmup_steps), int(total_steps)
    if not max_grad_norm >= 0.0:                                # NaN fails the comparison
        raise ValueError(f"max_grad_norm must be >= 0 (0 = no clipping), got {max_grad_norm}")
    if warmup_steps < 0 or total_steps < 0:
        raise ValueError(f"warmup_steps and total_steps must be >= 0, got {warmup_steps} and {total_steps}")
    if total_steps != 0 and total_steps <= warmup_steps:
        raise ValueError(f"total_steps must be 0 (no decay) or above warmup_steps, got total_steps={total_steps} warmup_steps={warmup_steps}")
    return max_grad_norm, warmup_steps, total_steps


def check_lr_schedule(lr_schedule, warmup_steps, total_steps):
    """The code of ``lr_schedule`` ("linear" 0, "cosine" 1); ValueError for another name, and for cosine without total_steps > warmup_steps."""
    if lr_schedule not in LR_SCHEDULES:
        raise ValueError(f"lr_schedule must be 'linear' or 'cosine', got {lr_schedule!r}")
    if lr_schedule == "cosine" and not int(total_steps) > max(0, int(warmup_steps)):
        raise ValueError(f"lr_schedule='cosine' needs total_steps above warmup_steps, got total_steps={total_steps} warmup_steps={warmup_steps}")
    return LR_SCHEDULES[lr_schedule]


def check_weight_decay(weight_decay):
    """Validated weight_decay (finite, >= 0; 0 = none); ValueError otherwise."""
    weight_decay = float(weight_decay)
    if not 0.0 <= weight_decay < float("inf"):                  # NaN fails both comparisons
        raise ValueError(f"weight_decay must be finite and >= 0 (0 = no decay), got {weight_decay}")
    return weight_decay


def ema_decay(k: int, decay: float, warmup: bool = False) -> float:
    """Decay d_k of EMA update ``k`` (0-based, counting updates actually made), in float64: d_0 = 0 - the first update copies the
    parameters, torch.optim.swa_utils.AveragedModel's ``n_averaged == 0`` - then ``decay``, or min(decay, (1 + k) / (10 + k)) with
    ``warmup`` (TensorFlow's ExponentialMovingAverage, timm's ModelEmaV2).  The update is ``torch.lerp(ema, p_new, 1 - d_k)``.  The host form
    of the law the fused step evaluates on the device (tests, logging)."""
    k, decay = int(k), float(decay)
    if k < 1:
        return 0.0
    return min(decay, (1.0 + k) / (10.0 + k)) if warmup else decay


def check_ema(decay, warmup=False):
    """Validated (ema_decay, ema_warmup); ValueError otherwise (the conditions of av_adam_multi_ema).  0 = no EMA."""
    decay, warmup = float(decay), bool(warmup)
    if not 0.0 <= decay < 1.0:                                  # NaN fails both comparisons
        raise ValueError(f"ema_decay must be in [0, 1) (0 = no EMA), got {decay}")
    return decay, warmup


def _chunk_table(numels, chunk):
    """(chunk_tensor, chunk_start) of a multi-tensor launch: tensor t is cut into chunks of ``chunk`` elements."""
    pairs = [(t, s0) for t, n in enumerate(numels) for s0 in range(0, n, chunk)]
    return [t for t, _ in pairs], [s0 for _, s0 in pairs]


def _size_tables(numels, chunk, dev):
    """Device tables (sizes, chunk_tensor, chunk_start) of the tensors with these element counts, and the number of chunks."""
    ct, cs = _chunk_table(numels, chunk)
    return (ops.h2d_async(np.asarray(numels, dtype=np.int64), dev), ops.h2d_async(np.asarray(ct, dtype=np.int32), dev),
            ops.h2d_async(np.asarray(cs, dtype=np.int64), dev), len(ct))


class _PtrTable:
    """Device table of ``n`` pointers, filled through a pinned host buffer and uploaded again only when a pointer changed (the caching
    allocator usually hands the gradients the same blocks)."""

    def __init__(self, n, dev):
        self.host = torch.empty(n, dtype=torch.long).pin_memory()
        self.dev = torch.empty(n, dtype=torch.long, device=dev)
        self.evt = self.flat = None

    def upload(self, flat):
        if self.flat != flat:
            if self.evt is not None:
                self.evt.synchronize()                              # the previous upload has left the pinned buffer
            self.host.copy_(torch.tensor(flat, dtype=torch.long))
            self.dev.copy_(self.host, non_blocking=True)
            self.evt = torch.cuda.Event(); self.evt.record()
            self.flat = flat


class _StateBlock:
    """Device block of ``n_words`` 32-bit words: floats, and an int32 counter at ``counter_index``.  It is made at first use and again when
    the device changes; until then, and into a fresh block, the counter is the host seed (load_state_dict)."""

    def __init__(self, n_words, counter_index):
        self.n_words, self.k, self.seed, self.dev = n_words, counter_index, 0, None

    def on(self, dev):
        if self.dev is None or self.dev.device != torch.device(dev):
            self.dev = torch.zeros(self.n_words, dtype=torch.float32, device=dev)
            if self.seed:
                self.set_counter(self.seed)
        return self.dev

    def counter(self) -> int:                                       # synchronises with the device once the block exists
        return self.seed if self.dev is None else int(self.dev.view(torch.int32)[self.k])

    def set_counter(self, k: int) -> None:
        self.seed = int(k)
        if self.dev is not None:
            self.dev.view(torch.int32)[self.k:self.k + 1].fill_(self.seed)

    def view(self, i):                                              # 0-dim device tensor (no sync); None before the first use
        return None if self.dev is None else self.dev[i]


class _Plan:
    """Static part of one multi-tensor launch (cached per set of (parameter, hyper-parameters)): sizes, {lr, beta1, beta2, eps} per tensor,
    chunk table, step-table slots - and the pointer table of its last launch.  With an EMA also sizes and chunk table of the "EMA-only"
    tensors (an average, no gradient in this pattern) and the EMA pointer table [n] + [n_only][2].  ``wd``: the weight decay of each tensor,
    None when every one is 0."""
    __slots__ = ("sizes", "hyper", "ct", "cs", "slots", "nch", "n", "ptrs", "eo_n", "eo_nch", "eo_sizes", "eo_ct", "eo_cs", "ema", "wd")


class _AccumPlan:
    """Static part of one av_grad_accum_multi launch (cached per set of (parameter, mode)): sizes, chunk table, the mode of each tensor (0: its
    first contribution of the cycle, a copy; 1: an add) - and the pointer table [n][2] = {grad, accumulator} of its last launch."""
    __slots__ = ("sizes", "ct", "cs", "nch", "mode", "ptrs")


class AvAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics, one fused launch per step whatever the set of parameters that received a gradient: step counts are
    PER TENSOR (torch keeps ``state[p]['step']`` per parameter; LayerDrop leaves a whole layer without gradients now and then,
    hf:774-789) and live in a device table the kernel reads and a trailing one-block launch advances.  The host-side ``state[p]['step']``
    mirrors it exactly without loss scaling; under loss scaling the device decides which steps count (``sync_steps``).

    ``max_grad_norm`` > 0 clips the gradients by their global L2 norm (torch.nn.utils.clip_grad_norm_'s law, taken over the gradients as
    the step sees them: times ``grad_scale``, un-scaled under loss scaling); ``warmup_steps`` / ``total_steps`` scale every group's ``lr``
    by ``lr_multiplier(k)``, k = steps actually taken.  Both are evaluated on the device inside the step (one more read of the gradients for
    the norm; no host synchronisation, no new plan); ``param_groups[i]["lr"]`` stays the base rate.

    ``ema_decay`` > 0 keeps ``state[p]["ema"]`` (fp32, created as a copy of ``p`` at the first step in which ``p`` has a gradient; a
    parameter that never gets one has no average: its averaged value is itself): every non-skipped step moves it by
    ``torch.lerp(ema, p_new, 1 - ema_decay(k))`` inside the Adam launch, parameters without a gradient in that step included; under loss
    scaling the device skips it with the step.  ``swap_averaged()`` / ``averaged()`` exchange parameters and averages in place, 16-bit
    shadows included.  Data parallel: every rank computes the same averages from the same bytes, nothing is communicated.

    ``weight_decay`` (a per-group key, as in torch.optim.AdamW; a group without it - a state dict from before - runs at the constructor's
    value) multiplies a tensor by ``1 - lr * lr_multiplier(k) * weight_decay`` ahead of its Adam update, inside the same launch: AdamW's
    decoupled law, so a skipped step, a warmup step at multiplier 0 and a tensor without a gradient decay nothing.  Tensors with
    ``ndim <= 1`` (biases, LayerNorm / BatchNorm weights, PReLU slopes) are not decayed unless ``decay_1d`` is set: the usual rule, without
    splitting groups.  ``lr_schedule="cosine"`` replaces the linear decay after the warmup by ``lr_multiplier(..., schedule="cosine")`` and
    needs ``total_steps``.

    ``accumulate()`` folds every ``p.grad`` into an fp32 accumulator of its own with one launch (av_grad_accum_multi: a copy for a tensor's
    first contribution of the cycle, an fp32 add after it - autograd's ``.grad +=``, bit for bit) and counts in ``accum_pending``.  The next
    ``step()`` then runs on the accumulators of the parameters that contributed, at ``grad_scale / accum_pending`` (the mean over the
    micro-batches; ``accum_mean=False``: the sum), and closes the cycle.  Everything above stays per optimizer step; a step the device skips
    for an overflow discards the whole cycle, as torch's GradScaler with accumulation does.  Without a call of ``accumulate()`` nothing of
    this runs and no accumulator exists.

    Every step is one call of ``av_adam_multi_wd`` with zeros and NULLs for what is off: by that function's contract this is
    ``av_adam_multi_ema`` without decay and cosine, ``av_adam_multi_ex`` without an EMA and ``av_adam_multi`` with clipping and schedule off as
    well - the same kernels are launched."""

    SCHEDULE_KEY = "av_schedule_step"     # state_dict entry of the schedule step; torch.optim.Adam.load_state_dict ignores it
    EMA_KEY = "av_ema_step"               # ... of the count of EMA updates

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0, warmup_steps=0, total_steps=0, ema_decay=0.0,
                 ema_warmup=False, weight_decay=0.0, decay_1d=False, lr_schedule="linear", accum_mean=True):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=check_weight_decay(weight_decay)))
        self.max_grad_norm, self.warmup_steps, self.total_steps = check_clip_schedule(max_grad_norm, warmup_steps, total_steps)
        self.lr_schedule, self.decay_1d = lr_schedule, bool(decay_1d)
        self._lr_schedule = check_lr_schedule(lr_schedule, self.warmup_steps, self.total_steps)
        self.ema_decay, self.ema_warmup = check_ema(ema_decay, ema_warmup)
        self._ema_state = _StateBlock(2, ES_K)     # {decay of the last update, count of updates}
        self._swapped = False         # swap_averaged(): the parameters currently hold the averages
        self._swap_plan = None
        self._clip_state = _StateBlock(4, CS_K)    # {norm, clip coefficient, lr multiplier, schedule step}
        self._clip_ws = None          # one double per chunk of all parameters
        self.grad_scale = 1.0
        self._plans = {}
        self._slot = None             # id(parameter) -> slot in the device step table
        self._steps_dev = None
        self._steps_seeded = False
        self._keep = None             # the last step's gradients, alive until the next step (stream-ordered use)
        self.fused_launches = 0       # diagnostics / tests: every step is one av_adam_multi_wd call
        self.accum_mean = bool(accum_mean)
        self.accum_pending = 0        # accumulate() calls of the open cycle (0: none is open)
        self._accum = {}              # parameter -> its fp32 accumulator, made at its first contribution (not in self.state: not saved)
        self._accum_open = set()      # id(parameter) of those that contributed to the open cycle: host knowledge, like p.grad is None
        self._accum_plans = {}
        self._accum_keep = None       # the last accumulate()'s gradients, alive until the next one

    CHUNK = 65536

    def _slots(self):
        if self._slot is None:
            self._slot, n = {}, 0
            for group in self.param_groups:
                for p in group["params"]:
                    self._slot[id(p)] = n
                    n += 1
        return self._slot

    def _step_table(self, dev):
        """Device int32 table of per-parameter step counts, seeded from the host state (fresh optimizer: zeros; after load_state_dict:
        the checkpoint's counts)."""
        slots = self._slots()
        if self._steps_dev is None or self._steps_dev.device != torch.device(dev):
            self._steps_dev = torch.zeros(max(1, len(slots)), dtype=torch.int32, device=dev)
            self._steps_seeded = False
        if not self._steps_seeded:
            host = np.zeros(max(1, len(slots)), dtype=np.int32)
            for group in self.param_groups:
                for p in group["params"]:
                    st = self.state.get(p)
                    if st and "step" in st:
                        host[slots[id(p)]] = int(st["step"])
            self._steps_dev.copy_(ops.h2d_async(host, dev))
            self._steps_seeded = True
        return self._steps_dev

    @property
    def clipping(self) -> bool:
        return self.max_grad_norm > 0.0

    @property
    def scheduled(self) -> bool:
        return self.warmup_steps > 0 or self.total_steps > 0

    def _clip_block(self, dev):
        """State block and norm workspace of clipping and schedule: allocated once, they live with the optimizer."""
        cstate = self._clip_state.on(dev)
        if self._clip_ws is None or self._clip_ws.device != cstate.device:
            nch = sum(-(-p.numel() // self.CHUNK) for group in self.param_groups for p in group["params"])
            self._clip_ws = torch.empty(max(1, nch), dtype=torch.float64, device=dev)
        return cstate, self._clip_ws

    @property
    def last_grad_norm(self):
        """0-dim device tensor (a view of the state block, no sync): global L2 norm of the last step's gradients as Adam saw them.  None
        before the first step with clipping or a schedule on; 0 with clipping off."""
        return self._clip_state.view(CS_NORM)

    @property
    def last_clip_coef(self):
        """0-dim device tensor: min(1, max_grad_norm / (norm + 1e-6)) of the last step."""
        return self._clip_state.view(CS_COEF)

    @property
    def last_lr_mult(self):
        """0-dim device tensor: learning-rate multiplier the last step ran at."""
        return self._clip_state.view(CS_LRM)

    def schedule_step(self) -> int:
        """Steps taken on the schedule so far (synchronises with the device; checkpoints and diagnostics, like AvGradScaler.steps_taken)."""
        return self._clip_state.counter()

    @property
    def averaging(self) -> bool:
        return self.ema_decay > 0.0

    @property
    def last_ema_decay(self):
        """0-dim device tensor (a view of the EMA state block, no sync): decay d_k the last step's EMA update ran at.  None before the
        first step with an EMA."""
        return self._ema_state.view(ES_DECAY)

    def ema_step(self) -> int:
        """EMA updates made so far (synchronises with the device, like schedule_step)."""
        return self._ema_state.counter()

    def _averaged_params(self):
        return [p for group in self.param_groups for p in group["params"] if "ema" in self.state.get(p, ())]

    @torch.no_grad()
    def swap_averaged(self) -> None:
        """Exchange every parameter that has an average with it, in place, in one launch (av_param_swap_multi): afterwards the model
        computes with the averaged weights and ``state[p]["ema"]`` holds the trained ones; a second call swaps back, bit for bit.  The
        16-bit shadows of those parameters are written by the same launch and every other compute-dtype cache rebuilds.  Parameters
        without an average stay as they are.  ``step()`` refuses to run in between."""
        ps = self._averaged_params()
        self._swapped = not self._swapped
        if not ps:
            return
        dev = ps[0].device
        shadows = shadow.lookup_many(ps)
        flat = []
        for p, sh in zip(ps, shadows):
            flat += [p.data_ptr(), self.state[p]["ema"].data_ptr(), sh.data_ptr() if sh is not None else 0]
        numels = [p.numel() for p in ps]
        key = (tuple(flat), tuple(numels))
        if self._swap_plan is None or self._swap_plan[0] != key:
            self._swap_plan = (key, ops.h2d_async(np.asarray(flat, dtype=np.int64), dev), *_size_tables(numels, self.CHUNK, dev))
        _, ptrs, sizes, ct, cs, nch = self._swap_plan
        L.check(L.lib().av_param_swap_multi(ops.ptr(ptrs), ops.ptr(sizes), ops.ptr(ct), ops.ptr(cs), nch, self.CHUNK, ops.stream()),
                "av_param_swap_multi")
        torch.autograd.graph.increment_version(ps)              # compute-dtype caches (re-layouts) rebuild
        shadow.mark_fresh([p for p, sh in zip(ps, shadows) if sh is not None])          # ... the shadows were just written

    @contextlib.contextmanager
    def averaged(self):
        """``with optimizer.averaged():`` - the model holds the averaged weights inside the block and the trained ones after it."""
        self.swap_averaged()
        try:
            yield self
        finally:
            self.swap_averaged()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._clip_state.set_counter(state_dict.get(self.SCHEDULE_KEY, 0))
        self._ema_state.set_counter(state_dict.get(self.EMA_KEY, 0))
        for st in self.state.values():                              # torch >= 2 stores 'step' as a tensor in its own checkpoints
            if "step" in st and torch.is_tensor(st["step"]):
                st["step"] = int(st["step"])
        self._steps_seeded = False                                  # the device table is re-seeded from the loaded counts
        self._close_cycle()                                         # an open accumulation cycle belongs to the state that was replaced

    def reset_state(self) -> None:
        """Forget moments and step counts (a fresh optimizer over the same parameters)."""
        self.state.clear()
        self._steps_seeded = False
        self._keep = None
        self._clip_state.set_counter(0)
        self._ema_state.set_counter(0)
        self._swapped = False
        self._close_cycle()

    def state_dict(self):
        """torch.optim.Adam's format.  Under loss scaling only the device table knows the per-parameter step counts (overflowing steps are
        skipped on the device): bring the host entries up to date first, so that a checkpoint taken through this method - not only through
        ``checkpoint_dict`` - resumes with the right bias corrections.  With a schedule the dict also carries its step (SCHEDULE_KEY), with an EMA
        the count of its updates (EMA_KEY) beside the ``ema`` tensors of the per-parameter state."""
        self.sync_steps()
        sd = super().state_dict()
        if self.scheduled:
            sd[self.SCHEDULE_KEY] = self.schedule_step()
        if self.averaging:
            sd[self.EMA_KEY] = self.ema_step()
        return sd

    def add_param_group(self, param_group):
        if getattr(self, "_steps_dev", None) is not None:
            self.sync_steps()                                       # the device table is rebuilt below: seed it from CURRENT counts
        super().add_param_group(param_group)
        check_weight_decay(self.param_groups[-1]["weight_decay"])
        self._slot = None
        self._steps_dev = None
        self._steps_seeded = False
        self._plans = {}
        self._accum_plans = {}
        self._clip_ws = None                                        # sized by the chunks of all parameters

    def _plan(self, plist, dev, ema_only=None, decays=None) -> _Plan:
        slots = self._slots()
        key = tuple((p.data_ptr(), p.numel(), hp, slots[id(p)]) for p, hp, _ in plist)
        if decays is not None:                                      # some tensor is decayed: the values are part of the plan
            key = (key, "wd", tuple(decays))
        if ema_only is not None:                                    # with an EMA the tensors WITHOUT a gradient are part of the pattern
            key = (key, tuple((p.data_ptr(), p.numel()) for p in ema_only))
        pl = self._plans.get(key)
        if pl is None:
            if len(self._plans) >= 64:                              # LayerDrop patterns: a handful of distinct parameter sets
                self._plans.clear()
            pl = _Plan()
            pl.n = len(plist)
            pl.sizes, pl.ct, pl.cs, pl.nch = _size_tables([p.numel() for p, _, _ in plist], self.CHUNK, dev)
            pl.hyper = ops.h2d_async(np.asarray([hp for _, hp, _ in plist], dtype=np.float32).reshape(-1, 4), dev)
            pl.slots = ops.h2d_async(np.asarray([slots[id(p)] for p, _, _ in plist], dtype=np.int32), dev)
            pl.ptrs = _PtrTable(5 * pl.n, dev)
            pl.eo_n = len(ema_only or ())
            pl.eo_sizes, pl.eo_ct, pl.eo_cs, pl.eo_nch = (_size_tables([p.numel() for p in ema_only], self.CHUNK, dev) if pl.eo_n
                                                          else (None, None, None, 0))
            pl.ema = _PtrTable(pl.n + 2 * pl.eo_n, dev) if ema_only is not None else None
            pl.wd = ops.h2d_async(np.asarray(decays, dtype=np.float32), dev) if decays is not None else None
            self._plans[key] = pl
        return pl

    @torch.no_grad()
    def sync_steps(self, scaler: "AvGradScaler" = None) -> None:
        """Copy the device-side per-parameter step counts into the torch.optim.Adam-compatible ``state[p]['step']`` entries (one host
        sync; checkpoints).  Needed under loss scaling, where overflowing steps are skipped without telling the host."""
        if self._steps_dev is None or not self._steps_seeded:
            return
        host = self._steps_dev.tolist()
        slots = self._slots()
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    st["step"] = int(host[slots[id(p)]])

    def _collect(self, contributed=None):
        """(plist, ema_only, decays): (parameter, {lr, beta1, beta2, eps}, state) of every parameter with a gradient, its state created at
        its first step; with an EMA, the parameters that have an average and no gradient in this step (still moved towards p), else None;
        the weight decay of each tensor of plist, or None when none of them is decayed.  ``contributed`` (a step that closes an accumulation
        cycle): the ids of the parameters that count as having a gradient, whatever their ``p.grad`` is now."""
        plist, decays = [], []
        ema_only = [] if self.averaging else None
        for group in self.param_groups:
            b1, b2 = group["betas"]
            hp = (float(group["lr"]), float(b1), float(b2), float(group["eps"]))
            wd = check_weight_decay(group.get("weight_decay", self.defaults["weight_decay"]))
            for p in group["params"]:
                if (p.grad is None) if contributed is None else (id(p) not in contributed):
                    if ema_only is not None and "ema" in self.state.get(p, ()):
                        ema_only.append(p)
                    continue
                if not p.is_cuda or p.dtype != torch.float32:
                    raise RuntimeError("AvAdam: parameters must be float32 CUDA tensors (no CPU fallback)")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if ema_only is not None and "ema" not in state:
                    state["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
                plist.append((p, hp, state))
                decays.append(wd if self.decay_1d or p.ndim > 1 else 0.0)
        return plist, ema_only, decays if any(decays) else None

    def _bind(self, pl, plist, ema_only, grads, shadows) -> None:
        """This step's pointers into the plan's tables: {param, grad, exp_avg, exp_avg_sq, shadow} per tensor and, with an EMA, the
        averages of those tensors followed by {param, ema} of the EMA-only ones."""
        flat = []
        for (p, _, st), g, sh in zip(plist, grads, shadows):
            flat += [p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), sh.data_ptr() if sh is not None else 0]
        pl.ptrs.upload(flat)
        if pl.ema is not None:
            eflat = [st["ema"].data_ptr() for _, _, st in plist]
            for p in ema_only:
                eflat += [p.data_ptr(), self.state[p]["ema"].data_ptr()]
            pl.ema.upload(eflat)

    def _launch(self, pl, steps, scaler, dev, grad_scale) -> None:
        """The one native call of a step.  Whatever is off is passed as zeros and NULLs."""
        scale = (None, 1.0, 1.0, 1) if scaler is None else (ops.ptr(scaler.state), scaler.growth_factor, scaler.backoff_factor,
                                                            scaler.growth_interval)
        cstate, ws = self._clip_block(dev) if self.clipping or self.scheduled else (None, None)
        ema = (None, None, None, None, None, 0, 0.0, 0, None)
        if self.averaging:
            only = pl.ema.dev.data_ptr() + 8 * pl.n if pl.eo_n else None
            ema = (ops.ptr(pl.ema.dev), only, ops.ptr(pl.eo_sizes), ops.ptr(pl.eo_ct), ops.ptr(pl.eo_cs), pl.eo_nch, self.ema_decay,
                   int(self.ema_warmup), ops.ptr(self._ema_state.on(dev)))
        L.check(L.lib().av_adam_multi_wd(ops.ptr(pl.ptrs.dev), ops.ptr(pl.sizes), ops.ptr(pl.hyper), ops.ptr(pl.ct), ops.ptr(pl.cs), pl.nch,
                                         self.CHUNK, ops.ptr(steps), ops.ptr(pl.slots), pl.n, float(grad_scale), *scale,
                                         self.max_grad_norm, self.warmup_steps, self.total_steps, ops.ptr(ws),
                                         ws.numel() * ws.element_size() if ws is not None else 0, ops.ptr(cstate), *ema, ops.ptr(pl.wd),
                                         self._lr_schedule, ops.stream()),
                "av_adam_multi_wd")
        self.fused_launches += 1

    def step(self, closure=None, scaler: "AvGradScaler" = None):
        """One fused multi-tensor launch for all parameters that have a gradient (per-tensor step counts, per-group lr / betas / eps).
        After ``accumulate()``: for the parameters that contributed to the open cycle, on their accumulators, and the cycle is closed."""
        if self._swapped:
            raise RuntimeError("AvAdam.step: the parameters hold the averaged weights (swap_averaged); swap back before stepping")
        loss = closure() if closure is not None else None
        if self.accum_pending > 0:
            return self._step_accumulated(loss, scaler)
        plist, ema_only, decays = self._collect()
        if not plist:
            return loss
        params = [p for p, _, _ in plist]
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in params]
        self._step_on(plist, ema_only, decays, grads, scaler, self.grad_scale)
        return loss

    def _step_accumulated(self, loss, scaler):
        """The step that closes an accumulation cycle.  The device may skip it for an overflow; the host neither knows nor needs to: the cycle
        is closed either way."""
        plist, ema_only, decays = self._collect(self._accum_open)
        if plist:
            scale = self.grad_scale / self.accum_pending if self.accum_mean else self.grad_scale
            self._step_on(plist, ema_only, decays, [self._accum[p] for p, _, _ in plist], scaler, scale)
        self._close_cycle()
        return loss

    def _step_on(self, plist, ema_only, decays, grads, scaler, grad_scale) -> None:
        """The fused step of ``plist`` on ``grads`` (contiguous fp32, one per tensor)."""
        params = [p for p, _, _ in plist]
        dev = params[0].device
        steps = self._step_table(dev)                               # BEFORE the host counts move: a fresh table is seeded from them
        pl = self._plan(plist, dev, ema_only, decays)
        shadows = shadow.lookup_many(params)                        # bf16 compute copies (perf path), written by the kernel
        self._bind(pl, plist, ema_only, grads, shadows)
        self._launch(pl, steps, scaler, dev, grad_scale)
        if scaler is None:
            for _, _, st in plist:                                  # exact host mirror (with a scaler the device decides: sync_steps)
                st["step"] = int(st["step"]) + 1
        self._keep = grads                                          # alive until the next step (stream-ordered use)
        torch.autograd.graph.increment_version(params)              # other compute-dtype caches (re-layouts) rebuild
        shadow.mark_fresh([p for p, sh in zip(params, shadows) if sh is not None])      # ... the shadows were just written

    def _close_cycle(self) -> None:
        self.accum_pending = 0
        self._accum_open.clear()
        self._accum_keep = None

    def _accum_plan(self, ps, modes, dev) -> _AccumPlan:
        key = tuple((p.data_ptr(), p.numel(), m) for p, m in zip(ps, modes))
        pl = self._accum_plans.get(key)
        if pl is None:
            if len(self._accum_plans) >= 64:                        # LayerDrop patterns, as in _plan
                self._accum_plans.clear()
            pl = _AccumPlan()
            pl.sizes, pl.ct, pl.cs, pl.nch = _size_tables([p.numel() for p in ps], self.CHUNK, dev)
            pl.mode = ops.h2d_async(np.asarray(modes, dtype=np.int32), dev)
            pl.ptrs = _PtrTable(2 * len(ps), dev)
            self._accum_plans[key] = pl
        return pl

    @torch.no_grad()
    def accumulate(self) -> None:
        """One micro-step: ``p.grad`` of every parameter that has one goes into that parameter's accumulator in one launch
        (av_grad_accum_multi) - copied if it is the parameter's first contribution of the open cycle, added in fp32 otherwise, which is the
        order and rounding of autograd's ``.grad +=`` - and ``accum_pending`` counts the call.  Nothing synchronises.  The gradients may be
        overwritten once the call has returned (stream order)."""
        ps = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        if ps:
            if any(not p.is_cuda or p.dtype != torch.float32 for p in ps):
                raise RuntimeError("AvAdam: parameters must be float32 CUDA tensors (no CPU fallback)")
            dev = ps[0].device
            modes = [1 if id(p) in self._accum_open else 0 for p in ps]
            for p in ps:
                if p not in self._accum:
                    self._accum[p] = torch.empty_like(p, memory_format=torch.contiguous_format)
            pl = self._accum_plan(ps, modes, dev)
            grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]
            flat = []
            for p, g in zip(ps, grads):
                flat += [g.data_ptr(), self._accum[p].data_ptr()]
            pl.ptrs.upload(flat)
            L.check(L.lib().av_grad_accum_multi(ops.ptr(pl.ptrs.dev), ops.ptr(pl.mode), ops.ptr(pl.sizes), ops.ptr(pl.ct), ops.ptr(pl.cs),
                                                pl.nch, self.CHUNK, ops.stream()), "av_grad_accum_multi")
            self._accum_keep = grads                                # alive until the next call (stream-ordered use)
            self._accum_open.update(id(p) for p in ps)
        self.accum_pending += 1
