"""GPU: the fused Adam step - plain, under the grad scaler, with clipping and schedule, with the weight EMA, with all of them, and the exchange
of weights and averages - against a recording of the commit before its kernels got one chunk walker and its host side one launch record
(tests/golden/optim_parent.npz, written by tests/golden/make_optim_parent.py on the commit, the device and the toolchain named inside the
file): after every step every parameter, moment, average and 16-bit shadow, the device's norm / coefficient / multiplier / decay, the scaler's
five floats and every step count are equal to the recording bit for bit, in both libraries (bfloat16 and IEEE-half shadows).

The tensors are those of test_optim_ema_gpu.py, the smallest that reach every path of the kernels: (70001,) is two chunks and a tail that is no
multiple of 4, (5,) is tail only, (128, 1024) exactly two aligned chunks, the (4097,) gradient a view one element into a larger buffer, the
(3001,) parameter a leaf that is not 16-byte aligned; parameters 0, 1, 4 and 5 have a 16-bit shadow.  Five steps; parameter 2 gets no gradient
in steps 1 and 3 (with an EMA: the EMA-only kernel).

Only AvAdam, AvGradScaler, step, state, swap_averaged, the last_* properties, schedule_step, ema_step, sync_steps and utils.shadow are used, so
``run`` works on any commit that has them.  These kernels have no atomics and a fixed order of additions, so the recorder, which runs every
case twice in fresh optimizers, records a case only if nothing differs between the two runs.  The recording is tied to the toolchain; after an
update of it, or a change that is MEANT to alter the arithmetic, record again on the commit before that change (make_optim_parent.py)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import pkg
from test_optim_ema_gpu import SHADOWED, _data, _groups, _params, _set_grads
from test_trainer_parent_gpu import bits, checksum

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_parent.npz")
STEPS = 5
CLIP = dict(max_grad_norm=1.0, warmup_steps=2, total_steps=9)      # the norm of these gradients is in the hundreds: the coefficient is active
EMA = dict(ema_decay=0.9, ema_warmup=True)
# name -> (constructor keywords, under the grad scaler, swaps after the steps)
CASES = {
    "plain": ({}, False, 0),
    "scaler": ({}, True, 0),
    "clip_schedule": (CLIP, False, 0),
    "clip_schedule_scaler": (CLIP, True, 0),                       # the norm pass is the non-finite check
    "schedule": (dict(warmup_steps=2, total_steps=9), False, 0),
    "ema": (EMA, False, 0),
    "ema_clip_schedule_scaler": (dict(EMA, **CLIP), True, 0),
    "swap": (dict(ema_decay=0.5), False, 2),                        # one swap_averaged(), and then a second one
}
RUNS = [(c, p) for c in CASES for p in ("bf16", "fp16")]
LOW = {"bf16": torch.bfloat16, "fp16": torch.float16}
INF_STEP = 2                                                         # under the scaler: an inf in this step's gradients (skip and backoff)


def record(opt, scaler, ps, shadows) -> dict:
    """name -> integer: checksums of the tensors, bit patterns of the device scalars, the counts."""
    out = {}
    for i, p in enumerate(ps):
        out[f"p{i}"] = checksum(p)
        for k in ("exp_avg", "exp_avg_sq", "ema"):
            if k in opt.state.get(p, ()):
                out[f"{k}{i}"] = checksum(opt.state[p][k])
    for i, s in zip(SHADOWED, shadows):
        out[f"shadow{i}"] = checksum(s)
    for k in ("last_grad_norm", "last_clip_coef", "last_lr_mult", "last_ema_decay"):
        v = getattr(opt, k)
        if v is not None:
            out[k] = int(bits(v)[0])
    if scaler is not None:
        for j, v in enumerate(scaler.state.cpu().numpy().view(np.uint32)):
            out[f"scaler{j}"] = int(v)
    opt.sync_steps()
    for i, p in enumerate(ps):
        out[f"step{i}"] = int(opt.state[p]["step"]) if "step" in opt.state.get(p, ()) else -1
    out["schedule_step"], out["ema_step"] = opt.schedule_step(), opt.ema_step()
    return out


def run(case: str, precision: str) -> dict:
    """One case in a fresh optimizer -> {"names": JSON list, "values": int64 [records, names]}; one record per step and per swap."""
    optim, shadow = pkg("optim"), pkg("utils.shadow")
    pkg("precision").set_precision(precision)
    kw, scaled, swaps = CASES[case]
    p0, grads = _data(steps=STEPS)
    ps = _params(p0)
    cache = shadow.ParamCache()
    low = LOW[precision]
    shadows = [cache.get(i, [ps[i]], low, lambda i=i: ps[i].data.to(low), flat=True) for i in SHADOWED]
    opt = optim.AvAdam(_groups(ps), **kw)
    scaler = optim.AvGradScaler(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2) if scaled else None
    records = []
    for k, gs in enumerate(grads):
        _set_grads(ps, gs, drop=k in (1, 3), factor=scaler.get_scale() if scaled else 1.0)
        if scaled and k == INF_STEP:
            ps[1].grad[17] = float("inf")
        if scaled:
            scaler.step(opt); scaler.update()
        else:
            opt.step()
        records.append(record(opt, scaler, ps, shadows))
    for _ in range(swaps):
        opt.swap_averaged()
        records.append(record(opt, scaler, ps, shadows))
    torch.cuda.synchronize()
    names = sorted(records[0])
    assert all(sorted(r) == names for r in records), case
    return {"names": np.array(json.dumps(names)), "values": np.array([[r[n] for n in names] for r in records], dtype=np.int64)}


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
def test_every_step_equals_the_recorded_one_bit_for_bit(recorded, case, precision):
    pre = f"{case}.{precision}."
    assert pre + "values" in recorded, f"{case} in {precision} is not in the recording"
    got = run(case, precision)
    names = json.loads(str(got["names"]))
    assert names == json.loads(str(recorded[pre + "names"]))
    want, have = recorded[pre + "values"], got["values"]
    assert want.dtype == have.dtype and want.shape == have.shape == (STEPS + CASES[case][2], len(names))
    bad = [(r, names[c]) for r, c in zip(*np.nonzero(want != have))]
    assert not bad, (len(bad), bad[:8])
