"""Checkpoint helpers with the reference's dict layout (main.py:47-64): ``epoch`` + four module state_dicts (the reference's key
sets: visual 129, audio 422, fusion 30, decoder 2) + the optimizer state (torch-Adam keys), so a file written by either side
loads on the other.  Optional entries beside them, written only when the feature is on and ignored by the reference: ``scaler`` (loss
scaling) and ``augment`` (augment.Augment: step and seed as plain ints).  Loading never unpickles code: ``torch.load(..., weights_only=True)``."""
from __future__ import annotations

import torch

KEYS = ("epoch", "visual_encoder", "audio_encoder", "fusion", "decoder1", "optimizer")


def checkpoint_dict(epoch: int, trainer, averaged: bool = False) -> dict:
    """``averaged``: the four module state_dicts hold the optimizer's averaged weights (AvAdam(ema_decay=...): taken under
    ``optimizer.averaged()`` and cloned; BatchNorm buffers and parameters without an average are the trained ones); the optimizer entry is
    the one from before the swap, so the file resumes training as an ordinary checkpoint would.  Same layout either way.  An open gradient
    accumulation cycle is not saved, and dropping it would make the resumed run differ from the uninterrupted one: it is refused."""
    if getattr(trainer.optimizer, "accum_pending", 0) > 0:
        raise ValueError(f"checkpoint_dict: {trainer.optimizer.accum_pending} accumulated micro-step(s) are waiting for their optimizer step; "
                         "call trainer.flush_accumulated() first (or save at a cycle boundary)")
    sc = getattr(trainer, "scaler", None)
    if sc is not None and sc.enabled:
        trainer.optimizer.sync_steps(sc)             # steps actually taken (overflowing steps are skipped on the device)
    extra = {"scaler": sc.state_dict()} if sc is not None and sc.enabled else {}
    aug = getattr(trainer, "augment", None)
    if aug is not None:
        extra["augment"] = aug.state_dict()          # plain ints (step, seed): the resumed run draws the plans the uninterrupted one would
    opt = trainer.optimizer.state_dict()
    mods = (("visual_encoder", trainer.visual_encoder), ("audio_encoder", trainer.audio_encoder), ("fusion", trainer.fusion_module),
            ("decoder1", trainer.decoder1))
    if averaged:
        if not getattr(trainer.optimizer, "averaging", False):
            raise ValueError("checkpoint_dict: averaged=True needs an optimizer that keeps an EMA (ema_decay > 0)")
        with trainer.optimizer.averaged():
            sds = {k: {n: v.detach().clone() for n, v in m.state_dict().items()} for k, m in mods}
    else:
        sds = {k: m.state_dict() for k, m in mods}
    return {**extra, "epoch": int(epoch), **sds, "optimizer": opt}


def save_checkpoint(epoch: int, trainer, path: str, averaged: bool = False) -> None:
    """main.py:47-55.  ``averaged``: save the averaged weights (checkpoint_dict)."""
    torch.save(checkpoint_dict(epoch, trainer, averaged), path)


def load_checkpoint(trainer, path: str, *, audio_encoder: bool = False, optimizer: bool = False) -> int:
    """main.py:57-64: restores visual encoder, fusion and decoder; the reference keeps the audio encoder and the optimizer
    lines commented out, so they are opt-in here.  Returns the epoch to resume at."""
    ck = torch.load(path, map_location=getattr(trainer, "device", "cpu"), weights_only=True)
    missing = [k for k in KEYS if k not in ck]
    if missing:
        raise KeyError(f"load_checkpoint: {path!r} lacks {missing}")
    trainer.visual_encoder.load_state_dict(ck["visual_encoder"])
    if audio_encoder:
        trainer.audio_encoder.load_state_dict(ck["audio_encoder"])
    trainer.fusion_module.load_state_dict(ck["fusion"])
    trainer.decoder1.load_state_dict(ck["decoder1"])
    if optimizer:
        trainer.optimizer.load_state_dict(ck["optimizer"])
        sc = getattr(trainer, "scaler", None)
        if sc is not None and sc.enabled and "scaler" in ck:
            sc.load_state_dict(ck["scaler"])                     # (AvAdam.load_state_dict re-seeds the device-side per-parameter step table)
        aug = getattr(trainer, "augment", None)
        if aug is not None and "augment" in ck:
            aug.load_state_dict(ck["augment"])
    return int(ck["epoch"]) + 1
