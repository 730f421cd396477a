"""BatchNorm running statistics under the step guard and the weight average (hn_state_guard, include/hydranet_hip.h).

The HIP Adam's guard (optim.Adam: train.grad_clip_norm / train.skip_nonfinite) decides about a step AFTER its forward has written
`running_mean`, `running_var` and `num_batches_tracked`, and its weight average (train.ema_decay) covers parameters only.  BufferKeeper
closes both gaps for the model's persistent BatchNorm buffers, opt-in, in two launches per step that obey the same device record and
synchronise nothing:

  snapshot()       before the forward: shadow = live                                                   (train.protect_bn_stats)
  settle(record)   after the optimizer step: a skipped step restores live from shadow; a taken one folds the live buffers into their
                   averages, avg' = avg + (1 - decay) * (live - avg), counters copied                  (train.ema_buffers)

swap() / averaged() exchange live and averaged VALUES in place (hn_swap_many, as optim.Adam.swap_ema does for parameters): no address
changes, so a captured training step and every table of raw pointers stay valid.
"""
from __future__ import annotations

import contextlib

import torch

from ._lib import lib
from .ops.core import bump_mutation_epoch, mutation_cells
from .optim import ema_decay_at

SUFFIXES = (".running_mean", ".running_var", ".num_batches_tracked")


def options(train_cfg: dict, hip_adam: bool):
    """cfgs["train"] -> (protect, ema_buffers): train.protect_bn_stats needs a guard record to obey (train.grad_clip_norm or
    train.skip_nonfinite), train.ema_buffers needs the weight average (train.ema_decay > 0), and both need the HIP Adam that keeps them"""
    protect = bool(train_cfg.get("protect_bn_stats", False))
    ema_buffers = bool(train_cfg.get("ema_buffers", False))
    clip, ema = train_cfg.get("grad_clip_norm"), train_cfg.get("ema_decay")
    guarded = (clip is not None and float(clip) > 0) or bool(train_cfg.get("skip_nonfinite", False))
    if (protect or ema_buffers) and not hip_adam:
        raise ValueError("train.protect_bn_stats / train.ema_buffers follow the HIP Adam step's record and average: they need hip_adam=True")
    if protect and not guarded:
        raise ValueError("train.protect_bn_stats obeys the step guard's record: it needs train.grad_clip_norm or train.skip_nonfinite")
    if ema_buffers and not (ema is not None and float(ema) > 0):
        raise ValueError("train.ema_buffers averages the buffers next to the weights: it needs train.ema_decay > 0")
    return protect, ema_buffers


class BufferKeeper:
    def __init__(self, named_buffers, protect: bool, ema_decay=None, ema_warmup: bool = True):
        """named_buffers: (name, tensor) pairs, e.g. model.named_buffers(); the persistent BatchNorm buffers among them are kept (names
        ending in .running_mean / .running_var: fp32, .num_batches_tracked: int64, two 32-bit words each), everything else -- the
        model's non-persistent _seg_class_weight -- is ignored.  protect: allocate shadows (snapshot() / a skipped settle()); ema_decay
        (None: off; else 0 <= ema_decay < 1), ema_warmup: allocate averages.  Shadows and averages start as clones of the live buffers
        as they are now.  The keeper holds the live tensor objects: build it after the model is on its device (a later .to() replaces a
        module's buffers; load_state_dict() copies in place and is fine)."""
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError("invalid BufferKeeper ema_decay")
        kept = [(n, t) for n, t in named_buffers if n.endswith(SUFFIXES)]
        if not kept:
            raise ValueError("BufferKeeper: no BatchNorm running statistics among the buffers")
        for n, t in kept:
            want = torch.int64 if n.endswith(".num_batches_tracked") else torch.float32
            if not (t.is_cuda and t.dtype == want and t.is_contiguous() and t.numel() > 0):
                raise RuntimeError("BufferKeeper: %s is not a contiguous CUDA %s tensor" % (n, want))
        self.names = [n for n, _ in kept]
        self.live = [t for _, t in kept]
        self.kinds = [1 if t.dtype == torch.int64 else 0 for t in self.live]
        self.words = [t.numel() * (2 if k else 1) for t, k in zip(self.live, self.kinds)]
        self.protect = bool(protect)
        self.ema_decay = float(ema_decay) if ema_decay is not None else None
        self.ema_warmup = bool(ema_warmup)
        with torch.no_grad():
            self.shadow = [t.detach().clone() for t in self.live] if self.protect else None
            self.avg = [t.detach().clone() for t in self.live] if self.ema_decay is not None else None
        self.settles = 0                # averaging settles issued (a host int; skipped steps count, as the parameters' EMA steps do)
        self._plan_cache = None         # (pointer signature, jobs, block_job, blocks, swap jobs, mutation cells)

    def _plan(self):
        sig = tuple(t.data_ptr() for t in self.live)    # (shadows and averages are the keeper's own: their storage is never replaced)
        pl = self._plan_cache
        if pl is not None and pl[0] == sig:
            return pl
        rows, swap_rows, owner, blk = [], [], [], 0
        for i, (t, w, k) in enumerate(zip(self.live, self.words, self.kinds)):
            s = self.shadow[i].data_ptr() if self.shadow is not None else 0
            a = self.avg[i].data_ptr() if self.avg is not None else 0
            nb = (w + 1023) // 1024
            rows.append([t.data_ptr(), s, a, w, blk, k])
            swap_rows.append([t.data_ptr(), a, w, blk])         # hn_swap_many moves words: a counter rides along as two
            owner += [i] * nb
            blk += nb
        dev = self.live[0].device
        pl = self._plan_cache = (sig, torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(owner, dtype=torch.int32).to(dev), blk,
                                 torch.tensor(swap_rows, dtype=torch.int64).to(dev) if self.avg is not None else None,
                                 mutation_cells(self.live))
        return pl

    def snapshot(self):
        """shadow = live (hn_state_guard mode 0), on the current stream, before the forward that writes the live buffers; nothing to do
        without train.protect_bn_stats"""
        if not self.protect:
            return
        _, jobs, owner, blk, _, _ = self._plan()
        lib().call("hn_state_guard", jobs.data_ptr(), owner.data_ptr(), blk, 0, None, 0.0)

    def settle(self, record):
        """after the optimizer step, on its stream: `record` = optim.Adam.guard_record (int32 [8] on the device) or None = not skipped.
        A skipped step restores the live buffers from their shadows and leaves the averages alone; a taken one updates the averages
        (mode 2; decay = ema_decay_at(number of averaging settles so far)) or, without averages, writes nothing (mode 1)."""
        if record is not None and not (record.is_cuda and record.dtype == torch.int32 and record.numel() >= 8):
            raise RuntimeError("BufferKeeper.settle: record is optim.Adam.guard_record (int32 [8] on the device)")
        if self.avg is None and (record is None or not self.protect):
            return                                             # neither a restore nor an average can follow
        _, jobs, owner, blk, _, cells = self._plan()
        rec = None if record is None else record.data_ptr()
        if self.avg is None:
            lib().call("hn_state_guard", jobs.data_ptr(), owner.data_ptr(), blk, 1, rec, 0.0)
        else:
            decay = ema_decay_at(self.settles, self.ema_decay, self.ema_warmup)
            self.settles += 1
            lib().call("hn_state_guard", jobs.data_ptr(), owner.data_ptr(), blk, 2, rec, decay)
        if self.protect and rec is not None:
            bump_mutation_epoch(cells)                         # a restore rewrites the live statistics through raw pointers

    def swap(self):
        """exchange live and averaged VALUES of every kept buffer in one launch (hn_swap_many); eval-mode operands folded from the
        statistics are rebuilt (the owners' mutation cells are bumped).  Twice restores every bit."""
        if self.avg is None:
            raise RuntimeError("BufferKeeper.swap: no averages (ema_decay)")
        _, _, owner, blk, swap_jobs, cells = self._plan()
        lib().call("hn_swap_many", swap_jobs.data_ptr(), owner.data_ptr(), blk)
        bump_mutation_epoch(cells)

    @contextlib.contextmanager
    def averaged(self):
        """`with keeper.averaged():` the buffers hold their averages inside the block and the live values again after it, also when the
        block raises"""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def ema_named(self) -> dict:
        """{name: average tensor} (the keeper's own tensors, not copies); empty without averages"""
        return dict(zip(self.names, self.avg)) if self.avg is not None else {}
