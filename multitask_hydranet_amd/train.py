"""Training-loop surface around the HIP hot path (reference: model/train.py:31-269 HydraTrainer).

Same roles and names as the reference's trainer for the part that touches the hot path: model construction (+ `module.`-prefixed
checkpoint loading and the joint warm start from three single-task checkpoints, train.py:90-126), the data-parallel wrap (train.py:130-137
-> multitask_hydranet_amd.ddp.GradReducer, one process per GPU over RCCL), Adam + per-iteration CosineAnnealingLR (train.py:147-150),
`cal_total_loss` (train.py:192-203), `to_gpu` (train.py:228-239), `train_one_epoch` (train.py:241-269), `valid` (train.py:271-438: losses, streaming mIoU on the device, detection results in COCO json form
from the device post-process, lane decode on the device) and `main`'s head-wise fine-tuning schedule (train.py:441-515: run_training /
tuning_phase / HydraTrainer.set_phase), the lane F1 metric of train.py:188,397,433 (lane_metric.LaneMetric: rasterisation + IoU counts on the
device).  COCOeval (pycocotools) stays outside (out of scope); any iterable of batch dicts with the Collater contract
(dataset/dataloader.py:557-633) drives the loop, or raw batches of dataset.MultitaskData, which to_gpu augments on the device (augment.py).

Launch for N GPUs of one node:  python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 your_script.py
(the trainer reads RANK / LOCAL_RANK / WORLD_SIZE; world size 1 needs no launcher).
"""
from __future__ import annotations

import contextlib
import os
import sys
from typing import Dict, Iterable, Optional

import numpy as np
import torch
import torch.distributed as dist

from .bn_state import BufferKeeper, options as bn_state_options
from .ddp import GradReducer, broadcast_state, capture_exchange_step, unused_parameters
from .metrics import IntersectionOverUnion
from .model import HydraNet
from .optim import Adam, GradAccumulator


PHASES = ("joint", "lane", "det", "seg")


def tuning_phase(epoch: int, epoch_all: int, epoch_tuning: int, tuning_turn: int):
    """main(), train.py:445-505: -> (turn, phase) of `epoch` under the head-wise fine-tuning schedule: every turn is `epoch_joint` joint
    epochs followed by `epoch_tuning` epochs each of lane-only, det-only and seg-only optimisation."""
    assert 3 * epoch_tuning * tuning_turn <= epoch_all
    epoch_joint = int(epoch_all / tuning_turn) - epoch_tuning * 3
    period = epoch_joint + epoch_tuning * 3
    turn, e = int(epoch / period), epoch % period
    if e < epoch_joint:
        return turn, "joint"
    if e < epoch_joint + epoch_tuning:
        return turn, "lane"
    if e < epoch_joint + 2 * epoch_tuning:
        return turn, "det"
    return turn, "seg"


def accum_options(train_cfg: dict, hip_adam: bool) -> int:
    """cfgs["train"]["accum_steps"] -> k, the number of micro-batches per optimizer step (absent: 1 = off).  An int >= 1; the
    accumulated mean is handed to the HIP Adam step (optim.Adam.step(grads=)), so k > 1 needs hip_adam=True."""
    k = train_cfg.get("accum_steps")
    if k is None:
        return 1
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError("train.accum_steps is an integer >= 1, not %r" % (k,))
    if k > 1 and not hip_adam:
        raise ValueError("train.accum_steps > 1 steps the HIP Adam on the accumulated gradients: it needs hip_adam=True")
    return k


def loss_balance_options(train_cfg: dict, hip_adam: bool):
    """cfgs["train"]["loss_balance"] -> None (absent or "none": the static weights alone) or dict(lr, init, clamp) for "uncertainty":
    learned homoscedastic-uncertainty weights.  loss_balance_lr (default train.lr; constant, not under the cosine schedule)
    > 0, loss_balance_clamp (default 6.0) in (0, 80], |loss_balance_init| (default 0.0) <= the clamp.  The log-variances are stepped
    by the HIP Adam, so it needs hip_adam=True.  Anything else raises ValueError."""
    mode = train_cfg.get("loss_balance")
    if mode is None or mode == "none":
        return None
    if mode != "uncertainty":
        raise ValueError("train.loss_balance is 'uncertainty' or 'none', not %r" % (mode,))
    if not hip_adam:
        raise ValueError("train.loss_balance steps the log-variances with the HIP Adam: it needs hip_adam=True")

    def number(key, default):
        v = train_cfg.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float("inf"):
            raise ValueError("train.%s is a finite number, not %r" % (key, v))
        return float(v)
    lr, init, clamp = number("loss_balance_lr", train_cfg["lr"]), number("loss_balance_init", 0.0), number("loss_balance_clamp", 6.0)
    if not lr > 0.0:
        raise ValueError("train.loss_balance_lr is > 0, not %r" % (lr,))
    if not 0.0 < clamp <= 80.0:
        raise ValueError("train.loss_balance_clamp lies in (0, 80], not %r" % (clamp,))
    if abs(init) > clamp:
        raise ValueError("train.loss_balance_init = %r lies outside the clamp +-%r" % (init, clamp))
    return dict(lr=lr, init=init, clamp=clamp)


class _BalanceGrads:
    """Adam.step(grads=) for the log-variances under train.accum_steps: the accumulator's mean of d total / d s (the first half of its
    view for the gradient-and-activity vector)"""

    def __init__(self, acc, key, s):
        self.acc, self.key, self.s, self._ds = acc, key, s, None

    @property
    def pending(self):
        return self.acc.pending

    def grad(self, p):
        if p is not self.s:
            return None
        if self._ds is None:
            self._ds = self.acc.grad(self.key)[:self.s.numel()]       # (one object: Adam's fast path compares gradients by identity)
        return self._ds

    def activity(self):
        return self.acc.grad(self.key)[self.s.numel():]


def optimizer_steps_per_epoch(n_iter: int, k: int) -> int:
    """optimizer steps of an epoch of n_iter loader batches with k micro-batches per step: ceil(n_iter / k) -- a trailing partial group
    is stepped at the epoch's end (HydraTrainer.flush_accumulated)"""
    return (int(n_iter) + int(k) - 1) // int(k)


def run_training(trainer: "HydraTrainer", valid_every_epoch: bool = True, log=print):
    """main(), train.py:441-515: the epoch loop with the fine-tuning schedule of cfgs["train"] (fine_tuning / epoch_tuning / tuning_turn)"""
    t = trainer.cfgs["train"]
    epoch_all = t["epoch"]
    fine = t.get("fine_tuning", False)
    # train.state_file (absent: off): the full training state, written after every train.state_every-th epoch (default 1) and picked up
    # again when the file exists at the start -- the loop then begins at the file's epoch; this wins over train.continue_train's weights
    state_file, first = t.get("state_file"), 0
    state_every = max(1, int(t.get("state_every", 1)))
    if state_file and os.path.isfile(state_file):
        first = int(trainer.load_state(state_file)["epoch"])
        log("======= RESUMED %s: EPOCH %i =======" % (state_file, first))
    try:
        for epoch in range(first, epoch_all):
            if fine:
                turn, phase = tuning_phase(epoch, epoch_all, t["epoch_tuning"], t["tuning_turn"])
                log("======= TURN %i %s TRAINING =======" % (turn, phase.upper()))
                trainer.set_phase(phase)
            trainer.train_one_epoch(epoch)
            if state_file and (epoch + 1) % state_every == 0:
                trainer.save_state(state_file, wait=False, epoch=epoch + 1)       # (the file is written while validation / the next epoch runs)
            if valid_every_epoch and trainer.validloader is not None:
                log("=========================== VALIDATION %i ===========================" % epoch)
                trainer.valid(epoch)
    finally:
        if state_file:
            trainer.checkpoint_wait()
    log("============== finish training ==============")


from .ops.xstage import xstage_assert_ok as K_xstage_assert_ok, xstage_status_word as K_xstage_status_word


class HydraTrainer:
    def __init__(self, cfgs: dict, trainloader: Optional[Iterable] = None, validloader: Optional[Iterable] = None, iters_per_epoch: Optional[int] = None,
                 grad_payload: torch.dtype = torch.float32, capture_step: bool = False, hip_adam: bool = True, force_distribute: bool = False):
        """capture_step: after two eager iterations the forward + loss + backward of an iteration is captured as ONE hipGraph and replayed
        on static input buffers (875 vs ~500 img/s on the bench workload: ~1200 launches per step are host-bound when issued one by one);
        Adam / LR steps stay eager.  Needs batches of one fixed shape; a different shape re-captures.  With more than one rank the
        gradient exchange is part of the captured step (RCCL: every bucket's gather + all-reduce captured in line where its last gradient
        appears, ddp.capture_exchange_step -- the form bench.py times; other backends, whose collectives cannot be captured: the graph holds
        forward + loss + backward and the buckets are exchanged right after each replay).
        force_distribute: run the data-parallel machinery (process group, bucketed all-reduce, in-graph exchange) at world size 1 too --
        the N > 1 code path on a single GPU (tests; the average over one rank is the identity).
        cfgs["train"]["grad_clip_norm"] / ["skip_nonfinite"] (optional, hip_adam only): global-norm clipping and a non-finite step guard,
        decided on the device inside the Adam step (optim.Adam).  With skip_nonfinite the reference's host-side divergence guard
        (HydraNet.check_finite) is off: a bad batch is skipped, and train_one_epoch ends the run only when a whole print interval was.
        cfgs["train"]["ema_decay"] (absent or <= 0: off) / ["ema_warmup"] (default True), hip_adam only: an exponential moving average of
        the weights, kept inside the Adam launch (optim.Adam); valid() then scores the averaged weights and save(path, ema=True)
        writes them.  Every rank holds the same parameters after the gradient exchange and therefore the same average: nothing is
        communicated for it.
        cfgs["train"]["protect_bn_stats"] (needs grad_clip_norm or skip_nonfinite) / ["ema_buffers"] (needs ema_decay), hip_adam only
        (bn_state.BufferKeeper): the BatchNorm running statistics and batch counters are snapshotted before every forward
        and restored on the device when the guard skips the step; and they are averaged next to the weights with the same decay
        schedule, exchanged with them in valid() and written by save(path, ema=True).  Two small launches per step around the (eager or
        replayed) step; with both keys absent none is issued and `buffer_keeper` stays None.  Every rank keeps its own statistics, as
        without the keys: nothing is communicated.
        cfgs["train"]["accum_steps"] = k (absent or 1: off; hip_adam only; optim.GradAccumulator): train_step still takes one
        loader batch -- a micro-batch -- per call; the optimizer step, the LR step, the weight average's update and the BufferKeeper's
        settle happen once per group of k micro-batches, on the MEAN of the group's gradients (one hn_grad_accum launch per micro-batch
        keeps it; train_step returns the group's loss means so far).  train_one_epoch steps a trailing partial group at the epoch's end
        (flush_accumulated); total_iters counts optimizer steps, so the cosine schedule ends where training ends.  Every micro-batch of
        a group weighs the same whatever its size (a short last batch included); the detection and lane losses normalise by per-batch
        positive counts, so k micro-batches of B images are not bit for bit one batch of k * B; BatchNorm statistics are per
        micro-batch (and are snapshotted once per group: a skipped group restores what they were before its first micro-batch).
        Data parallel: nothing in the reducer changes -- every micro-batch's backward is a complete exchange and the accumulator reads
        the exchanged gradients (the mean of the averages is the average of the means), which is k times the traffic of exchanging
        once per group; that form is not built.
        cfgs["train"]["loss_balance"] = "uncertainty" (absent or "none": off; hip_adam only) / ["loss_balance_lr"] /
        ["loss_balance_init"] / ["loss_balance_clamp"]: one learned log-variance per loss term weighs the six terms next to the static
        weights (HydraNet.enable_loss_balance; hn_balanced_sum in place of hn_weighted_sum).  The six scalars are one plain device
        tensor, stepped by a second, one-tensor HIP Adam (`balance_optimizer`: no weight decay, a constant learning rate of its own)
        right after the weights' step and under the same decision: a step the guard skips leaves them and their moments untouched,
        under accum_steps they step once per group on the mean of the group's gradients; they take no part in the clipping norm or the
        weight average.  A term whose loss was exactly 0 in the step (a task without a labelled image, a head-only phase's other
        terms) keeps its log-variance and both moments to the bit."""
        self.cfgs = cfgs
        self.capture_step = capture_step
        self._cap = None                       # (shape key, graph, static batch, static loss dict)
        self._eager_iters = 0
        self._lane_coder = None                # LaneCodec of the cfg's geometry, built when a batch needs its lane targets encoded
        self._stream = None                    # data-parallel captured steps: ONE stream for the eager iterations and the capture (ddp.py)
        t = cfgs["train"]
        self.train_detect, self.train_seg, self.train_lane = t["train_detect"], t["train_seg"], t["train_lane"]
        self.print_interval = t.get("print_interval", 10)
        # train.grad_clip_norm (absent or <= 0: off) / train.skip_nonfinite: decided on the device inside the HIP Adam step (optim.py)
        clip = t.get("grad_clip_norm")
        self.grad_clip_norm = float(clip) if clip is not None and float(clip) > 0 else None
        self.skip_nonfinite = bool(t.get("skip_nonfinite", False))
        if (self.grad_clip_norm is not None or self.skip_nonfinite) and not hip_adam:
            raise ValueError("train.grad_clip_norm / train.skip_nonfinite are applied inside the HIP Adam step: they need hip_adam=True")
        ema = t.get("ema_decay")
        self.ema_decay = float(ema) if ema is not None and float(ema) > 0 else None
        self.ema_warmup = bool(t.get("ema_warmup", True))
        if self.ema_decay is not None and not hip_adam:
            raise ValueError("train.ema_decay is kept inside the HIP Adam step: it needs hip_adam=True")
        self.protect_bn_stats, self.ema_buffers = bn_state_options(t, hip_adam)
        self.buffer_keeper = None              # bn_state.BufferKeeper, built at the first training step when either key is on
        self.accum_steps = accum_options(t, hip_adam)
        self.loss_balance = loss_balance_options(t, hip_adam)      # None, or dict(lr, init, clamp) of train.loss_balance: uncertainty
        self.balance_optimizer = None          # the log-variances' own optim.Adam
        self.accumulator = None                # optim.GradAccumulator when train.accum_steps > 1
        self._packer = None                    # checkpoint.StatePacker of save_state / load_state, rebuilt when the set of state tensors changes
        self._ckpt_thread = None               # the background writer of save_state(wait=False)
        self._ckpt_error = None
        self.next_epoch = 0                    # the epoch a state file written now would resume at (run_training / load_state set it)
        self.trainloader, self.validloader = trainloader, validloader
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(self.device)
        self._force_distribute = bool(force_distribute)
        if (self.world > 1 or force_distribute) and not dist.is_initialized():
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            if self.world == 1:
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                if "MASTER_PORT" not in os.environ:          # a free port: a constant collides with a second trainer / a socket in TIME_WAIT
                    import socket
                    with socket.socket() as sk:
                        sk.bind(("127.0.0.1", 0))
                        os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=self.device)

        self.hydranet = HydraNet(cfgs=cfgs).to(self.device)
        # train.py:90-126; files written from a DDP wrapper carry "module." prefixes (deparallel_model): load_state_dict strips them
        flag_joint = self.train_detect and self.train_seg and self.train_lane and t.get("weight_file", "") == ""
        if t.get("continue_train") and flag_joint:
            # the joint warm start: the three single-task checkpoints in turn, non-strict, each overriding the shared backbone and neck
            for key in ("weight_file_lane", "weight_file_seg", "weight_file_det"):
                path = t.get(key)
                if not path:
                    raise ValueError("train.continue_train with all three heads and weight_file \"\" loads train.%s, which is not set" % key)
                if not os.path.isfile(path):
                    raise FileNotFoundError("train.%s: no such checkpoint: %s" % (key, path))
                self.hydranet.load_state_dict(torch.load(path, map_location=self.device), strict=False)
        elif t.get("continue_train") and t.get("weight_file"):
            self.hydranet.load_state_dict(torch.load(t["weight_file"], map_location=self.device))
        broadcast_state(self.hydranet)                               # what DDP does at construction (train.py:137)
        self.use_distribute = self.world > 1 or self._force_distribute
        self.reducer = None
        self.phase = "joint"
        self._grad_payload = grad_payload
        self._reducers = {}                                          # one bucket plan per fine-tuning phase (the set of live gradients differs)
        if self.use_distribute:
            self.reducer = self._reducers["joint"] = self._make_reducer("joint")
            if capture_step:
                self._stream = torch.cuda.Stream(device=self.device)

        self.lr, self.weight_decay, self.epoch = t["lr"], t["weight_decay"], t["epoch"]
        n_iter = iters_per_epoch if iters_per_epoch is not None else (len(trainloader) if hasattr(trainloader, "__len__") else 1)
        self.total_iters = max(1, optimizer_steps_per_epoch(n_iter, self.accum_steps) * self.epoch)
        # torch.optim.Adam's update rule and state layout (train.py:147); hip_adam: all 693 tensors in one launch (optim.py) instead of the
        # foreach implementation's ~10 multi-tensor launches (3.9 -> 0.4 ms per step)
        if hip_adam:
            self.optimizer = Adam(self.hydranet.parameters(), self.lr, weight_decay=self.weight_decay, max_grad_norm=self.grad_clip_norm,
                                  skip_nonfinite=self.skip_nonfinite, **({} if self.ema_decay is None else
                                                                         dict(ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)))
        else:
            self.optimizer = torch.optim.Adam(self.hydranet.parameters(), self.lr, weight_decay=self.weight_decay)
        self._guarded = self.grad_clip_norm is not None or self.skip_nonfinite
        extra = []
        if self.loss_balance is not None:
            extra = [self._enable_loss_balance()]
        if self.accum_steps > 1:
            self.accumulator = GradAccumulator(list(self.hydranet.parameters()) + extra)
            if extra:
                self._balance_grads = _BalanceGrads(self.accumulator, extra[0], self.hydranet.loss_log_vars)
        if self.skip_nonfinite:
            # the device guard replaces the reference's host guard (HydraNet._guard: seven synchronising reads of device scalars per step,
            # sys.exit() on the first bad batch): a non-finite step is skipped, and only a whole print interval of them ends the run
            self.hydranet.check_finite = False
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, self.total_iters, eta_min=1e-8)     # iteration based

        self._one = torch.ones((), device=self.device)            # root gradient, allocated once
        s, d, l = cfgs["segment"], cfgs["detection"], cfgs["lane"]
        self.segment_weight = s["segment_weight"]
        self.loss_cls_weight, self.loss_reg_weight, self.detection_weight = d["loss_cls_weight"], d["loss_reg_weight"], d["detection_weight"]
        self.loss_cls_pos_weight, self.loss_cls_neg_weight = l["loss_cls_pos_weight"], l["loss_cls_neg_weight"]
        self.loss_loc_weight, self.lane_weight = l["loss_loc_weight"], l["lane_weight"]
        if self.train_seg:
            self.metric_evaluator_iou = IntersectionOverUnion(n_classes=len(s["class_list"]), device=self.device)

    # ------------------------------------------------------------------------------------------------------------------------------
    def _phase_module(self, phase):
        return {"joint": self.hydranet, "lane": self.hydranet.laneheader, "det": self.hydranet.detectheader, "seg": self.hydranet.segheader}[phase]

    def _make_reducer(self, phase):
        if phase == "joint":
            named = list(self.hydranet.named_parameters())
        else:
            prefix = {"lane": "laneheader.", "det": "detectheader.", "seg": "segheader."}[phase]
            named = [(n, p) for n, p in self.hydranet.named_parameters() if n.startswith(prefix)]
        red = GradReducer(named, world_size=self.world, skip=unused_parameters(self.hydranet), payload_dtype=self._grad_payload,
                          force_collectives=self._force_distribute)
        if getattr(self, "balance_optimizer", None) is not None:
            red.extras.append(self.hydranet.loss_balance_grad_act)      # d total / d s and the activity: the ranks' mean, so they cannot drift
        return red

    def set_phase(self, phase: str):
        """One branch of main()'s schedule (train.py:462-505): the optimizer's first param group holds the parameters of the whole model
        ("joint") or of ONE head; Adam's per-parameter state is kept across phases, exactly as swapping `param_groups[0]['params']` does.
        In a head-only phase only that head's parameters can change, so the HIP path does not run the backward of the backbone, the neck
        and the other two heads at all (HydraNet.grad_scope: those parts run forward under no_grad -- BatchNorm running statistics still
        update, all six losses are still reported); the reference computes those gradients and throws them away."""
        assert phase in PHASES
        if self._phase_module(phase) is None:
            raise ValueError("phase %r needs the %s head (cfgs['train'])" % (phase, phase))
        if self.accumulator is not None and self.accumulator.pending:
            raise RuntimeError("set_phase with %i accumulated micro-batch(es) pending: call flush_accumulated() first" % self.accumulator.pending)
        self.optimizer.param_groups[0]["params"] = list(self._phase_module(phase).parameters())
        if phase != self.phase:
            self.hydranet.zero_grad(set_to_none=True)               # gradients of parameters leaving the group must not linger (or feed Adam later)
            self._cap = None                                         # a captured step belongs to one phase
            self._eager_iters = 0
            if self.accumulator is not None:
                self.accumulator.invalidate()                        # another set of gradients: a fresh job table
            if self.use_distribute:
                self.reducer.remove()
                if phase not in self._reducers:
                    self._reducers[phase] = self._make_reducer(phase)
                else:
                    self._reducers[phase].arm()
                self.reducer = self._reducers[phase]
        self.phase = phase
        self.hydranet.grad_scope = None if phase == "joint" else phase

    def _enable_loss_balance(self):
        """train.loss_balance: the model's log-variances, their one-tensor Adam with its state (allocated now: a state file lists the
        same tensors before and after the first step) and the hold buffer of _balance_step -> the tensor that stands for the
        gradient-and-activity vector in a GradAccumulator (its .grad is that vector; its own values are never read)"""
        b, net = self.loss_balance, self.hydranet
        net.enable_loss_balance(b["clamp"], b["init"])
        s = net.loss_log_vars
        s._hn_mut_cell = [0]                   # (a cell of its own: stepping it leaves every eval-mode cache of the weights alone)
        s.grad = net.loss_log_vars_grad        # written by every backward of total_loss: never accumulated into, never zeroed
        opt = self.balance_optimizer = Adam([s], b["lr"], weight_decay=0.0, skip_nonfinite=self.skip_nonfinite)
        opt.state[s] = dict(step=torch.zeros((), dtype=torch.float32), exp_avg=torch.zeros_like(s), exp_avg_sq=torch.zeros_like(s))
        self._balance_hold = torch.zeros((3 * s.numel(),), device=self.device, dtype=torch.float32)
        self._balance_grads = None
        for red in self._reducers.values():
            red.extras.append(net.loss_balance_grad_act)
        key = torch.zeros_like(net.loss_balance_grad_act)
        key.grad = net.loss_balance_grad_act
        return key

    def _balance_step(self, accumulated: bool = False):
        """the log-variances' Adam step, right after the weights': the guard's skip word of the weights' step decides for it too
        (train.skip_nonfinite), and hn_balance_hold around it gives every slot without an active term in this step (or group) its
        value and moments back.  Three small launches (and the guard's three with train.skip_nonfinite); none without train.loss_balance."""
        opt = self.balance_optimizer
        if opt is None:
            return
        from ._lib import lib
        net = self.hydranet
        s = net.loss_log_vars
        st, n = opt.state[s], s.numel()
        tensors = (s.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), self._balance_hold.data_ptr())
        lib().call("hn_balance_hold", *tensors, None, n)
        kw = dict(guard_words=[self.optimizer.guard_record[2:3]]) if self.skip_nonfinite else {}
        if accumulated:
            opt.step(grads=self._balance_grads, **kw)
            act = self._balance_grads.activity()
        else:
            opt.step(**kw)
            act = net.loss_balance_grad_act[n:]
        lib().call("hn_balance_hold", *tensors, act.data_ptr(), n)

    def _optimizer_step(self, total_loss: torch.Tensor):
        """Adam step; with train.skip_nonfinite the guard also sees the total loss and the persistent stage kernels' status word (a replayed
        step whose persistent launch expired must not reach Adam).  With more than one rank only the exchanged gradients are identical
        everywhere, so only they may decide: every rank then takes the same decision without exchanging it."""
        if self.skip_nonfinite and self.world == 1:
            self.optimizer.step(losses=[total_loss.detach()], guard_words=[K_xstage_status_word(self.device)])
        else:
            self.optimizer.step()

    def _finish_step(self, loss_dict: Dict[str, torch.Tensor], keeper, out: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """what follows a forward + backward (eager or replayed, gradients exchanged).  Without train.accum_steps: Adam step, the
        keeper's settle, LR step, and `out` is returned.  With it: the gradients, the losses and the persistent stage kernels' status
        word are folded into the accumulator (one launch), and the k-th micro-batch of a group steps on the means; the losses returned
        are the group's means so far.  loss_dict: tensors that are valid now (a replayed graph's static ones serve)."""
        acc = self.accumulator
        if acc is None:
            self._optimizer_step(loss_dict["total_loss"])
            self._balance_step()
            if keeper is not None:
                keeper.settle(self.optimizer.guard_record)          # a skipped step: the statistics back; a taken one: their average
            self.scheduler.step()
            return out
        names = [k for k in loss_dict if k != "total_loss"] + ["total_loss"]       # (the total last: _accumulated_step hands it to the guard)
        acc.add(losses=[loss_dict[k].detach() for k in names], guard_words=[K_xstage_status_word(self.device)])
        means = acc.loss_means().clone()                             # (the accumulator's own are rewritten by the next micro-batch)
        if acc.pending >= self.accum_steps:
            self._accumulated_step()
        by_name = {k: means[i] for i, k in enumerate(names)}
        return {k: by_name[k] for k in loss_dict}

    def _accumulated_step(self):
        """the optimizer step of a group, on the accumulator's means; the guard sees the group's mean total loss and its sticky word
        where _optimizer_step hands it the loss and the status word (train.skip_nonfinite at world size 1)"""
        acc = self.accumulator
        if self.skip_nonfinite and self.world == 1:
            self.optimizer.step(grads=acc, losses=[acc.loss_means()[-1:]], guard_words=[K_xstage_status_word(self.device), acc.sticky_word])
        else:
            self.optimizer.step(grads=acc)
        self._balance_step(accumulated=True)
        if self.buffer_keeper is not None:
            self.buffer_keeper.settle(self.optimizer.guard_record)
        self.scheduler.step()
        acc.reset()

    def flush_accumulated(self):
        """step with the micro-batches accumulated so far (a group cut short: the accumulator holds their mean already); a no-op with
        none pending or without train.accum_steps.  train_one_epoch calls it after its loop, so that a trailing partial group is not
        carried into the next epoch or phase."""
        if self.accumulator is None or self.accumulator.pending == 0:
            return
        if self._stream is None:
            return self._accumulated_step()
        cur = torch.cuda.current_stream()
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            self._accumulated_step()
        cur.wait_stream(self._stream)

    def _keeper(self):
        """the BufferKeeper of train.protect_bn_stats / train.ema_buffers (None with both off), built at the first training step: the
        model is on its device by then, and a load_state_dict() since construction is what the shadows and averages start from"""
        if self.buffer_keeper is None and (self.protect_bn_stats or self.ema_buffers):
            self.buffer_keeper = BufferKeeper(self.hydranet.named_buffers(), self.protect_bn_stats,
                                              ema_decay=self.ema_decay if self.ema_buffers else None, ema_warmup=self.ema_warmup)
        return self.buffer_keeper

    def cal_total_loss(self, loss_dict: Dict[str, torch.Tensor]):
        """train.py:192-203: the weighted sum of the task losses (same weights, same association order); on the device it is one launch
        (HydraNet.total_loss -> ops.WeightedLossSum)"""
        return self.hydranet.total_loss(loss_dict)

    def to_gpu(self, batch_data: dict) -> dict:
        """train.py:228-239.  A raw batch (dataset.MultitaskData: `src_frames` + `aug_plans`, no `image`) is first assembled and augmented on
        the device (augment.augment_batch) into the Collater contract; lane targets are then encoded from its annot_lane as for any batch
        without gt_loc / gt_cls.  A batch of MultitaskData(decode="device") carries `src_coefs` (entropy-decoded JPEG coefficients) instead
        of `src_frames`, one of decode="device-entropy" `src_streams` (the files' bytes): jpeg.decode_batch finishes the decode on the device
        into the same packed frames first.  A batch of MultitaskData(decode_labels="device") carries `src_seg_streams` (the label PNGs'
        zlib streams) instead of `src_segs`: png.decode_batch inflates and unfilters them on the device into the packed label maps."""
        if "image" not in batch_data and ("src_frames" in batch_data or "src_coefs" in batch_data or "src_streams" in batch_data):
            batch_data = self._augment(batch_data)
        batch_data["image"] = batch_data["image"].to(self.device).float()
        if self.train_lane:
            if batch_data.get("gt_loc") is None or batch_data.get("gt_cls") is None:
                batch_data["gt_cls"], batch_data["gt_loc"] = self._encode_lane_targets(batch_data)
            batch_data["gt_loc"] = batch_data["gt_loc"].to(self.device).float()
            batch_data["gt_cls"] = batch_data["gt_cls"].to(self.device).float()
        if self.train_seg:
            batch_data["gt_seg"] = batch_data["gt_seg"].to(self.device).float()
        if self.train_detect:
            batch_data["gt_det"] = batch_data["gt_det"].to(self.device).float()
        tv = batch_data.get("task_valid")
        if tv is not None and "task_valid_host" not in batch_data and not (isinstance(tv, torch.Tensor) and tv.is_cuda):
            # per-image task masks (dataloader.allow_missing_labels): the device copy feeds the losses (and rides into a captured
            # step's static set like every device tensor of the batch); the host copy indexes valid()'s metrics without a synchronisation.
            # (A mask that arrives on the device already is used as it is: copying it back would synchronise, so valid() then scores
            # every image.)
            host = torch.as_tensor(tv).to(torch.uint8).contiguous()
            batch_data["task_valid_host"] = host
            batch_data["task_valid"] = host.to(self.device, non_blocking=True)
        return batch_data

    def _augment(self, batch_data: dict) -> dict:
        from .augment import augment_batch
        dl = self.cfgs["dataloader"]
        if "src_coefs" in batch_data or "src_streams" in batch_data:
            from .jpeg import decode_batch
            frames = decode_batch(batch_data.get("src_coefs", batch_data.get("src_streams")), device=self.device)
        else:
            frames = batch_data["src_frames"]
        segs = batch_data.get("src_segs") if self.train_seg else None
        if self.train_seg and "src_seg_streams" in batch_data:
            from .png import decode_batch as decode_labels
            segs = decode_labels(batch_data["src_seg_streams"], device=self.device)
        out = augment_batch(frames, batch_data.get("lane_raw") if self.train_lane else None,
                            batch_data.get("det_raw") if self.train_detect else None, segs,
                            batch_data["aug_plans"], (dl["network_input_height"], dl["network_input_width"]), device=self.device)
        rest = {k: v for k, v in batch_data.items() if k not in ("src_frames", "src_coefs", "src_streams", "src_segs", "src_seg_streams", "lane_raw", "det_raw", "aug_plans")}
        rest.update(out)
        return rest

    def _encode_lane_targets(self, batch_data: dict):
        """lane targets of a batch without gt_loc / gt_cls, encoded on the device from the raw annotations the reference's Collater hands
        over (annot_lane: JSON per image, src_image_shape: source width / height per image; dataloader.py:343-352,367-377,620-625) with the
        cfg's geometry (points_per_line = input height // lane.interval, dataloader.py:202).  No host synchronisation."""
        if "annot_lane" not in batch_data or "src_image_shape" not in batch_data:
            raise KeyError("train_lane: the batch carries neither gt_loc / gt_cls nor annot_lane + src_image_shape to encode them from")
        if self._lane_coder is None:
            from .lane_codec import LaneCodec
            dl, ln = self.cfgs["dataloader"], self.cfgs["lane"]
            if ln["anchor_lane_num"] != 1:
                raise ValueError("lane.anchor_lane_num = %r: lane targets are encoded for anchor_lane_num == 1 only" % (ln["anchor_lane_num"],))
            W, H = dl["network_input_width"], dl["network_input_height"]
            self._lane_coder = LaneCodec(input_width=W, input_height=H, anchor_stride=ln["anchor_stride"],
                                         points_per_line=int(H / ln["interval"]), do_interpolate=ln["interpolate"],
                                         anchor_lane_num=ln["anchor_lane_num"], scale_invariance=ln["scale_invariance"])
        return self._lane_coder.encode_lanes(list(batch_data["annot_lane"]), list(batch_data["src_image_shape"]), device=self.device,
                                             div_interval=self.cfgs["lane"]["interval"])

    @staticmethod
    def _batch_sig(batch_data: dict):
        return tuple((k, tuple(v.shape), v.dtype) for k, v in batch_data.items() if isinstance(v, torch.Tensor) and v.is_cuda)

    def _captured_fwd_bwd(self, batch_data: dict, clone: bool = True) -> Dict[str, torch.Tensor]:
        """forward + loss + backward (+ the gradient exchange) as one hipGraph replay (built on first use for this batch shape) -> the
        losses, as clones of the graph's static tensors, or with clone=False those tensors themselves (valid until the next replay)"""
        keys = [k for k, v in batch_data.items() if isinstance(v, torch.Tensor) and v.is_cuda]
        sig = self._batch_sig(batch_data)
        if self._cap is None or self._cap[0] != sig:
            static = {k: batch_data[k].clone() for k in keys}
            net = self.hydranet
            guard, net.check_finite = net.check_finite, False        # the divergence guard reads the loss on the host: after the replay

            def fwd_bwd():
                outputs = net(static["image"])
                loss_dict = net.cal_loss(outputs, static)
                loss_dict["total_loss"] = self.cal_total_loss(loss_dict)
                loss_dict["total_loss"].backward(self._one)
                return loss_dict
            # parameter gradients become tensors of the graph's pool (stored by the captured backward, rewritten by every replay)
            zero = lambda: self.optimizer.zero_grad(set_to_none=True)
            try:
                red = self.reducer
                in_graph = red is not None and red.active and red.on_gpu and dist.get_backend(red.group) == "nccl"
                if in_graph:
                    # (no extra warm-up: the two eager iterations ran on self._stream with the hooks armed)
                    graph, loss_dict = capture_exchange_step(red, fwd_bwd, zero, self._stream, warmup=0)
                else:
                    if red is not None:
                        red.remove()                                 # no hooks inside this capture: the exchange follows every replay
                    zero()
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    # thread-local capture mode: helper threads (the autograd engine's allocator calls, an RCCL watchdog) must not invalidate it
                    with torch.cuda.graph(graph, capture_error_mode="thread_local", **({"stream": self._stream} if self._stream is not None else {})):
                        loss_dict = fwd_bwd()
                    if red is not None:
                        red.bind_static_grads()                      # reduce_now() gathers what each replay leaves in these tensors
            finally:
                net.check_finite = guard
            self._cap = (sig, graph, static, loss_dict, in_graph)
        _, graph, static, loss_dict, in_graph = self._cap
        for k in static:
            static[k].copy_(batch_data[k])
        graph.replay()
        if self.reducer is not None and not in_graph:
            self.reducer.reduce_now()
        if self.hydranet.check_finite:
            masked = "task_valid" in static             # (a task without a labelled image in the batch has loss 0: no divergence)
            for name, v in loss_dict.items():
                self.hydranet._guard(v, "cal %s diverge!" % name, allow_zero=masked or name.startswith("loss_det"))
        if not clone:
            return loss_dict
        return {k: v.detach().clone() for k, v in loss_dict.items()}      # the static tensors are rewritten by the next replay

    def train_step(self, batch_data: dict) -> Dict[str, torch.Tensor]:
        """one iteration of train.py:243-267: forward, multitask loss, backward (gradient exchange overlapped), Adam step, LR step"""
        if self._stream is None:
            return self._train_step(batch_data)
        # data-parallel + capture_step: every iteration (eager or replayed) runs on the trainer's own stream, the one the capture uses
        cur = torch.cuda.current_stream()
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            out = self._train_step(batch_data)
        cur.wait_stream(self._stream)
        return out

    def _train_step(self, batch_data: dict) -> Dict[str, torch.Tensor]:
        batch_data = self.to_gpu(batch_data)
        keeper = self._keeper()
        if keeper is not None and (self.accumulator is None or self.accumulator.pending == 0):
            keeper.snapshot()                  # eager, before the forward (or the replay) that writes the running statistics
        if self.capture_step and self._eager_iters >= 2 and self._cap is not None and self._cap[0] != self._batch_sig(batch_data):
            # A different batch shape than the captured one (the loaders' short last batch: drop_last=False, model/train.py:71,81).  The step is
            # NOT captured again on the spot (with the exchange in the graph that would be a second capture of RCCL collectives with no
            # warm-up at the new shape): this iteration and the next run on the eager path (hooks armed), the one after that
            # captures at the shape it sees.
            self._eager_iters = 0
        if self.capture_step and self._eager_iters >= 2:
            # (accumulating: the means are formed from the replayed graph's static tensors, no per-loss clones)
            loss_dict = self._captured_fwd_bwd(batch_data, clone=self.accumulator is None)
            return self._finish_step(self._cap[3], keeper, loss_dict)      # (the guard reads the replayed graph's static total loss)
        self._eager_iters += 1
        if self._cap is not None:              # back on the eager path after captured steps: gradients must not stay in the graph's pool
            self.optimizer.zero_grad(set_to_none=True)
            self._cap = None
        if self.reducer is not None:
            self.reducer.arm()                 # (a captured step removed the hooks; no-op while they are registered)
        outputs = self.hydranet(batch_data["image"])
        loss_dict = self.hydranet.cal_loss(outputs, batch_data)
        loss_total = self.cal_total_loss(loss_dict)
        loss_dict.update({"total_loss": loss_total})
        # gradients accumulate straight into the exchange buckets after the first step: zero them in place instead of dropping them
        self.optimizer.zero_grad(set_to_none=self.reducer is None)
        loss_total.backward(self._one)
        if self.reducer is not None:
            self.reducer.finish()
        # detached: the losses are for logging; a caller that keeps them must not keep this iteration's autograd nodes alive (stale
        # AccumulateGrad nodes bound to another stream break a later capture)
        loss_dict = {k: v.detach() for k, v in loss_dict.items()}
        return self._finish_step(loss_dict, keeper, loss_dict)

    def train_one_epoch(self, epoch: int):
        self.hydranet.train()
        for iter_idx, batch_data in enumerate(self.trainloader):
            loss_dict = self.train_step(batch_data)
            if iter_idx % self.print_interval == 0:
                if self.device.type == "cuda":
                    K_xstage_assert_ok(self.device)          # (a replayed step cannot check its persistent launches itself: ops/xstage.py)
                guard = self.optimizer.grad_guard_record() if self._guarded else None
                if self.rank == 0:
                    self.print_loss_info(loss_dict, epoch, iter_idx, guard=guard)
                # (the record counts optimizer steps, one per group under train.accum_steps: the run ends after print_interval consecutive
                # skipped STEPS, that is print_interval * accum_steps micro-batches -- one skipped group never ends it)
                if guard is not None and guard["skipped_consecutive"] >= self.print_interval:
                    print("training diverged")                   # every step since the last print was skipped
                    sys.exit()
        self.flush_accumulated()

    def print_loss_info(self, loss_dict, epoch, batch_idx, mode="train", guard=None):
        lr = self.optimizer.param_groups[0]["lr"]
        print("%s Epoch [%i|%i] Iter [%i] Lr %.5f  " % (mode.upper(), epoch, self.epoch, batch_idx, lr) +
              "  ".join("%s %.3f" % (k, float(v.detach())) for k, v in loss_dict.items()) +
              ("" if guard is None else "  grad_norm %.3f  coef %.3f  skipped %i" % (guard["norm"], guard["coef"], guard["skipped"])))
        if mode == "train" and self.balance_optimizer is not None:
            print(self.loss_balance_line())

    def loss_balance_line(self) -> str:
        """the print interval's line under train.loss_balance: per term its log-variance s, exp(-s) and exp(-s) x its static weights
        (term weight x group weight).  One read of the model's record, after the reads the loss line has just made."""
        c = self.cfgs
        static = dict(loss_seg=c["segment"]["segment_weight"],
                      loss_det_cls=c["detection"]["loss_cls_weight"] * c["detection"]["detection_weight"],
                      loss_det_reg=c["detection"]["loss_reg_weight"] * c["detection"]["detection_weight"],
                      loss_lane_cls_pos=c["lane"]["loss_cls_pos_weight"] * c["lane"]["lane_weight"],
                      loss_lane_cls_neg=c["lane"]["loss_cls_neg_weight"] * c["lane"]["lane_weight"],
                      loss_lane_loc=c["lane"]["loss_loc_weight"] * c["lane"]["lane_weight"])
        return "      balance (s, exp(-s), x static)  " + "  ".join(
            "%s %.3f %.3f %.4g%s" % (k[5:], s, e, e * static[k], "" if on else " (inactive)") for k, (s, e, on) in self.hydranet.loss_balance.items())

    def valid(self, epoch: int = 0, eval_dir: Optional[str] = None, lane_coder=None, det_conf_thres: float = 0.3, det_iou_thres: float = 0.3,
              coco_gt=None, use_ema: Optional[bool] = None):
        """_valid() (below) on the live weights or, with use_ema (None: on when train.ema_decay is on and a step has been taken), on the averaged ones: the whole
        validation loop then runs inside optimizer.averaged(), which exchanges the VALUES of live and averaged parameters in one launch
        and exchanges them back when the loop ends or raises -- parameter addresses never change, so a captured training step replays
        correctly afterwards.  BatchNorm running statistics are the live ones either way, unless train.ema_buffers is on: then the loop
        also runs inside buffer_keeper.averaged(), with the averaged statistics and counters.  With train.ema_decay on, last_valid["ema"]
        says which weights were scored."""
        if use_ema is None:                     # (before the first optimizer step there is no average yet: the live weights)
            use_ema = self.ema_decay is not None and bool(self.optimizer.ema_named(self.hydranet.named_parameters()))
        if use_ema and self.ema_decay is None:
            raise ValueError("valid(use_ema=True) needs train.ema_decay")
        buffers = self.buffer_keeper if use_ema and self.ema_buffers else None
        with (self.optimizer.averaged() if use_ema else contextlib.nullcontext()), \
                (buffers.averaged() if buffers is not None else contextlib.nullcontext()):
            scores = self._valid(epoch, eval_dir, lane_coder, det_conf_thres, det_iou_thres, coco_gt)
        if self.ema_decay is not None:           # (without the option last_valid keeps exactly its keys)
            self.last_valid["ema"] = use_ema
        return scores

    @torch.no_grad()
    def _valid(self, epoch: int = 0, eval_dir: Optional[str] = None, lane_coder=None, det_conf_thres: float = 0.3, det_iou_thres: float = 0.3,
               coco_gt=None):
        """train.py:271-438 without the third-party evaluators: eval-mode forward + the six losses per batch, streaming mIoU on the device
        (train.py:293-306), detection results through the device post-process in COCO-json form (train.py:308-364; written to
        `eval_dir`/val_bbox_results.json like train.py:416-421 -- the file COCOeval reads), lane decode + NMS on the device and the
        prediction json of LaneHeader.scale_to_org (train.py:366-395) when a `lane_coder` (LaneCodec) is given, and -- when the batches carry
        the ground-truth lanes of train.py:393 as `gt_lane_json` (one {"Lines": [...], "Labels": [...]} dict per image) -- the lane F1 of
        train.py:188,397,433 (LaneMetric, f1_measure, IoU 0.5, width 30, score threshold 0.5).  With `coco_gt` (the GT dataset dict of
        coco_json.coco_ground_truth or a path to gt_bbox_results.json) and detection trained, the COCO bbox mAP of train.py:416-426 on the
        device (det_eval.CocoBoxEvaluator over the GT's first detection.max_images images, every batch's boxes as the json records them):
        last_valid["det_eval"] = its compute() (dict(stats, precision, recall), None without any detection) and rank 0 prints the
        "metric detection" block.  At world size > 1 only rank 0's images are evaluated, as only rank 0's records are written (no gather).
        Deliberate deviation: train.py:397 calls `self.lane_metric(output=lane_result)` inside the batch loop with the CUMULATIVE list, so the
        reference counts image k of a validation run (number of batches - batch index of k) times, and never resets the evaluator between
        epochs; here every image is scored exactly once per valid() call (for a single-batch validation the two agree).
        Returns the per-class IoU tensor; everything else is left in self.last_valid."""
        from .coco_json import detections_to_coco, write_results
        from .lane_metric import LaneMetric
        # train.py:188.  batched: every batch's lanes are rasterised and counted on the device while the next batch's forward runs; one
        # synchronisation, in summary()
        lane_metric = LaneMetric(method="f1_measure", iou_thresh=0.5, lane_width=30, thresh_list=[0.5], batched=True, device=self.device)
        lane_pairs = 0
        net = self.hydranet
        net.eval()
        if self.train_seg:
            self.metric_evaluator_iou = IntersectionOverUnion(n_classes=self.metric_evaluator_iou.n_classes, device=self.device)
        detect_result, lane_result, losses = [], [], []
        det_eval = None
        if coco_gt is not None and self.train_detect and self.rank == 0:
            from .det_eval import CocoBoxEvaluator
            det_eval = CocoBoxEvaluator(coco_gt, max_images=self.cfgs["detection"].get("max_images", 10000), device=self.device)
        net_w, net_h = net.net_input_width, net.net_input_height
        for iter_idx, batch_data in enumerate(self.validloader):
            batch_data = self.to_gpu(batch_data)
            inputs = batch_data["image"]
            n = inputs.shape[0]
            outputs = net(inputs)
            have_gt = all(k in batch_data for k, on in (("gt_seg", self.train_seg), ("gt_det", self.train_detect), ("gt_cls", self.train_lane),
                                                         ("gt_loc", self.train_lane)) if on)
            if have_gt:
                loss_dict = net.cal_loss(outputs, batch_data)
                loss_dict["total_loss"] = self.cal_total_loss(loss_dict)
                losses.append({k: float(v) for k, v in loss_dict.items()})
                if self.rank == 0 and iter_idx % self.print_interval == 0:
                    self.print_loss_info(loss_dict, epoch, iter_idx, mode="valid")
            shapes = batch_data.get("src_image_shape") or [{"width": net_w, "height": net_h}] * n
            # per-image task masks: every task is scored on its labelled images only, picked with the HOST copy of the mask (no sync)
            tvh = batch_data.get("task_valid_host")
            labelled = (lambda row: [True] * n) if tvh is None else (lambda row: [bool(v) for v in tvh[row].tolist()])
            if self.train_seg and "gt_seg" in batch_data:
                from . import ops as K
                pred_seg, gt_seg = K.argmax_channels(outputs["seg"]), batch_data["gt_seg"]
                if tvh is not None:
                    keep = torch.tensor([i for i, on in enumerate(labelled(0)) if on], dtype=torch.int64).to(self.device)
                    pred_seg, gt_seg = pred_seg.index_select(0, keep), gt_seg.index_select(0, keep)
                if pred_seg.shape[0]:
                    self.metric_evaluator_iou.update(pred_seg, gt_seg)
            if self.train_detect:
                d = outputs["detection"]
                preds = net.detectheader.decode(inputs, d["regression"], d["classification"], d["anchors"], conf_thres=det_conf_thres,
                                                iou_thres=det_iou_thres)
                metas = [[net_w, net_h, sh["width"], sh["height"], 0, 0] for sh in shapes]
                preds = net.detectheader.invert_affine(metas, preds)                                       # train.py:334-336
                if tvh is not None:                  # an image without a box label leaves no record; the others keep their image ids
                    none = dict(rois=np.zeros((0, 4), np.float32), class_ids=np.zeros((0,), np.int64), scores=np.zeros((0,), np.float32))
                    preds = [pr if on else none for pr, on in zip(preds, labelled(1))]
                first_id = iter_idx * self.cfgs["train"].get("batch_size_valid", n) + 1
                detect_result += detections_to_coco(preds, first_id)
                if det_eval is not None:
                    det_eval.update(preds, first_id)
            if self.train_lane and lane_coder is not None:
                l = self.cfgs["lane"]
                lanes = net.laneheader.decode_batch(outputs["lane"]["predict_cls"], outputs["lane"]["predict_loc"], lane_coder,
                                                    l.get("conf_thres", 0.5), l.get("nms_thres", 100), False)
                gts = batch_data.get("gt_lane_json")
                pairs = []
                for i, (ln, sh) in enumerate(zip(lanes, shapes)):
                    pj = net.laneheader.scale_to_org(ln, net_w, net_h, sh["width"], sh["height"])
                    lane_result.append(dict(pr_result={**pj, **dict(Shape=sh)}))
                    if gts is not None and labelled(2)[i]:
                        pairs.append(dict(pr_result=lane_result[-1]["pr_result"], gt_result={**gts[i], **dict(Shape=sh)}))
                if pairs:
                    lane_metric(output=pairs)                                                                      # train.py:397
                    lane_pairs += len(pairs)
        net.train()
        scores = self.metric_evaluator_iou.compute() if self.train_seg else None
        path = write_results(detect_result, eval_dir) if (eval_dir and self.train_detect and self.rank == 0) else None
        lane_f1 = None
        if lane_pairs:
            lane_f1 = lane_metric.summary()                                                                        # train.py:433
            if self.rank == 0:
                print("=========================== metric lane %i ===========================" % epoch)
                print(lane_f1)
        self.last_valid = dict(losses=losses, detect_result=detect_result, detect_json=path, lane_result=lane_result, iou=scores, lane_f1=lane_f1)
        if coco_gt is not None and self.train_detect:
            res = det_eval.compute() if det_eval is not None else None
            if self.rank == 0:
                print("=========================== metric detection %i ===========================" % epoch)         # train.py:414
                if res is not None:
                    print("\n".join(det_eval.summary()))
            self.last_valid["det_eval"] = res
        return scores

    # ------------------------------------------------------------------------------------------------------------------------------
    # Full-state checkpoints (checkpoint.py, hn_ckpt.hip)
    STATE_KEYS = ("grad_clip_norm", "skip_nonfinite", "ema_decay", "ema_warmup", "protect_bn_stats", "ema_buffers", "accum_steps")

    def _state_keys(self) -> dict:
        """the train keys that shape the state, as this trainer resolved them: a state file loads only where they agree"""
        keys = dict(grad_clip_norm=self.grad_clip_norm, skip_nonfinite=self.skip_nonfinite, ema_decay=self.ema_decay,
                    ema_warmup=self.ema_warmup if self.ema_decay is not None else None, protect_bn_stats=self.protect_bn_stats,
                    ema_buffers=self.ema_buffers, accum_steps=self.accum_steps)
        if self.loss_balance is not None:       # (only when on: a file written without it keeps exactly its manifest)
            keys["loss_balance"] = "uncertainty"
        return keys

    def _state_tensors(self):
        """[(name, tensor)] of everything that travels in a state file's blob, in a fixed order: the model's parameters and persistent
        buffers ("model/<state_dict key>"), Adam's moments and weight averages ("optim/<parameter>/exp_avg" ...), the guard's record,
        the BufferKeeper's averages.  The keeper's shadows are rewritten before every forward, gradients and the accumulator's buffer
        by every group's first micro-batch: they do not travel."""
        net, opt = self.hydranet, self.optimizer
        named = [("model/" + k, v.detach()) for k, v in net.state_dict(keep_vars=True).items()]
        for n, p in net.named_parameters():
            st = opt.state.get(p)
            if st:
                named += [("optim/%s/%s" % (n, k), st[k]) for k in ("exp_avg", "exp_avg_sq", "ema") if k in st]
        if getattr(opt, "guarded", False):
            named.append(("guard/record", opt.guard_record))
        if self.buffer_keeper is not None and self.buffer_keeper.avg is not None:
            named += [("keeper/avg/" + n, a) for n, a in zip(self.buffer_keeper.names, self.buffer_keeper.avg)]
        if self.balance_optimizer is not None:
            s = self.hydranet.loss_log_vars
            st = self.balance_optimizer.state[s]
            named += [("balance/log_vars", s), ("balance/exp_avg", st["exp_avg"]), ("balance/exp_avg_sq", st["exp_avg_sq"])]
        return named

    def _state_packer(self):
        from .checkpoint import StatePacker
        named = self._state_tensors()
        pk = self._packer
        if pk is None or [n for n, _ in pk.named] != [n for n, _ in named] or any(a is not b and a.data_ptr() != b.data_ptr()
                                                                                     for (_, a), (_, b) in zip(pk.named, named)):
            pk = self._packer = StatePacker(named)
        return pk

    def _host_state(self, epoch: int) -> dict:
        """what travels in the manifest: JSON values only; floats come back bit for bit (json's shortest round-trip repr)"""
        opt = self.optimizer
        per = {}
        for n, p in self.hydranet.named_parameters():
            st = opt.state.get(p)
            if st:
                per[n] = dict(step=int(st["step"]), **({"ema_start": int(st["ema_start"])} if "ema_start" in st else {}))
        groups = [{k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items() if k != "params"} for g in opt.param_groups]
        host = dict(epoch=int(epoch), phase=self.phase, train=self._state_keys(), params=per, param_groups=groups,
                    scheduler=self.scheduler.state_dict(), settles=None if self.buffer_keeper is None else int(self.buffer_keeper.settles),
                    world=self.world)
        if self.balance_optimizer is not None:
            host["balance_step"] = int(self.balance_optimizer.state[self.hydranet.loss_log_vars]["step"])
        return host

    def checkpoint_wait(self):
        """join a save_state(wait=False) in flight (a no-op without one); an error of the background writer is raised here"""
        th, self._ckpt_thread = self._ckpt_thread, None
        if th is not None:
            th.join()
        err, self._ckpt_error = self._ckpt_error, None
        if err is not None:
            raise err

    def save_state(self, path: str, wait: bool = True, epoch: Optional[int] = None):
        """the full training state into `path` (checkpoint.py's format): ONE pack launch on the training stream gathers ~3 300 tensors
        and their checksums into a staging buffer, one device-to-host copy on a side stream follows it, and the file is written from
        the pinned buffer -- with wait=False by a background thread that launches nothing, while training goes on (later steps write
        the live tensors, not the staging buffer).  A second save_state, load_state or checkpoint_wait() joins a write in flight
        first.  epoch: the epoch a resumed run starts at (default: next_epoch).  Only rank 0 writes.  Raises RuntimeError with
        micro-batches pending in the accumulator (flush_accumulated() first), as set_phase does."""
        from .checkpoint import write_file
        if not isinstance(self.optimizer, Adam):
            raise RuntimeError("save_state carries the HIP Adam's state: it needs hip_adam=True")
        if self.accumulator is not None and self.accumulator.pending:
            raise RuntimeError("save_state with %i accumulated micro-batch(es) pending: call flush_accumulated() first" % self.accumulator.pending)
        self.checkpoint_wait()
        if epoch is not None:
            self.next_epoch = int(epoch)
        if self.rank != 0:
            return
        pk = self._state_packer()
        if self._stream is None:
            pk.pack()
        else:                                   # the trainer's own stream, the way flush_accumulated steps on it
            cur = torch.cuda.current_stream()
            self._stream.wait_stream(cur)
            with torch.cuda.stream(self._stream):
                pk.pack()
            cur.wait_stream(self._stream)
        host = self._host_state(self.next_epoch)                     # (now: the thread must not see what later steps make of it)

        def finish():
            entries, blob = pk.wait_host()                           # an event wait; nothing is launched from here
            write_file(path, entries, blob, host)
        if wait:
            return finish()

        def run():
            try:
                finish()
            except BaseException as e:                               # raised by checkpoint_wait()
                self._ckpt_error = e
        import threading
        self._ckpt_thread = threading.Thread(target=run, name="hydranet-state-writer", daemon=True)
        self._ckpt_thread.start()

    def load_state(self, path: str) -> dict:
        """continue from a save_state file: -> its host-side state (["epoch"] = the epoch to run next, also left in next_epoch).
        The file is read and validated on the host (checkpoint.CheckpointError) and compared with this trainer -- the train keys that
        shape the state, every tensor's name, shape and dtype: the first difference raises ValueError -- before anything is touched.
        Then optimizer state (and the BufferKeeper) the file lists is allocated, the blob goes to the device in one copy, is verified
        there and scattered IN PLACE under the verdict (no tensor object is replaced: captured graphs and cached pointers stay valid).
        A tensor whose checksum fails raises checkpoint.CheckpointCorrupt naming it, with every device tensor and the optimizer's
        state dict as they were.  Every rank loads the file (it holds rank 0's BatchNorm statistics, which is what broadcast_state
        hands out at construction)."""
        from .checkpoint import CheckpointCorrupt, read_file, _DTYPES
        if not isinstance(self.optimizer, Adam):
            raise RuntimeError("load_state carries the HIP Adam's state: it needs hip_adam=True")
        if self.accumulator is not None and self.accumulator.pending:
            raise RuntimeError("load_state with %i accumulated micro-batch(es) pending: call flush_accumulated() first" % self.accumulator.pending)
        self.checkpoint_wait()
        manifest, blob = read_file(path)
        host, opt, net = manifest["host"], self.optimizer, self.hydranet
        # ---- compare: nothing is touched before every check has passed
        try:
            theirs, per, phase = host["train"], host["params"], host["phase"]
            groups, sched, epoch, settles = host["param_groups"], host["scheduler"], int(host["epoch"]), host["settles"]
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError("%s: the manifest lacks host-side state (%s)" % (path, e))
        mine = self._state_keys()
        for k in self.STATE_KEYS + ("loss_balance",):
            if theirs.get(k) != mine.get(k):
                raise ValueError("%s was saved with train.%s = %r, this trainer has %r" % (path, k, theirs.get(k), mine.get(k)))
        if self.balance_optimizer is not None and not isinstance(host.get("balance_step"), int):
            raise ValueError("%s: the manifest lacks the log-variances' step count" % path)
        if phase not in PHASES or self._phase_module(phase) is None or len(groups) != len(opt.param_groups):
            raise ValueError("%s: phase %r / %i param groups do not fit this trainer" % (path, phase, len(groups)))
        params = dict(net.named_parameters())
        want = [("model/" + k, v) for k, v in net.state_dict(keep_vars=True).items()]
        for n, p in params.items():
            if n in per:
                want += [("optim/%s/%s" % (n, k), p) for k in ("exp_avg", "exp_avg_sq")]
                if "ema_start" in per[n]:
                    want.append(("optim/%s/ema" % n, p))
        unknown = [n for n in per if n not in params]
        if unknown:
            raise ValueError("%s holds optimizer state of %s, which this model does not have" % (path, unknown[0]))
        if opt.guarded:
            want.append(("guard/record", torch.empty(8, dtype=torch.int32)))
        if self.ema_buffers and settles is not None:
            from .bn_state import SUFFIXES
            want += [("keeper/avg/" + n, b) for n, b in net.named_buffers() if n.endswith(SUFFIXES)]
        if self.balance_optimizer is not None:
            want += [("balance/" + k, net.loss_log_vars) for k in ("log_vars", "exp_avg", "exp_avg_sq")]
        ents = manifest["tensors"]
        for i in range(max(len(ents), len(want))):
            if i >= len(ents) or i >= len(want):
                raise ValueError("%s: %s" % (path, ("this trainer's state also has %s" % want[i][0]) if i >= len(ents) else
                                             ("the file also holds %s" % ents[i]["name"])))
            e, (n, t) = ents[i], want[i]
            if e["name"] != n:
                raise ValueError("%s: tensor %i is %s, this trainer's state has %s there" % (path, i, e["name"], n))
            if tuple(e["shape"]) != tuple(t.shape) or _DTYPES[e["dtype"]] != t.dtype:
                raise ValueError("%s: %s is %s %s, this trainer's is %s %s" % (path, n, e["dtype"], tuple(e["shape"]), t.dtype, tuple(t.shape)))
        # ---- allocate what the file lists and this trainer lacks (remembered: a corrupt file takes it away again)
        made, made_ema = [], []
        keeper_was, record_was = self.buffer_keeper, opt._record
        for n, p in params.items():
            if n not in per:
                continue
            st = opt.state[p]
            if not st:
                st["step"] = torch.zeros((), dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                made.append(p)
            if "ema_start" in per[n] and "ema" not in st:
                st["ema"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["ema_start"] = int(per[n]["ema_start"])
                made_ema.append(p)
        if settles is not None:
            self._keeper()
        else:
            self.buffer_keeper = None           # saved before the first step: the keeper is built at the next one, from the loaded statistics
        # this trainer's own state that the file does not list leaves only after a good load: keep it aside
        extra = {p: {k: st.pop(k) for k in ("ema", "ema_start") if k in st} for n, p in params.items()
                 for st in [opt.state.get(p)] if st and n in per and "ema_start" not in per[n] and "ema" in st}
        gone = {p: opt.state.pop(p) for n, p in params.items() if n not in per and opt.state.get(p)}

        def undo():
            for p, st in gone.items():
                opt.state[p] = st
            for p, kv in extra.items():
                opt.state[p].update(kv)
            fresh = {id(p) for p in made}
            for p in made_ema:
                if id(p) not in fresh:
                    opt.state[p].pop("ema"), opt.state[p].pop("ema_start")
            for p in made:
                del opt.state[p]
            self.buffer_keeper, opt._record = keeper_was, record_was
            self._packer = None
        try:
            pk = self._state_packer()
            pk.host_blob()[:] = blob
            if self._stream is None:
                bad = pk.restore(manifest)
            else:
                cur = torch.cuda.current_stream()
                self._stream.wait_stream(cur)
                with torch.cuda.stream(self._stream):
                    bad = pk.restore(manifest)
                cur.wait_stream(self._stream)
        except BaseException:
            undo()
            raise
        if bad >= 0:
            undo()
            raise CheckpointCorrupt("%s: the words of %s do not give the checksum its manifest records; nothing was loaded" %
                                    (path, ents[bad]["name"]), tensor=ents[bad]["name"])
        # ---- the host-side state
        for n, p in params.items():
            if n in per:
                opt.state[p]["step"] = torch.full((), float(per[n]["step"]), dtype=torch.float32)   # (Adam.step's slow path regroups the cohorts)
                if "ema_start" in per[n]:
                    opt.state[p]["ema_start"] = int(per[n]["ema_start"])
        opt._plans.clear()
        opt._fast.clear()
        opt._guard_plan = None
        opt._swap_plan = None
        if self.balance_optimizer is not None:
            bo = self.balance_optimizer
            bo.state[net.loss_log_vars]["step"] = torch.full((), float(host["balance_step"]), dtype=torch.float32)
            bo._plans.clear()
            bo._fast.clear()
            bo._guard_plan = None
        self.scheduler.load_state_dict(sched)
        for g, saved in zip(opt.param_groups, groups):
            g.update({k: (tuple(v) if k == "betas" else v) for k, v in saved.items()})
        if self.buffer_keeper is not None and settles is not None:
            self.buffer_keeper.settles = int(settles)
        self.set_phase(phase)
        self.next_epoch = epoch
        # parameters and statistics were rewritten through raw pointers: eval-mode caches are stale, as after swap_ema()
        from .ops.core import bump_mutation_epoch, mutation_cells
        bump_mutation_epoch(mutation_cells(list(net.parameters()) + list(net.buffers())))
        return host

    def save(self, path: str, ema: bool = False):
        """checkpoint in the reference's format: a DDP-wrapped module's state_dict carries "module." prefixes (train.py:437).  ema: every
        parameter that has an average (optim.Adam.ema_named) is written as its average; buffers (BatchNorm running statistics among them)
        and parameters without one as they are -- with train.ema_buffers the BatchNorm running statistics and counters are written as
        their averages too (buffer_keeper.ema_named).  Nothing is exchanged for it."""
        if ema and self.ema_decay is None:
            raise ValueError("save(ema=True) needs train.ema_decay")
        if self.rank != 0:
            return
        sd = self.hydranet.state_dict()
        if ema:
            avg = self.optimizer.ema_named(self.hydranet.named_parameters())
            if self.buffer_keeper is not None:
                avg.update(self.buffer_keeper.ema_named())
            sd = {k: (avg[k].detach() if k in avg else v) for k, v in sd.items()}
        if self.use_distribute:
            sd = {"module." + k: v for k, v in sd.items()}
        torch.save(sd, path)
