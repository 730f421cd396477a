"""torch.optim.Adam's update as ONE HIP launch over all parameters (hn_adam_step).

The reference trains with `torch.optim.Adam(params, lr, weight_decay=wd)` (model/train.py:147).  On this model that is 693 parameter
tensors: the foreach implementation issues ~10 multi-tensor launches and takes 3.9 ms per step on MI355X, 17 % on top of the 22.5 ms
forward + loss + backward.  One pass over (p, g, m, v) moves 1.2 GB: ~0.35 ms.  Same update rule, same state layout (`step`, `exp_avg`,
`exp_avg_sq` per parameter -- state_dict() / load_state_dict() are interchangeable with torch.optim.Adam's), same operation order (so it tracks torch's result to
the last bit or two of fp32); LR schedulers work on `param_groups[i]["lr"]` as usual.  fp32 CUDA parameters only; not amsgrad / maximize.

Opt-in, decided on the device with no host synchronisation (hn_grad_guard + hn_adam_step_guarded, include/hydranet_hip.h):
`max_grad_norm` = torch.nn.utils.clip_grad_norm_ over every parameter that has a gradient, in every param group; `skip_nonfinite` = a step
whose gradient norm (or one of the `losses` handed to step()) is not finite leaves parameters and moments untouched.  With both off, step()
issues exactly the launches it always did.

Opt-in as well: `ema_decay` keeps an exponential moving average of every stepped parameter, updated INSIDE the Adam launch
(hn_adam_step_ema: e' = e + (1 - decay) * (p' - e) while the new value p' is in its register), and exchanges averaged and live VALUES in
place in one launch (hn_swap_many: swap_ema() / averaged()), so that every raw pointer held elsewhere -- a captured training step, the job
tables here, eval-mode caches -- stays valid.  With ema_decay=None step() issues exactly the launches it issues without the option.
"""
from __future__ import annotations

import contextlib
import ctypes
import weakref

import torch

from ._lib import lib
from .ops.core import bump_mutation_epoch, mutation_cells


def ema_decay_at(n: int, decay: float, warmup: bool = True) -> float:
    """the average's decay at its step number n (0-based: the number of EMA steps already issued), in double:
    min(decay, (1 + n) / (10 + n)) with warm-up -- 0.1 at first, so that a young average follows the weights instead of its start -- else
    `decay`"""
    decay = float(decay)
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, max_grad_norm=None,
                 skip_nonfinite: bool = False, ema_decay=None, ema_warmup: bool = True):
        """max_grad_norm: clip the global L2 norm of all gradients to it (None or <= 0: off).  The clipping coefficient is applied inside
        the Adam launch: the gradient tensors themselves are NOT modified (no extra pass over them), `p.grad` after step() is what backward
        left.  skip_nonfinite: a non-finite gradient norm or loss skips the step on the device.  On a skipped step the per-parameter
        `step` count (host side; the bias corrections are computed from it on the host in double) and any LR scheduler still advance --
        torch's GradScaler-style skip would not bump them.
        ema_decay (None: off; else 0 <= ema_decay < 1), ema_warmup: the weight average.  `state[p]["ema"]` is created at the parameter's
        first EMA step as a clone of p taken before that step's update, next to `state[p]["ema_start"]` (a Python int: the parameter's
        `step` count at that moment), so both travel in state_dict() / load_state_dict(); torch.optim.Adam loads such a state dict and
        ignores the two keys.  The decay of a step is ema_decay_at(n, ema_decay, ema_warmup), n = the number of EMA steps already issued
        for the parameter = its `step` count before the update - ema_start: it advances on skipped steps too, as the bias corrections do
        (the average itself is untouched by a skipped step).  Only tensors that a step's launch actually steps get an average and have
        it updated: a parameter outside the current param group (a head-only fine-tuning phase), or one without a gradient (the model's
        four p5_to_p6 tensors never get one), is left alone -- and is not exchanged by swap_ema() unless an earlier phase gave it an
        average.  BatchNorm running statistics are buffers, not parameters: the optimizer neither averages nor exchanges them
        (bn_state.BufferKeeper does, next to it)."""
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or lr < 0.0 or eps < 0.0 or weight_decay < 0.0:
            raise ValueError("invalid Adam hyper-parameter")
        if max_grad_norm is not None and max_grad_norm != max_grad_norm:
            raise ValueError("invalid Adam hyper-parameter")
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._plans = {}                # (group index, cohort) -> (pointer signature, jobs, block_job, blocks, parameters, ema pointers)
        self._fast = {}                 # group index -> (gradient tensors of the last step, shared step scalar, plan, ema_start)
        self.ema_decay = float(ema_decay) if ema_decay is not None else None
        self.ema_warmup = bool(ema_warmup)
        self._swap_plan = None          # (pointer signature, jobs, block_job, blocks, mutation cells) of swap_ema()
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm is not None and max_grad_norm > 0 else None
        self.skip_nonfinite = bool(skip_nonfinite)
        self._guard_plan = None         # (plans of the last guarded step, jobs, block_job, blocks, n_jobs, workspace)
        self._record = None             # 8 int32 words on the device: hn_grad_guard's record
        self.grad_sq_by_param = None    # device double [n]: sum of squares of every gradient of the last guarded step (see guard_params)
        self.guard_params = []          # the parameters grad_sq_by_param's entries belong to, in order

    @property
    def guarded(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite

    @property
    def guard_record(self):
        """hn_grad_guard's record on the device (int32 [8]; words 0 and 1 hold fp32 bits): norm, coef, skip, steps, skipped,
        skipped_consecutive, pad, pad.  None when neither option is on.  The counters are not part of state_dict()."""
        if self._record is None and self.guarded:
            dev = next(p.device for g in self.param_groups for p in g["params"])
            self._record = torch.zeros((8,), dtype=torch.int32, device=dev)
        return self._record

    def grad_guard_record(self) -> dict:
        """the record as a dict (this call synchronises): norm, coef of the last step, its skip mask (1: gradient norm not finite, 2: a
        loss not finite, 4: a guard word raised), and the counters since construction"""
        rec = self.guard_record
        if rec is None:
            raise RuntimeError("multitask_hydranet_amd.optim.Adam: neither max_grad_norm nor skip_nonfinite is set")
        host = rec.cpu()
        norm, coef = host[:2].view(torch.float32).tolist()
        skip, steps, skipped, consecutive = host[2:6].tolist()
        return dict(norm=norm, coef=coef, skip=skip, steps=steps, skipped=skipped, skipped_consecutive=consecutive)

    def state_dict(self):
        """torch.optim.Adam's layout.  Internally all parameters of a cohort share ONE host `step` scalar (one increment per step instead of
        693); torch.optim.Adam bumps every parameter's `step` separately, so a shared tensor would advance by #params per step once loaded
        there: the exported state gives every parameter its own copy."""
        sd = super().state_dict()
        sd["state"] = {k: ({**v, "step": v["step"].clone()} if isinstance(v.get("step"), torch.Tensor) else dict(v)) for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """the cached job tables hold raw exp_avg / exp_avg_sq pointers of the state they were built from: drop them with it"""
        super().load_state_dict(state_dict)
        self._plans.clear()
        self._fast.clear()
        self._guard_plan = None
        self._swap_plan = None

    def __getstate__(self):
        return {**super().__getstate__(), "max_grad_norm": self.max_grad_norm, "skip_nonfinite": self.skip_nonfinite,
                "ema_decay": self.ema_decay, "ema_warmup": self.ema_warmup}

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plans, self._fast, self._guard_plan, self._swap_plan = {}, {}, None, None
        self.__dict__.setdefault("ema_decay", None)
        self.__dict__.setdefault("ema_warmup", True)
        self._record, self.grad_sq_by_param, self.guard_params = None, None, []    # (a copy counts its own steps)

    def _plan(self, key, ps, ema=False, gof=None):
        """gof: parameter -> its gradient tensor (None: p.grad; step(grads=accumulator): the accumulator's view)"""
        gof = gof or (lambda p: p.grad)
        sig = tuple((p.data_ptr(), gof(p).data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr()) for p in ps)
        if ema:
            sig += tuple(self.state[p]["ema"].data_ptr() for p in ps)
        pl = self._plans.get(key)
        if pl is not None and pl[0] == sig:
            return pl
        rows, owner, blk = [], [], 0
        for i, p in enumerate(ps):
            st = self.state[p]
            nb = (p.numel() + 1023) // 1024
            rows.append([p.data_ptr(), gof(p).data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), blk])
            owner += [i] * nb
            blk += nb
        dev = ps[0].device
        # the rows stay 6 wide (hn_grad_guard reads the same tables): the averages' pointers are a table of their own, one per job
        etab = torch.tensor([self.state[p]["ema"].data_ptr() for p in ps], dtype=torch.int64).to(dev) if ema else None
        pl = (sig, torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(owner, dtype=torch.int32).to(dev), blk, list(ps), etab)
        self._plans[key] = pl
        return pl

    def _run_guard(self, plans, losses, guard_words):
        """ONE hn_grad_guard over the gradients of every launch of this step (the norm is global, as clip_grad_norm_'s is).  A single
        launch's tables serve as they are; several (param groups, step cohorts) are concatenated once and cached while the plans live."""
        gd = self._guard_plan
        if gd is None or len(gd[0]) != len(plans) or any(a is not b for a, b in zip(gd[0], plans)):
            if len(plans) == 1:
                _, jobs, owner, blocks, ps, _ = plans[0]
            else:
                jobs, owner, ps, blocks, nj = [], [], [], 0, 0
                for _, j, o, b, q, _ in plans:
                    j = j.clone()
                    j[:, 5] += blocks
                    jobs.append(j)
                    owner.append(o + nj)
                    ps += q
                    blocks += b
                    nj += len(q)
                jobs, owner = torch.cat(jobs), torch.cat(owner)
            nbytes = lib().query("hn_grad_guard_ws_bytes", blocks, len(ps))
            if nbytes < 0:
                raise RuntimeError("multitask_hydranet_amd.optim.Adam: gradient tables out of hn_grad_guard's range")
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=jobs.device)
            self.grad_sq_by_param = torch.zeros((len(ps),), dtype=torch.float64, device=jobs.device)
            self.guard_params = ps
            gd = self._guard_plan = (list(plans), jobs, owner, blocks, len(ps), ws)
        _, jobs, owner, blocks, nj, ws = gd
        ls = [t for t in (losses or ()) if t is not None]
        ws_ = [t for t in (guard_words or ()) if t is not None]
        for t in ls:
            if not (t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
                raise RuntimeError("multitask_hydranet_amd.optim.Adam.step: losses are fp32 device scalars")
        for t in ws_:
            if not (t.is_cuda and t.dtype == torch.int32 and t.numel() == 1):
                raise RuntimeError("multitask_hydranet_amd.optim.Adam.step: guard_words are int32 device words")
        la = (ctypes.c_void_p * max(len(ls), 1))(*[t.data_ptr() for t in ls])
        wa = (ctypes.c_void_p * max(len(ws_), 1))(*[t.data_ptr() for t in ws_])
        lib().call("hn_grad_guard", jobs.data_ptr(), owner.data_ptr(), blocks, nj, self.max_grad_norm or 0.0, 1 if self.skip_nonfinite else 0,
                   ctypes.addressof(la), len(ls), ctypes.addressof(wa), len(ws_), ws.data_ptr(), ws.numel(), self.grad_sq_by_param.data_ptr(),
                   self.guard_record.data_ptr())

    @torch.no_grad()
    def step(self, closure=None, *, losses=None, guard_words=None, grads=None):
        """losses: fp32 device scalars whose finiteness the guard checks (skip_nonfinite); guard_words: int32 device words, a non-zero one
        skips the step (whenever either option is on).  Both need max_grad_norm or skip_nonfinite.
        grads: a GradAccumulator with micro-batches pending -- the step's gradients are the accumulator's means (grads.grad(p)) instead
        of p.grad: the job tables' g column and the guard's tables point at the accumulator's views, the kernels are the same.  Only
        parameters that are in the accumulated group are stepped.  p.grad is neither read, rebound nor written (a captured step owns
        those tensors).  Without it every path is as it always was."""
        if grads is not None and grads.pending < 1:
            raise RuntimeError("multitask_hydranet_amd.optim.Adam.step: grads= is an accumulator without a pending micro-batch")
        gof = (lambda p: p.grad) if grads is None else grads.grad
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        guarded = self.guarded
        if not guarded and (losses or guard_words):
            raise ValueError("multitask_hydranet_amd.optim.Adam.step: losses / guard_words need max_grad_norm or skip_nonfinite")
        # hn_adam_step writes the parameters through raw pointers: eval-mode caches keyed on `_version` are stale -- those of the modules that own
        # these parameters (the owner cells are collected once per parameter list, not per step)
        sig = tuple(len(g["params"]) for g in self.param_groups)
        if getattr(self, "_mut_sig", None) != sig:
            self._mut_sig, self._mut_cells = sig, mutation_cells([p for g in self.param_groups for p in g["params"]])
        bump_mutation_epoch(self._mut_cells)
        ema = self.ema_decay is not None
        launches = []                   # (plan, lr, beta1, beta2, eps, weight decay, step, the average's decay or None) in issue order
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            hyper = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
            fast = self._fast.get(gi)
            if fast is not None and (fast[2][5] is not None) == ema and len(fast[0]) == len(group["params"]) and (
                    all((p.grad is None) if g is None else (p.grad is g()) for p, g in zip(group["params"], fast[0])) if grads is None else
                    all((gof(p) is None) if g is None else (gof(p) is g()) for p, g in zip(group["params"], fast[0]))):
                # the same gradient tensors as last time (a captured step rewrites them in place): no per-parameter work on the host
                _, step_t, plan, start = fast
                step_t += 1
                launches.append((plan, *hyper, int(step_t), ema_decay_at(int(step_t) - 1 - start, self.ema_decay, self.ema_warmup) if ema else None))
                continue
            by_step = {}
            for p in group["params"]:
                g = gof(p)
                if g is None or p.numel() == 0:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and g.dtype == torch.float32 and
                        g.is_contiguous() and not g.is_sparse):
                    raise RuntimeError("multitask_hydranet_amd.optim.Adam: fp32 contiguous CUDA parameters / gradients only")
                st = self.state[p]
                if not st:
                    st["step"] = torch.zeros((), dtype=torch.float32)                      # host scalar, as torch.optim.Adam keeps it
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if not ema:
                    by_step.setdefault(int(st["step"]), []).append(p)
                    continue
                if "ema" not in st:                                                        # the parameter's first EMA step: the value before it
                    st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
                    st["ema_start"] = int(st["step"])
                    self._swap_plan = None
                by_step.setdefault((int(st["step"]), int(st["ema_start"])), []).append(p)  # a cohort shares its step count AND its decay
            self._fast.pop(gi, None)
            for t, ps in by_step.items():
                t, start = t if ema else (t, 0)
                shared = torch.full((), float(t + 1), dtype=torch.float32)                 # one host scalar for the whole cohort
                for p in ps:
                    self.state[p]["step"] = shared
                plan = self._plan((gi, len(by_step) > 1 and ((t, start) if ema else t)), ps, ema, gof)
                launches.append((plan, *hyper, t + 1, ema_decay_at(t - start, self.ema_decay, self.ema_warmup) if ema else None))
                if len(by_step) == 1:
                    # weak references: never keep a dropped gradient alive (its address could not be reused by the next backward)
                    self._fast[gi] = ([None if gof(p) is None else weakref.ref(gof(p)) for p in group["params"]], shared, plan, start)
        if guarded and launches:
            self._run_guard([l[0] for l in launches], losses, guard_words)
        for plan, *args, decay in launches:
            if ema:
                lib().call("hn_adam_step_ema", plan[1].data_ptr(), plan[2].data_ptr(), plan[3], plan[5].data_ptr(), *args, decay,
                           self._record.data_ptr() if guarded else None)
            elif guarded:
                lib().call("hn_adam_step_guarded", plan[1].data_ptr(), plan[2].data_ptr(), plan[3], *args, self._record.data_ptr())
            else:
                lib().call("hn_adam_step", plan[1].data_ptr(), plan[2].data_ptr(), plan[3], *args)
        return loss

    # ------------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def swap_ema(self):
        """exchange live and averaged VALUES of every parameter that has an average, in one launch (hn_swap_many): no tensor object and
        no address changes, so a captured step, the job tables and every cache keyed on a pointer stay valid; eval-mode caches keyed on
        the values are dropped (the same mutation cells step() bumps, plus those of averaged parameters outside the current param
        groups).  Calling it twice restores every bit.  Not for use between a captured step's replay and its optimizer step."""
        ps = [p for p, st in self.state.items() if "ema" in st]
        if not ps:
            raise RuntimeError("multitask_hydranet_amd.optim.Adam.swap_ema: no parameter has an average yet (ema_decay, and one step)")
        sig = tuple((p.data_ptr(), self.state[p]["ema"].data_ptr()) for p in ps)
        sp = self._swap_plan
        if sp is None or sp[0] != sig:
            rows, owner, blk = [], [], 0
            for i, p in enumerate(ps):
                e = self.state[p]["ema"]
                if not (e.is_cuda and e.dtype == torch.float32 and e.is_contiguous() and e.numel() == p.numel() and p.is_contiguous()):
                    raise RuntimeError("multitask_hydranet_amd.optim.Adam: fp32 contiguous CUDA parameters / averages only")
                nb = (p.numel() + 1023) // 1024
                rows.append([p.data_ptr(), e.data_ptr(), p.numel(), blk])
                owner += [i] * nb
                blk += nb
            dev = ps[0].device
            cells = mutation_cells(ps + [p for g in self.param_groups for p in g["params"]])
            sp = self._swap_plan = (sig, torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(owner, dtype=torch.int32).to(dev), blk, cells)
        lib().call("hn_swap_many", sp[1].data_ptr(), sp[2].data_ptr(), sp[3])
        bump_mutation_epoch(sp[4])

    @contextlib.contextmanager
    def averaged(self):
        """`with optimizer.averaged():` the parameters hold their averages inside the block and the live values again after it, also
        when the block raises"""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def ema_named(self, named_parameters) -> dict:
        """{name: average tensor} of the parameters among `named_parameters` that have an average (the optimizer's own tensors, not
        copies)"""
        return {n: self.state[p]["ema"] for n, p in named_parameters if p in self.state and "ema" in self.state[p]}


class GradAccumulator:
    """The running mean of several backward passes' gradients (train.accum_steps; hn_grad_accum, include/hydranet_hip.h).

    add() after every backward folds the parameters' current `p.grad` into the accumulator's own flat fp32 buffer in ONE launch:
    micro-batch 1 of a group copies (the buffer is not read), micro-batch j gives acc + (g - acc) * (float)(1 / j) in three rounded
    operations, so the buffer holds the mean of the group so far after every call, and Adam.step(grads=accumulator) can be taken after
    any number of micro-batches.  `p.grad` is only read: a captured step's static gradients, the eager path's fresh tensors and a
    reducer's bucket views all serve.  The same launch keeps the means of up to 8 loss scalars and a sticky word (2: a loss of some
    micro-batch was not finite, 4: a guard word of some micro-batch was raised) to hand to Adam.step(guard_words=[...]) at the group's
    end.  Nothing is synchronised."""

    def __init__(self, params):
        ps, seen = [], set()
        for p in params:
            if id(p) in seen or p.numel() == 0:
                continue
            seen.add(id(p))
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("multitask_hydranet_amd.optim.GradAccumulator: fp32 contiguous CUDA parameters only")
            ps.append(p)
        if not ps:
            raise ValueError("multitask_hydranet_amd.optim.GradAccumulator: no parameters")
        self.params = ps
        # every parameter's slot starts on a 16-byte boundary of the flat buffer (ddp.GradReducer._close's layout rule)
        offs, off = [], 0
        for p in ps:
            offs.append(off)
            off += (p.numel() + 3) // 4 * 4
        dev = ps[0].device
        self.flat = torch.zeros(off, device=dev, dtype=torch.float32)
        self.offsets = offs
        self._views = {p: self.flat[o:o + p.numel()].view_as(p) for o, p in zip(offs, ps)}
        self._means = torch.zeros(8, device=dev, dtype=torch.float32)
        self._sticky = torch.zeros(1, device=dev, dtype=torch.int32)
        self.pending = 0                # micro-batches in the current group
        self._n_losses = 0
        self._member_ids = frozenset()  # the parameters (by id) of the current (or last) group's jobs
        self._table = None              # (pointer signature, jobs, block_job, blocks)
        self._fast = None               # weak references to the gradient tensors of the table (None where there was none)

    @property
    def sticky_word(self) -> torch.Tensor:
        """int32 [1] on the device: the group's sticky word (written by every add())"""
        return self._sticky

    def loss_means(self) -> torch.Tensor:
        """fp32 view of the means of the losses handed to add(), in their order (the accumulator's own memory: clone to keep)"""
        return self._means[:self._n_losses]

    def grad(self, p):
        """the accumulator's view for p (p's shape) if p has a job in the current group -- the last one after reset() -- else None"""
        return self._views[p] if id(p) in self._member_ids else None

    def reset(self):
        """start a new group: the next add() is micro-batch 1 (and overwrites the buffer without reading it)"""
        self.pending = 0

    def invalidate(self):
        """drop the job table (the set of parameters that get gradients changes: another training phase)"""
        self._table, self._fast = None, None

    def _jobs(self):
        fast = self._fast
        # (a dropped gradient's reference is dead: None, which a parameter that lost its gradient must not match)
        if fast is not None and all((p.grad is None) if g is None else (p.grad is not None and p.grad is g()) for p, g in zip(self.params, fast)):
            return self._table                                     # a captured step's static gradients, a reducer's bucket views
        ps = [p for p in self.params if p.grad is not None]
        if not ps:
            raise RuntimeError("multitask_hydranet_amd.optim.GradAccumulator.add: no parameter has a gradient")
        for p in ps:
            g = p.grad
            if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and not g.is_sparse and g.numel() == p.numel()):
                raise RuntimeError("multitask_hydranet_amd.optim.GradAccumulator: fp32 contiguous CUDA gradients only")
        ids = frozenset(id(p) for p in ps)
        if self.pending > 0 and ids != self._member_ids:
            raise RuntimeError("multitask_hydranet_amd.optim.GradAccumulator.add: the parameters that have a gradient differ from those of "
                               "the group's first micro-batch")
        sig = tuple((id(p), p.grad.data_ptr()) for p in ps)
        tb = self._table
        if tb is None or tb[0] != sig:                             # (fresh tensors at the old addresses, the eager path's usual case: kept)
            rows, owner, blk = [], [], 0
            for i, p in enumerate(ps):
                nb = (p.numel() + 1023) // 1024
                rows.append([p.grad.data_ptr(), self._views[p].data_ptr(), p.numel(), blk])
                owner += [i] * nb
                blk += nb
            dev = self.flat.device
            tb = self._table = (sig, torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(owner, dtype=torch.int32).to(dev), blk)
        self._member_ids = ids
        # weak references: never keep a dropped gradient alive (its address could not be reused by the next backward)
        self._fast = [None if p.grad is None else weakref.ref(p.grad) for p in self.params]
        return tb

    @torch.no_grad()
    def add(self, losses=None, guard_words=None):
        """fold the parameters' current gradients in as micro-batch `pending + 1` of the group.  losses: <= 8 fp32 device scalars (the
        same number in every micro-batch of a group); guard_words: <= 4 int32 device words.  Parameters without a gradient get no job; the
        set of parameters that have one must not change inside a group."""
        ls = [t for t in (losses or ()) if t is not None]
        ws = [t for t in (guard_words or ()) if t is not None]
        if len(ls) > 8 or len(ws) > 4:
            raise ValueError("multitask_hydranet_amd.optim.GradAccumulator.add: at most 8 losses and 4 guard words")
        for t in ls:
            if not (t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
                raise RuntimeError("multitask_hydranet_amd.optim.GradAccumulator.add: losses are fp32 device scalars")
        for t in ws:
            if not (t.is_cuda and t.dtype == torch.int32 and t.numel() == 1):
                raise RuntimeError("multitask_hydranet_amd.optim.GradAccumulator.add: guard_words are int32 device words")
        if self.pending > 0 and len(ls) != self._n_losses:
            raise RuntimeError("multitask_hydranet_amd.optim.GradAccumulator.add: the number of losses changed inside a group")
        _, jobs, owner, blocks = self._jobs()
        la = (ctypes.c_void_p * max(len(ls), 1))(*[t.data_ptr() for t in ls])
        wa = (ctypes.c_void_p * max(len(ws), 1))(*[t.data_ptr() for t in ws])
        lib().call("hn_grad_accum", jobs.data_ptr(), owner.data_ptr(), blocks, self.pending + 1, ctypes.addressof(la), len(ls),
                   self._means.data_ptr(), ctypes.addressof(wa), len(ws), self._sticky.data_ptr())
        self._n_losses = len(ls)
        self.pending += 1


def grad_norms_by_prefix(optimizer: Adam, named_parameters, prefixes):
    """per-submodule gradient norms of the optimizer's last guarded step (the multitask-balance view: prefixes such as "backbone", "neck",
    "segheader", "detectheader", "laneheader") -> {prefix: device double scalar}, from grad_sq_by_param; no synchronisation.  A prefix
    matches the parameter names that equal it or start with it + "."."""
    if optimizer.grad_sq_by_param is None:
        raise RuntimeError("grad_norms_by_prefix: the optimizer has not run a guarded step (max_grad_norm / skip_nonfinite)")
    index = {id(p): i for i, p in enumerate(optimizer.guard_params)}
    named = [(n, index[id(p)]) for n, p in named_parameters if id(p) in index]
    sq = optimizer.grad_sq_by_param
    out = {}
    for pre in prefixes:
        idx = [i for n, i in named if n == pre or n.startswith(pre + ".")]
        out[pre] = sq[torch.tensor(idx, dtype=torch.long, device=sq.device)].sum().sqrt() if idx else torch.zeros((), dtype=sq.dtype, device=sq.device)
    return out
