"""train.accum_steps in HydraTrainer on the device (tiny cfg, the fixture batch with different images per micro-batch, as
tests/test_train_gpu.py sets them up): grouping, equality with a hand-driven run on the yardstick's means (tests/grad_accum_ref.py),
captured == eager, off is off, a trailing partial group, the guard and the BatchNorm statistics per group, phase changes, and the
data-parallel code path at world size 1.  Every comparison is bit for bit."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import ema_ref, grad_accum_ref as ref
from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    g = torch.Generator().manual_seed(3)
    loader = []
    for i in range(8):                                                             # different images per micro-batch, same targets
        b = dict(batch)
        b["image"] = batch["image"] + 0.05 * torch.randn(batch["image"].shape, generator=g)
        loader.append(b)
    return z, cfgs, loader


def fresh(b):
    return {k: v.clone() for k, v in b.items()}


def make_trainer(tiny, capture=False, distribute=False, loader=None, **keys):
    from multitask_hydranet_amd.train import HydraTrainer
    z, cfgs, ld = tiny
    cfgs = copy.deepcopy(cfgs)
    cfgs["train"].update(keys)
    loader = ld if loader is None else loader
    tr = HydraTrainer(cfgs, trainloader=loader, validloader=None, iters_per_epoch=len(loader), capture_step=capture, force_distribute=distribute)
    tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    return tr


def bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().contiguous()


def params_of(tr):
    return {n: bits(p).clone() for n, p in tr.hydranet.named_parameters()}


def buffers_of(tr):
    return {n: bits(b).clone() for n, b in tr.hydranet.named_buffers()}


def moments_of(tr, keys=("exp_avg", "exp_avg_sq")):
    names = {p: n for n, p in tr.hydranet.named_parameters()}
    return {names[p] + "/" + k: bits(st[k]).clone() for p, st in tr.optimizer.state.items() for k in keys if k in st}


def same(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[n], b[n]) for n in a)


def differing(a, b):
    return [n for n in a if not torch.equal(a[n], b[n])]


def step(tr, b):
    return {k: float(v) for k, v in tr.train_step(fresh(b)).items()}


def hand_group(tr, batches):
    """one optimizer step of a trainer WITHOUT the key on the yardstick's mean of the micro-batches' gradients"""
    net, seen = tr.hydranet, []
    for b in batches:
        bd = tr.to_gpu(fresh(b))
        loss_dict = net.cal_loss(net(bd["image"]), bd)
        total = tr.cal_total_loss(loss_dict)
        tr.optimizer.zero_grad(set_to_none=True)
        total.backward(tr._one)
        seen.append({n: p.grad.detach().cpu().numpy().copy() for n, p in net.named_parameters() if p.grad is not None})
    assert all(sorted(s) == sorted(seen[0]) for s in seen)
    for n, p in net.named_parameters():
        if n in seen[0]:
            p.grad = torch.from_numpy(ref.mean_of([s[n] for s in seen])).to(p.device)
    tr.optimizer.step()
    tr.scheduler.step()


@pytest.fixture(scope="module")
def eager_k2(tiny):
    """k = 2, eager, eight micro-batches: the losses returned, and parameters / buffers / moments / LR step count after every one"""
    tr = make_trainer(tiny, accum_steps=2)
    assert tr.accumulator is not None and tr.accum_steps == 2
    trace = [dict(params=params_of(tr), epoch=tr.scheduler.last_epoch)]
    for b in tiny[2]:
        losses = step(tr, b)
        trace.append(dict(losses=losses, params=params_of(tr), buffers=buffers_of(tr), moments=moments_of(tr), epoch=tr.scheduler.last_epoch,
                          pending=tr.accumulator.pending, adam_steps={int(st["step"]) for st in tr.optimizer.state.values()}))
    steps = {int(st["step"]) for st in tr.optimizer.state.values()}
    assert tr._cap is None
    return trace, steps


def test_grouping(eager_k2):
    trace, steps = eager_k2
    for i in (1, 3):                                                               # after micro-batches 1 and 3: nothing stepped
        assert same(trace[i]["params"], trace[i - 1]["params"]) and trace[i]["epoch"] == trace[i - 1]["epoch"] and trace[i]["pending"] == 1
    for i in (2, 4):
        moved = differing(trace[i]["params"], trace[i - 1]["params"])
        assert len(moved) >= 0.5 * len(trace[i]["params"]), (i, len(moved))
        assert trace[i]["epoch"] == i // 2 and trace[i]["pending"] == 0
    assert trace[4]["epoch"] == 2 and trace[4]["adam_steps"] == {2}                # after four micro-batches: two LR steps, two Adam steps
    assert trace[3]["adam_steps"] == {1} and trace[8]["epoch"] == 4 and steps == {4}
    assert not trace[1]["moments"] and trace[2]["moments"]                         # Adam's state appears with the first group's step
    assert all(v == v and abs(v) < 1e9 for t in trace[1:] for v in t["losses"].values())


def test_returned_losses_are_the_means_of_the_group(tiny, eager_k2):
    trace, _ = eager_k2
    tr = make_trainer(tiny)                                                        # key absent: per-batch losses, and the same first step
    first = step(tr, tiny[2][0])
    assert first == trace[1]["losses"]                                             # micro-batch 1: the mean of one
    # micro-batch 2 ran on the SAME parameters under accumulation: a hand-driven forward on a trainer that has not stepped
    tr2 = make_trainer(tiny)
    net = tr2.hydranet
    got = []
    for b in tiny[2][:2]:
        bd = tr2.to_gpu(fresh(b))
        ld = net.cal_loss(net(bd["image"]), bd)
        ld["total_loss"] = tr2.cal_total_loss(ld)
        got.append({k: np.float32(float(v)) for k, v in ld.items()})
    for k, v in trace[2]["losses"].items():
        want = ref.mean_of([np.array([g[k]], dtype=np.float32) for g in got])[0]
        assert np.float32(v) == want, (k, v, want)


def test_equals_a_hand_driven_run(tiny, eager_k2):
    trace, _ = eager_k2
    loader = tiny[2]
    tr = make_trainer(tiny, loader=loader[:4])                                     # four optimizer steps per epoch: the same LR schedule
    assert tr.accumulator is None and tr.total_iters == 4
    for pair in ((0, 1), (2, 3)):
        hand_group(tr, [loader[i] for i in pair])
    assert same(params_of(tr), trace[4]["params"]), differing(params_of(tr), trace[4]["params"])[:5]
    assert same(moments_of(tr), trace[4]["moments"])
    assert same(buffers_of(tr), trace[4]["buffers"])
    assert tr.scheduler.last_epoch == trace[4]["epoch"] == 2


def test_captured_equals_eager(tiny, eager_k2):
    trace, _ = eager_k2
    tr = make_trainer(tiny, capture=True, accum_steps=2)
    for i, b in enumerate(tiny[2]):
        assert step(tr, b) == trace[i + 1]["losses"], i
    assert tr._cap is not None and tr.accumulator.pending == 0
    assert same(params_of(tr), trace[8]["params"]), differing(params_of(tr), trace[8]["params"])[:5]
    assert same(buffers_of(tr), trace[8]["buffers"])
    assert same(moments_of(tr), trace[8]["moments"])


def test_off_is_off(tiny):
    runs = []
    for keys in ({}, dict(accum_steps=1)):
        tr = make_trainer(tiny, **keys)
        assert tr.accumulator is None and tr.accum_steps == 1
        for b in tiny[2][:3]:
            step(tr, b)
        assert tr.scheduler.last_epoch == 3
        runs.append((params_of(tr), buffers_of(tr)))
    assert same(runs[0][0], runs[1][0]) and same(runs[0][1], runs[1][1])


def test_partial_group_is_stepped_at_the_end_of_the_epoch(tiny):
    loader = tiny[2][:3]
    tr = make_trainer(tiny, loader=[fresh(b) for b in loader], accum_steps=2)
    assert tr.total_iters == 2                                                     # ceil(3 / 2) optimizer steps: the cosine schedule ends there
    tr.train_one_epoch(0)
    assert tr.accumulator.pending == 0 and tr.scheduler.last_epoch == 2
    assert {int(st["step"]) for st in tr.optimizer.state.values()} == {2}
    tr.flush_accumulated()                                                         # nothing pending: a no-op
    assert tr.scheduler.last_epoch == 2
    hand = make_trainer(tiny, loader=loader[:2])                                   # (two optimizer steps: the same schedule)
    assert hand.total_iters == 2
    hand_group(hand, loader[:2])
    hand_group(hand, loader[2:])                                                   # micro-batch 3's gradient alone
    assert same(params_of(tr), params_of(hand)), differing(params_of(tr), params_of(hand))[:5]
    assert same(moments_of(tr), moments_of(hand)) and same(buffers_of(tr), buffers_of(hand))


def test_guard_and_statistics_follow_the_group(tiny):
    keys = dict(accum_steps=2, skip_nonfinite=True, protect_bn_stats=True, ema_decay=0.9, ema_buffers=True)
    tr = make_trainer(tiny, **keys)
    loader = tiny[2]
    step(tr, loader[0])
    step(tr, loader[1])                                                            # moments, averages and the keeper exist from here on
    everything = lambda: (params_of(tr), moments_of(tr, ("exp_avg", "exp_avg_sq", "ema")), buffers_of(tr),
                          {n: bits(t).clone() for n, t in tr.buffer_keeper.ema_named().items()})
    before = everything()
    assert any(n.endswith("/ema") for n in before[1]) and before[3] and tr.buffer_keeper.settles == 1
    r = tr.optimizer.grad_guard_record()
    assert r["steps"] == 1 and r["skipped"] == 0, r
    bad = fresh(loader[2])
    bad["image"][0, 0, 0, 0] = float("nan")
    tr.train_step(bad)
    assert tr.accumulator.pending == 1
    mid = buffers_of(tr)
    assert differing(mid, before[2])                                               # the poisoned forward did write the statistics
    tr.train_step(fresh(loader[3]))
    assert tr.accumulator.pending == 0
    r = tr.optimizer.grad_guard_record()
    # (behind the stem's BatchNorm + ReLU the poisoned forward is finite again, and so are its losses: it is the accumulated gradient
    # of the stem's weights -- NaN from micro-batch 1 on, whatever micro-batch 2 adds -- that the guard sees in the norm)
    # (measured: total losses 129.24 and 128.74, sticky word 0, norm NaN, skip mask 1)
    assert r["skip"] != 0 and r["steps"] == 2 and r["skipped"] == 1 and r["skipped_consecutive"] == 1, r
    after = everything()
    for x, y, what in zip(before, after, ("parameters", "moments and weight averages", "buffers", "buffer averages")):
        assert same(x, y), (what, differing(x, y)[:5])
    assert tr.scheduler.last_epoch == 2                                            # (the LR schedule advances on a skipped step, as without the key)
    # the next clean group is applied, and the averages advance once for it
    step(tr, loader[4])
    assert same(params_of(tr), before[0])
    step(tr, loader[5])
    r = tr.optimizer.grad_guard_record()
    assert r["skip"] == 0 and r["steps"] == 3 and r["skipped"] == 1 and r["skipped_consecutive"] == 0, r
    now = everything()
    moved = differing(now[0], before[0])
    assert len(moved) >= 0.5 * len(now[0]), len(moved)
    assert tr.buffer_keeper.settles == 3
    decay = ema_ref.ema_decay_at(2, 0.9)                                           # the third EMA step (a skipped one counts in the schedule)
    for n in moved:
        e0 = before[1][n + "/ema"].view(torch.float32).cpu().numpy()
        p1 = now[0][n].view(torch.float32).cpu().numpy()
        want = ema_ref.ema_step(e0, p1, decay)
        assert np.array_equal(now[1][n + "/ema"].cpu().numpy(), want.view(np.int32)), n
    assert all(bool(torch.isfinite(p).all()) for p in tr.hydranet.parameters())
    assert all(bool(torch.isfinite(b).all()) for b in tr.hydranet.buffers() if b.dtype == torch.float32)


def nan_lane_target(b):
    """a NaN lane target: the loss is NaN while activations and statistics stay finite"""
    b = fresh(b)
    row = (b["gt_cls"][..., 1] > 0).nonzero()[0]
    b["gt_loc"][row[0], row[1], 0] = float("nan")
    return b


def test_one_skipped_group_does_not_end_the_run(tiny):
    """train_one_epoch with accum_steps >= print_interval and one poisoned micro-batch: the divergence exit counts consecutive skipped
    optimizer steps against print_interval, so a single skipped group -- all a print interval holds here -- must not end the run"""
    loader = [fresh(b) for b in tiny[2][:6]]
    loader[2] = nan_lane_target(loader[2])                                         # the second group's first micro-batch
    tr = make_trainer(tiny, loader=loader, accum_steps=2, print_interval=2, skip_nonfinite=True)
    assert tr.print_interval == 2 and tr.accum_steps >= tr.print_interval
    p0 = params_of(tr)
    tr.train_one_epoch(0)                                                          # prints at micro-batches 0, 2, 4: returns, no SystemExit
    r = tr.optimizer.grad_guard_record()
    assert r["steps"] == 3 and r["skipped"] == 1 and r["skipped_consecutive"] == 0 and r["skip"] == 0, r
    assert tr.accumulator.pending == 0 and tr.scheduler.last_epoch == 3
    assert len(differing(params_of(tr), p0)) >= 0.5 * len(p0)
    assert all(bool(torch.isfinite(p).all()) for p in tr.hydranet.parameters())


def test_status_word_of_the_first_micro_batch_reaches_the_guard(tiny, monkeypatch):
    """a status word raised during micro-batch 1 only (a stand-in for the persistent stage kernels' word, which is clear again when
    the group's step is taken): losses and gradients are clean, only the accumulator's sticky word can skip the step"""
    import multitask_hydranet_amd.train as T
    word = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    monkeypatch.setattr(T, "K_xstage_status_word", lambda dev: word)
    tr = make_trainer(tiny, accum_steps=2, skip_nonfinite=True)
    loader = tiny[2]
    step(tr, loader[0])
    step(tr, loader[1])                                                            # moments exist from here on
    before = (params_of(tr), moments_of(tr))
    word.fill_(1)
    l1 = step(tr, loader[2])
    word.fill_(0)
    l2 = step(tr, loader[3])
    r = tr.optimizer.grad_guard_record()
    assert all(v == v and abs(v) < 1e9 for l in (l1, l2) for v in l.values())
    assert int(tr.accumulator.sticky_word.item()) == 4
    assert r["skip"] == 4 and r["steps"] == 2 and r["skipped"] == 1 and r["norm"] == r["norm"], r
    assert same(params_of(tr), before[0]) and same(moments_of(tr), before[1])
    step(tr, loader[4])
    step(tr, loader[5])
    r = tr.optimizer.grad_guard_record()
    assert r["skip"] == 0 and r["steps"] == 3 and r["skipped"] == 1 and int(tr.accumulator.sticky_word.item()) == 0, r
    assert len(differing(params_of(tr), before[0])) >= 0.5 * len(before[0])


def test_phase_change_needs_a_flushed_group(tiny):
    tr = make_trainer(tiny, accum_steps=2)
    loader = tiny[2]
    step(tr, loader[0])
    p0 = params_of(tr)
    with pytest.raises(RuntimeError):
        tr.set_phase("seg")
    assert tr.phase == "joint" and tr.accumulator.pending == 1
    tr.flush_accumulated()
    assert tr.accumulator.pending == 0 and tr.scheduler.last_epoch == 1 and differing(params_of(tr), p0)
    tr.set_phase("seg")
    assert tr.phase == "seg"
    p1 = params_of(tr)
    step(tr, loader[1])
    assert same(params_of(tr), p1)
    step(tr, loader[2])
    moved = differing(params_of(tr), p1)
    assert moved and all(n.startswith("segheader.") for n in moved), moved[:5]
    assert tr.scheduler.last_epoch == 2


def test_data_parallel_code_path_at_world_size_one(tiny, eager_k2):
    """force_distribute + capture_step, k = 2: every micro-batch's backward is a complete exchange (in the hipGraph once captured), the
    accumulator reads the exchanged gradients -- the average over one rank is the identity"""
    import socket
    trace, _ = eager_k2
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(so.getsockname()[1])
    tr = make_trainer(tiny, capture=True, distribute=True, accum_steps=2)
    for i, b in enumerate(tiny[2][:6]):
        assert step(tr, b) == trace[i + 1]["losses"], i
    torch.cuda.synchronize()
    assert tr._cap is not None and tr.reducer is not None and tr.accumulator.pending == 0
    assert same(params_of(tr), trace[6]["params"]), differing(params_of(tr), trace[6]["params"])[:5]
    assert same(buffers_of(tr), trace[6]["buffers"])
    assert tr.scheduler.last_epoch == 3
