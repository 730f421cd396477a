"""train.loss_balance: uncertainty in HydraTrainer on the device (tiny cfg, the fixture batch with different images per step, as
tests/test_grad_accum_train_gpu.py sets them up): off is off, the first Adam step of the log-variances, inactive terms, the guard,
accumulation, captured == eager, full-state resume, key mismatch, a head-only phase, and the data-parallel code path at world size 1.
Every comparison of device state is bit for bit."""
import copy
import os

import numpy as np
import pytest
import torch

from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu

LR_S = 0.05
NAMES = ("loss_seg", "loss_det_cls", "loss_det_reg", "loss_lane_cls_pos", "loss_lane_cls_neg", "loss_lane_loc")


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
    g = torch.Generator().manual_seed(5)
    loader = []
    for i in range(6):
        b = dict(batch)
        b["image"] = batch["image"] + 0.05 * torch.randn(batch["image"].shape, generator=g)
        loader.append(b)
    return z, cfgs, loader


def fresh(b):
    return {k: v.clone() for k, v in b.items()}


def make_trainer(tiny, capture=False, distribute=False, balance=True, **keys):
    from multitask_hydranet_amd.train import HydraTrainer
    z, cfgs, loader = tiny
    cfgs = copy.deepcopy(cfgs)
    if balance:
        cfgs["train"].update(dict(loss_balance="uncertainty", loss_balance_lr=LR_S))
    cfgs["train"].update(keys)
    tr = HydraTrainer(cfgs, trainloader=loader, validloader=None, iters_per_epoch=len(loader), capture_step=capture, force_distribute=distribute)
    tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    return tr


def bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().contiguous()


def params_of(tr):
    return {n: bits(p).clone() for n, p in tr.hydranet.named_parameters()}


def balance_of(tr):
    """bit patterns of the log-variances and their two moments, on the host"""
    s = tr.hydranet.loss_log_vars
    st = tr.balance_optimizer.state[s]
    return {k: bits(t).cpu().clone() for k, t in (("s", s), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"]))}


def same(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[n], b[n]) for n in a)


def differing(a, b):
    return [n for n in a if not torch.equal(a[n], b[n])]


def step(tr, b):
    return {k: float(v) for k, v in tr.train_step(fresh(b)).items()}


def static_weights(cfgs):
    d, l = cfgs["detection"], cfgs["lane"]
    return [cfgs["segment"]["segment_weight"], d["loss_cls_weight"] * d["detection_weight"], d["loss_reg_weight"] * d["detection_weight"],
            l["loss_cls_pos_weight"] * l["lane_weight"], l["loss_cls_neg_weight"] * l["lane_weight"], l["loss_loc_weight"] * l["lane_weight"]]


def test_key_absent_is_the_trainer_without_the_feature(tiny):
    """the same cfg minus the key, and 'none': no log-variances, no second optimizer, hn_weighted_sum's launches -- and three steps end
    on the same bits, which at s = 0 and a zero learning rate's worth of movement is also what the balanced path's first forward gives"""
    runs = []
    for keys in ({}, dict(loss_balance="none")):
        tr = make_trainer(tiny, balance=False, **keys)
        assert tr.balance_optimizer is None and tr.hydranet.loss_log_vars is None and tr.hydranet.loss_balance is None
        losses = [step(tr, b) for b in tiny[2][:3]]
        grads = {n: bits(p.grad).clone() for n, p in tr.hydranet.named_parameters() if p.grad is not None}
        runs.append((losses, grads, params_of(tr)))
        keys_off = list(tr.hydranet.state_dict())
    assert runs[0][0] == runs[1][0] and same(runs[0][1], runs[1][1]) and same(runs[0][2], runs[1][2])
    # with the key on, step 1 starts from s = 0: its loss and every gradient are the static path's bit for bit
    tr = make_trainer(tiny)
    assert list(tr.hydranet.state_dict()) == keys_off         # neither a parameter nor a buffer: the same keys
    assert len(list(tr.hydranet.parameters())) == len(list(make_trainer(tiny, balance=False).hydranet.parameters()))
    off = make_trainer(tiny, balance=False)
    l_on, l_off = step(tr, tiny[2][0]), step(off, tiny[2][0])
    assert l_on == l_off
    g_on = {n: bits(p.grad).clone() for n, p in tr.hydranet.named_parameters() if p.grad is not None}
    g_off = {n: bits(p.grad).clone() for n, p in off.hydranet.named_parameters() if p.grad is not None}
    assert same(g_on, g_off), differing(g_on, g_off)[:5]
    assert same(params_of(tr), params_of(off))


def test_first_step_moves_every_active_term_by_the_learning_rate(tiny):
    tr = make_trainer(tiny)
    z0 = balance_of(tr)
    assert not z0["s"].any() and not z0["m"].any()
    losses = step(tr, tiny[2][0])
    s = tr.hydranet.loss_log_vars.cpu().numpy().astype(np.float64)
    cw = static_weights(tr.cfgs)
    info = tr.hydranet.loss_balance
    assert list(info) == list(NAMES)
    print("losses", losses, "s after one step", s)
    for i, name in enumerate(NAMES):
        L = losses[name]
        assert info[name][2] == (L != 0.0)
        if L == 0.0:
            assert s[i] == 0.0
            continue
        # ds = 1 - c L gw: above 1 the term's weight must shrink, so s grows; Adam's first step has size lr (eps = 1e-8 against |ds|)
        want = np.sign(cw[i] * L - 1.0)
        assert np.sign(s[i]) == want, (name, s[i], cw[i] * L)
        assert abs(abs(s[i]) - LR_S) <= 1e-6 * LR_S, (name, s[i])
    assert "balance" in tr.loss_balance_line()


def test_masked_task_keeps_its_slots(tiny):
    """task_valid with no image labelled for detection: both det losses are exactly 0, their slots and moments keep their bits"""
    tr = make_trainer(tiny)
    step(tr, tiny[2][0])
    step(tr, tiny[2][1])                                 # moments exist and differ from 0
    before = balance_of(tr)
    b = fresh(tiny[2][2])
    n = b["image"].shape[0]
    tv = torch.ones((3, n), dtype=torch.uint8)
    tv[1] = 0                                            # rows: seg, det, lane
    b["task_valid"] = tv
    losses = {k: float(v) for k, v in tr.train_step(b).items()}
    assert losses["loss_det_cls"] == 0.0 and losses["loss_det_reg"] == 0.0 and losses["loss_seg"] != 0.0
    after = balance_of(tr)
    for k in before:
        assert torch.equal(before[k][1:3], after[k][1:3]), k
        moved = (before[k] != after[k]).tolist()
        assert moved[0] and all(moved[3:]), (k, moved)
    info = tr.hydranet.loss_balance
    assert not info["loss_det_cls"][2] and not info["loss_det_reg"][2] and info["loss_seg"][2]


def nan_lane_target(b):
    b = fresh(b)
    row = (b["gt_cls"][..., 1] > 0).nonzero()[0]
    b["gt_loc"][row[0], row[1], 0] = float("nan")
    return b


def test_skipped_step_leaves_the_log_variances_alone(tiny):
    tr = make_trainer(tiny, skip_nonfinite=True)
    step(tr, tiny[2][0])
    before, p0 = balance_of(tr), params_of(tr)
    tr.train_step(nan_lane_target(tiny[2][1]))
    r = tr.optimizer.grad_guard_record()
    assert r["skip"] != 0 and r["skipped"] == 1, r
    assert same(balance_of(tr), before) and same(params_of(tr), p0)
    step(tr, tiny[2][2])
    assert tr.optimizer.grad_guard_record()["skip"] == 0
    assert sorted(differing(balance_of(tr), before)) == ["m", "s", "v"]


def test_accumulation_steps_once_per_group_on_the_mean(tiny):
    tr = make_trainer(tiny, accum_steps=2)
    z0 = balance_of(tr)
    step(tr, tiny[2][0])
    assert same(balance_of(tr), z0)                      # micro-batch 1: nothing stepped
    ds1 = tr.hydranet.loss_log_vars_grad.cpu().numpy().copy()
    step(tr, tiny[2][1])
    ds2 = tr.hydranet.loss_log_vars_grad.cpu().numpy().copy()
    one = balance_of(tr)
    assert differing(one, z0) and int(tr.balance_optimizer.state[tr.hydranet.loss_log_vars]["step"]) == 1
    # the mean as hn_grad_accum forms it (acc + (g - acc) * (float)(1 / 2)), then Adam's first step: m = (1 - beta1) * mean
    mean = (ds1 + (ds2 - ds1) * np.float32(0.5)).astype(np.float32)
    m = one["m"].view(torch.float32).numpy()
    want = np.float32(1.0 - 0.9) * mean                      # exp_avg.lerp_(grad, 1 - beta1) from 0
    np.testing.assert_allclose(m, want, rtol=1e-6)
    assert (np.sign(one["s"].view(torch.float32).numpy()) == -np.sign(mean)).all()
    step(tr, tiny[2][2])
    assert same(balance_of(tr), one)


@pytest.fixture(scope="module")
def eager_run(tiny):
    tr = make_trainer(tiny)
    trace = []
    for b in tiny[2][:5]:
        losses = step(tr, b)
        trace.append(dict(losses=losses, params=params_of(tr), balance=balance_of(tr)))
    return trace


def test_captured_equals_eager(tiny, eager_run):
    tr = make_trainer(tiny, capture=True)
    for i, b in enumerate(tiny[2][:5]):
        assert step(tr, b) == eager_run[i]["losses"], i
        assert same(balance_of(tr), eager_run[i]["balance"]), i
    assert tr._cap is not None
    assert same(params_of(tr), eager_run[4]["params"])


def test_resume_is_bit_for_bit(tiny, eager_run, tmp_path):
    path = str(tmp_path / "state.bin")
    a = make_trainer(tiny)
    for b in tiny[2][:3]:
        step(a, b)
    a.save_state(path)
    b_ = make_trainer(tiny, loss_balance_init=1.5)       # a fresh trainer, its log-variances elsewhere
    b_.load_state(path)
    assert same(balance_of(b_), eager_run[2]["balance"])
    for i in (3, 4):
        assert step(b_, tiny[2][i]) == eager_run[i]["losses"], i
    assert same(balance_of(b_), eager_run[4]["balance"]) and same(params_of(b_), eager_run[4]["params"])
    assert int(b_.balance_optimizer.state[b_.hydranet.loss_log_vars]["step"]) == 5


def test_key_mismatch_is_refused_and_changes_nothing(tiny, tmp_path):
    with_key, without = str(tmp_path / "with.bin"), str(tmp_path / "without.bin")
    on, off = make_trainer(tiny), make_trainer(tiny, balance=False)
    step(on, tiny[2][0])
    step(off, tiny[2][0])
    on.save_state(with_key)
    off.save_state(without)
    for tr, path in ((on, without), (off, with_key)):
        p0 = params_of(tr)
        b0 = balance_of(tr) if tr.balance_optimizer is not None else None
        with pytest.raises(ValueError, match="loss_balance"):
            tr.load_state(path)
        assert same(params_of(tr), p0)
        assert b0 is None or same(balance_of(tr), b0)
    # the reference-format file has the parent's keys
    on.save(str(tmp_path / "w.pth"))
    off.save(str(tmp_path / "w_off.pth"))
    assert list(torch.load(str(tmp_path / "w.pth"))) == list(torch.load(str(tmp_path / "w_off.pth")))


def test_head_only_phase_leaves_the_other_slots_alone(tiny):
    tr = make_trainer(tiny)
    step(tr, tiny[2][0])
    tr.set_phase("seg")
    before = balance_of(tr)
    step(tr, tiny[2][1])
    assert list(tr.hydranet.loss_balance) == ["loss_seg"]
    after = balance_of(tr)
    for k in before:
        assert torch.equal(before[k][1:], after[k][1:]) and before[k][0] != after[k][0], k
    tr.set_phase("joint")
    step(tr, tiny[2][2])
    now = balance_of(tr)
    assert all((now[k] != after[k]).all() for k in now)


def test_data_parallel_code_path_at_world_size_one(tiny, eager_run):
    """force_distribute + capture_step: the gradient-and-activity vector is averaged by a collective of its own with the last bucket
    (in the hipGraph once captured) -- over one rank the identity"""
    import socket
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(so.getsockname()[1])
    tr = make_trainer(tiny, capture=True, distribute=True)
    assert tr.reducer.extras and tr.reducer.extras[0] is tr.hydranet.loss_balance_grad_act
    for i, b in enumerate(tiny[2][:4]):
        assert step(tr, b) == eager_run[i]["losses"], i
    torch.cuda.synchronize()
    assert tr._cap is not None
    assert same(balance_of(tr), eager_run[3]["balance"]) and same(params_of(tr), eager_run[3]["params"])
