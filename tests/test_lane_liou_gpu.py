"""The lane line-IoU location loss (lane.loss_loc_type: liou, csrc/hn_lane_liou.hip) on the device, held to the float64
reference of tests/lane_liou_ref.py: the C entry points on guarded buffers, degenerate inputs, the ops layer with and without a task
mask, the module with and without the cfg key, and the trainer (captured == eager; accumulation, save_state / load_state).

Bounds: loss, pos_liou and gradient within 2e-5 * max(|ref|, 1) of float64, the bound of the lane losses in tests/test_loss_exact_gpu.py
(tests/test_lane_liou_cpu.py shows an fp32 evaluation in the kernels' order uses under 1 % of it); the row normaliser exact; elements
that must be 0 are +0.0 bit for bit."""
import copy

import numpy as np
import pytest
import torch

from tests import lane_liou_ref as R
from tests.guards import Guarded, dev
from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu

BOUND = 2e-5
GOUT = 1.7


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def K(lib):
    from multitask_hydranet_amd import ops
    return ops


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def within(got, want, name):
    """|got - want| <= BOUND * max(|want|, 1), element by element; prints the largest share of the bound in use"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    used = float((np.abs(got - want) / (BOUND * np.maximum(np.abs(want), 1.0))).max()) if got.size else 0.0
    print(f"{name}: {100 * used:.2f} % of the bound")
    assert used <= 1.0, f"{name}: error is {used:.3f} x the bound of {BOUND:g} * max(|ref|, 1)"


def run(lib, p, t, pmask, posn, P, e, gout=GOUT):
    """hn_lane_liou_loss_fwd + _bwd on guarded outputs -> dict of host arrays (every guard checked)"""
    M, L = p.shape
    pd, td, pm = to_dev(p), to_dev(t), to_dev(np.asarray(pmask).astype(np.uint8))
    aux = to_dev(np.array([0.0, posn, pmask.sum(), (~np.asarray(pmask, bool)).sum()], np.float32))
    ws = {nm: Guarded(1, M) for nm in ("rowI", "rowU", "rownorm", "rowloss")}
    out = torch.full((2,), float("nan"), device=dev())
    lib.call("hn_lane_liou_loss_fwd", pd.data_ptr(), td.data_ptr(), pm.data_ptr(), aux.data_ptr(), M, L, P, float(e), 10.0, ws["rowI"].ptr(),
             ws["rowU"].ptr(), ws["rownorm"].ptr(), ws["rowloss"].ptr(), out.data_ptr())
    g = to_dev(np.array([gout], np.float32))
    dp = Guarded(M, L)
    lib.call("hn_lane_liou_loss_bwd", pd.data_ptr(), td.data_ptr(), pm.data_ptr(), ws["rowU"].ptr(), ws["rownorm"].ptr(), aux.data_ptr(),
             g.data_ptr(), M, L, P, float(e), 10.0, dp.ptr())
    torch.cuda.synchronize()
    res = {nm: w.view.cpu().numpy()[0].copy() for nm, w in ws.items()}
    res.update(out=out.cpu().numpy(), dpred=dp.view.cpu().numpy().copy())
    for nm, w in ws.items():
        w.check(nm)
    dp.check("dpred")
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# the C entry points
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [0.5, 1.875])
@pytest.mark.parametrize("P,M", [(1, 203), (16, 37), (32, 203), (160, 37)])
def test_entry_points_against_float64(lib, P, M, e):
    """L = 4 (one column per part), 34 (fewer columns than lanes), 66 (one trip and a remainder), 322 (many trips); M % 8 != 0"""
    p, t, pmask, posn = R.lane_liou_case(P, M, 0)
    loss, liou, grad, I, U, nrm = R.lane_liou(p, t, pmask, posn, P, e, gout=GOUT)
    got = run(lib, p, t, pmask, posn, P, e)
    what = f"P={P} M={M} e={e}"
    within(got["out"][0], loss, what + " loss")
    within(got["out"][1], liou, what + " pos_liou")
    within(got["dpred"], grad, what + " dpred")
    within(got["rowI"], I, what + " rowI")
    within(got["rowU"], U, what + " rowU")
    assert (got["rownorm"] == nrm).all(), what
    zero = np.broadcast_to(~pmask[:, None], t.shape) | (t == 0)
    assert (bits(got["dpred"][zero]) == 0).all(), what + ": an element that must be +0.0 is not"
    xc = R.x_columns(P)
    assert (bits(got["dpred"][4][xc]) == 0).all() and got["rowI"][4] == got["rowU"][4] > 0              # liou = 1 exactly
    assert got["rowI"][5] < 0 and (bits(got["rowU"][~pmask]) == 0).all() and (bits(got["rowloss"][~pmask]) == 0).all()
    assert bits(got["rowU"][3]) == 0 and bits(got["rowU"][8]) == 0 and bits(got["rowloss"][8]) == 0     # no valid x-column


def test_no_positive_row(lib):
    P, M = 16, 37
    p, t, _, _ = R.lane_liou_case(P, M, 1)
    got = run(lib, p, t, np.zeros(M, bool), 1.0, P, 1.875)
    assert bits(got["out"][0]) == 0 and bits(got["out"][1]) == 0 and (bits(got["dpred"]) == 0).all()
    assert (got["rownorm"] == np.maximum((t != 0).sum(1), 1)).all()


def test_two_runs_give_the_same_bits(lib):
    P, M = 32, 203
    p, t, pmask, posn = R.lane_liou_case(P, M, 2)
    a, b = run(lib, p, t, pmask, posn, P, 0.5), run(lib, p, t, pmask, posn, P, 0.5)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------------------------------------------
# ops layer
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [None, (1, 0, 1, 0)], ids=["unmasked", "masked"])
def test_ops_layer_follows_the_cls_loss(K, mask):
    """4 images x 25 rows; with the mask images 1 and 3 are unlabelled: the labelled sub-batch's loss, exact zeros elsewhere"""
    N, rows, P, e = 4, 25, 16, 1.875
    M = N * rows
    p, t, pos, _ = R.lane_liou_case(P, M, 3)
    g = np.random.default_rng(5)
    z = torch.from_numpy((g.standard_normal((N, rows, 2)) * 2).astype(np.float32)).to(dev()).requires_grad_(True)
    ct = torch.from_numpy(np.stack([~pos, pos], 1).astype(np.float32)).to(dev()).view(N, rows, 2)
    lt = to_dev(t).view(N, rows, 2 * P + 2)
    lp = to_dev(p).view(N, rows, 2 * P + 2).requires_grad_(True)
    kw = {} if mask is None else dict(valid=torch.tensor(list(mask), dtype=torch.uint8, device=dev()), rows_per_image=rows)
    cpos, cneg, pmask, aux = K.lane_cls_loss_hip(ct, z, **kw)
    loss, liou = K.lane_liou_loss_hip(pmask, aux, lt, lp, e, **kw)
    assert loss.shape == () and liou.shape == () and loss.requires_grad and not liou.requires_grad
    (dp,) = torch.autograd.grad(loss * GOUT, lp)
    keep = np.repeat(np.array(mask if mask is not None else (1,) * N, bool), rows)
    sub = pos & keep
    assert (pmask.cpu().numpy().astype(bool) == sub).all() and sub.sum() > 0 and (pos & ~keep).sum() > (0 if mask else -1)
    want, want_liou, grad, *_ = R.lane_liou(p[keep], t[keep], pos[keep], float(max(sub.sum(), 1)), P, e, gout=GOUT)
    within(float(loss.detach()), want, "ops loss")
    within(float(liou), want_liou, "ops pos_liou")
    d = dp.cpu().numpy().reshape(M, -1)
    within(d[keep], grad, "ops dpred")
    assert (bits(d[~keep]) == 0).all(), "an unlabelled image's rows have a gradient"
    if mask is not None:
        with pytest.raises(ValueError):
            K.lane_liou_loss_hip(pmask, aux, lt, lp, e, valid=kw["valid"], rows_per_image=7)
    with pytest.raises(ValueError, match="points_per_line"):
        K.lane_liou_loss_hip(pmask, aux, lt, lp, e, points_per_line=15)


# ------------------------------------------------------------------------------------------------------------------------------------
# module
# ------------------------------------------------------------------------------------------------------------------------------------
def tiny_net(loc_type):
    from multitask_hydranet_amd import HydraNet
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    if loc_type is not None:
        cfgs["lane"]["loss_loc_type"] = loc_type
    net = HydraNet(cfgs)
    net.load_state_dict(tiny_state(z))
    net = net.to(dev()).train()
    net.lane_points_per_line = int(z["meta/lane_points_per_line"])
    batch = {k[3:]: torch.from_numpy(z[k].copy()).to(dev()) for k in z.files if k.startswith("in/")}
    return net, batch, cfgs


def test_module_trains_the_lane_head_on_liou(K):
    net, batch, cfgs = tiny_net("liou")
    out = net(batch["image"])
    ld = net.cal_loss(out, batch)
    plain, _, _ = tiny_net(None)
    assert sorted(ld) == sorted(plain.cal_loss(plain(batch["image"]), batch))            # the keys of loss_dict do not change
    pl = out["lane"]["predict_loc"]
    L = pl.shape[-1]
    P = (L - 2) // 2
    e = 15.0 / cfgs["lane"]["interval"]
    assert P == cfgs["dataloader"]["network_input_height"] // cfgs["lane"]["interval"] and net.lane_liou_half_width == e
    p = pl.detach().float().cpu().numpy().reshape(-1, L)
    t = batch["gt_loc"].cpu().numpy().reshape(-1, L)
    pmask = batch["gt_cls"].cpu().numpy().reshape(-1, 2)[:, 1] > 0
    assert pmask.sum() > 0
    want, want_liou, grad, *_ = R.lane_liou(p, t, pmask, float(max(pmask.sum(), 1)), P, e)
    got, got_liou = float(ld["loss_lane_loc"].detach()), net.lane_pos_liou
    assert got_liou.shape == () and got_liou.is_cuda and not got_liou.requires_grad
    print(f"module: loss_lane_loc {got:.7f} / {want:.7f}  lane_pos_liou {float(got_liou):.6f} / {want_liou:.6f}  positives {int(pmask.sum())}")
    within(got, want, "module loss_lane_loc")
    within(float(got_liou), want_liou, "module lane_pos_liou")
    (dp,) = torch.autograd.grad(ld["loss_lane_loc"], pl, retain_graph=True)
    within(dp.float().cpu().numpy().reshape(-1, L), grad, "module d loss_lane_loc / d predict_loc")
    net.total_loss(ld).backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for n, q in net.named_parameters() if n.startswith("laneheader."))
    assert any(bool((q.grad != 0).any()) for n, q in net.named_parameters() if n.startswith("laneheader.conv_up_conv.3"))


def test_without_the_key_nothing_changes(K):
    net, batch, _ = tiny_net(None)
    out = net(batch["image"])
    ld = net.cal_loss(out, batch)
    assert net.lane_pos_liou is None and net.loss_reg is K.lane_loc_loss_hip
    pl = out["lane"]["predict_loc"]
    (dp,) = torch.autograd.grad(ld["loss_lane_loc"], pl)
    with torch.no_grad():
        _, _, pmask, aux = K.lane_cls_loss_hip(batch["gt_cls"], out["lane"]["predict_cls"].detach())
    leaf = pl.detach().clone().requires_grad_(True)
    want = K.lane_loc_loss_hip(pmask, aux, batch["gt_loc"], leaf, points_per_line=net.lane_points_per_line)
    (dw,) = torch.autograd.grad(want, leaf)
    assert torch.equal(ld["loss_lane_loc"].detach().view(torch.int32), want.detach().view(torch.int32))
    assert torch.equal(dp.contiguous().view(torch.int32), dw.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------------
# trainer: capture, accumulation, checkpoints
# ------------------------------------------------------------------------------------------------------------------------------------
def fresh(b):
    return {k: v.clone() for k, v in b.items()}


def make_trainer(capture, weights=True, seed=0, **train_keys):
    from multitask_hydranet_amd.train import HydraTrainer
    z = load_npz("tiny_hydranet.npz")
    cfgs = copy.deepcopy(load_cfg("hydranet_tiny.yml"))
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0), **train_keys)
    cfgs["lane"]["loss_loc_type"] = "liou"
    if not weights:
        torch.manual_seed(seed)
    tr = HydraTrainer(cfgs, trainloader=None, validloader=None, iters_per_epoch=8, capture_step=capture)
    if weights:
        tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    return tr


@pytest.fixture(scope="module")
def batch():
    z = load_npz("tiny_hydranet.npz")
    return {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}


def test_captured_step_replays_the_eager_bits(K, batch):
    """forward + cal_loss + backward as one hipGraph (HydraTrainer(capture_step=True): iterations 3 and 4 are replays), lr = 0 so that
    every iteration sees the same inputs and weights: both replays give the eager iterations' bits"""
    seen = {}
    for capture in (False, True):
        tr = make_trainer(capture, lr=0.0)
        steps = []
        for _ in range(4):
            ld = tr.train_step(fresh(batch))
            steps.append(({k: v.detach().clone() for k, v in ld.items()}, tr.hydranet.lane_pos_liou.clone(),
                          {n: q.grad.detach().clone() for n, q in tr.hydranet.named_parameters() if n.startswith("laneheader.") and q.grad is not None}))
        assert (tr._cap is not None) == capture
        seen[capture] = steps
    eager, cap = seen[False], seen[True]
    assert float(eager[0][0]["loss_lane_loc"]) > 0 and 0.0 < float(eager[0][1]) <= 1.0 and len(eager[0][2]) > 0
    for i in range(4):
        for k in eager[0][0]:
            assert torch.equal(cap[i][0][k], eager[0][0][k]) and torch.equal(eager[i][0][k], eager[0][0][k]), (i, k)
        assert torch.equal(cap[i][1], eager[0][1]), i
        assert sorted(cap[i][2]) == sorted(eager[0][2])
        for n in eager[0][2]:
            assert torch.equal(cap[i][2][n], eager[0][2][n]), (i, n)


def test_trainer_accumulates_saves_and_resumes_under_liou(K, batch, tmp_path):
    g = torch.Generator().manual_seed(3)
    loader = []
    for i in range(6):
        b = dict(batch)
        b["image"] = batch["image"] + 0.05 * torch.randn(batch["image"].shape, generator=g)
        loader.append(b)
    a = make_trainer(True, accum_steps=2)
    before = {n: q.detach().clone() for n, q in a.hydranet.named_parameters()}
    for b in loader[:4]:
        losses = a.train_step(fresh(b))
        assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
        assert float(losses["loss_lane_loc"]) > 0
    assert a._cap is not None and a.accumulator is not None and a.accumulator.pending == 0
    assert -1.0 < float(a.hydranet.lane_pos_liou) <= 1.0
    changed = [n for n, q in a.hydranet.named_parameters() if not torch.equal(q.detach(), before[n])]
    assert any(n.startswith("laneheader.conv_up_conv") for n in changed) and any(n.startswith("laneheader.conv_down_conv") for n in changed)
    path = str(tmp_path / "liou.hn")
    a.save_state(path)
    want = [{k: v.clone() for k, v in a.train_step(fresh(b)).items()} for b in loader[4:]]
    c = make_trainer(True, weights=False, seed=1234, accum_steps=2)
    c.load_state(path)
    got = [c.train_step(fresh(b)) for b in loader[4:]]
    for w_, g_ in zip(want, got):
        assert sorted(g_) == sorted(w_)
        for k in w_:
            assert torch.equal(g_[k], w_[k]), (k, float(g_[k]), float(w_[k]))
    for (n1, q1), (n2, q2) in zip(a.hydranet.named_parameters(), c.hydranet.named_parameters()):
        assert n1 == n2 and torch.equal(q1, q2), n1
