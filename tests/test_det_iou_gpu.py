"""GPU: the IoU-family box regression losses (detection.loss_reg_type = giou | diou | ciou; csrc/hn_det_loss.hip) against the float64
restatement tests/det_iou_ref.py.  Bounds are the project's for the smooth-L1 detection loss (test_det_loss_matches_reference_loop):
losses 2e-5 relative, dcls / dreg 2e-4 of the reference's maximum; tests/test_det_iou_cpu.py measures what float32 alone costs on the
same inputs (1e-7 / 5e-7).  The classification half must keep hn_det_loss_fwd/bwd's bits."""
import copy
import math

import pytest
import torch

from tests import det_iou_ref as R
from tests.helpers import load_cfg, load_npz, tiny_state
from tests.test_kernels_gpu import close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KIND_ID = {"giou": 1, "diou": 2, "ciou": 3}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops
    return ops


def reference(cls, reg, anc, ann, kind, reg_weight=50.0):
    """float64 losses and gradients of cls + reg_weight * reg (the weighting of test_det_loss_matches_reference_loop)"""
    c, r = cls.double().requires_grad_(True), reg.double().requires_grad_(True)
    out = R.det_iou_loss(c, r, anc, ann, kind)
    (out["cls"].sum() + reg_weight * out["reg"]).backward()
    out.update(cls=float(out["cls"].detach()), reg=float(out["reg"].detach()), pos_iou=float(out["pos_iou"]), dcls=c.grad,
               dreg=r.grad if r.grad is not None else torch.zeros_like(r))
    return out


def hip(K, cls, reg, anc, ann, kind, reg_weight=50.0):
    c, r = cls.clone().to(DEV).requires_grad_(True), reg.clone().to(DEV).requires_grad_(True)
    lc, lr, iou = K.det_iou_loss_hip(c, r, anc.to(DEV), ann.to(DEV), kind)
    assert not iou.requires_grad and iou.grad_fn is None
    (lc.sum() + reg_weight * lr.sum()).backward()
    return dict(cls=float(lc.detach()), reg=float(lr.detach()), pos_iou=float(iou), dcls=c.grad.cpu(), dreg=r.grad.cpu())


def compare(got, ref, what, grads=True):
    print(f"{what}: cls {got['cls']:.7f} / {ref['cls']:.7f}  reg {got['reg']:.7f} / {ref['reg']:.7f}  pos_iou {got['pos_iou']:.6f} / "
          f"{ref['pos_iou']:.6f}  npos {ref['npos']}  margin {ref['margin']:.3e}  max|dreg err| / max "
          f"{float((got['dreg'].double() - ref['dreg']).abs().max()) / max(float(ref['dreg'].abs().max()), 1e-30):.2e}")
    for k in ("cls", "reg", "pos_iou"):
        assert abs(got[k] - ref[k]) <= 2e-5 * max(abs(ref[k]), 1e-6), (what, k, got[k], ref[k])
    assert math.isfinite(got["reg"]) and bool(torch.isfinite(got["dreg"]).all()) and bool(torch.isfinite(got["dcls"]).all())
    if grads:
        assert ref["margin"] > 1e-3, (what, ref["margin"])             # no min / max / clamp tie anywhere: the gradient is unambiguous
        close(got["dcls"], ref["dcls"], 2e-4, what + " dcls")
        close(got["dreg"], ref["dreg"], 2e-4, what + " dreg")


# ------------------------------------------------------------------------------------------------------------------------------------
# the recorded KAT inputs (6138 anchors, 71 / 35 / 0 positives), regressions x1 and x8, and an annotation tensor without any match
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kats():
    z = load_npz("loss_kats.npz")
    t = lambda k: torch.from_numpy(z[k])
    cls = (t("det/cls") * 4.5).clamp(0, 1)                              # spread over (0, 0.9]: exercises both focal branches and the clamp
    cls[0, :50] = 0.0
    cls[0, 50:100] = 1.0
    return dict(cls=cls, reg=t("det/reg"), anc=t("det/anchors"), ann=t("det/ann"))


@pytest.mark.parametrize("case", ["x1", "x8", "ones"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_values_and_gradients_on_the_recorded_inputs(K, kats, kind, case):
    reg = kats["reg"] * (8.0 if case == "x8" else 1.0)
    ann = torch.ones(3, 16, 5) if case == "ones" else kats["ann"]
    ref = reference(kats["cls"], reg, kats["anc"], ann, kind)
    assert ref["npos"] == ([0, 0, 0] if case == "ones" else [71, 35, 0])
    got = hip(K, kats["cls"], reg, kats["anc"], ann, kind)
    compare(got, ref, f"{kind} {case}", grads=case != "ones")
    assert bool((got["dreg"][2] == 0).all())                            # the image without positives
    if case == "ones":
        assert got["reg"] == 0.0 and got["pos_iou"] == 0.0 and bool((got["dreg"] == 0).all())
        close(got["dcls"], ref["dcls"], 2e-4, "dcls")


@pytest.mark.parametrize("kind", R.KINDS)
def test_an_image_without_positives_alone(K, kats, kind):
    got = hip(K, kats["cls"][2:3], kats["reg"][2:3], kats["anc"], kats["ann"][2:3], kind)
    assert got["reg"] == 0.0 and got["pos_iou"] == 0.0 and bool((got["dreg"] == 0).all()) and got["cls"] > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# tail shapes: A on both sides of the 256-anchor block, one and nine classes
# ------------------------------------------------------------------------------------------------------------------------------------
def grid_anchors(levels=((32, 128.0), (16, 64.0), (8, 32.0)), hw=(128, 256), ratios=((1.0, 1.0), (0.7, 1.4), (1.4, 0.7))):
    """(y1, x1, y2, x2) anchors of a small multi-scale grid, coarse level first; stride = size / 4, so a box has several positives"""
    out = []
    for stride, size in levels:
        for y in range(stride // 2, hw[0], stride):
            for x in range(stride // 2, hw[1], stride):
                for rh, rw in ratios:
                    out.append([y - size * rh / 2, x - size * rw / 2, y + size * rh / 2, x + size * rw / 2])
    return torch.tensor(out, dtype=torch.float32)


THIN = 7                                                               # this anchor is replaced by one 0.8 px wide


def tail_case(A, Kc):
    g = torch.Generator().manual_seed(1000 * A + Kc)
    anc = grid_anchors()[:A].clone()
    assert anc.shape[0] == A
    anc[THIN] = torch.tensor([40.0, 100.0, 72.0, 100.8])
    src = [3, 40, 77, 120, 150, 181, 215, 250, 20, 60, 100, 140, 200]  # anchors the boxes are perturbed copies of (all < 255)
    ann = torch.full((3, 8, 5), -1.0)

    def box(i, n_cls):
        y1, x1, y2, x2 = anc[i].tolist()
        h, w = y2 - y1, x2 - x1
        d = (torch.rand(4, generator=g) - 0.5) * 0.12                  # corners move by up to 6 % of the side: IoU with the anchor > 0.75
        return torch.tensor([x1 + d[0] * w, y1 + d[1] * h, x2 + d[2] * w, y2 + d[3] * h, float(torch.randint(0, n_cls, (1,), generator=g))])
    for j in range(5):
        ann[0, j] = box(src[j], Kc)
    for j in range(7):
        ann[1, j] = box(src[5 + j], Kc)
    ann[1, 7] = torch.tensor([100.1, 40.0, 100.6, 72.0, 0.0])           # 0.5 px wide: IoU 0.625 with the thin anchor, gw clamps to 1
    cls = torch.rand(3, A, Kc, generator=g) * 0.98 + 0.01
    reg = torch.randn(3, A, 4, generator=g) * 0.2
    # rows forced onto known positives of image 0 (the anchors its boxes were copied from)
    reg[0, src[0]] = torch.tensor([0.05, 3.0, 0.1, -0.1])              # dx = 3: the prediction is disjoint from its target
    reg[0, src[1]] = torch.tensor([0.1, -0.05, 5.0, 0.2])              # dh above the clip
    reg[0, src[2]] = torch.tensor([-0.1, 0.1, -3.0, 0.05])             # a very flat prediction
    return cls, reg, anc[None], ann, src


@pytest.mark.parametrize("Kc", [1, 9])
@pytest.mark.parametrize("A", [255, 256, 257, 600])
@pytest.mark.parametrize("kind", R.KINDS)
def test_tail_shapes(K, kind, A, Kc):
    cls, reg, anc, ann, src = tail_case(A, Kc)
    ref = reference(cls, reg, anc, ann, kind, reg_weight=1.0)
    assert ref["npos"][0] >= 8 and ref["npos"][1] >= 8 and ref["npos"][2] == 0, ref["npos"]
    a64 = anc[0].double()
    pos0, arg0 = R.assign(a64, ann[0].double())
    pos1, arg1 = R.assign(a64, ann[1].double())
    assert all(bool(pos0[src[j]]) and int(arg0[src[j]]) == j for j in range(3))
    assert bool(pos1[THIN]) and int(arg1[THIN]) == 7                    # the clamp of the annotation's width is on the path
    _, iou_d, _ = R.box_losses(reg[0, src[0]][None].double(), a64[src[0]][None], ann[0, 0, :4][None].double(), kind)
    assert float(iou_d) == 0.0                                          # the forced row: no overlap with its target at all ...
    assert float(ref["dreg"][0, src[0]].abs().max()) > 1e-3 * float(ref["dreg"].abs().max())     # ... and still pulled towards it
    got = hip(K, cls, reg, anc, ann, kind, reg_weight=1.0)
    compare(got, ref, f"{kind} A={A} K={Kc}")
    assert float(got["dreg"][0, src[0]].abs().max()) > 0
    assert float(got["dreg"][0, src[1], 2]) == 0.0 and float(ref["dreg"][0, src[1], 2]) == 0.0    # exactly zero under the clip
    assert float(got["dreg"][0, src[2], 2]) != 0.0
    assert bool((got["dreg"][2] == 0).all()) and bool((got["dreg"][0][~pos0] == 0).all())


@pytest.mark.parametrize("kind", R.KINDS)
def test_predictions_equal_to_their_targets(K, kind):
    """square, non-overlapping anchors; every box is a copy of an anchor and every regression is zero: each box has one positive whose
    decoded prediction IS the box.  Every min / max ties here, so only the value (0 within 1e-6) and finite gradients are asserted."""
    anc = grid_anchors(levels=((32, 32.0),), ratios=((1.0, 1.0),))      # 4 x 8 anchors
    ann = torch.full((2, 4, 5), -1.0)
    for n, idx in enumerate(((1, 10, 20), (5, 31))):
        for j, i in enumerate(idx):
            y1, x1, y2, x2 = anc[i].tolist()
            ann[n, j] = torch.tensor([x1, y1, x2, y2, 0.0])
    cls = torch.full((2, anc.shape[0], 2), 0.3)
    reg = torch.zeros(2, anc.shape[0], 4)
    ref = R.det_iou_loss(cls, reg, anc, ann, kind)
    assert ref["npos"] == [3, 2] and abs(float(ref["reg"])) < 1e-8
    got = hip(K, cls, reg, anc[None], ann, kind)
    assert abs(got["reg"]) <= 1e-6 and abs(got["pos_iou"] - 1.0) <= 1e-6
    assert bool(torch.isfinite(got["dreg"]).all()) and bool(torch.isfinite(got["dcls"]).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# the classification half keeps the smooth-L1 path's bits; the IoU path repeats its own
# ------------------------------------------------------------------------------------------------------------------------------------
def raw_run(K, name, cls, reg, anc, ann, kind=None):
    """the C entry points themselves -> every tensor they write"""
    from multitask_hydranet_amd._lib import lib
    n, a, k = cls.shape
    cols = 3 if kind is None else 4
    blocks = lib().query("hn_det_loss_blocks", a)
    assign = torch.full((n, a), -7, device=DEV, dtype=torch.int16)
    part = torch.zeros((n, blocks, cols), device=DEV)
    npos = torch.zeros((n,), device=DEV)
    out = torch.zeros((cols - 1,), device=DEV)
    dcls, dreg = torch.full_like(cls, 7.0), torch.full_like(reg, 7.0)
    g = torch.tensor([1.25, 50.0], device=DEV)
    extra = () if kind is None else (KIND_ID[kind],)
    p = K.ptr
    lib().call(name + "_fwd", p(cls), p(reg), p(anc), p(ann), n, a, k, ann.shape[1], *extra, p(assign), p(part), p(npos), p(out))
    lib().call(name + "_bwd", p(cls), p(reg), p(anc), p(ann), n, a, k, ann.shape[1], *extra, p(assign), p(npos), p(g), p(dcls), p(dreg))
    torch.cuda.synchronize()
    return dict(assign=assign, part=part, npos=npos, out=out, dcls=dcls, dreg=dreg)


@pytest.mark.parametrize("kind", R.KINDS)
def test_classification_is_untouched_and_runs_repeat(K, kats, kind):
    inputs = [(kats["cls"], kats["reg"], kats["anc"].reshape(-1, 4), kats["ann"])]
    cls, reg, anc, ann, _ = tail_case(600, 9)
    inputs.append((cls, reg, anc[0], ann))
    for cls, reg, anc, ann in inputs:
        dev_in = [t.to(DEV).contiguous() for t in (cls, reg, anc, ann)]
        base = raw_run(K, "hn_det_loss", *dev_in)
        one = raw_run(K, "hn_det_loss_iou", *dev_in, kind=kind)
        two = raw_run(K, "hn_det_loss_iou", *dev_in, kind=kind)
        assert int(base["npos"].sum()) > 0
        assert torch.equal(one["assign"], base["assign"]) and torch.equal(one["npos"], base["npos"])
        assert torch.equal(one["out"][0], base["out"][0]) and torch.equal(one["dcls"], base["dcls"])
        assert torch.equal(one["part"][..., 0], base["part"][..., 0])
        assert not torch.equal(one["dreg"], base["dreg"])
        for k in one:
            assert torch.equal(one[k], two[k]), k


# ------------------------------------------------------------------------------------------------------------------------------------
# module and trainer
# ------------------------------------------------------------------------------------------------------------------------------------
def tiny_net(kind):
    from multitask_hydranet_amd import HydraNet
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    if kind is not None:
        cfgs["detection"]["loss_reg_type"] = kind
    net = HydraNet(cfgs)
    net.load_state_dict(tiny_state(z))
    net = net.to(DEV).train()
    net.lane_points_per_line = int(z["meta/lane_points_per_line"])
    batch = {k[3:]: torch.from_numpy(z[k].copy()).to(DEV) for k in z.files if k.startswith("in/")}
    return net, batch


def test_module_selects_the_loss_by_the_cfg_key(K):
    plain, batch = tiny_net(None)
    ciou, _ = tiny_net("ciou")
    out_p, out_c = plain(batch["image"]), ciou(batch["image"])
    d = out_p["detection"]
    assert torch.equal(d["classification"], out_c["detection"]["classification"]) and torch.equal(d["regression"], out_c["detection"]["regression"])
    ld_p, ld_c = plain.cal_loss(out_p, batch), ciou.cal_loss(out_c, batch)
    assert sorted(ld_p) == sorted(ld_c)                                 # the keys of loss_dict do not change
    assert plain.det_pos_iou is None and ciou.det_pos_iou.shape == () and ciou.det_pos_iou.is_cuda and not ciou.det_pos_iou.requires_grad
    assert torch.equal(ld_p["loss_det_cls"], ld_c["loss_det_cls"])
    want_c, want_r = K.det_loss_hip(d["classification"].detach(), d["regression"].detach(), d["anchors"], batch["gt_det"])
    assert torch.equal(ld_p["loss_det_reg"], want_r.reshape(())) and torch.equal(ld_p["loss_det_cls"], want_c.reshape(()))
    ref = R.det_iou_loss(d["classification"].detach().cpu(), d["regression"].detach().cpu(), d["anchors"].cpu(), batch["gt_det"].cpu(), "ciou")
    got_r, got_i = float(ld_c["loss_det_reg"].detach()), float(ciou.det_pos_iou)
    print(f"module: ciou {got_r:.7f} / {float(ref['reg']):.7f}  pos_iou {got_i:.6f} / {float(ref['pos_iou']):.6f}  npos {ref['npos']}")
    assert sum(ref["npos"]) > 0
    assert abs(got_r - float(ref["reg"])) <= 2e-5 * abs(float(ref["reg"])) and abs(got_i - float(ref["pos_iou"])) <= 2e-5 * float(ref["pos_iou"])
    tot = ciou.total_loss(ld_c)
    tot.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in ciou.named_parameters() if n.startswith("detectheader."))
    ld_c2 = ciou.cal_loss(ciou(batch["image"]), batch)                  # refreshed on every cal_loss
    assert ciou.det_pos_iou is not None and float(ciou.det_pos_iou) == got_i and float(ld_c2["loss_det_reg"].detach()) == got_r


def make_trainer(kind, loader, weights=True, seed=0):
    from multitask_hydranet_amd.train import HydraTrainer
    z = load_npz("tiny_hydranet.npz")
    cfgs = copy.deepcopy(load_cfg("hydranet_tiny.yml"))
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    cfgs["detection"]["loss_reg_type"] = kind
    if not weights:
        torch.manual_seed(seed)
    tr = HydraTrainer(cfgs, trainloader=loader, validloader=None, iters_per_epoch=len(loader), capture_step=True)
    if weights:
        tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    return tr


def test_trainer_steps_saves_and_resumes_under_giou(K, tmp_path):
    z = load_npz("tiny_hydranet.npz")
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    g = torch.Generator().manual_seed(3)
    loader = []
    for i in range(5):
        b = dict(batch)
        b["image"] = batch["image"] + 0.05 * torch.randn(batch["image"].shape, generator=g)
        loader.append(b)
    fresh = lambda b: {k: v.clone() for k, v in b.items()}
    a = make_trainer("giou", loader)
    before = {n: p.detach().clone() for n, p in a.hydranet.named_parameters()}
    for b in loader[:4]:
        losses = a.train_step(fresh(b))
        assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
        assert float(losses["loss_det_reg"]) > 0
    assert a._cap is not None                                           # the step was captured and replayed
    assert 0.0 < float(a.hydranet.det_pos_iou) <= 1.0
    changed = [n for n, p in a.hydranet.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(changed) > 0.9 * len(before) and any(n.startswith("detectheader.") for n in changed)
    path = str(tmp_path / "giou.hn")
    a.save_state(path)
    want = {k: v.clone() for k, v in a.train_step(fresh(loader[4])).items()}
    c = make_trainer("giou", loader, weights=False, seed=1234)
    c.load_state(path)
    got = c.train_step(fresh(loader[4]))
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (k, float(got[k]), float(want[k]))
