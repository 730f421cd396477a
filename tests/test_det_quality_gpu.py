"""GPU: the quality focal / varifocal detection losses (detection.loss_cls_type = qfl | vfl; csrc/hn_det_loss.hip) against the float64
restatement tests/det_quality_ref.py.  Bounds are the project's for the detection losses (test_det_iou_gpu.py): losses and pos_iou 2e-5
relative, dcls / dreg 2e-4 of the reference's maximum -- and dcls once more over the positive anchors' rows alone, against the maximum
over those rows; tests/test_det_quality_cpu.py measures what float32 alone costs on the same inputs (6e-7 / 1.4e-6).  The regression
half must keep hn_det_loss_iou_fwd/bwd's bits."""
import copy
import math

import pytest
import torch

from tests import det_iou_ref as R
from tests import det_quality_ref as Q
from tests.helpers import load_cfg, load_npz, tiny_state
from tests.test_det_iou_gpu import tail_case
from tests.test_kernels_gpu import close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KIND_ID = {"giou": 1, "diou": 2, "ciou": 3}
CLS_ID = {"qfl": 1, "vfl": 2}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops
    return ops


def reference(cls, reg, anc, ann, kind, cls_kind, reg_weight, assign=None, valid=None):
    """float64 losses and gradients of cls + reg_weight * reg"""
    c, r = cls.double().requires_grad_(True), reg.double().requires_grad_(True)
    out = Q.det_quality_loss(c, r, anc, ann, kind, cls_kind, assign=assign, valid=valid)
    (out["cls"] + reg_weight * out["reg"]).backward()
    out.update(cls=float(out["cls"].detach()), reg=float(out["reg"].detach()), pos_iou=float(out["pos_iou"]), dcls=c.grad, dreg=r.grad)
    return out


def hip(K, cls, reg, anc, ann, kind, cls_kind, reg_weight, assign=None, valid=None):
    c, r = cls.clone().to(DEV).requires_grad_(True), reg.clone().to(DEV).requires_grad_(True)
    lc, lr, iou = K.det_iou_loss_hip(c, r, anc.to(DEV), ann.to(DEV), kind, assign=assign, valid=valid, cls_kind=cls_kind)
    assert not iou.requires_grad and iou.grad_fn is None
    (lc.sum() + reg_weight * lr.sum()).backward()
    return dict(cls=float(lc.detach()), reg=float(lr.detach()), pos_iou=float(iou), dcls=c.grad.cpu(), dreg=r.grad.cpu())


def compare(got, ref, what):
    rows = torch.stack(ref["pos"])
    rel = lambda a, b: float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-30)
    print(f"{what}: cls {got['cls']:.7f} / {ref['cls']:.7f}  reg {got['reg']:.7f} / {ref['reg']:.7f}  pos_iou {got['pos_iou']:.6f} / "
          f"{ref['pos_iou']:.6f}  npos {ref['npos']}  margin {ref['margin']:.3e}  positive rows' share {ref['pos_share']:.4f}  max|err| / max: "
          f"dcls {rel(got['dcls'], ref['dcls']):.2e}  positive rows of dcls "
          f"{rel(got['dcls'][rows], ref['dcls'][rows]) if bool(rows.any()) else 0.0:.2e}  dreg {rel(got['dreg'], ref['dreg']):.2e}")
    for k in ("cls", "reg", "pos_iou"):
        assert abs(got[k] - ref[k]) <= 2e-5 * max(abs(ref[k]), 1e-6), (what, k, got[k], ref[k])
    assert math.isfinite(got["cls"]) and bool(torch.isfinite(got["dreg"]).all()) and bool(torch.isfinite(got["dcls"]).all())
    assert ref["margin"] > 1e-3, (what, ref["margin"])                 # no min / max / clamp tie: q = 0 against q > 0 is unambiguous
    close(got["dcls"], ref["dcls"], 2e-4, what + " dcls")
    close(got["dreg"], ref["dreg"], 2e-4, what + " dreg")
    if bool(rows.any()):
        close(got["dcls"][rows], ref["dcls"][rows], 2e-4, what + " dcls, positive anchors' rows")


# ------------------------------------------------------------------------------------------------------------------------------------
# tail shapes: A on both sides of the 256-anchor block, one and nine classes; as generated and with a quiet background
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quiet", [False, True])
@pytest.mark.parametrize("Kc", [1, 9])
@pytest.mark.parametrize("A", [255, 256, 257, 600])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("cls_kind", Q.CLS_KINDS)
def test_tail_shapes(K, cls_kind, kind, A, Kc, quiet):
    cls, reg, anc, ann, src = tail_case(A, Kc)
    if quiet:
        cls = Q.quiet(cls, anc, ann)
    ref = reference(cls, reg, anc, ann, kind, cls_kind, reg_weight=1.0)
    assert ref["npos"][0] >= 8 and ref["npos"][1] >= 8 and ref["npos"][2] == 0, ref["npos"]
    q0 = ref["q"][0]
    assert int((q0 == 0).sum()) == 1, q0                               # the forced disjoint row: vfl's y = 0 branch for a positive
    # plenty of sizeable targets next to it.  (Image 0 alone has 6 .. 11 positives with q > 0.5 on these inputs, not 15; the batch has
    # 17 .. 29, image 0 has 19 .. 28 with q > 0.3.)
    assert int((q0 > 0.3).sum()) >= 15 and sum(int((q > 0.5).sum()) for q in ref["q"]) >= 15, ref["q"]
    assert float(q0[int(ref["pos"][0][:src[0]].sum())]) == 0.0                    # (it IS the row of src[0])
    if quiet:
        assert ref["pos_share"] >= 0.90, ref["pos_share"]              # the positive branch carries the loss (measured >= 0.94)
    else:
        assert ref["pos_share"] < 0.05                                  # ... which the generated inputs alone would not show (< 1 % there)
    got = hip(K, cls, reg, anc, ann, kind, cls_kind, reg_weight=1.0)
    compare(got, ref, f"{cls_kind} {kind} A={A} K={Kc}{' quiet' if quiet else ''}")
    assert bool((got["dreg"][2] == 0).all()) and bool((got["dreg"][0][~ref["pos"][0]] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# the recorded KAT inputs (6138 anchors, 71 / 35 / 0 positives), regressions x1 and x8
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kats():
    return Q.kat_inputs(load_npz("loss_kats.npz"))


@pytest.mark.parametrize("scale", [1.0, 8.0])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("cls_kind", Q.CLS_KINDS)
def test_values_and_gradients_on_the_recorded_inputs(K, kats, cls_kind, kind, scale):
    reg = kats["reg"] * scale
    ref = reference(kats["cls"], reg, kats["anc"], kats["ann"], kind, cls_kind, reg_weight=50.0)
    assert ref["npos"] == [71, 35, 0]
    zeros = sum(int((q == 0).sum()) for q in ref["q"])
    assert zeros == (42 if scale == 8.0 else 0), zeros                  # x8 throws 42 of the 106 predictions clear of their targets
    got = hip(K, kats["cls"], reg, kats["anc"], kats["ann"], kind, cls_kind, reg_weight=50.0)
    compare(got, ref, f"{cls_kind} {kind} x{scale:g}")
    clamped = (kats["cls"] <= 1e-4) | (kats["cls"] >= 1.0 - 1e-4)
    assert int((kats["cls"] <= 1e-4).sum()) >= 50 and int((kats["cls"] >= 1.0 - 1e-4).sum()) >= 50       # both clamp ends are hit
    assert bool((got["dcls"][clamped] == 0).all()) and bool((got["dreg"][2] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# the regression half keeps the IoU path's bits; runs repeat; a given assignment is not written
# ------------------------------------------------------------------------------------------------------------------------------------
def raw_run(K, cls, reg, anc, ann, kind, cls_kind=None, given=None, valid=None):
    """the C entry points themselves -> every tensor they write.  cls_kind None: hn_det_loss_iou_fwd / _bwd"""
    from multitask_hydranet_amd._lib import lib
    n, a, k = cls.shape
    blocks = lib().query("hn_det_loss_blocks", a)
    assign = torch.full((n, a), -7, device=DEV, dtype=torch.int16) if given is None else given.clone()
    part = torch.zeros((n, blocks, 4), device=DEV)
    npos = torch.zeros((n,), device=DEV)
    out = torch.zeros((3,), device=DEV)
    dcls, dreg = torch.full_like(cls, 7.0), torch.full_like(reg, 7.0)
    g = torch.tensor([1.25, 50.0], device=DEV)
    p = K.ptr
    head = (p(cls), p(reg), p(anc), p(ann), n, a, k, ann.shape[1], KIND_ID[kind])
    if cls_kind is None:
        assert given is None and valid is None
        lib().call("hn_det_loss_iou_fwd", *head, p(assign), p(part), p(npos), p(out))
        lib().call("hn_det_loss_iou_bwd", *head, p(assign), p(npos), p(g), p(dcls), p(dreg))
    else:
        lib().call("hn_det_loss_quality_fwd", *head, CLS_ID[cls_kind], p(valid), 0 if given is None else 1, p(assign), p(part), p(npos), p(out))
        lib().call("hn_det_loss_quality_bwd", *head, CLS_ID[cls_kind], p(valid), p(assign), p(npos), p(g), p(dcls), p(dreg))
    torch.cuda.synchronize()
    return dict(assign=assign, part=part, npos=npos, out=out, dcls=dcls, dreg=dreg)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("cls_kind", Q.CLS_KINDS)
def test_regression_half_is_untouched_and_runs_repeat(K, kats, cls_kind, kind):
    inputs = [(kats["cls"], kats["reg"], kats["anc"], kats["ann"]), (kats["cls"], kats["reg"] * 8.0, kats["anc"], kats["ann"])]
    cls, reg, anc, ann, _ = tail_case(600, 9)
    inputs.append((cls, reg, anc[0], ann))
    for cls, reg, anc, ann in inputs:
        dev_in = [t.to(DEV).contiguous() for t in (cls, reg, anc, ann)]
        base = raw_run(K, *dev_in, kind)
        one = raw_run(K, *dev_in, kind, cls_kind)
        two = raw_run(K, *dev_in, kind, cls_kind)
        assert int(base["npos"].sum()) > 0
        assert torch.equal(one["assign"], base["assign"]) and torch.equal(one["npos"], base["npos"])
        assert torch.equal(one["out"][1], base["out"][1]) and torch.equal(one["out"][2], base["out"][2])
        assert torch.equal(one["part"][..., 1:], base["part"][..., 1:]) and torch.equal(one["dreg"], base["dreg"])
        assert not torch.equal(one["out"][0], base["out"][0]) and not torch.equal(one["dcls"], base["dcls"])
        for k in one:
            assert torch.equal(one[k], two[k]), k
        # the same assignment handed in: the same bits everywhere, and it is read, not written
        given = one["assign"].clone()
        three = raw_run(K, *dev_in, kind, cls_kind, given=given)
        assert torch.equal(three["assign"], given)
        for k in one:
            assert torch.equal(one[k], three[k]), k
        marked = given.clone()
        marked[marked == -1] = -9                                       # outside -2 .. Mx - 1: counts as ignored, stays as it is
        four = raw_run(K, *dev_in, kind, cls_kind, given=marked)
        assert torch.equal(four["assign"], marked) and torch.equal(four["npos"], one["npos"]) and torch.equal(four["dreg"], one["dreg"])
        assert bool((four["dcls"][marked == -9] == 0).all()) and float(four["out"][0]) < float(one["out"][0])


# ------------------------------------------------------------------------------------------------------------------------------------
# task masks and a given ATSS assignment
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("cls_kind", Q.CLS_KINDS)
def test_masked_batch_under_an_atss_assignment(K, kats, cls_kind, kind):
    from tests import det_atss_ref
    from tests.test_det_atss_cpu import DET
    _, sizes = det_atss_ref.make_anchors(128, 256, DET)
    cls, reg, anc, ann = kats["cls"], kats["reg"] * 1.5, kats["anc"], kats["ann"]          # x 1.5: no min / max tie within 1e-3 px
    assign, _ = K.det_atss_assign(anc.to(DEV), sizes, ann.to(DEV))
    assert [int((assign[n] >= 0).sum()) for n in range(3)] == [516, 199, 0] and not bool((assign == -2).any())
    for mask in ([1, 0, 1], [1, 1, 1]):
        valid = torch.tensor(mask, dtype=torch.uint8, device=DEV)
        ref = reference(cls, reg, anc, ann, kind, cls_kind, 50.0, assign=assign.cpu(), valid=mask)
        assert ref["npos"] == [516, 199 * mask[1], 0]
        before = assign.clone()
        got = hip(K, cls, reg, anc, ann, kind, cls_kind, 50.0, assign=assign, valid=valid)
        assert torch.equal(assign, before)
        compare(got, ref, f"{cls_kind} {kind} atss mask={mask}")
        if not mask[1]:                                                 # the unlabelled image: exactly nothing
            assert bool((got["dcls"][1] == 0).all()) and bool((got["dreg"][1] == 0).all())
            assert bool((ref["dcls"][1] == 0).all()) and bool((ref["dreg"][1] == 0).all())
    # no image labelled: every output is 0 (own assignment: its rows are -2 throughout)
    dev_in = [t.to(DEV).contiguous() for t in (cls, reg, anc, ann)]
    none = raw_run(K, *dev_in, kind, cls_kind, valid=torch.zeros(3, dtype=torch.uint8, device=DEV))
    assert bool((none["assign"] == -2).all())
    for k in ("part", "npos", "out", "dcls", "dreg"):
        assert bool((none[k] == 0).all()), k
    none = hip(K, cls, reg, anc, ann, kind, cls_kind, 50.0, assign=assign, valid=torch.zeros(3, dtype=torch.uint8, device=DEV))
    assert none["cls"] == 0.0 and none["reg"] == 0.0 and none["pos_iou"] == 0.0
    assert bool((none["dcls"] == 0).all()) and bool((none["dreg"] == 0).all())


def test_masked_batch_under_the_own_assignment(K):
    cls, reg, anc, ann, _ = tail_case(600, 9)
    cls = Q.quiet(cls, anc, ann)
    valid = torch.tensor([0, 1, 1], dtype=torch.uint8, device=DEV)
    for cls_kind in Q.CLS_KINDS:
        ref = reference(cls, reg, anc, ann, "ciou", cls_kind, 1.0, valid=[0, 1, 1])
        got = hip(K, cls, reg, anc, ann, "ciou", cls_kind, 1.0, valid=valid)
        compare(got, ref, f"{cls_kind} ciou own assignment mask=[0, 1, 1]")
        assert bool((got["dcls"][0] == 0).all()) and bool((got["dreg"][0] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# module and trainer
# ------------------------------------------------------------------------------------------------------------------------------------
def tiny_net(**det_keys):
    from multitask_hydranet_amd import HydraNet
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["detection"].update(det_keys)
    net = HydraNet(cfgs)
    net.load_state_dict(tiny_state(z))
    net = net.to(DEV).train()
    net.lane_points_per_line = int(z["meta/lane_points_per_line"])
    batch = {k[3:]: torch.from_numpy(z[k].copy()).to(DEV) for k in z.files if k.startswith("in/")}
    return net, batch


def test_module_selects_the_loss_by_the_cfg_key(K):
    absent, batch = tiny_net(loss_reg_type="giou")
    focal, _ = tiny_net(loss_reg_type="giou", loss_cls_type="focal")
    qfl, _ = tiny_net(loss_reg_type="giou", loss_cls_type="qfl")
    outs = [net(batch["image"]) for net in (absent, focal, qfl)]
    d = outs[0]["detection"]
    for o in outs[1:]:
        assert torch.equal(d["classification"], o["detection"]["classification"]) and torch.equal(d["regression"], o["detection"]["regression"])
    ld_a, ld_f, ld_q = (net.cal_loss(o, batch) for net, o in zip((absent, focal, qfl), outs))
    assert sorted(ld_a) == sorted(ld_f) == sorted(ld_q)                 # the keys of loss_dict do not change
    for k in ld_a:                                                      # focal is the absent key, bit for bit
        assert torch.equal(ld_a[k], ld_f[k]), k
    assert torch.equal(absent.det_pos_iou, focal.det_pos_iou)
    assert not torch.equal(ld_q["loss_det_cls"], ld_f["loss_det_cls"])
    assert torch.equal(ld_q["loss_det_reg"], ld_f["loss_det_reg"]) and torch.equal(qfl.det_pos_iou, focal.det_pos_iou)
    assert qfl.det_pos_iou.shape == () and qfl.det_pos_iou.is_cuda and not qfl.det_pos_iou.requires_grad
    ref = Q.det_quality_loss(d["classification"].detach().cpu(), d["regression"].detach().cpu(), d["anchors"].cpu(), batch["gt_det"].cpu(),
                             "giou", "qfl")
    got = float(ld_q["loss_det_cls"].detach())
    print(f"module: qfl {got:.7f} / {float(ref['cls']):.7f}  focal {float(ld_f['loss_det_cls'].detach()):.7f}  npos {ref['npos']}")
    assert sum(ref["npos"]) > 0 and abs(got - float(ref["cls"])) <= 2e-5 * abs(float(ref["cls"]))
    qfl.total_loss(ld_q).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in qfl.named_parameters() if n.startswith("detectheader."))


def make_trainer(loader, weights=True, seed=0):
    from multitask_hydranet_amd.train import HydraTrainer
    z = load_npz("tiny_hydranet.npz")
    cfgs = copy.deepcopy(load_cfg("hydranet_tiny.yml"))
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    cfgs["detection"].update(loss_cls_type="vfl", loss_reg_type="giou", assigner="atss")
    if not weights:
        torch.manual_seed(seed)
    tr = HydraTrainer(cfgs, trainloader=loader, validloader=None, iters_per_epoch=len(loader), capture_step=True)
    if weights:
        tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    return tr


def test_trainer_steps_saves_and_resumes_under_vfl_giou_atss(K, tmp_path):
    z = load_npz("tiny_hydranet.npz")
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    g = torch.Generator().manual_seed(3)
    loader = []
    for i in range(5):
        b = dict(batch)
        b["image"] = batch["image"] + 0.05 * torch.randn(batch["image"].shape, generator=g)
        loader.append(b)
    fresh = lambda b: {k: v.clone() for k, v in b.items()}
    a = make_trainer(loader)
    before = {n: p.detach().clone() for n, p in a.hydranet.named_parameters()}
    for b in loader[:4]:
        losses = a.train_step(fresh(b))
        assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
        assert float(losses["loss_det_cls"]) > 0 and float(losses["loss_det_reg"]) > 0
    assert a._cap is not None                                           # the step was captured and replayed
    assert 0.0 < float(a.hydranet.det_pos_iou) <= 1.0
    changed = [n for n, p in a.hydranet.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(changed) > 0.9 * len(before) and any(n.startswith("detectheader.") for n in changed)
    path = str(tmp_path / "vfl.hn")
    a.save_state(path)
    want = {k: v.clone() for k, v in a.train_step(fresh(loader[4])).items()}
    c = make_trainer(loader, weights=False, seed=1234)
    c.load_state(path)
    got = c.train_step(fresh(loader[4]))
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (k, float(got[k]), float(want[k]))
