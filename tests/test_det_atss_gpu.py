"""GPU: the ATSS anchor assignment (detection.assigner = atss; csrc/hn_det_atss.hip) against the numpy reference tests/det_atss_ref.py, the
loss forwards that read a given assignment against the ones that compute it, the losses under ATSS against tests/torch_losses.det_loss /
tests/det_iou_ref restated for a given assignment (det_atss_ref.losses_given_assign, held to both on the CPU), and the module and trainer
with the cfg key.  The candidate sets are exact (float32 keys); the float32 evaluation of mean + std, of the inside test and of IoU
conflicts may differ from the float64 reference only inside the reference's ambiguous set (bands in det_atss_ref), and the test first
asserts that set to be at most 0.2 % of the candidates.  Loss bounds are the project's for the detection loss: 2e-5 relative, gradients
2e-4 of the reference's maximum."""
import copy

import numpy as np
import pytest
import torch

from tests import det_atss_ref as R
from tests.helpers import load_cfg, load_npz, tiny_state
from tests.test_det_atss_cpu import DET, concentric_case, hand_ann, random_boxes
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


@pytest.fixture(scope="module")
def kats():
    z = load_npz("loss_kats.npz")
    t = lambda k: torch.from_numpy(z[k])
    cls = (t("det/cls") * 4.5).clamp(0, 1)                              # spread over (0, 0.9]: both focal branches and the clamp
    _, sizes = R.make_anchors(128, 256, DET)
    return dict(cls=cls, reg=t("det/reg"), anc=t("det/anchors").reshape(-1, 4), ann=t("det/ann"), sizes=sizes)


def device_assign(K, anc, sizes, ann, topk=9):
    assign, thr = K.det_atss_assign(torch.as_tensor(anc).to(DEV), sizes, torch.as_tensor(ann).to(DEV), topk=topk)
    torch.cuda.synchronize()
    assert assign.dtype == torch.int16 and thr.dtype == torch.float32
    return assign.cpu().numpy().astype(np.int64), thr.cpu().numpy().astype(np.float64)


def check_assignment(K, anc, sizes, ann, topk=9, what="", exact=False):
    """the device's assignment and thresholds against the reference's, image by image"""
    anc, ann = np.asarray(anc, np.float32), np.asarray(ann, np.float32)
    ref = R.atss(anc, sizes, ann, topk=topk)
    n_cand, n_amb = sum(r["n_cand"] for r in ref), sum(r["n_amb"] for r in ref)
    got_assign, got_thr = device_assign(K, anc, sizes, ann, topk)
    again, again_thr = device_assign(K, anc, sizes, ann, topk)
    npos = int((got_assign >= 0).sum())
    thr_err = 0.0
    for n, r in enumerate(ref):
        v = ann[n, :, 4] != -1
        if v.any():
            thr_err = max(thr_err, float(np.abs(got_thr[n][v] - r["thr"][v]).max()))
    print(f"{what}: A {anc.shape[0]} boxes {int((ann[..., 4] != -1).sum())} candidates {n_cand} ambiguous {n_amb} positives {npos} "
          f"max |thr err| {thr_err:.2e}")
    if not exact:
        assert n_cand > 0 and n_amb <= 0.002 * n_cand, (n_amb, n_cand)  # the reference's own ambiguous share on these inputs
    assert thr_err <= 5e-5
    assert not (got_assign == -2).any() and got_assign.min() >= -1 and got_assign.max() < ann.shape[1]
    for n, r in enumerate(ref):
        amb = np.zeros(anc.shape[0], bool) if exact else np.isin(np.arange(anc.shape[0]), list(r["allowed"]))
        bad = np.nonzero((got_assign[n] != r["assign"]) & ~amb)[0]
        assert bad.size == 0, (what, n, bad[:8], got_assign[n][bad[:8]], r["assign"][bad[:8]])
        for a in np.nonzero(amb)[0]:
            assert int(got_assign[n][a]) in r["allowed"][int(a)], (what, n, a, got_assign[n][a], r["allowed"][int(a)])
        v = ann[n, :, 4] != -1
        assert np.array_equal(again_thr[n][v], got_thr[n][v])
    assert np.array_equal(again, got_assign)                           # run to run
    return ref, got_assign


def test_assignment_128x128(K):
    anc, sizes = R.make_anchors(128, 128, DET)
    check_assignment(K, anc, sizes, random_boxes(3, 8, 128, 128, seed=1, valid=[8, 5, 0]), what="128x128")
    check_assignment(K, anc, sizes, random_boxes(3, 8, 128, 128, seed=2, valid=[8, 5, 0]), topk=1, what="128x128 topk 1")


def test_assignment_recorded_inputs(K, kats):
    ref, got = check_assignment(K, kats["anc"], kats["sizes"], kats["ann"], what="recorded 128x256")
    assert kats["anc"].shape[0] == 6138 and (got[2] == -1).all() and (got[0] >= 0).sum() > 71      # the max-IoU rule gives 71 / 35 / 0


def test_assignment_one_box_per_image(K, kats):
    check_assignment(K, kats["anc"], kats["sizes"], random_boxes(3, 1, 128, 256, seed=1), what="128x256 Mx 1")


def test_assignment_512x1024(K):
    anc, sizes = R.make_anchors(512, 1024, DET)
    assert anc.shape[0] == 98208 and sizes[0] == 73728
    check_assignment(K, anc, sizes, random_boxes(2, 32, 512, 1024, seed=1, valid=[32, 20]), what="512x1024")


def test_assignment_when_every_distance_ties(K):
    """4096 concentric anchors: the prefilter cannot shrink the level, the select runs on global memory and two index digits decide"""
    anc, sizes, ann = concentric_case()
    ref, got = check_assignment(K, anc, sizes, ann, what="concentric")
    assert sum(int((g >= 0).sum()) for g in got) > 0


def test_hand_made_boxes_match_exactly(K):
    """the cases of tests/test_det_atss_cpu.py: index-decided distance ties, k_l = A_l, no centre inside, a box half outside, identical
    boxes (identical IoU bits on the device: the lower index must win), no boxes"""
    anc, sizes = R.make_anchors(128, 128, DET)
    ref, got = check_assignment(K, anc, sizes, hand_ann(), what="hand-made", exact=True)
    assert [int((g >= 0).sum()) for g in got] == [int((r["assign"] >= 0).sum()) for r in ref]
    assert (got[2] == -1).all() and (got[5] == -1).all() and set(np.unique(got[4]).tolist()) == {-1, 0}


# ------------------------------------------------------------------------------------------------------------------------------------
# the forwards that read an assignment against the ones that compute it
# ------------------------------------------------------------------------------------------------------------------------------------
def raw_run(K, name, cls, reg, anc, ann, kind=None, given=None):
    """the C entry points themselves -> every tensor they write; given: run <name>_fwd_assigned on this assignment"""
    from multitask_hydranet_amd._lib import lib
    n, a, k = cls.shape
    cols = 3 if kind is None else 4
    blocks = lib().query("hn_det_loss_blocks", a)
    assign = torch.full((n, a), -7, device=DEV, dtype=torch.int16) if given is None else given.clone()
    part = torch.zeros((n, blocks, cols), device=DEV)
    npos = torch.zeros((n,), device=DEV)
    out = torch.zeros((cols - 1,), device=DEV)
    dcls, dreg = torch.full_like(cls, 7.0), torch.full_like(reg, 7.0)
    g = torch.tensor([1.25, 50.0], device=DEV)
    extra = () if kind is None else (KIND_ID[kind],)
    p = K.ptr
    lib().call(name + ("_fwd" if given is None else "_fwd_assigned"), p(cls), p(reg), p(anc), p(ann), n, a, k, ann.shape[1], *extra, p(assign),
               p(part), p(npos), p(out))
    lib().call(name + "_bwd", p(cls), p(reg), p(anc), p(ann), n, a, k, ann.shape[1], *extra, p(assign), p(npos), p(g), p(dcls), p(dreg))
    torch.cuda.synchronize()
    return dict(assign=assign, part=part, npos=npos, out=out, dcls=dcls, dreg=dreg)


@pytest.mark.parametrize("kind", [None, "giou"])
def test_assigned_forward_is_bit_identical_on_the_same_assignment(K, kats, kind):
    dev_in = [kats[k].to(DEV).contiguous() for k in ("cls", "reg", "anc", "ann")]
    name = "hn_det_loss" if kind is None else "hn_det_loss_iou"
    base = raw_run(K, name, *dev_in, kind=kind)
    assert int(base["npos"].sum()) == 106 and int((base["assign"] == -2).sum()) > 0       # positives, background and the ignore zone
    same = raw_run(K, name, *dev_in, kind=kind, given=base["assign"])
    for k in base:
        assert torch.equal(base[k], same[k]), k
    # a stray value never indexes the annotations: it counts as ignored
    stray = base["assign"].clone()
    stray[0, :4] = torch.tensor([16, 300, -3, -32768], dtype=torch.int16)
    want = base["assign"].clone()
    want[0, :4] = -2
    a, b = raw_run(K, name, *dev_in, kind=kind, given=stray), raw_run(K, name, *dev_in, kind=kind, given=want)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["npos"], b["npos"]) and bool(torch.isfinite(a["out"]).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# the losses under ATSS
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kats_atss(kats):
    ref = R.atss(kats["anc"].numpy(), kats["sizes"], kats["ann"].numpy())
    assert sum(r["n_amb"] for r in ref) == 0 and not any(r["allowed"] for r in ref)       # an empty ambiguous set
    return np.stack([r["assign"] for r in ref])


@pytest.mark.parametrize("kind", ["smooth_l1", "giou", "diou", "ciou"])
def test_losses_under_atss(K, kats, kats_atss, kind, reg_weight=50.0):
    cls, reg, anc, ann = kats["cls"], kats["reg"] * 1.5, kats["anc"], kats["ann"]          # x 1.5: no min / max tie within 1e-3 px
    c64, r64 = cls.double().requires_grad_(True), reg.double().requires_grad_(True)
    ref = R.losses_given_assign(c64, r64, anc, ann, kats_atss, kind)
    (ref["cls"] + reg_weight * ref["reg"]).backward()
    ref.update(cls=ref["cls"].detach(), reg=ref["reg"].detach())
    assert ref["npos"] == [516, 199, 0] and (kind == "smooth_l1" or ref["margin"] > 1e-3)

    def run():
        c, r = cls.clone().to(DEV).requires_grad_(True), reg.clone().to(DEV).requires_grad_(True)
        assign, _ = K.det_atss_assign(anc.to(DEV), kats["sizes"], ann.to(DEV))
        if kind == "smooth_l1":
            lc, lr = K.det_loss_hip(c, r, anc.to(DEV), ann.to(DEV), assign=assign)
            iou = torch.zeros(1)
        else:
            lc, lr, iou = K.det_iou_loss_hip(c, r, anc.to(DEV), ann.to(DEV), kind, assign=assign)
            assert not iou.requires_grad
        (lc.sum() + reg_weight * lr.sum()).backward()
        return assign.cpu(), float(lc.detach()), float(lr.detach()), float(iou), c.grad.cpu(), r.grad.cpu()
    assign, lc, lr, iou, dcls, dreg = run()
    assert np.array_equal(assign.numpy().astype(np.int64), kats_atss)
    print(f"{kind}: cls {lc:.7f} / {float(ref['cls']):.7f}  reg {lr:.7f} / {float(ref['reg']):.7f}  pos_iou {iou:.6f} / "
          f"{float(ref['pos_iou']):.6f}  npos {ref['npos']}")
    for got, want in ((lc, float(ref["cls"])), (lr, float(ref["reg"])), (iou, float(ref["pos_iou"]))):
        assert abs(got - want) <= 2e-5 * max(abs(want), 1e-6), (kind, got, want)
    close(dcls, c64.grad, 2e-4, kind + " dcls")
    close(dreg, r64.grad, 2e-4, kind + " dreg")
    assert bool((dreg[2] == 0).all()) and bool((dreg[0][torch.from_numpy(kats_atss[0] < 0)] == 0).all())
    for a, b in zip(run(), (assign, lc, lr, iou, dcls, dreg)):         # bit-identical run to run
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b


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


def test_module_assigns_by_the_cfg_key(K):
    plain, batch = tiny_net()
    atss, _ = tiny_net(assigner="atss", loss_reg_type="giou")
    out_p, out_a = plain(batch["image"]), atss(batch["image"])
    d = out_p["detection"]
    assert torch.equal(d["classification"], out_a["detection"]["classification"])
    ld_p, ld_a = plain.cal_loss(out_p, batch), atss.cal_loss(out_a, batch)
    assert sorted(ld_p) == sorted(ld_a)
    # the key absent: the parent's path, bit for bit
    want_c, want_r = K.det_loss_hip(d["classification"].detach(), d["regression"].detach(), d["anchors"], batch["gt_det"])
    assert torch.equal(ld_p["loss_det_reg"], want_r.reshape(())) and torch.equal(ld_p["loss_det_cls"], want_c.reshape(()))
    assert plain.det_pos_iou is None
    # atss + giou: the reference's assignment on the module's own outputs
    da = out_a["detection"]
    anc, sizes = R.make_anchors(128, 128, DET)
    assert np.array_equal(da["anchors"][0].cpu().numpy(), anc) and atss.anchor_level_sizes(128, 128) == sizes
    ref = R.atss(anc, sizes, batch["gt_det"].cpu().numpy())
    assign, _ = K.det_atss_assign(da["anchors"], sizes, batch["gt_det"])
    for n, r in enumerate(ref):
        diff = np.nonzero(assign[n].cpu().numpy() != r["assign"])[0]
        assert all(int(assign[n][a]) in r["allowed"].get(int(a), ()) for a in diff)
    want = R.losses_given_assign(da["classification"].detach().cpu().double(), da["regression"].detach().cpu().double(), torch.from_numpy(anc),
                                 batch["gt_det"].cpu(), assign.cpu().numpy(), "giou")
    got_c, got_r, got_i = float(ld_a["loss_det_cls"].detach()), float(ld_a["loss_det_reg"].detach()), float(atss.det_pos_iou)
    print(f"module: cls {got_c:.6f} / {float(want['cls']):.6f} reg {got_r:.7f} / {float(want['reg']):.7f} pos_iou {got_i:.6f} npos {want['npos']}")
    assert sum(want["npos"]) > 0 and atss.det_pos_iou.shape == () and atss.det_pos_iou.is_cuda
    for got, w in ((got_c, want["cls"]), (got_r, want["reg"]), (got_i, want["pos_iou"])):
        assert abs(got - float(w)) <= 2e-5 * abs(float(w))
    assert not torch.equal(ld_a["loss_det_cls"], ld_p["loss_det_cls"])
    atss.total_loss(ld_a).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in atss.named_parameters() if n.startswith("detectheader."))


def test_trainer_steps_under_atss_eagerly_and_captured(K):
    from multitask_hydranet_amd.train import HydraTrainer
    z = load_npz("tiny_hydranet.npz")
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    g = torch.Generator().manual_seed(3)
    loader = []
    for i in range(4):
        b = dict(batch)
        b["image"] = batch["image"] + 0.05 * torch.randn(batch["image"].shape, generator=g)
        loader.append(b)
    cfgs = copy.deepcopy(load_cfg("hydranet_tiny.yml"))
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    cfgs["detection"].update(assigner="atss", loss_reg_type="giou")
    tr = HydraTrainer(cfgs, trainloader=loader, validloader=None, iters_per_epoch=len(loader), capture_step=True)
    tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    seen = []
    for b in loader:
        losses = tr.train_step({k: v.clone() for k, v in b.items()})
        assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
        seen.append((float(losses["loss_det_cls"]), float(losses["loss_det_reg"])))
        assert seen[-1][1] > 0 and 0.0 < float(tr.hydranet.det_pos_iou) <= 1.0
    assert tr._cap is not None                                          # the later steps were captured and replayed
    assert len(set(seen)) == len(seen), seen                            # the loss changes from step to step
