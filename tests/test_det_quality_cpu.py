"""CPU: the quality focal / varifocal detection losses (detection.loss_cls_type = qfl | vfl).  The float64 restatement
tests/det_quality_ref.py, which the GPU tests hold the HIP kernels to, is itself held to autograd and to the closed forms it must reduce
to; its float32 run bounds what single precision costs on the GPU tests' inputs; the cfg keys are validated by the constructor without a
GPU; the library exports the two entry points and rejects bad arguments before any launch."""
import copy
import ctypes

import pytest
import torch

from tests import det_iou_ref as R
from tests import det_quality_ref as Q
from tests.helpers import load_cfg, load_npz
from tests.test_det_iou_gpu import tail_case


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


def random_pairs():
    g = torch.Generator().manual_seed(11)
    p = torch.rand(4000, generator=g, dtype=torch.float64) * 0.9996 + 2e-4        # inside the clamp, away from its ends
    y = torch.rand(4000, generator=g, dtype=torch.float64)
    y[::5] = 0.0                                                                   # exact zeros: vfl's other branch
    y[1::50] = 1.0
    outside = torch.tensor([0.0, 1e-5, 9.9e-5, 1.0 - 9.9e-5, 1.0 - 1e-6, 1.0], dtype=torch.float64)
    p = torch.cat([p, outside, outside])
    y = torch.cat([y, torch.zeros(6, dtype=torch.float64), torch.full((6,), 0.6, dtype=torch.float64)])
    return p, y


@pytest.mark.parametrize("cls_kind", Q.CLS_KINDS)
def test_analytic_derivatives_equal_autograd(cls_kind):
    p, y = random_pairs()
    assert int((y == 0).sum()) > 700 and int(((p <= Q.LO) | (p >= Q.HI)).sum()) == 12
    pa = p.clone().requires_grad_(True)
    Q.term(pa, y, cls_kind).sum().backward()
    want = Q.analytic_grad(p, y, cls_kind)
    err = float((pa.grad - want).abs().max() / want.abs().max())
    print(f"{cls_kind}: max |autograd - analytic| / max = {err:.2e}")
    assert err <= 1e-12
    out = (p <= Q.LO) | (p >= Q.HI)
    assert bool((pa.grad[out] == 0).all()) and bool((want[out] == 0).all())       # outside the clamp both are exactly 0


def test_closed_forms_at_the_ends_of_the_target_range():
    p = torch.linspace(0.001, 0.999, 999, dtype=torch.float64)
    one, zero = torch.ones_like(p), torch.zeros_like(p)
    tight = lambda a, b: float((a - b).abs().max()) <= 1e-14 * float(b.abs().max())
    # qfl: the focal terms without their 0.25 / 0.75
    assert tight(Q.term(p, one, "qfl"), (1 - p) ** 2 * -torch.log(p))
    assert tight(Q.term(p, zero, "qfl"), p ** 2 * -torch.log(1 - p))
    # vfl: plain cross-entropy at y = 1, the focal background term at y = 0
    assert tight(Q.term(p, one, "vfl"), -torch.log(p))
    assert tight(Q.term(p, zero, "vfl"), 0.75 * p ** 2 * -torch.log(1 - p))
    # qfl has its minimum where the score equals the quality
    assert float(Q.analytic_grad(p, p.clone(), "qfl").abs().max()) == 0.0
    assert float(Q.term(p, p.clone(), "qfl").abs().max()) == 0.0


def gpu_test_inputs():
    """(name, cls, reg, anc, ann) of every input tests/test_det_quality_gpu.py compares values on"""
    for A in (255, 256, 257, 600):
        for Kc in (1, 9):
            cls, reg, anc, ann, _ = tail_case(A, Kc)
            yield f"tail A={A} K={Kc}", cls, reg, anc, ann
            yield f"tail A={A} K={Kc} quiet", Q.quiet(cls, anc, ann), reg, anc, ann
    k = Q.kat_inputs(load_npz("loss_kats.npz"))
    for scale in (1.0, 8.0):
        yield f"recorded x{scale:g}", k["cls"], k["reg"] * scale, k["anc"], k["ann"]


def test_float32_headroom_on_the_gpu_test_inputs():
    """the float32 run of the reference against its float64 run: loss, and gradients relative to their maximum (over all rows, and over
    the positive anchors' rows alone), within 1e-5; measured at most 6.0e-7 (loss) and 1.4e-6 (gradients, all rows and positive rows alike)"""
    worst = [0.0, 0.0, 0.0]
    for name, cls, reg, anc, ann in gpu_test_inputs():
        for kind in R.KINDS:
            for cls_kind in Q.CLS_KINDS:
                res = []
                for dtype in (torch.float64, torch.float32):
                    c = cls.clone().to(dtype).requires_grad_(True)
                    o = Q.det_quality_loss(c, reg, anc, ann, kind, cls_kind, dtype=dtype)
                    o["cls"].backward()
                    o["cls"] = o["cls"].detach()
                    res.append((o, c.grad.double()))
                (o64, g64), (o32, g32) = res
                assert o64["npos"] == o32["npos"] and sum(o64["npos"]) > 0
                rows = torch.stack(o64["pos"])
                dl = abs(float(o32["cls"]) - float(o64["cls"])) / abs(float(o64["cls"]))
                dg = float((g32 - g64).abs().max() / g64.abs().max())
                dp = float((g32 - g64)[rows].abs().max() / g64[rows].abs().max())
                worst = [max(a, b) for a, b in zip(worst, (dl, dg, dp))]
                assert dl <= 1e-5 and dg <= 1e-5 and dp <= 1e-5, (name, kind, cls_kind, dl, dg, dp)
    print(f"float32 against float64: loss {worst[0]:.2e}, gradient / max {worst[1]:.2e}, positive rows' gradient / their max {worst[2]:.2e}")


def test_reference_under_the_focal_assignment_and_masks():
    """the restated assignment is torch_losses.det_loss's (npos, and the focal loss on it); a valid row is the sub-batch"""
    from tests import det_atss_ref
    k = Q.kat_inputs(load_npz("loss_kats.npz"))
    anc64 = k["anc"].double()
    assign = torch.stack([Q.max_iou_assign(anc64, k["ann"][n].double()) for n in range(3)])
    assert [int((a >= 0).sum()) for a in assign] == [71, 35, 0] and int((assign == -2).sum()) > 0
    focal = det_atss_ref.losses_given_assign(k["cls"].double(), k["reg"].double(), k["anc"], k["ann"], assign, "giou")
    want = R.det_iou_loss(k["cls"], k["reg"], k["anc"], k["ann"], "giou")
    assert abs(float(focal["cls"]) - float(want["cls"])) <= 1e-12 * float(want["cls"])
    full = Q.det_quality_loss(k["cls"][[0, 2]], k["reg"][[0, 2]], k["anc"], k["ann"][[0, 2]], "ciou", "vfl")
    sub = Q.det_quality_loss(k["cls"], k["reg"], k["anc"], k["ann"], "ciou", "vfl", valid=[1, 0, 1])
    assert float(sub["cls"]) == float(full["cls"]) and float(sub["reg"]) == float(full["reg"]) and sub["npos"] == [71, 0, 0]
    none = Q.det_quality_loss(k["cls"], k["reg"], k["anc"], k["ann"], "ciou", "vfl", valid=[0, 0, 0])
    assert float(none["cls"]) == 0.0 and float(none["reg"]) == 0.0 and float(none["pos_iou"]) == 0.0


def test_constructor_validates_loss_cls_type(built):
    from multitask_hydranet_amd import HydraNet
    from multitask_hydranet_amd import ops as K
    cfgs = load_cfg("hydranet_tiny.yml")
    assert "loss_cls_type" not in cfgs["detection"] and "loss_reg_type" not in cfgs["detection"]
    assert sorted(K.DET_CLS_KINDS) == ["focal", "qfl", "vfl"]

    def make(**keys):
        c = copy.deepcopy(cfgs)
        c["detection"].update(keys)
        return HydraNet(c)
    assert make().loss_cls_type == "focal" and make().loss_detect is K.det_loss_hip
    assert make(loss_cls_type="focal").loss_detect is K.det_loss_hip
    for cls_kind in ("qfl", "vfl"):
        for keys in (dict(), dict(loss_reg_type="smooth_l1")):        # a quality target needs the IoU kernel's decoded box
            with pytest.raises(ValueError) as ei:
                make(loss_cls_type=cls_kind, **keys)
            assert "loss_cls_type" in str(ei.value) and "loss_reg_type" in str(ei.value)
        for kind in R.KINDS:
            for assigner in ("max_iou", "atss"):
                net = make(loss_cls_type=cls_kind, loss_reg_type=kind, assigner=assigner)
                assert net.loss_cls_type == cls_kind and net.loss_detect.keywords == dict(kind=kind, cls_kind=cls_kind)
    assert list(net.state_dict()) == list(make().state_dict())        # the key adds no state
    with pytest.raises(ValueError) as ei:
        make(loss_cls_type="gfl", loss_reg_type="giou")
    assert all(name in str(ei.value) for name in ("focal", "qfl", "vfl"))
    with pytest.raises(ValueError):
        K.det_iou_loss_hip(None, None, None, None, "giou", cls_kind="gfl")


def test_library_exports_the_entry_points_and_rejects_bad_arguments(built):
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    for name in ("hn_det_loss_quality_fwd", "hn_det_loss_quality_bwd"):
        assert name in sig and hasattr(dll, name)
    assert "hn_det_loss.hip" in built.SOURCES
    l = built.lib()
    # HN_CHECK_ARG returns 1 before any launch: the pointers are never dereferenced (1 stands for 'not null'); valid may be null
    fwd = lambda cls=1, K=9, kind=1, ck=1, given=0, assign=1: l.raw("hn_det_loss_quality_fwd")(cls, 1, 1, 1, 2, 300, K, 8, kind, ck, None, given,
                                                                                               assign, 1, 1, 1, None)
    bwd = lambda cls=1, K=9, kind=1, ck=1, dreg=1: l.raw("hn_det_loss_quality_bwd")(cls, 1, 1, 1, 2, 300, K, 8, kind, ck, None, 1, 1, 1, 1, dreg,
                                                                                    None)
    for kind in (0, 4, -1):
        assert fwd(kind=kind) == 1 and bwd(kind=kind) == 1
    for ck in (0, 3, -1):                                               # 0 is the focal loss: it has its own entry points
        assert fwd(ck=ck) == 1 and bwd(ck=ck) == 1
    assert fwd(cls=None) == 1 and fwd(assign=None) == 1 and bwd(cls=None) == 1 and bwd(dreg=None) == 1
    assert fwd(K=33) == 1 and bwd(K=33) == 1                            # K beyond the LDS tile's bound
    assert fwd(given=2) == 1
