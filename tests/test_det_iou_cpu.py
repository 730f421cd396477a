"""CPU: the IoU-family box regression losses (detection.loss_reg_type).  The float64 restatement tests/det_iou_ref.py, which the GPU tests
hold the HIP kernels to, is itself held to closed-form numbers on hand-made boxes and to the assignment of tests/torch_losses.det_loss
on the recorded KAT inputs; its float32 run bounds what single precision costs on those inputs; the cfg key is validated by the
constructor without a GPU; the library exports the two new entry points and rejects a kind outside 1..3 before any launch."""
import copy
import ctypes
import math

import pytest
import torch

from tests import det_iou_ref as R
from tests import torch_losses as L
from tests.helpers import load_cfg, load_npz


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


def one(anchor_yxyx, box_xyxy, kind, reg=(0.0, 0.0, 0.0, 0.0)):
    t = lambda v: torch.tensor([v], dtype=torch.float64)
    loss, iou, _ = R.box_losses(t(reg), t(anchor_yxyx), t(box_xyxy), kind)
    return float(loss), float(iou)


def test_hand_made_boxes_have_their_closed_form_values():
    # a zero regression decodes to the anchor itself (y1, x1, y2, x2); annotations are (x1, y1, x2, y2)
    for kind in R.KINDS:
        loss, iou = one((10.0, 20.0, 30.0, 60.0), (20.0, 10.0, 60.0, 30.0), kind)           # identical boxes
        assert abs(loss) < 1e-8 and abs(iou - 1.0) < 1e-8, (kind, loss, iou)
    # two 10 x 10 squares, one shifted by half a side along x: inter 50, union 150, enclosing box 15 x 10
    want = {"giou": 2.0 / 3.0, "diou": 2.0 / 3.0 + 25.0 / 325.0, "ciou": 2.0 / 3.0 + 25.0 / 325.0}      # equal aspect ratios: v = 0
    for kind in R.KINDS:
        loss, iou = one((0.0, 0.0, 10.0, 10.0), (5.0, 0.0, 15.0, 10.0), kind)
        assert abs(iou - 1.0 / 3.0) < 1e-8 and abs(loss - want[kind]) < 1e-8, (kind, loss, iou)
    # disjoint: iou 0, enclosing box 30 x 10 against a union of 200 -> 1 + 100 / 300
    loss, iou = one((0.0, 0.0, 10.0, 10.0), (20.0, 0.0, 30.0, 10.0), "giou")
    assert iou == 0.0 and loss > 1.0 and abs(loss - 4.0 / 3.0) < 1e-8
    # the decode: dx = 0.5 moves the 10-wide anchor by 5, dw = log 2 doubles its width; dh above the clip is clipped
    loss, iou = one((0.0, 0.0, 10.0, 10.0), (0.0, 0.0, 20.0, 10.0), "giou", reg=(0.0, 0.5, 0.0, math.log(2.0)))
    assert abs(loss) < 1e-8 and abs(iou - 1.0) < 1e-8
    a, _ = one((0.0, 0.0, 10.0, 10.0), (0.0, 0.0, 10.0, 625.0), "ciou", reg=(0.0, 0.0, 5.0, 0.0))
    b, _ = one((0.0, 0.0, 10.0, 10.0), (0.0, 0.0, 10.0, 625.0), "ciou", reg=(0.0, 0.0, R.CLIP, 0.0))
    assert a == b and a == a
    # ciou: the aspect term on concentric boxes of equal area (diou sees only 1 - iou)
    d, iou = one((0.0, 0.0, 20.0, 20.0), (-10.0, 5.0, 30.0, 15.0), "diou")
    c, _ = one((0.0, 0.0, 20.0, 20.0), (-10.0, 5.0, 30.0, 15.0), "ciou")
    v = (4 / torch.pi ** 2) * float(torch.atan(torch.tensor(4.0, dtype=torch.float64)) - torch.pi / 4) ** 2
    assert abs(iou - 1.0 / 3.0) < 1e-8 and abs(d - 2.0 / 3.0) < 1e-8 and abs(c - (d + v * v / (1 - iou + v + R.EPS))) < 1e-9


@pytest.fixture(scope="module")
def kats():
    z = load_npz("loss_kats.npz")
    return {k: torch.from_numpy(z["det/" + k]) for k in ("anchors", "reg", "ann", "cls")}


def run(kats, kind, scale, dtype):
    reg = (kats["reg"] * scale).to(dtype).requires_grad_(True)
    out = R.det_iou_loss(kats["cls"], reg, kats["anchors"], kats["ann"], kind, dtype=dtype)
    out["reg"].backward()
    out["reg"] = out["reg"].detach()
    return out, reg.grad


def test_golden_fixture_assignment_and_float32_headroom(kats):
    """71, 35 and 0 positives; the restated assignment gives torch_losses.det_loss's smooth-L1 value; float32 against float64 within
    1e-6 of the loss and of the gradient's maximum (measured: 1e-7 and 5e-7, the same with the regressions x 8)"""
    assert tuple(kats["anchors"].reshape(-1, 4).shape) == (6138, 4)
    anc, ann, reg = kats["anchors"].reshape(-1, 4).double(), kats["ann"].double(), kats["reg"].double()
    per_image = []
    for n in range(3):
        pos, arg = R.assign(anc, ann[n])
        if not bool(pos.any()):
            per_image.append(torch.zeros((), dtype=torch.float64))
            continue
        a, b = anc[pos], ann[n][arg[pos]]
        aw, ah = a[:, 3] - a[:, 1], a[:, 2] - a[:, 0]
        gw, gh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        t = torch.stack(((b[:, 1] + gh / 2 - a[:, 0] - ah / 2) / ah, (b[:, 0] + gw / 2 - a[:, 1] - aw / 2) / aw,
                         torch.log(gh.clamp(min=1) / ah), torch.log(gw.clamp(min=1) / aw)), dim=1)
        d = (t - reg[n][pos]).abs()
        per_image.append(torch.where(d <= 1 / 9, 4.5 * d * d, d - 0.5 / 9).mean())
    want = L.det_loss(kats["cls"].double(), reg, anc[None], ann)[1]
    assert abs(float(torch.stack(per_image).mean()) - float(want)) <= 1e-12 * abs(float(want))
    for kind in R.KINDS:
        for scale in (1.0, 8.0):
            o64, g64 = run(kats, kind, scale, torch.float64)
            o32, g32 = run(kats, kind, scale, torch.float32)
            assert o64["npos"] == [71, 35, 0] and o32["npos"] == [71, 35, 0]
            dl = abs(float(o32["reg"]) - float(o64["reg"])) / abs(float(o64["reg"]))
            di = abs(float(o32["pos_iou"]) - float(o64["pos_iou"]))
            dg = float((g32.double() - g64).abs().max() / g64.abs().max())
            print(f"{kind} x{scale:g}: loss {float(o64['reg']):.6f} pos_iou {float(o64['pos_iou']):.4f} margin {o64['margin']:.3e} px; "
                  f"float32 deviates {dl:.2e} (loss) {di:.2e} (pos_iou) {dg:.2e} (gradient / max)")
            assert float(o64["reg"]) > 0 and float(g64.abs().max()) > 0 and bool((g64[2] == 0).all())
            assert dl <= 1e-6 and di <= 1e-6 and dg <= 1e-6


def test_constructor_validates_loss_reg_type(built):
    from multitask_hydranet_amd import HydraNet
    from multitask_hydranet_amd import ops as K
    cfgs = load_cfg("hydranet_tiny.yml")
    assert "loss_reg_type" not in cfgs["detection"]
    net = HydraNet(copy.deepcopy(cfgs))
    assert net.loss_detect is K.det_loss_hip and net.det_pos_iou is None
    explicit = copy.deepcopy(cfgs)
    explicit["detection"]["loss_reg_type"] = "smooth_l1"
    assert HydraNet(explicit).loss_detect is K.det_loss_hip
    bad = copy.deepcopy(cfgs)
    bad["detection"]["loss_reg_type"] = "l2"
    with pytest.raises(ValueError) as ei:
        HydraNet(bad)
    assert all(name in str(ei.value) for name in ("smooth_l1", "giou", "diou", "ciou"))
    for kind in R.KINDS:
        c = copy.deepcopy(cfgs)
        c["detection"]["loss_reg_type"] = kind
        net = HydraNet(c)
        assert net.loss_detect is not K.det_loss_hip and net.loss_reg_type == kind and net.det_pos_iou is None
    assert list(HydraNet(c).state_dict()) == list(HydraNet(cfgs).state_dict())        # the key adds no state
    with pytest.raises(ValueError):
        K.det_iou_loss_hip(None, None, None, None, "l2")


def test_library_exports_the_entry_points_and_rejects_a_bad_kind(built):
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    for name in ("hn_det_loss_iou_fwd", "hn_det_loss_iou_bwd"):
        assert name in sig and hasattr(dll, name)
    l = built.lib()
    # HN_CHECK_ARG returns 1 before any launch: the pointers are never dereferenced (1 stands for 'not null')
    for kind in (0, 4, -1):
        assert l.raw("hn_det_loss_iou_fwd")(1, 1, 1, 1, 2, 300, 9, 8, kind, 1, 1, 1, 1, None) == 1
        assert l.raw("hn_det_loss_iou_bwd")(1, 1, 1, 1, 2, 300, 9, 8, kind, 1, 1, 1, 1, 1, None) == 1
    assert l.raw("hn_det_loss_iou_fwd")(None, 1, 1, 1, 2, 300, 9, 8, 1, 1, 1, 1, 1, None) == 1
    assert l.raw("hn_det_loss_iou_fwd")(1, 1, 1, 1, 2, 300, 33, 8, 1, 1, 1, 1, 1, None) == 1          # K beyond the LDS tile's bound
    assert l.raw("hn_det_loss_iou_bwd")(1, 1, 1, 1, 2, 300, 33, 8, 1, 1, 1, 1, 1, 1, None) == 1
