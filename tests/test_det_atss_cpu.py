"""CPU: the ATSS anchor assignment (detection.assigner = atss).  The numpy reference tests/det_atss_ref.py, which the GPU tests hold the HIP
kernels to, is itself held to a second restatement written independently (torch, one box and one level at a time, torch.topk on the
integer keys) and to hand-made boxes whose answers follow from the geometry of the 128 x 128 anchor grid; the cfg keys are validated by the
constructor without a GPU; the library exports the new entry points and rejects bad arguments before any launch."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import det_atss_ref as R
from tests.helpers import load_cfg, load_npz


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


DET = load_cfg("hydranet_tiny.yml")["detection"]


def random_boxes(n, mx, h, w, seed, valid=None):
    """log-uniform sides between 6 px and the image, uniform centres, clipped to the image; rows beyond valid[i] are padding"""
    g = np.random.default_rng(seed)
    ann = np.full((n, mx, 5), -1.0, np.float32)
    for i in range(n):
        m = mx if valid is None else valid[i]
        side = np.exp(g.uniform(np.log(6.0), np.log(float(max(h, w))), (m, 2)))
        c = g.uniform(0, 1, (m, 2)) * [w, h]
        ann[i, :m, 0] = np.clip(c[:, 0] - side[:, 0] / 2, 0, w - 1)
        ann[i, :m, 1] = np.clip(c[:, 1] - side[:, 1] / 2, 0, h - 1)
        ann[i, :m, 2] = np.clip(c[:, 0] + side[:, 0] / 2, 0, w - 1)
        ann[i, :m, 3] = np.clip(c[:, 1] + side[:, 1] / 2, 0, h - 1)
        ann[i, :m, 4] = g.integers(0, 9, m)
    return ann


# ------------------------------------------------------------------------------------------------------------------------------------
# the second restatement: torch, a loop over boxes and levels
# ------------------------------------------------------------------------------------------------------------------------------------
def brute_force(anchors, level_sizes, ann, topk=9, apl=9):
    anc = torch.from_numpy(np.asarray(anchors, np.float32).reshape(-1, 4))
    ann = torch.from_numpy(np.asarray(ann, np.float32))
    A = anc.shape[0]
    assign = torch.full((A,), -1, dtype=torch.long)
    thr = torch.full((ann.shape[0],), float("nan"), dtype=torch.float64)
    best = torch.full((A,), -1.0, dtype=torch.float64)
    acy, acx = (anc[:, 0] + anc[:, 2]) * 0.5, (anc[:, 1] + anc[:, 3]) * 0.5
    a64 = anc.double()
    for j in range(ann.shape[0]):
        x1, y1, x2, y2, c = ann[j]
        if float(c) == -1.0:
            continue
        gcx, gcy = (x1 + x2) * 0.5, (y1 + y2) * 0.5
        dx, dy = acx - gcx, acy - gcy
        d2 = dx * dx + dy * dy
        assert d2.dtype == torch.float32
        picked, off = [], 0
        for size in level_sizes:
            key = (d2[off:off + size].view(torch.int32).long() << 32) | torch.arange(size)
            picked.append(off + torch.topk(key, min(topk * apl, size), largest=False).indices)
            off += size
        idx = torch.cat(picked)
        bx1, by1, bx2, by2 = (float(v) for v in (x1, y1, x2, y2))
        iw = (torch.clamp(a64[idx, 3], max=bx2) - torch.clamp(a64[idx, 1], min=bx1)).clamp(min=0)
        ih = (torch.clamp(a64[idx, 2], max=by2) - torch.clamp(a64[idx, 0], min=by1)).clamp(min=0)
        union = (a64[idx, 2] - a64[idx, 0]) * (a64[idx, 3] - a64[idx, 1]) + (bx2 - bx1) * (by2 - by1) - iw * ih
        iou = iw * ih / union.clamp(min=1e-8)
        thr[j] = iou.mean() + (iou.std(unbiased=True) if iou.numel() > 1 else 0.0)
        cx, cy = acx[idx].double(), acy[idx].double()
        inside = torch.stack([cx - bx1, cy - by1, bx2 - cx, by2 - cy]).min(dim=0).values > 0.01
        for i, v, ok in zip(idx.tolist(), iou.tolist(), (inside & (iou >= thr[j])).tolist()):
            if ok and v > best[i]:                                     # boxes in index order and a strict >: the lowest index keeps a tie
                best[i], assign[i] = v, j
    return assign.numpy(), thr.numpy()


def check_against_brute_force(anchors, sizes, ann, topk=9):
    total = 0
    for n, r in enumerate(R.atss(anchors, sizes, ann, topk=topk)):
        want_assign, want_thr = brute_force(anchors, sizes, ann[n], topk=topk)
        assert np.array_equal(r["assign"], want_assign), n
        v = ann[n, :, 4] != -1
        assert np.all(np.isnan(r["thr"][~v])) and np.allclose(r["thr"][v], want_thr[v], rtol=0, atol=1e-12)
        assert not (r["assign"] == -2).any() and r["assign"].max() < ann.shape[1]
        total += int((r["assign"] >= 0).sum())
    return total


def test_reference_equals_the_brute_force_restatement_on_the_recorded_inputs():
    z = load_npz("loss_kats.npz")
    anc, ann = z["det/anchors"].reshape(-1, 4), z["det/ann"]
    mine, sizes = R.make_anchors(128, 256, DET)
    assert np.array_equal(mine, anc) and sizes == [4608, 1152, 288, 72, 18]
    assert check_against_brute_force(anc, sizes, ann) > 0
    assert not (R.atss(anc, sizes, ann)[2]["assign"] >= 0).any()        # the recorded image without boxes


@pytest.mark.parametrize("topk", [1, 9])
def test_reference_equals_the_brute_force_restatement_on_random_boxes(topk):
    anc, sizes = R.make_anchors(128, 128, DET)
    ann = random_boxes(3, 8, 128, 128, seed=11 + topk, valid=[8, 3, 1])
    assert check_against_brute_force(anc, sizes, ann, topk=topk) > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# hand-made boxes at 128 x 128: A = 3069, levels 2304 / 576 / 144 / 36 / 9 (level 7: k_l = A_l)
# ------------------------------------------------------------------------------------------------------------------------------------
HAND = {
    "corner": [44.0, 44.0, 84.0, 84.0],          # centre (64, 64): a corner of four level-3 cells
    "whole": [0.0, 0.0, 128.0, 128.0],
    "tiny": [61.0, 61.0, 64.0, 64.0],            # 3 x 3 px between the level-3 centres 60 and 68
    "half_out": [-40.0, 30.0, 40.0, 90.0],
}


def hand_ann():
    """[6, 3, 5]: the four boxes above alone, two identical boxes around a padding row, an image without boxes"""
    ann = np.full((6, 3, 5), -1.0, np.float32)
    for i, k in enumerate(("corner", "whole", "tiny", "half_out")):
        ann[i, 0] = HAND[k] + [float(i)]
    ann[4, 0] = [20.0, 30.0, 90.0, 100.0, 1.0]
    ann[4, 2] = [20.0, 30.0, 90.0, 100.0, 2.0]
    return ann


def test_hand_made_boxes():
    anc, sizes = R.make_anchors(128, 128, DET)
    assert anc.shape == (3069, 4) and sizes == [2304, 576, 144, 36, 9]
    res = R.atss(anc, sizes, hand_ann())
    acy, acx = (anc[:, 0] + anc[:, 2]) * np.float32(0.5), (anc[:, 1] + anc[:, 3]) * np.float32(0.5)
    # corner: on level 3 (16 x 16 cells of 8 px, 9 anchors each) the four cells around (64, 64) tie at d2 = 32, then eight cells tie at
    # d2 = 160, of which five are needed: the five lowest indices, cells (row, col) in row-major order
    r = res[0]
    d2 = R.distances(anc, np.array([HAND["corner"]], np.float32))[0]
    cells = lambda rc: [(y * 16 + x) * 9 for y, x in rc]
    ring0, ring1 = cells([(7, 7), (7, 8), (8, 7), (8, 8)]), cells([(6, 7), (6, 8), (7, 6), (7, 9), (8, 6), (8, 9), (9, 7), (9, 8)])
    assert all(d2[i] == 32.0 for i in ring0) and all(d2[i] == 160.0 for i in ring1)          # the ties are exact in float32
    got = sorted(set((np.nonzero(r["cand"][0, :2304])[0] // 9).tolist()))
    assert got == sorted(c // 9 for c in ring0 + ring1[:5]) and int(r["cand"][0, :2304].sum()) == 81
    assert int(r["cand"][0].sum()) == 81 * 3 + 36 + 9 and r["cand"][0, 3024:].all()         # levels 6 and 7: k_l = A_l
    pos = r["assign"] >= 0
    assert pos.sum() > 0 and (r["iou"][0, pos] >= r["thr"][0]).all() and r["cand"][0, pos].all()
    # whole image: every positive is a candidate at or above the threshold with its centre inside; the threshold is mean + std
    r = res[1]
    pos = r["assign"] >= 0
    v = r["iou"][0, r["cand"][0]]
    assert v.size == 288 and abs(r["thr"][0] - (v.mean() + v.std(ddof=1))) < 1e-12
    assert pos.sum() == 57 and (pos == (r["cand"][0] & (r["iou"][0] >= r["thr"][0]))).all()
    # 3 x 3 px: no anchor centre lies inside (they sit at 4 + 8 i on level 3, coarser above), so nothing is positive
    assert not ((acx > 61.01) & (acx < 63.99) & (acy > 61.01) & (acy < 63.99)).any()
    assert not (res[2]["assign"] >= 0).any() and res[2]["thr"][0] > 0
    # half outside: positives exist and none has its centre left of the image's edge side of the box ... or outside the box at all
    r = res[3]
    pos = r["assign"] >= 0
    assert pos.sum() == 42 and (acx[pos] > -40.0).all() and (acx[pos] < 40.0).all() and (acy[pos] > 30.0).all() and (acy[pos] < 90.0).all()
    # two identical boxes: the lower index wins every anchor
    r = res[4]
    assert set(np.unique(r["assign"]).tolist()) == {-1, 0} and np.array_equal(r["cand"][0], r["cand"][2]) and r["thr"][0] == r["thr"][2]
    assert np.isnan(r["thr"][1])
    # no boxes
    assert (res[5]["assign"] == -1).all() and np.isnan(res[5]["thr"]).all()


def concentric_case():
    """4096 concentric anchors (one centre, sides growing with index % 97) as level 0 and nine distinct anchors as level 1: every
    distance on level 0 ties, so the 81 candidates are the indices 0..80 and twelve index bits decide (no prefilter can shrink this)"""
    i = np.arange(4096)
    half = (10.0 + (i % 97) * 0.25).astype(np.float32)
    lvl0 = np.stack([64.0 - half, 64.0 - half * 1.5, 64.0 + half, 64.0 + half * 1.5], axis=1).astype(np.float32)
    c = np.array([[y, x] for y in (32.0, 64.0, 96.0) for x in (32.0, 64.0, 96.0)], np.float32)
    lvl1 = np.concatenate([c - 40.0, c + 40.0], axis=1)
    ann = np.full((2, 3, 5), -1.0, np.float32)
    ann[0, 0] = [30.0, 44.0, 95.0, 90.0, 1.0]
    ann[0, 2] = [50.0, 50.0, 81.0, 79.0, 2.0]
    ann[1, 1] = [10.0, 20.0, 120.0, 110.0, 0.0]
    return np.concatenate([lvl0, lvl1]), [4096, 9], ann


def test_concentric_anchors_are_taken_by_index():
    anc, sizes, ann = concentric_case()
    res = R.atss(anc, sizes, ann)
    for r, j in ((res[0], 0), (res[0], 2), (res[1], 1)):
        assert np.array_equal(np.nonzero(r["cand"][j])[0], np.concatenate([np.arange(81), 4096 + np.arange(9)]))
    assert check_against_brute_force(anc, sizes, ann) > 0 and sum(r["n_amb"] for r in res) == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# the cfg keys, the exported symbols, the argument checks
# ------------------------------------------------------------------------------------------------------------------------------------
def test_constructor_validates_the_assigner_keys(built):
    from multitask_hydranet_amd import HydraNet
    from multitask_hydranet_amd import ops as K
    cfgs = load_cfg("hydranet_tiny.yml")
    assert "assigner" not in cfgs["detection"] and "atss_topk" not in cfgs["detection"]
    net = HydraNet(copy.deepcopy(cfgs))
    assert net.loss_detect is K.det_loss_hip and net.det_assigner == "max_iou"
    explicit = copy.deepcopy(cfgs)
    explicit["detection"]["assigner"] = "max_iou"
    net = HydraNet(explicit)
    assert net.loss_detect is K.det_loss_hip and net.det_assigner == "max_iou"
    for kind in ("smooth_l1", "giou", "diou", "ciou"):
        c = copy.deepcopy(cfgs)
        c["detection"].update(assigner="atss", loss_reg_type=kind)
        net = HydraNet(c)
        assert net.det_assigner == "atss" and net.atss_topk == 9 and net.loss_reg_type == kind
        assert (net.loss_detect is K.det_loss_hip) == (kind == "smooth_l1")
    c["detection"]["atss_topk"] = 4
    assert HydraNet(c).atss_topk == 4
    assert list(HydraNet(c).state_dict()) == list(HydraNet(cfgs).state_dict())        # the keys add no state
    bad = copy.deepcopy(cfgs)
    bad["detection"]["assigner"] = "simota"
    with pytest.raises(ValueError) as ei:
        HydraNet(bad)
    assert "max_iou" in str(ei.value) and "atss" in str(ei.value)
    for k in (0, -3, 2.5, "9", True):
        bad = copy.deepcopy(cfgs)
        bad["detection"].update(assigner="atss", atss_topk=k)
        with pytest.raises(ValueError):
            HydraNet(bad)
    # anchors_for's companion
    net = HydraNet(copy.deepcopy(cfgs))
    for h, w in ((128, 128), (128, 256)):
        anc, sizes = R.make_anchors(h, w, cfgs["detection"])
        assert net.anchor_level_sizes(h, w) == sizes and net.anchors_per_location == 9
        assert np.array_equal(net.anchors_for(h, w, "cpu")[0].numpy(), anc)


def test_library_exports_the_entry_points_and_rejects_bad_arguments(built):
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    for name in ("hn_det_atss_assign", "hn_det_atss_ws_bytes", "hn_det_loss_fwd_assigned", "hn_det_loss_iou_fwd_assigned"):
        assert name in sig and hasattr(dll, name)
    l = built.lib()
    sizes = (ctypes.c_int * 5)(2304, 576, 144, 36, 9)
    sp = ctypes.addressof(sizes)
    f = l.raw("hn_det_atss_assign")
    # HN_CHECK_ARG returns 1 before any launch: the device pointers are never dereferenced (1 and 16 stand for 'not null')
    ok = dict(anchors=16, ann=1, N=2, A=3069, Mx=8, sizes=sp, L=5, topk=9, apl=9, ws=1, assign=1, thr=1)
    call = lambda **kw: f(*{**ok, **kw}.values(), None)
    for name in ("anchors", "ann", "sizes", "ws", "assign", "thr"):
        assert call(**{name: None}) == 1, name
    assert call(topk=0) == 1 and call(topk=-1) == 1 and call(apl=0) == 1
    assert call(anchors=20) == 1                                        # anchors are read as 16-byte rows
    assert call(topk=114) == 1                                          # 114 * 9 candidates exceed the LDS lists
    assert call(A=3068) == 1 and call(A=3070) == 1 and call(L=4) == 1   # the offsets do not sum to A
    assert call(L=0) == 1 and call(L=9) == 1 and call(N=0) == 1 and call(Mx=0) == 1
    q = l.raw("hn_det_atss_ws_bytes")
    assert q(2, 3069, 8, sp, 5, 9, 9) == (2 * 8 * 5 * 8 + 255) // 256 * 256 + 2 * 8 * (81 * 3 + 36 + 9) * 4
    assert q(2, 3068, 8, sp, 5, 9, 9) == -1 and q(2, 3069, 8, sp, 5, 0, 9) == -1
    for kind in (0, 4):
        assert l.raw("hn_det_loss_iou_fwd_assigned")(1, 1, 1, 1, 2, 300, 9, 8, kind, 1, 1, 1, 1, None) == 1
    assert l.raw("hn_det_loss_iou_fwd_assigned")(1, 1, 1, 1, 2, 300, 9, 8, 1, None, 1, 1, 1, None) == 1
    assert l.raw("hn_det_loss_fwd_assigned")(1, 1, 1, 1, 2, 300, 9, 8, None, 1, 1, 1, None) == 1
    assert l.raw("hn_det_loss_fwd_assigned")(1, 1, 1, 1, 2, 300, 33, 8, 1, 1, 1, 1, None) == 1
    from multitask_hydranet_amd import ops as K
    with pytest.raises(ValueError):
        K.det_atss_assign(torch.zeros(3069, 4), [2304, 576, 144, 36], torch.zeros(1, 2, 5))


def test_losses_given_assign_equals_the_loss_references_under_their_own_assignment():
    """det_atss_ref.losses_given_assign, the loss reference of the GPU tests, handed the max-IoU assignment (>= 0.5 positive, < 0.4
    background, between ignored) reproduces tests/torch_losses.det_loss and tests/det_iou_ref.det_iou_loss on the recorded inputs"""
    from tests import det_iou_ref as RI
    from tests import torch_losses as L
    z = load_npz("loss_kats.npz")
    t = lambda k: torch.from_numpy(z[k]).double()
    cls, reg, anc, ann = t("det/cls"), t("det/reg"), t("det/anchors").reshape(-1, 4), t("det/ann")
    assign = torch.full((3, anc.shape[0]), -1, dtype=torch.long)
    for n in range(3):
        valid = ann[n, :, 4] != -1
        if not bool(valid.any()):
            continue
        iou = torch.from_numpy(R.iou_matrix(anc.numpy(), ann[n, :, :4].numpy()))
        iou[~valid] = -1.0
        best, arg = iou.max(dim=0)
        assign[n] = torch.where(best >= 0.5, arg, torch.where(best < 0.4, torch.tensor(-1), torch.tensor(-2)))
    assert [int((assign[n] >= 0).sum()) for n in range(3)] == [71, 35, 0] and int((assign == -2).sum()) > 0
    want_c, want_r = L.det_loss(cls, reg, anc[None], ann)
    got = R.losses_given_assign(cls, reg, anc, ann, assign)
    assert abs(float(got["cls"]) - float(want_c)) <= 1e-12 * float(want_c) and abs(float(got["reg"]) - float(want_r)) <= 1e-12 * float(want_r)
    for kind in RI.KINDS:
        want = RI.det_iou_loss(cls, reg, anc, ann, kind)
        got = R.losses_given_assign(cls, reg, anc, ann, assign, kind)
        for k in ("cls", "reg", "pos_iou"):
            assert abs(float(got[k]) - float(want[k])) <= 1e-12 * abs(float(want[k])), (kind, k)
        assert got["npos"] == want["npos"] and got["margin"] == want["margin"]
