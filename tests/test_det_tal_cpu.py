"""CPU: the task-aligned anchor assignment (detection.assigner = tal).  The numpy float64 reference tests/det_tal_ref.py, which the GPU tests
hold the HIP kernels to, is itself held to a second restatement written independently (torch, one box at a time, float32 like the device,
torch.topk on integer keys built from the float32 t) and to hand-made cases on the 128 x 128 anchor grid whose answers follow from the
geometry; the inputs of the GPU tests are held to the ambiguity cap (the reference's own ambiguous decisions are at most 1 % of its
candidates: a condition on the inputs); the cfg keys are validated by the constructor without a GPU; the library exports the new entry
points and rejects bad arguments before any launch."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import det_atss_ref as RA
from tests import det_iou_ref as RI
from tests import det_tal_ref as R
from tests.helpers import load_cfg, load_npz
from tests.test_det_atss_cpu import DET, concentric_case, random_boxes


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests (tests/test_det_tal_gpu.py imports them): name -> (anchors, annotations, regression, classification, topk)
# ------------------------------------------------------------------------------------------------------------------------------------
def _random_case(h, w, n, mx, box_seed, pred_seed, topk, valid=None):
    anc, _ = RA.make_anchors(h, w, DET)
    cls, reg = R.random_preds(n, anc.shape[0], 9, pred_seed)
    return anc, random_boxes(n, mx, h, w, seed=box_seed, valid=valid), reg, cls, topk


def _recorded(topk):
    z = load_npz("loss_kats.npz")
    cls = np.clip(z["det/cls"] * np.float32(4.5), 0, 1).astype(np.float32)
    return z["det/anchors"].reshape(-1, 4), z["det/ann"], z["det/reg"], cls, topk


CASES = {
    "128x128": lambda: _random_case(128, 128, 3, 8, 1, 1, 13, [8, 5, 0]),
    "128x128 topk 1": lambda: _random_case(128, 128, 3, 8, 3, 3, 1, [8, 5, 0]),
    "128x128 topk above every count": lambda: _random_case(128, 128, 3, 8, 2, 2, 2048, [8, 5, 0]),
    "recorded 128x256": lambda: _recorded(13),
    "recorded 128x256 topk 300": lambda: _recorded(300),      # above the 256 shares of the prefilter: the select on global memory
    "128x256 Mx 1": lambda: _random_case(128, 256, 3, 1, 1, 1, 13),
    "512x1024": lambda: _random_case(512, 1024, 2, 32, 1, 1, 13, [32, 20]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, the reference's result on them): computed once, shared, never written to"""
    inputs = CASES[name]()
    return inputs, R.tal(*inputs[:4], topk=inputs[4])


# ------------------------------------------------------------------------------------------------------------------------------------
# the second restatement: torch, float32, a loop over boxes
# ------------------------------------------------------------------------------------------------------------------------------------
def brute_force(anchors, ann, reg, cls, topk):
    """one image -> (assign int64 [A], target float32 [A])"""
    anc = torch.from_numpy(np.asarray(anchors, np.float32).reshape(-1, 4))
    ann, reg, cls = (torch.from_numpy(np.asarray(v, np.float32)) for v in (ann, reg, cls))
    A, K = anc.shape[0], cls.shape[1]
    acy, acx = (anc[:, 0] + anc[:, 2]) * 0.5, (anc[:, 1] + anc[:, 3]) * 0.5
    assign = torch.full((A,), -1, dtype=torch.long)
    best_u, best_t = torch.full((A,), -1.0), torch.zeros(A)
    for j in range(ann.shape[0]):
        x1, y1, x2, y2, c = ann[j]
        if float(c) == -1.0:
            continue
        s = cls[:, int(c)] if 0 <= float(c) < K else torch.zeros(A)
        _, u, _ = RI.box_losses(reg, anc, ann[j, :4].expand(A, 4), "giou")
        u2 = u * u
        t = (s * (u2 * u2)) * u2
        assert t.dtype == torch.float32
        inside = torch.stack([acx - x1, acy - y1, x2 - acx, y2 - acy]).min(dim=0).values > 0.01
        idx = torch.nonzero(inside & (t > 0))[:, 0]
        if idx.numel() == 0:
            continue
        key = (t[idx].view(torch.int32).long() << 32) | (A - 1 - idx)   # t > 0: the bits order like the value; then the lower index
        for i in idx[torch.topk(key, min(topk, idx.numel())).indices].tolist():
            if u[i] > best_u[i]:                                       # boxes in index order and a strict >: the lowest index keeps a tie
                best_u[i], best_t[i], assign[i] = u[i], t[i], j
    target = torch.zeros(A)
    for j in range(ann.shape[0]):
        mine = assign == j
        if bool(mine.any()):
            target[mine] = best_t[mine] / best_t[mine].max() * best_u[mine].max()
    return assign.numpy(), target.numpy()


def check_against_brute_force(inputs, ref, exact=False, what=""):
    anc, ann, reg, cls, topk = inputs
    got = [brute_force(anc, ann[n], reg[n], cls[n], topk) for n in range(len(ann))]
    worst = R.check(ref, np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), ann.shape[1], exact=exact, what=what)
    assert worst <= 1e-3, (what, worst)           # float32 against float64: t carries six times u's cancellation error
    return sum(int((g[0] >= 0).sum()) for g in got), worst


@pytest.mark.parametrize("name", ["128x128", "128x128 topk 1", "recorded 128x256", "128x256 Mx 1"])
def test_reference_equals_the_brute_force_restatement(name):
    inputs, ref = case(name)
    npos, worst = check_against_brute_force(inputs, ref, what=name)
    print(f"{name}: positives {npos} worst target error {worst:.2e}")
    assert npos > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# the ambiguity cap: a condition on every input a GPU test uses
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_inputs_meet_the_ambiguity_cap(name):
    (anc, ann, reg, cls, topk), ref = case(name)
    n_cand, n_amb = sum(r["n_cand"] for r in ref), sum(r["n_amb"] for r in ref)
    elig = max(int(r["elig"].sum(axis=1).max()) for r in ref)
    print(f"{name}: A {anc.shape[0]} candidates {n_cand} ambiguous {n_amb} most eligible anchors of a box {elig}")
    assert n_cand > 0 and n_amb <= 0.01 * n_cand, (n_amb, n_cand)
    boxes = int((ann[..., 4] != -1).sum())
    if name == "128x128 topk above every count":
        assert elig < topk and n_cand == sum(int(r["elig"].sum()) for r in ref)
    elif topk == 13:
        assert n_cand == 13 * boxes                                      # every box has its 13
    if name.startswith("recorded"):
        assert elig > 2048 and anc.shape[0] == 6138                      # one box's eligible anchors: more than the LDS list holds
        assert (n_cand == 273) == (topk == 13)
    if name == "512x1024":
        assert anc.shape[0] == 98208 and n_cand == 676


# ------------------------------------------------------------------------------------------------------------------------------------
# hand-made cases at 128 x 128: A = 3069; level 3 has its centres at 4 + 8 i, level 4 at 8 + 16 i, level 5 at 16 + 32 i, ...
# ------------------------------------------------------------------------------------------------------------------------------------
NAN_ANCHORS = 3                                                        # image 5: the best three anchors of its box get a NaN regression


@functools.lru_cache(maxsize=None)
def hand_case():
    """[6 images, 3 rows]: two identical boxes around a padding row; a 3 x 3 px box; a box around one level-3 centre; a class id of 9
    with K = 9; no boxes; image 0's first box with a NaN regression on the NAN_ANCHORS anchors that would have been its best"""
    anc, _ = RA.make_anchors(128, 128, DET)
    ann = np.full((6, 3, 5), -1.0, np.float32)
    ann[0, 0] = [20.0, 30.0, 90.0, 100.0, 1.0]
    ann[0, 2] = [20.0, 30.0, 90.0, 100.0, 1.0]
    ann[1, 0] = [61.0, 61.0, 64.0, 64.0, 2.0]
    ann[2, 1] = [58.0, 58.0, 62.0, 62.0, 3.0]
    ann[3, 0] = [20.0, 30.0, 90.0, 100.0, 9.0]
    ann[5, 0] = [20.0, 30.0, 90.0, 100.0, 1.0]
    cls, reg = R.random_preds(6, anc.shape[0], 9, seed=5)
    cls[5], reg[5] = cls[0], reg[0]
    plain = R.tal_image(anc, ann[5], reg[5], cls[5])
    order = np.nonzero(plain["elig"][0])[0]
    order = order[np.lexsort((order, -plain["t"][0, order]))]
    reg[5, order[:NAN_ANCHORS], np.arange(NAN_ANCHORS) % 4] = np.nan     # one NaN each, in dy, dx, dh
    return (anc, ann, reg, cls, 13), R.tal(anc, ann, reg, cls), order


def test_hand_made_cases():
    (anc, ann, reg, cls, topk), res, order = hand_case()
    assert anc.shape == (3069, 4)
    acy, acx = (anc[:, 0] + anc[:, 2]) * np.float32(0.5), (anc[:, 1] + anc[:, 3]) * np.float32(0.5)
    # two identical boxes: the same candidates, and the lower index wins every one of them
    r = res[0]
    assert np.array_equal(r["cand"][0], r["cand"][2]) and r["cand"][0].sum() == 13 and not r["cand"][1].any()
    assert set(np.unique(r["assign"]).tolist()) == {-1, 0} and (r["assign"] == 0).sum() == 13
    pos = r["assign"] == 0
    assert (acx[pos] > 20.0).all() and (acx[pos] < 90.0).all() and (acy[pos] > 30.0).all() and (acy[pos] < 100.0).all()
    assert r["target"][pos].max() == r["u"][0, pos].max() and (r["target"][~pos] == 0).all()      # the best t gets the best u
    # 3 x 3 px: no anchor centre lies inside
    assert not ((acx > 61.01) & (acx < 63.99) & (acy > 61.01) & (acy < 63.99)).any()
    assert (res[1]["assign"] == -1).all() and (res[1]["target"] == 0).all() and not res[1]["elig"].any()
    # one level-3 centre, (60, 60), inside: its nine anchors are all there is, and all are positive
    inside = (np.abs(acx - 60.0) < 2) & (np.abs(acy - 60.0) < 2)
    assert inside.sum() == 9 and np.array_equal(res[2]["assign"] == 1, inside) and (res[2]["assign"][~inside] == -1).all()
    assert (res[2]["target"][inside] > 0).all()
    # a class id of 9 with K = 9: s = 0, nothing is eligible
    assert cls.shape[2] == 9 and (res[3]["assign"] == -1).all() and not res[3]["elig"].any()
    # no boxes
    assert (res[4]["assign"] == -1).all() and (res[4]["target"] == 0).all()
    # a NaN regression: never chosen, and the rest as if those anchors were not there
    assert np.isnan(res[5]["t"][0, order[:NAN_ANCHORS]]).all() and np.array_equal(np.nonzero(res[0]["cand"][0])[0], np.sort(order[:13]))
    assert np.array_equal(np.nonzero(res[5]["assign"] == 0)[0], np.sort(order[NAN_ANCHORS:NAN_ANCHORS + 13]))
    assert [r["n_amb"] for r in res] == [13, 0, 0, 0, 0, 0]             # (the reference counts the identical boxes' ties in u; no other)
    npos, _ = check_against_brute_force((anc, ann, reg, cls, topk), res, exact=True, what="hand-made")
    assert npos == 13 + 9 + 13


@functools.lru_cache(maxsize=None)
def concentric_tal_case():
    """concentric_case() of tests/test_det_atss_cpu.py with regression 0 and a uniform score: anchors i and i + 97 of level 0 are
    identical, so their t ties bit for bit and the index decides"""
    anc, _, ann = concentric_case()
    reg = np.zeros((2, anc.shape[0], 4), np.float32)
    cls = np.full((2, anc.shape[0], 3), 0.5, np.float32)
    return (anc, ann, reg, cls, 13), R.tal(anc, ann, reg, cls)


def test_concentric_anchors_tie_and_the_index_decides():
    inputs, res = concentric_tal_case()
    anc = inputs[0]
    assert np.array_equal(anc[5], anc[5 + 97]) and not np.array_equal(anc[5], anc[6])
    for r, j in ((res[0], 0), (res[0], 2), (res[1], 1)):
        c = np.nonzero(r["cand"][j])[0]
        assert c.size == 13
        for i in c[c < 4096]:                                          # every identical anchor with a lower index is a candidate too
            twins = np.arange(i % 97, i, 97)
            assert r["cand"][j, twins].all() and (r["t"][j, twins] == r["t"][j, i]).all()
        assert (c < 4096).sum() > 1                                    # (so ties were there to be decided)
    npos, _ = check_against_brute_force(inputs, res, exact=True, what="concentric")
    assert npos > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# the cfg keys, the exported symbols, the argument checks
# ------------------------------------------------------------------------------------------------------------------------------------
def test_constructor_validates_the_assigner_keys(built):
    import functools as ft
    from multitask_hydranet_amd import HydraNet
    from multitask_hydranet_amd import ops as K
    cfgs = load_cfg("hydranet_tiny.yml")
    assert "assigner" not in cfgs["detection"] and "tal_topk" not in cfgs["detection"]
    for reg_kind in ("smooth_l1", "giou", "diou", "ciou"):
        for cls_kind in ("focal", "qfl", "vfl"):
            if reg_kind == "smooth_l1" and cls_kind != "focal":
                continue
            c = copy.deepcopy(cfgs)
            c["detection"].update(loss_reg_type=reg_kind, loss_cls_type=cls_kind)
            plain = HydraNet(copy.deepcopy(c))
            c["detection"]["assigner"] = "tal"
            net = HydraNet(c)
            assert net.det_assigner == "tal" and net.tal_topk == 13 and net.atss_topk == 9
            # loss_detect is what the same loss keys give without the assigner: assign and target are passed at call time
            if isinstance(plain.loss_detect, ft.partial):
                assert net.loss_detect.func is plain.loss_detect.func and net.loss_detect.keywords == plain.loss_detect.keywords
            else:
                assert net.loss_detect is plain.loss_detect is K.det_loss_hip
    c["detection"]["tal_topk"] = 4
    assert HydraNet(c).tal_topk == 4
    assert list(HydraNet(c).state_dict()) == list(HydraNet(cfgs).state_dict())        # the keys add no state
    bad = copy.deepcopy(cfgs)
    bad["detection"]["assigner"] = "simota"
    with pytest.raises(ValueError) as ei:
        HydraNet(bad)
    assert all(k in str(ei.value) for k in ("max_iou", "atss", "tal"))
    for k in (0, -3, 2.5, "13", True):
        bad = copy.deepcopy(cfgs)
        bad["detection"].update(assigner="tal", tal_topk=k)
        with pytest.raises(ValueError):
            HydraNet(bad)


def test_library_exports_the_entry_points_and_rejects_bad_arguments(built):
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    for name in ("hn_det_tal_assign", "hn_det_tal_ws_bytes", "hn_det_loss_aligned_fwd", "hn_det_loss_aligned_bwd"):
        assert name in sig and hasattr(dll, name)
    l = built.lib()
    f = l.raw("hn_det_tal_assign")
    # HN_CHECK_ARG returns 1 before any launch: the device pointers are never dereferenced (1 and 16 stand for 'not null')
    ok = dict(anchors=16, reg=32, cls=1, ann=1, N=2, A=3069, K=9, Mx=8, topk=13, ws=1, assign=1, target=1)
    call = lambda **kw: f(*{**ok, **kw}.values(), None)
    for name in ("anchors", "reg", "cls", "ann", "ws", "assign", "target"):
        assert call(**{name: None}) == 1, name
    assert call(anchors=20) == 1 and call(reg=40) == 1                  # an anchor and a regression row are 16-byte loads
    assert call(topk=0) == 1 and call(topk=-1) == 1 and call(topk=2049) == 1          # the LDS list's capacity
    assert call(N=0) == 1 and call(N=65536) == 1 and call(Mx=0) == 1 and call(Mx=32768) == 1 and call(A=0) == 1
    assert call(K=0) == 1 and call(K=33) == 1
    q = l.raw("hn_det_tal_ws_bytes")
    assert q(2, 3069, 8, 13) == 256 + 2 * 8 * 8 and q(16, 98208, 32, 2048) == 16 * 32 * 8 + 16 * 32 * 8
    for bad in ((0, 3069, 8, 13), (65536, 3069, 8, 13), (2, 0, 8, 13), (2, 3069, 0, 13), (2, 3069, 32768, 13), (2, 3069, 8, 0), (2, 3069, 8, 2049)):
        assert q(*bad) == -1, bad
    fwd, bwd = l.raw("hn_det_loss_aligned_fwd"), l.raw("hn_det_loss_aligned_bwd")
    okf = dict(cls=1, reg=1, anc=1, ann=1, N=2, A=300, K=9, Mx=8, kind=1, cls_kind=1, valid=None, given=1, assign=1, target=1, part=1, npos=1, out=1)
    callf = lambda **kw: fwd(*{**okf, **kw}.values(), None)
    assert callf(target=None) == 1 and callf(given=0) == 1 and callf(kind=0) == 1 and callf(kind=4) == 1 and callf(cls_kind=0) == 1
    assert callf(cls_kind=3) == 1 and callf(assign=None) == 1 and callf(K=33) == 1
    okb = dict(cls=1, reg=1, anc=1, ann=1, N=2, A=300, K=9, Mx=8, kind=1, cls_kind=2, valid=None, assign=1, target=1, npos=1, gout=1, dcls=1, dreg=1)
    callb = lambda **kw: bwd(*{**okb, **kw}.values(), None)
    assert callb(target=None) == 1 and callb(kind=0) == 1 and callb(cls_kind=0) == 1 and callb(assign=None) == 1 and callb(K=33) == 1
    from multitask_hydranet_amd import ops as K
    with pytest.raises(ValueError) as ei:
        K.det_tal_assign(torch.zeros(3069, 4), torch.zeros(1, 3069, 4), torch.zeros(1, 3069, 9), torch.zeros(1, 2, 5), topk=4096)
    assert "2048" in str(ei.value) and "65535" in str(ei.value)
    with pytest.raises(ValueError):                                     # a target without a quality term
        K.det_iou_loss_hip(torch.zeros(1, 8, 9), torch.zeros(1, 8, 4), torch.zeros(8, 4), torch.zeros(1, 2, 5), "giou",
                           assign=torch.zeros(1, 8, dtype=torch.int16), target=torch.zeros(1, 8))
