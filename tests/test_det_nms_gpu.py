"""GPU: the detection NMS options (hn_det_postprocess_ex: hard, DIoU, Soft-NMS linear / gaussian, max_det, class-agnostic)
against the numpy restatement tests/det_nms_ref.py.

The inputs have regression 0 and integer-valued anchor boxes, so decode and clip are exact and every comparison is EXACT: kept counts,
order, class ids, box bits and score bits.  (The five output arrays carry no anchor index: the order is checked through the boxes,
classes and scores of the rows.)  The conditions that keep these comparisons from passing vacuously are asserted on the reference in
tests/test_det_nms_cpu.py; the ones a case here depends on are asserted again where it builds its inputs."""
import numpy as np
import pytest
import torch

from tests import det_nms_ref as R
from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu

THR, IOU, SIGMA = 0.05, 0.5, 0.5
SOFT_THREADS = 1024          # workgroup size of the soft kernel (hn_post.hip SOFT_NT)
SOFT_REG_BOXES = 4096        # candidates whose boxes the soft kernel holds in registers (SOFT_RB * SOFT_NT)
SOFT_LDS_N = 8192            # candidates whose working scores live in LDS; more: the workspace


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    import multitask_hydranet_amd as P
    return P


def options(kind="hard", **kw):
    from multitask_hydranet_amd.postprocess import NmsOptions
    return NmsOptions(kind=kind, sigma=SIGMA, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def device_rows(res):
    """postprocess_device's dict -> per image (class ids, boxes, scores) of the kept rows, on the host"""
    kept = res["kept"].cpu().numpy()
    c, b, s = res["class_ids"].cpu().numpy(), res["rois"].cpu().numpy(), res["scores"].cpu().numpy()
    assert int(kept.max(initial=0)) <= res["cap"]
    return [(c[i, :k].copy(), b[i, :k].copy(), s[i, :k].copy()) for i, k in enumerate(kept)]


def run_device(inputs, hw, nms, cap=4096, thr=THR, iou=IOU):
    from multitask_hydranet_amd.postprocess import postprocess_device
    anchors, reg, cls = (torch.from_numpy(v).cuda() for v in inputs)
    return postprocess_device(hw, anchors, reg, cls, thr, iou, cap, nms=nms)


def assert_rows_equal(mine, ref, what=""):
    """mine: device_rows(); ref: det_nms_ref.nms_batch() -- counts, classes, box bits and score bits"""
    assert len(mine) == len(ref)
    for i, ((c, b, s), (_, rc, rb, rs)) in enumerate(zip(mine, ref)):
        assert len(c) == len(rc), "%s image %d: kept %d, reference %d" % (what, i, len(c), len(rc))
        assert np.array_equal(c, rc), (what, i)
        assert np.array_equal(bits(b), bits(rb).reshape(-1, 4)), (what, i)
        diff = np.nonzero(bits(s) != bits(rs))[0]
        assert len(diff) == 0, "%s image %d: %d of %d scores differ, first at row %d: %r vs %r" % (
            what, i, len(diff), len(s), diff[0], s[diff[0]], rs[diff[0]])


def check(inputs, hw, cap=4096, what="", **opts):
    nms = options(**opts)
    res = run_device(inputs, hw, nms, cap)
    assert np.array_equal(res["total"].cpu().numpy(), R.count_over(inputs[2], THR))
    ref = R.nms_batch(*inputs, hw, THR, IOU, sigma=SIGMA, **opts)
    assert_rows_equal(device_rows(res), ref, what or repr(nms))
    return ref


@pytest.fixture(scope="module")
def base():
    """case 1's batch: the recipe, an image with no score over the threshold, an image with one candidate"""
    a = R.recipe()
    b = R.recipe(seed=8)
    b = (b[0], b[1], b[2] * np.float32(0.01))
    c = R.recipe(seed=9, keep=1)
    inputs = R.batch_of([a, b, c])
    assert list(R.count_over(inputs[2], THR)) == [246, 0, 1]
    return inputs


# ---- 1. every kind, class-aware and class-agnostic --------------------------------------------------------------------------------------
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("kind", R.KINDS)
def test_kinds_on_the_base_recipe(pkg, base, kind, agnostic):
    ref = check(base, (128, 128), kind=kind, class_agnostic=agnostic)
    assert len(ref[0][0]) > 50 and len(ref[1][0]) == 0 and len(ref[2][0]) == 1


# ---- 2. candidate counts where a wave loop, the workgroup loop or a storage choice changes ---------------------------------------------
def sized(count):
    """one image of the recipe with exactly `count` candidates; the frame grows with the count so that the boxes do not all overlap"""
    frame = 128 if count <= 260 else 256 if count <= 2500 else 512
    inputs = R.batch_of([R.recipe(seed=11 + count, clusters=count // 12 + 2, frame=frame, keep=count)])
    assert list(R.count_over(inputs[2], THR)) == [count]
    return inputs, (frame, frame)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("count", [1, 63, 64, 65, SOFT_THREADS - 1, SOFT_THREADS + 1, 2 * SOFT_THREADS + 52])
def test_candidate_count_boundaries(pkg, kind, count):
    inputs, hw = sized(count)
    check(inputs, hw, kind=kind)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("count", [SOFT_REG_BOXES, SOFT_REG_BOXES + 1, SOFT_LDS_N, SOFT_LDS_N + 1])
def test_storage_boundaries(pkg, kind, count):
    """either side of the soft kernel's register / L2 box boundary and of its LDS / workspace boundary (max_det keeps the walk short)"""
    inputs, hw = sized(count)
    ref = check(inputs, hw, cap=16384, kind=kind, max_det=100)
    assert len(ref[0][0]) == 100


# ---- 3. max_det ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hard", "soft_gaussian"])
def test_max_det_is_a_prefix(pkg, base, kind):
    full = device_rows(run_device(base, (128, 128), options(kind)))
    k0 = len(full[0][0])
    assert k0 > 10
    for max_det in (1, 10, k0, k0 + 1):
        res = run_device(base, (128, 128), options(kind, max_det=max_det))
        assert np.array_equal(res["total"].cpu().numpy(), [246, 0, 1])
        assert np.array_equal(res["kept"].cpu().numpy(), [min(k0, max_det), 0, 1])
        for got, want in zip(device_rows(res), full):
            for u, v in zip(got, want):
                assert np.array_equal(u, v[:max_det])
        check(base, (128, 128), kind=kind, max_det=max_det)


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_equal_scores_keep_the_anchor_order(pkg, kind):
    """40 overlapping boxes of one class share one score, among the recipe's other boxes: the anchor index decides at every step"""
    anchors, reg, cls = R.recipe(seed=21, clusters=6)
    g = np.random.default_rng(5)
    lo, hi = g.integers(30, 42, (40, 2)), g.integers(70, 90, (40, 2))
    tied = np.concatenate([lo, hi], axis=1).astype(np.float32)
    at = g.permutation(len(anchors))[:40]
    anchors[at] = tied
    cls[at] = 0
    cls[at, 1] = 0.5
    ref = check(R.batch_of([(anchors, reg, cls)]), (128, 128), kind=kind)
    if kind.startswith("soft"):
        assert len(set(at) & set(ref[0][0])) >= 2


# ---- 5. degenerate boxes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("kind", R.KINDS)
def test_degenerate_boxes(pkg, kind, agnostic):
    """zero-area boxes at one point (their IoU is 0 / 0), a box that covers the frame, ordinary boxes around them"""
    anchors, reg, cls = R.recipe(seed=22, clusters=4)
    anchors[:6] = [40, 50, 40, 50]
    anchors[6] = [0, 0, 127, 127]
    anchors[7] = [40, 30, 40, 90]                                     # zero height
    cls[:8] = 0
    cls[:8, 0] = [0.5, 0.5, 0.75, 0.25, 0.5, 0.125, 0.625, 0.5]
    ref = check(R.batch_of([(anchors, reg, cls)]), (128, 128), kind=kind, class_agnostic=agnostic)
    assert {0, 1, 2, 3, 4, 5} <= set(ref[0][0])                       # a NaN IoU suppresses nothing


# ---- 6. new entry point versus the old one -----------------------------------------------------------------------------------------------------
def assert_same_outputs(a, b):
    assert a["cap"] == b["cap"]
    kept = a["kept"].cpu().numpy()
    assert np.array_equal(kept, b["kept"].cpu().numpy()) and torch.equal(a["total"], b["total"])
    for i, k in enumerate(kept):
        for name in ("rois", "class_ids", "scores"):
            assert torch.equal(a[name][i, :k], b[name][i, :k]), (name, i)
    return int(kept.sum())


def test_hard_defaults_equal_the_old_entry_point(pkg, base):
    assert assert_same_outputs(run_device(base, (128, 128), None), run_device(base, (128, 128), options("hard"))) > 50


def test_hard_defaults_equal_the_old_entry_point_fullsize(pkg):
    """98 208 anchors x 9 classes at 512 x 1024, real-valued regression, about 2 000 candidates per image"""
    from oracle import hydranet_oracle as O
    H, W = 512, 1024
    anchors = O.anchors_for(H, W, load_cfg("hydranet_big.yml")).astype(np.float32)
    g = torch.Generator().manual_seed(3)
    n, a = 2, len(anchors)
    reg = (torch.randn(n, a, 4, generator=g) * 0.2).numpy()
    cls = torch.sigmoid(torch.randn(n, a, 9, generator=g) * 1.5 - 4.0).numpy()
    thr = float(np.sort(cls.max(axis=2), axis=1)[:, -2000].max())
    inputs = (anchors, reg, cls)
    old = run_device(inputs, (H, W), None, thr=thr, iou=0.4)
    new = run_device(inputs, (H, W), options("hard"), thr=thr, iou=0.4)
    total = old["total"].cpu().numpy()
    assert total.min() > 1500 and total.max() <= 2000
    assert assert_same_outputs(old, new) > 500


# ---- 7. capacity overflow ----------------------------------------------------------------------------------------------------------------------
def test_overflow_retry_runs_with_the_options(pkg):
    from multitask_hydranet_amd.postprocess import postprocess
    inputs, hw = sized(4500)                                          # over postprocess's first capacity of 4096
    nms = options("soft_linear", max_det=100)
    out = postprocess(hw, *(torch.from_numpy(v).cuda() for v in inputs), THR, IOU, nms=nms)
    ref = R.nms_batch(*inputs, hw, THR, IOU, kind="soft_linear", sigma=SIGMA, max_det=100)
    assert len(ref[0][0]) == 100
    assert_rows_equal([(o["class_ids"], o["rois"], o["scores"]) for o in out], ref)


# ---- 8. capture ---------------------------------------------------------------------------------------------------------------------------------
def test_soft_gaussian_under_graph_capture(pkg, base):
    from multitask_hydranet_amd.postprocess import postprocess_device
    nms = options("soft_gaussian")
    variants = [base, R.batch_of([R.recipe(seed=s) for s in (31, 32, 33)]), R.batch_of([R.recipe(seed=s) for s in (34, 35, 36)])]
    anchors = torch.from_numpy(base[0]).cuda()
    for v in variants:
        assert np.array_equal(v[0].shape, base[0].shape)
    eager = []
    for v in variants:
        runs = [device_rows(run_device((base[0], v[1], v[2]), (128, 128), nms)) for _ in range(2)]
        for x, y in zip(*runs):
            assert all(np.array_equal(bits(u) if u.dtype == np.float32 else u, bits(w) if w.dtype == np.float32 else w) for u, w in zip(x, y))
        eager.append(runs[0])
    reg, cls = torch.from_numpy(base[1]).cuda(), torch.from_numpy(base[2]).cuda()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        res = postprocess_device((128, 128), anchors, reg, cls, THR, IOU, 4096, nms=nms)
    for v, want in list(zip(variants, eager))[1:]:
        cls.copy_(torch.from_numpy(v[2]))
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(device_rows(res), want):
            assert len(x[0]) == len(y[0]) and len(y[0]) > 50
            assert np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1])) and np.array_equal(bits(x[2]), bits(y[2]))


# ---- 9. plumbing ----------------------------------------------------------------------------------------------------------------------------------
def assert_rows_close(mine, ref):
    """for real-valued boxes: the device's expf and the host's exp differ by an ulp in a box corner (rtol 5e-6, atol 1e-5, as
    tests/test_post_gpu.py states it); an IoU then moves by a few 1e-6 relative, and a soft score is a product of at most max_det - 1 = 4
    such weights: rtol 2e-5.  Counts, order and classes are exact."""
    assert len(mine) == len(ref)
    kept = 0
    for (c, b, s), (_, rc, rb, rs) in zip(mine, ref):
        assert np.array_equal(c, rc)
        np.testing.assert_allclose(b.reshape(-1, 4), rb.reshape(-1, 4), rtol=5e-6, atol=1e-5)
        np.testing.assert_allclose(s, rs, rtol=2e-5, atol=0)
        kept += len(c)
    return kept


def test_cfg_keys_reach_decode_and_deploy(pkg):
    from multitask_hydranet_amd import model as M
    from multitask_hydranet_amd.postprocess import NmsOptions
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    plain = pkg.HydraNet(cfgs)
    assert plain.det_nms is None and plain.detectheader.decode is M._det_decode
    for bad in ({"nms_type": "matrix"}, {"max_det": -1}, {"nms_sigma": 0.0}):
        c = load_cfg("hydranet_tiny.yml")
        c["detection"].update(bad)
        with pytest.raises(ValueError, match="detection\\."):
            pkg.HydraNet(c)
    cfgs["detection"].update({"nms_type": "soft_linear", "max_det": 5})
    net = pkg.HydraNet(cfgs)
    assert net.det_nms == NmsOptions("soft_linear", max_det=5)
    net.load_state_dict(tiny_state(z))
    net = net.cuda().eval()
    thr = float(z["deploy/pp_thresh"])
    net.deploy_postprocess = (thr, 0.3)
    x = torch.from_numpy(z["in/image"]).cuda()
    with torch.no_grad():
        dep = net(x, "deploy")
    hw = tuple(x.shape[2:])
    ref = R.nms_batch(dep[1][0].cpu().numpy(), dep[2].cpu().numpy(), dep[3].cpu().numpy(), hw, thr, 0.3, kind="soft_linear", max_det=5)
    hard = R.nms_batch(dep[1][0].cpu().numpy(), dep[2].cpu().numpy(), dep[3].cpu().numpy(), hw, thr, 0.3)
    assert any(len(r[0]) == 5 for r in ref) and any(len(h[0]) > 5 for h in hard)          # max_det is what ends the walk
    assert assert_rows_close(device_rows(dep[6]), ref) > 0
    out = net.detectheader.decode(x, dep[2], dep[3], dep[1], conf_thres=thr, iou_thres=0.3)
    rows = [(np.asarray(o["class_ids"], np.int64), np.asarray(o["rois"], np.float32).reshape(-1, 4), np.asarray(o["scores"], np.float32))
            for o in out]
    assert assert_rows_close(rows, ref) > 0


def test_demo_single_and_batch_agree(pkg):
    from multitask_hydranet_amd import jpeg
    from multitask_hydranet_amd.demo import Demo
    from tests import avi_ref
    nms = options("soft_linear", max_det=3)
    demos = []
    for rule in (nms, None):
        demo = Demo(load_cfg("hydranet_tiny.yml"), fold_batchnorm=False, det_nms=rule)
        demo.net.load_state_dict(tiny_state(load_npz("tiny_hydranet.npz")))
        demo.net.eval().prepare_inference()
        demo.lane_conf, demo.det_conf = 0.3, 0.3
        demos.append(demo)
    demo, plain = demos
    frames = list(avi_ref.clip()[1][:2])
    single = [demo.process_device(jpeg.imread_bgr_device(f, device=demo.device))["detections"][0] for f in frames]
    batch = demo.process_device_batch(jpeg.imread_bgr_device(frames, device=demo.device))["detections"]
    base = [plain.process_device(jpeg.imread_bgr_device(f, device=plain.device))["detections"][0] for f in frames]
    assert any(len(b["scores"]) > 3 for b in base)                    # the hard NMS draws more than max_det boxes ...
    assert any(len(s["scores"]) == 3 for s in single)                 # ... the option caps them
    for s, b in zip(single, batch):
        assert len(s["scores"]) <= 3
        for k in ("rois", "class_ids", "scores"):
            assert np.array_equal(np.asarray(s[k]), np.asarray(b[k])), k


def test_dispatcher_op_equals_postprocess_device(pkg, base):
    import multitask_hydranet_amd.torch_ops  # noqa: F401
    anchors, reg, cls = (torch.from_numpy(v).cuda() for v in base)
    got = torch.ops.hydranet_hip.det_postprocess_ex(anchors, reg, cls, 128, 128, THR, IOU, 4096, "soft_gaussian", SIGMA, THR, 7, True)
    want = run_device(base, (128, 128), options("soft_gaussian", max_det=7, class_agnostic=True))
    named = dict(zip(("rois", "class_ids", "scores", "kept", "total"), got), cap=want["cap"])
    assert assert_same_outputs(named, want) == 8
