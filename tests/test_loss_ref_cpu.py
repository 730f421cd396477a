"""tests/loss_ref.py, the float64 / integer reference of the loss kernel tests (tests/test_loss_exact_gpu.py), held to torch double
(F.cross_entropy, tests/torch_losses.py with autograd) and to np.sort, and the conditions its seeded inputs must meet so that an fp32
kernel and the float64 reference select the same elements:
  * seg CE: the chosen k leaves a relative gap >= 5e-4 between the k-th and (k+1)-th largest loss of every image (about 100 times the
    error of an fp32 loss), at every class count and shape of the GPU test and the seeds 0..2;
  * space-to-depth gradient: fp32 torch's own gradient, rounded to bf16, differs from the bf16 rounding of the float64 gradient on fewer
    than 1 % of the elements and never by more than one bf16 ulp;
  * detection: no anchor's best IoU within 1e-4 of 0.4 / 0.5, no second-best IoU within 1e-4 of the best.
It also prints what fp32 F.cross_entropy alone costs against float64 on these inputs (the GPU bounds 1e-5 / 1e-4 are not widened by it)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_ref as R
from tests import torch_losses as L

F64 = torch.float64
TOL = 1e-12

SEG_CS = (2, 3, 5, 16)
SEG_SHAPES = ((3, 50, 82), (2, 33, 61), (2, 8, 12), (3, 66, 64))
S2D_CASES = ((3, 3, 50, 82), (5, 3, 50, 82), (5, 2, 8, 12), (5, 3, 66, 64), (3, 2, 8, 12))
DET_NS, DET_AS, DET_KS = (1, 16, 17, 33), (1, 255, 257, 600), (1, 9)
GAP_MIN = 5e-4


def close(got, want, name, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    ref = max(float(np.abs(want).max()) if want.size else 0.0, 1e-30)
    assert err <= tol * ref, f"{name}: max err {err:.3e} (ref max {ref:.3e})"


# ------------------------------------------------------------------------------------------------------------------------------------
# selection
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hi", [(1, 5), (7, 3), (1000, 50), (4098, 1 << 32)])
def test_topk_select_is_the_sorted_rank(n, hi):
    g = np.random.default_rng(n)
    keys = g.integers(0, hi, n, dtype=np.uint64).astype(np.uint32)
    s = np.sort(keys)[::-1]
    for k in sorted({1, 2, n // 3 + 1, n // 2 + 1, n}):
        if k > n:
            continue
        thr, remaining, ties = R.topk_select(keys, k)
        assert thr == s[k - 1]
        assert ties == int((s == thr).sum()) and remaining == k - int((s > thr).sum()) and 1 <= remaining <= ties
        w = R.topk_weights(keys[None], k)[0]
        assert abs(w.sum() - k) < 1e-9 and set(np.unique(w)) <= {0.0, 1.0, remaining / ties}
        # the mean is the sort's mean
        assert abs((w * keys).sum() - s[:k].astype(np.float64).sum()) <= 1e-9 * s[:k].astype(np.float64).sum() + 1e-9


def test_injected_patterns_select_what_they_are_built_for():
    """the designed thresholds, remainders and tie counts of loss_ref.seg_pattern, from np.sort"""
    bits = lambda v: int(np.float32(v).view(np.uint32))
    for HW in (4098, 4100):
        b, _, ks = R.seg_pattern("low10", HW)
        assert [int(R.topk_select(R.f32_bits(b), k)[0]) - bits(32.0) for k in ks] == [0, 15, 16, 1023]
        b, _, ks = R.seg_pattern("mid11", HW)
        assert [(int(R.topk_select(R.f32_bits(b), k)[0]) - bits(32.0)) >> 10 for k in ks] == [0, 31, 32, 2016, 2047]
        assert all(int(R.topk_select(R.f32_bits(b), k)[0]) & 1023 == 0 for k in ks)
        b, _, ks = R.seg_pattern("ties", HW)
        T = HW // 4
        assert [R.topk_select(R.f32_bits(b), k)[1:] for k in ks] == [(1, T), (T // 2, T), (T, T)]
        per = (HW + 1) // 2                                                  # two blocks per image: the group lies in both
        assert 0 < int((b[:per] == 36.0).sum()) < T
        b, ign, ks = R.seg_pattern("sparse", HW)
        nnz = int((b > 0).sum())
        assert abs(ign.mean() - 0.6) < 0.01 and not (ign & (b > 0)).any()
        assert [R.topk_select(R.f32_bits(b), k) for k in ks] == [(0, k - nnz, HW - nnz) for k in ks]
    for HW in (200, 4098, 4100):
        b, _, ks = R.seg_pattern("top", HW)
        sel = {k: R.topk_select(R.f32_bits(b), k) for k in ks}
        bins = sorted({int(v) >> 21 for v in R.f32_bits(b[b > 0])})
        assert len(bins) == 64 and all(int(v) & ((1 << 21) - 1) == 0 for v in R.f32_bits(b))
        assert [int(sel[k][0]) >> 21 for k in (64 - 15, 64 - 16, 64 - 47, 64 - 48)] == [543, 544, 575, 576]      # level-0 chunks of 32 bins
        assert sel[HW] == (0, HW - 64, HW - 64) and int(sel[1][0]) == bits(1.75 * 2.0 ** 20)
    for HW in (1, 4, 200, 4098, 4100):
        b, ign, ks = R.seg_pattern("equal", HW)
        assert [R.topk_select(R.f32_bits(b), k)[1:] for k in ks] == [(k, HW) for k in ks] and 1 in ks and HW in ks
        assert R.seg_pattern("ignored", HW)[1].all()


# ------------------------------------------------------------------------------------------------------------------------------------
# seg CE
# ------------------------------------------------------------------------------------------------------------------------------------
def torch_ce(logits, target, cw, dtype):
    """F.cross_entropy per pixel and its gradient under a sum; ids outside [0, C) are mapped to ignore_index (torch raises on them)"""
    C = logits.shape[-1]
    t = torch.from_numpy(np.where(R.seg_valid(target, C), target, 255))
    x = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    loss = F.cross_entropy(x.permute(0, 2, 1), t, weight=torch.from_numpy(cw).to(dtype), ignore_index=255, reduction="none")
    loss.sum().backward()
    return loss.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("C", SEG_CS)
@pytest.mark.parametrize("n,h,w", SEG_SHAPES)
def test_seg_ce_matches_torch_and_keeps_its_margin(C, n, h, w):
    for seed in (0, 1, 2):
        logits, target, cw = R.seg_case(seed, C, n, h, w)
        assert (target == 255).any() and (target == C).any() and (target == -1).any() and (cw == 0).sum() == 1
        loss, dloss = R.seg_ce(logits, target, cw)
        want, dwant = torch_ce(logits, target, cw, F64)
        close(loss, want, "loss")
        close(dloss, dwant, "dloss")
        k, gap = R.choose_k(loss)
        assert 0.25 * h * w <= k <= 0.35 * h * w
        assert gap >= GAP_MIN, (C, (n, h, w), seed, k, gap)
        # the top-k mean and its gradient against the sort of tests/torch_losses.py (no tie at the threshold: the two contracts agree)
        valid_t = torch.from_numpy(np.where(R.seg_valid(target, C), target, 255)).reshape(n, h, w)
        x = torch.from_numpy(logits).to(F64).reshape(n, h, w, C).permute(0, 3, 1, 2).requires_grad_(True)
        for use_topk in (True, False):
            x.grad = None
            ref = L.seg_loss(x, valid_t, torch.from_numpy(cw).to(F64), use_topk, k / (h * w) + 1e-9, False)
            assert not use_topk or int((k / (h * w) + 1e-9) * h * w) == k
            ref.backward()
            val, grad = R.seg_ce_mean(logits, target, cw, use_topk, k)
            assert abs(val - float(ref.detach())) <= TOL * abs(float(ref.detach()))
            close(grad.reshape(n, h, w, C), x.grad.permute(0, 2, 3, 1).numpy(), "dlogits")
        if seed == 0:
            l32, d32 = torch_ce(logits, target, cw, torch.float32)
            print(f"C={C} {(n, h, w)} k={k} gap={gap:.2e}  fp32 F.cross_entropy vs float64: mean rel {abs(l32.mean(dtype=np.float64) - loss.mean()) / loss.mean():.1e}"
                  f"  dlogits max err / max {np.abs(d32 - dloss).max() / np.abs(dloss).max():.1e}")


@pytest.mark.parametrize("C,n,h,w", S2D_CASES)
def test_fp32_gradient_stays_under_the_bf16_mismatch_cap(C, n, h, w):
    """what fp32 alone costs the space-to-depth bf16 operand: torch's fp32 gradient, rounded to bf16, against the bf16 rounding of the
    float64 gradient -- under the 1 % cap of the GPU test, and never more than one bf16 ulp apart"""
    logits, target, cw = R.seg_case(0, C, n, h, w)
    loss, _ = R.seg_ce(logits, target, cw)
    k, _ = R.choose_k(loss)
    for use_topk in (True, False):
        _, grad = R.seg_ce_mean(logits, target, cw, use_topk, k)
        grad = grad * 3.0
        w64 = R.topk_weights(loss, k) / (n * k) if use_topk else np.full_like(loss, 1.0 / loss.size)
        _, d32 = torch_ce(logits, target, cw, torch.float32)
        g32 = d32 * (np.float32(3.0) * w64.astype(np.float32))[..., None]
        a, b = R.bf16_line(g32), R.bf16_line(grad)
        frac = float((a != b).mean())
        print(f"C={C} {(n, h, w)} topk={use_topk}: {100 * frac:.3f} % of the bf16 elements differ")
        assert frac < 0.01 and int(np.abs(a - b).max()) <= 1
        z = R.s2d_channels(grad.reshape(-1, C), n, h, w, C, 4 * C + 4)
        assert (z[..., 4 * C:] == 0).all() and z[1, 2, 3, 3 * C + 1] == grad.reshape(n, h, w, C)[1, 5, 7, 1]


# ------------------------------------------------------------------------------------------------------------------------------------
# focal
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 5, 16])
@pytest.mark.parametrize("gamma,alpha", [(2.0, 1.0), (1.5, 0.25), (1.0, 0.25), (1.5, 1.0)])
def test_focal_matches_torch(C, gamma, alpha):
    """float64 torch gives NaN on a saturated pixel for a fractional gamma (negative base, see loss_ref.seg_focal): those are compared
    without saturated pixels, and with them only asked to be finite.  tests/torch_losses.py forms t = onehot + 1e-8 from an int64 one-hot,
    which torch promotes to fp32 whatever the logits' type: t is 1 there and 1 + 1e-8 here, hence 1e-7 and not 1e-12."""
    sat = gamma != 1.5
    logits, target, cw = R.focal_case(C, saturated=sat)
    x = torch.from_numpy(logits).to(F64).t().reshape(1, C, -1, 1).requires_grad_(True)
    ref = L.seg_loss(x, torch.from_numpy(target).reshape(1, -1, 1), torch.from_numpy(cw).to(F64), False, 0.3, True, gamma=gamma, alpha=alpha)
    ref.backward()
    val, grad = R.seg_focal(logits, target, cw, gamma, alpha)
    assert abs(val - float(ref.detach())) <= 1e-7 * abs(float(ref.detach()))
    close(grad, x.grad.reshape(C, -1).t().numpy(), "dlogits", 1e-7)
    val, grad = R.seg_focal(*R.focal_case(C, saturated=True), gamma, alpha)
    assert np.isfinite(val) and np.isfinite(grad).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# lane
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.LANE_PATTERNS)
@pytest.mark.parametrize("M", [384, 8193])
def test_lane_cls_matches_torch(M, name):
    for z, t, ratio, inj in R.lane_pattern(name, M):
        ref = R.lane_cls(z, t, ratio, 10.0, gpos=1.3, gneg=0.7)
        zz = torch.from_numpy(z).to(F64).requires_grad_(True)
        pos, neg, pm, pn = L.lane_cls_loss(torch.from_numpy(t).to(F64), zz, negative_ratio=ratio)
        (1.3 * pos + 0.7 * neg).backward()
        assert abs(ref["pos"] - float(pos)) <= TOL * max(abs(float(pos)), 1) and abs(ref["neg"] - float(neg)) <= TOL * max(abs(float(neg)), 1)
        assert (ref["pmask"] == pm.numpy()).all() and ref["posn"] == int(pn)
        close(ref["dlogits"], zz.grad.numpy(), "dlogits")
        # the injected rows: log p_bg = -b exactly (already in float64), and the integer select finds the float threshold
        lsm32 = ref["lsm"].astype(np.float32)
        assert (lsm32[inj, 0] == z[inj, 0]).all()
        thr = R.lane_select(lsm32[:, 0], ref["pmask"], ref["k"])
        if ref["nneg"]:
            assert thr == np.sort(lsm32[~ref["pmask"], 0])[ref["k"] - 1]
        else:
            assert np.isinf(thr) and ref["neg"] == 0.0
        if name in ("lowbyte", "topbyte", "ties", "no_positive"):
            assert inj[np.argmin(np.abs(ref["lsm"][:, 0] - ref["thr"]))]         # the threshold is an injected key
        if name == "every_negative":
            assert ref["k"] == ref["nneg"]


def test_lane_keys_are_order_preserving():
    v = np.array([-np.inf, -3e38, -40.0, -32.000004, -32.0, -1e-30, -0.0, 0.0, 1e-30, 2.5, np.inf], np.float32)
    k = R.f2ord(R.f32_bits(v))
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert all(R.ord2f(x).view(np.uint32) == y for x, y in zip(k, R.f32_bits(v)))


@pytest.mark.parametrize("L_", [3, 33, 42, 322])
def test_lane_loc_matches_torch(L_):
    for wcol in sorted({1, L_ - 2}):
        p, t, pmask, posn = R.lane_loc_case(L_, wcol=wcol)
        m3 = min(3, L_)
        assert pmask[0] and pmask[5] and (p[0, :m3].astype(np.float64) - t[0, :m3] == R.LOC_EDGES[:m3].astype(np.float64)).all()
        assert (t[5, :m3].astype(np.float64) - p[5, :m3] == R.LOC_EDGES[:m3].astype(np.float64)).all()
        assert list(R.LOC_EDGES.astype(np.float64)) == [1.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23]
        pp = torch.from_numpy(p).to(F64).requires_grad_(True)
        ref = L.lane_loc_loss(torch.from_numpy(pmask), posn, torch.from_numpy(t).to(F64), pp, points_per_line=wcol)
        (ref * 1.7).backward()
        val, grad, nrm = R.lane_loc(p, t, pmask, posn, wcol, gout=1.7)
        assert abs(val - float(ref)) <= TOL * abs(float(ref)) and float(ref) > 0
        close(grad, pp.grad.numpy(), "dpred")
        assert nrm[3] == 1.0 and (grad[3] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# detection
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", DET_KS)
@pytest.mark.parametrize("A", DET_AS)
@pytest.mark.parametrize("N", DET_NS)
def test_det_smooth_l1_matches_torch_and_keeps_its_margins(N, A, K):
    cls, reg, anc, ann = R.det_case(N, A, K)
    thr_m, gap_m = R.det_margins(anc, ann)
    assert thr_m > 1e-4 and gap_m > 1e-4, (thr_m, gap_m)
    assert (ann[:, :, 4] == -1).any() and (N == 1 or (ann[1, :, 4] == -1).all())
    ref = R.det_smooth_l1(cls, reg, anc, ann, gcls=1.0, greg=50.0)
    assert sum(ref["npos"]) > 0 and (N == 1 or ref["npos"][1] == 0)
    c, r = torch.from_numpy(cls).to(F64).requires_grad_(True), torch.from_numpy(reg).to(F64).requires_grad_(True)
    lc, lr = L.det_loss(c, r, torch.from_numpy(anc).to(F64)[None], torch.from_numpy(ann).to(F64))
    (lc.sum() + 50.0 * lr.sum()).backward()
    assert abs(ref["cls"] - float(lc)) <= TOL * abs(float(lc)) and abs(ref["reg"] - float(lr)) <= TOL * abs(float(lr))
    close(ref["dcls"], c.grad.numpy(), "dcls")
    close(ref["dreg"], r.grad.numpy(), "dreg")


# ------------------------------------------------------------------------------------------------------------------------------------
# weighted sum
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,groups", [(1, 1), (5, 1), (5, 2), (5, 3), (8, 1), (8, 2), (8, 3)])
def test_weighted_sum_is_sequential_fp32(n, groups):
    x, w, gw, grp = R.weighted_sum_case(n, groups)
    assert (np.diff(grp) >= 0).all() and len(set(grp)) == groups
    tot, grads = R.weighted_sum(x, w, gw, grp, gout=1.7)
    x64, w64, gw64 = (v.astype(np.float64) for v in (x, w, gw))
    exact = sum(gw64[g] * (x64 * w64)[grp == g].sum() for g in range(groups))
    assert abs(float(tot) - exact) <= 1e-6 * abs(exact)
    close(grads, 1.7 * gw64[grp] * w64, "grads", 1e-6)
    if n > 1:
        # another association order (right to left) and the correctly rounded exact total differ in the last bits: the order is observable
        rev, once = R.weighted_sum_other_orders(x, w, gw, grp)
        assert rev != tot and once != tot
