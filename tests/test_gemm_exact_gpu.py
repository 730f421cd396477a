"""The conv GEMM families of csrc/hn_gemm.hip held to EXACT integer references, plan by plan.

Operands are small integers (bf16 represents them exactly), so every product is exact in fp32 and so is every partial sum, in any order,
while its magnitude stays below 2^24: a weight / bias gradient or an fp32 GEMM output must equal the float64 reference bit for bit,
whatever the kernel's split count, MFMA K order or reduce tree; a bf16 output must equal the reference rounded to bf16 (the device
conversion is round-to-nearest-even, as torch's).  One dropped or doubled slab, one lost ragged tail, one mis-stored tile edge shows up
as a wrong integer.  Every case first asserts the plan branch it claims to land on (tests/gemm_plans.py, held to the library's own plan
queries by tests/test_gemm_plans_cpu.py), every output lives between sentinel guard bands, and a mismatch names the split it points at.
One random-operand companion per family bounds |err| <= 2e-5 * (|x|^T |dz|) elementwise."""
import ctypes
import zlib

import pytest
import torch

from tests import gemm_plans as P
from tests.guards import BAND, Guarded, dev

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EXACT_LIMIT = 1 << 24
RAND_TOL = 2e-5


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops
    return ops


def seed_of(name):
    return zlib.crc32(name.encode()) & 0xFFFF


def gen(seed):
    g = torch.Generator(device=dev())
    g.manual_seed(seed)
    return g


def ints(shape, lo, hi, g, density=1.0, width=None):
    """bf16 tensor of integers uniform in [lo, hi] (a fraction 1 - density zeroed); width > shape[-1]: a channel slice of a wider
    tensor (row stride width) whose extra columns hold other integers"""
    full = tuple(shape[:-1]) + ((width or shape[-1]),)
    v = torch.randint(lo, hi + 1, full, generator=g, device=dev()).float()
    if density < 1.0:
        v = v * (torch.rand(full, generator=g, device=dev()) < density).float()
    v = v.to(BF16)
    return v[..., :shape[-1]] if width else v


def randn(shape, g, width=None):
    full = tuple(shape[:-1]) + ((width or shape[-1]),)
    v = torch.randn(full, generator=g, device=dev()).to(BF16)
    return v[..., :shape[-1]] if width else v


# ---- exact comparison ----------------------------------------------------------------------------------------------------------------
def exact(got, want, name, why=None):
    """got (fp32 / bf16) == want (float64 integers, or bf16) bit for bit; why(first bad indices) -> text naming the plan branch / split"""
    g = got.double()
    w = want.double()
    assert g.shape == w.shape, (name, g.shape, w.shape)
    bad = ~(g == w)
    n = int(bad.sum())
    if n:
        idx = bad.nonzero()[:5]
        lines = [f"  at {tuple(int(v) for v in i)}: got {float(g[tuple(i)])!r} want {float(w[tuple(i)])!r}" for i in idx]
        extra = why([tuple(int(v) for v in i) for i in bad.nonzero()[:16]]) if why else ""
        pytest.fail(f"{name}: {n} of {g.numel()} elements differ\n" + "\n".join(lines) + (f"\n  {extra}" if extra else ""))


def budget(bound, name):
    assert bound < EXACT_LIMIT, f"{name}: partial sums may reach {bound} >= 2^24, the case would not be exact"


# ---- float64 reference: the gather modes of include/hydranet_hip.h ---------------------------------------------------------------------
def border(v, L, kind):
    """source index of padded position v: reflect (ReflectionPad2d(1)), clamp (replicate), zero (-1 = outside)"""
    if kind == "reflect":
        return torch.where(v < 0, -v, torch.where(v >= L, 2 * L - 2 - v, v))
    if kind == "clamp":
        return v.clamp(0, L - 1)
    return torch.where((v < 0) | (v >= L), torch.full_like(v, -1), v)


def taps_of(mode, x0, x1, grid, up=0):
    """-> list of [M, C] float64 operands X(pixel, tap) in tap order ky * 3 + kx, pixel rows of the OUTPUT grid (n, H, W)"""
    n, h, w = grid
    if mode == 0:
        return [x0.double().reshape(-1, x0.shape[-1])]
    if mode == 1:
        return [x0[:, ::2, ::2].double().reshape(-1, x0.shape[-1])]
    if mode == 3:                                       # full correlation of the zero-extended x0 [n, H-2, W-2, C]
        src, kind, hs, ws = x0.double(), "zero", h - 2, w - 2
        off = lambda o, k: o - k
    else:
        s0 = x0.double()
        if up:
            s0 = s0.repeat_interleave(2, 1).repeat_interleave(2, 2)
        src = torch.cat([s0, x1.double()], -1) if x1 is not None else s0
        kind = {2: "reflect", 4: "clamp", 5: "zero"}[mode]
        hs, ws = h, w
        off = lambda o, k: o + k - 1
    out = []
    ar_h = torch.arange(h, device=dev())
    ar_w = torch.arange(w, device=dev())
    for ky in range(3):
        iy = border(off(ar_h, ky), hs, kind)
        for kx in range(3):
            ix = border(off(ar_w, kx), ws, kind)
            t = src[:, iy.clamp(min=0)][:, :, ix.clamp(min=0)]
            t = t * ((iy >= 0)[None, :, None, None] & (ix >= 0)[None, None, :, None])
            out.append(t.reshape(-1, src.shape[-1]))
    return out


def wgrad_ref(xs, dz, nout, absval=False):
    """dw [nout][C][taps] = sum_pixel dz[pixel][o] * X(pixel, tap)[c] in float64"""
    d = dz.double().reshape(-1, dz.shape[-1])[:, :nout]
    if absval:
        d = d.abs()
    return torch.stack([d.t() @ (x.abs() if absval else x) for x in xs], -1)


def diag_blocks(full):
    """[C][C][taps] -> the grouped (width 8) weight gradient [C][8][taps]"""
    c = full.shape[0]
    f = full.view(c // 8, 8, c // 8, 8, -1)
    return torch.stack([f[g, :, g] for g in range(c // 8)]).reshape(c, 8, -1)


def split_blame(q, xs, dz, idxs, got, want, grid=None, grouped=False):
    """name the plan split whose contribution the first bad dw elements [o][c][tap] are all off by (dropped: -contribution; doubled: +)"""
    rows = torch.arange(xs[0].shape[0], device=dev())
    if q["patch"]:
        n, h, w = grid
        img, r = rows // (h * w), rows % (h * w)
        patch = (img * P.cdiv(h, 8) + (r // w) // 8) * P.cdiv(w, 16) + (r % w) // 16
        sid = patch // q["rows_per_split"]
        unit = "patch split (of %d patches each)" % q["rows_per_split"]
    else:
        sid = rows // q["rows_per_split"]
        unit = "pixel split (of %d rows each)" % q["rows_per_split"]
    ns = int(sid.max()) + 1
    cand = {-1.0: None, 1.0: None}
    for idx in idxs:
        o, c, t = idx[0], idx[1], idx[2] if len(idx) > 2 else 0
        if grouped:
            c = 8 * (o // 8) + c
        d = dz.double().reshape(-1, dz.shape[-1])[:, o]
        contrib = torch.zeros(ns, dtype=F64, device=dev()).index_add_(0, sid, d * xs[t][:, c])
        delta = float(got[idx]) - float(want[idx])
        for sign in cand:
            hit = set(int(v) for v in (contrib * sign == delta).nonzero()[:, 0]) if delta != 0 else set()
            cand[sign] = hit if cand[sign] is None else cand[sign] & hit
    plan = f"plan {q['kernel']} splits={q['splits']} rows_per_split={q['rows_per_split']} reduce={P.REDUCE_NAMES[q['reduce']]}"
    for sign, what in ((-1.0, "dropped"), (1.0, "counted twice")):
        if cand[sign]:
            s = sorted(cand[sign])
            where = "the last, ragged split" if s == [ns - 1] else ("an inner split" if len(s) == 1 else "ambiguous")
            return f"{plan}: the errors of {len(idxs)} elements equal {unit} {s[:4]} of {ns} {what} ({where})"
    return f"{plan}: the errors match no single split's contribution"


# ---- wgrad calls (the argument lists of ops.k_gemm_tn, with guard-banded outputs) ---------------------------------------------------
def tn_call(K, which, x0, x1, mode, grid, dz, nout, kp, taps, up=0, defer=None):
    n, h, w = grid
    m = n * h * w
    cin = x0.shape[3] + (x1.shape[3] if x1 is not None else 0)
    q = P.wgrad_plan(mode, n, h, w, m, nout, kp, taps)
    s, r, wsb = ctypes.c_int(), ctypes.c_long(), ctypes.c_long()
    K.lib().query("hn_wgrad_plan", mode, n, h, w, m, nout, kp, taps, ctypes.addressof(s), ctypes.addressof(r), ctypes.addressof(wsb))
    assert (s.value, r.value, wsb.value) == (q["splits"], q["rows_per_split"], q["ws_bytes"]), "plan restatement out of date"
    ws = torch.empty((wsb.value // 4,), device=dev(), dtype=F32)
    cw = 8 if mode == 5 else cin
    dw = Guarded(nout, cw * taps)
    db = Guarded(1, nout) if which == "bias" else None
    c0, c1 = x0.shape[3], (x1.shape[3] if x1 is not None else 0)
    ldz = dz.stride(2) if dz.dim() == 4 else dz.stride(0)
    args = (K.ptr(x0), K.ptr(x1), mode, n, h, w, c0, c1, K.ld(x0), K.ld(x1) if x1 is not None else 0, up, m, K.ptr(dz), ldz, nout, kp, taps,
            K.ptr(ws), dw.ptr())
    if which == "deferred":
        K.lib().call("hn_conv_gemm_tn_deferred", *args, defer.slot(ws))
        job = defer.jobs[8 * (defer.n - 1):8 * defer.n]
        assert job[2] == q["splits"] and job[7] == q["reduce"], f"deferred job {list(job)} vs plan {q}"
    elif which == "bias":
        K.lib().call("hn_conv_gemm_tn_bias", *args, db.ptr())
    else:
        K.lib().call("hn_conv_gemm_tn", *args)
    return q, dw, db, ws


def check_wgrad(q, dw, db, xs, dz, nout, name, grid=None, grouped=False):
    torch.cuda.synchronize()
    want = wgrad_ref(xs, dz, nout) if not grouped else None
    if grouped:
        want = diag_blocks(wgrad_ref(xs, dz, nout))
    got = dw.view.reshape(want.shape)
    exact(got, want, f"{name} dW", lambda ii: split_blame(q, xs, dz, ii, got, want, grid, grouped))
    dw.check(f"{name} dW")
    if db is not None:
        wb = dz.double().reshape(-1, dz.shape[-1])[:, :nout].sum(0)
        exact(db.view[0], wb, f"{name} db")
        db.check(f"{name} db")


def wgrad_budget(xs, dz, nout, name):
    b = float(wgrad_ref(xs, dz, nout, absval=True).max())
    budget(b, name)


# ---- 2. weight-gradient matrix ----------------------------------------------------------------------------------------------------------
# (name, mode, grid, C0, C1, up, Nout, expected kernel, expected splits (None: any), expected reduce kind, ldz / ld0 widths)
TN_ROW_CASES = [
    # all 11 TN_CASE tiles (mode 0 / 1, Nout and cin across the thresholds, not multiples of the tile)
    ("tn128x128", 0, (2, 16, 24), 232, 0, 152, "tn<128,128>", None),
    ("tn128x64_s2", 1, (2, 9, 13), 40, 0, 152, "tn<128,64>", None),
    ("tn128x32", 0, (1, 24, 40), 24, 0, 232, "tn<128,32>", None),
    ("tn64x128", 0, (2, 12, 20), 152, 0, 40, "tn<64,128>", None),
    ("tn64x64", 0, (2, 12, 20), 40, 0, 56, "tn<64,64>", None),
    ("tn64x32_s2", 1, (1, 17, 23), 24, 0, 40, "tn<64,32>", None),
    ("tn32x128", 0, (1, 20, 30), 232, 0, 24, "tn<32,128>", None),
    ("tn32x64", 0, (1, 20, 30), 40, 0, 24, "tn<32,64>", None),
    ("tn32x32", 0, (1, 20, 30), 24, 0, 32, "tn<32,32>", None),
    ("tn16x128", 0, (1, 20, 30), 152, 0, 8, "tn<16,128>", None),
    ("tn16x64", 0, (1, 20, 30), 24, 0, 16, "tn<16,64>", None),
    # split regimes
    ("one_split", 0, (1, 8, 24), 40, 0, 56, "tn<64,64>", 1),
    ("ragged_splits", 0, (3, 17, 23), 64, 0, 56, "tn<64,64>", 5),
    ("splits512_112", 0, (16, 64, 128), 112, 0, 112, "tn<128,128>", 512),
    ("splits512_64", 0, (16, 64, 128), 64, 0, 64, "tn<64,64>", 512),
    ("splits411_ragged", 0, (1, 1, 131072 + 64 * 3 + 17), 112, 0, 112, "tn<128,128>", 411),
    # reduce kind 0 (splits <= 128, Nout * taps * KP >= 65 536)
    ("reduce4_936", 0, (2, 32, 32), 936, 0, 936, "tn<128,128>", 8),
]


def _tn_inputs(mode, grid, c0, nout, g, dens=1.0, lo=-3, hi=3, rand=False):
    n, h, w = grid
    hi_, wi_ = (2 * h, 2 * w) if mode == 1 else (h, w)
    mk = (lambda s, width=None: randn(s, g, width)) if rand else (lambda s, width=None: ints(s, lo, hi, g, dens, width))
    x = mk((n, hi_, wi_, c0), width=c0 + 8)             # ld0 > C0
    dz = mk((n, h, w, nout), width=nout + 16)           # ldz > Nout
    return x, dz


@pytest.mark.parametrize("case", TN_ROW_CASES, ids=[c[0] for c in TN_ROW_CASES])
def test_wgrad_row_gather_exact(K, case):
    name, mode, grid, c0, c1, nout, kern, splits = case
    n, h, w = grid
    q = P.wgrad_plan(mode, n, h, w, n * h * w, nout, P.kp32(c0), 1)
    assert q["kernel"] == kern and (splits is None or q["splits"] == splits), f"{name} no longer lands on {kern}/{splits}: {q}"
    g = gen(seed_of(name))
    x, dz = _tn_inputs(mode, grid, c0, nout, g)
    xs = taps_of(mode, x, None, grid)
    wgrad_budget(xs, dz, nout, name)
    for which in ("plain", "bias"):
        q2, dw, db, _ = tn_call(K, which, x, None, mode, grid, dz, nout, P.kp32(c0), 1)
        check_wgrad(q2, dw, db, xs, dz, nout, f"{name} [{which}] {kern} reduce={P.REDUCE_NAMES[q['reduce']]}")


# 3x3 patch kernel (mode 2 reflect with / without up + C1, mode 4 replicate, mode 5 grouped) and the big-slab plans
PATCH_CASES = [
    # name, mode, grid (output), C0, C1, up, Nout, kernel, splits (None: any), reduce
    ("p16x64_reflect", 2, (1, 13, 21), 64, 0, 0, 16, "patch<16,64>", None, -1),
    ("p32x64_up_c1", 2, (2, 14, 22), 24, 16, 1, 24, "patch<32,64>", None, -1),
    ("p64x64_clamp", 4, (2, 13, 35), 64, 0, 0, 64, "patch<64,64>", None, -1),
    ("p128x64", 2, (1, 21, 19), 128, 0, 0, 128, "patch<128,64>", None, -1),
    ("p128x32", 2, (2, 11, 37), 24, 0, 0, 128, "patch<128,32>", None, -1),
    ("p128x64_reduce4", 2, (4, 64, 128), 128, 0, 0, 128, "patch<128,64>", 128, 0),
    ("p32x64_1024slabs", 2, (16, 128, 256), 64, 0, 0, 24, "patch<32,64>", 1024, 1),
    ("p128x32_512slabs_up", 2, (4, 128, 256), 16, 8, 1, 128, "patch<128,32>", None, 1),
]


@pytest.mark.parametrize("case", PATCH_CASES, ids=[c[0] for c in PATCH_CASES])
def test_wgrad_patch_exact(K, case):
    name, mode, grid, c0, c1, up, nout, kern, splits, red = case
    n, h, w = grid
    kp = P.kp32(c0 + c1)
    q = P.wgrad_plan(mode, n, h, w, n * h * w, nout, kp, 9)
    assert q["kernel"] == kern and q["reduce"] == red and (splits is None or q["splits"] == splits), f"{name} moved: {q}"
    g = gen(seed_of(name))
    big = n * h * w > 200000
    dens = 0.5 if big else 1.0
    s0 = (n, h // 2, w // 2, c0) if up else (n, h, w, c0)
    x0 = ints(s0, -3, 3, g, dens, width=c0 + 8)
    x1 = ints((n, h, w, c1), -3, 3, g, dens) if c1 else None
    dz = ints((n, h, w, nout), -3, 3, g, dens, width=P.cdiv(nout, 8) * 8 + 8)
    xs = taps_of(mode, x0, x1, grid, up)
    wgrad_budget(xs, dz, nout, name)
    for which in (("plain", "bias") if not big else ("bias",)):
        q2, dw, db, _ = tn_call(K, which, x0, x1, mode, grid, dz, nout, kp, 9, up=up)
        check_wgrad(q2, dw, db, xs, dz, nout, f"{name} [{which}] {kern} reduce={P.REDUCE_NAMES[red]}", grid=grid)


GCONV_CASES = [("g64", (2, 13, 21), 64), ("g152_ragged_tile", (1, 16, 40), 152), ("g376", (2, 8, 16), 376)]


@pytest.mark.parametrize("case", GCONV_CASES, ids=[c[0] for c in GCONV_CASES])
def test_wgrad_grouped_exact(K, case):
    """mode 5 (grouped 3x3, group width 8): the block-diagonal patch kernel + gconv_diag_extract_kernel (reduce kind 2)"""
    name, grid, c = case
    n, h, w = grid
    q = P.wgrad_plan(5, n, h, w, n * h * w, c, 64, 9)
    assert q["kernel"] == "patch<64,64>" and q["reduce"] == 2, q
    g = gen(seed_of(name))
    x = ints((n, h, w, c), -3, 3, g, width=c + 8)
    dz = ints((n, h, w, c), -3, 3, g, width=c + 8)
    xs = taps_of(5, x, None, grid)
    budget(9 * n * h * w, name)
    q2, dw, _, _ = tn_call(K, "plain", x, None, 5, grid, dz, c, 64, 9)
    check_wgrad(q2, dw, None, xs, dz, c, f"{name} grouped", grid=grid, grouped=True)


def test_wgrad_gconv_group_exact(K):
    """hn_gconv_wgrad_group (GradQueue.add_gconv): several grouped jobs of different C / H / W in one launch, each exact"""
    jobs = [(2, 13, 21, 64), (1, 16, 40, 152), (2, 8, 16, 376), (1, 9, 17, 40)]
    gp = P.gconv_group_plan(jobs)
    q = K.GradQueue()
    g = gen(77)
    wts, refs, slots = [], [], []
    for (n, h, w, c) in jobs:
        x = ints((n, h, w, c), -3, 3, g, width=c + 8)
        dz = ints((n, h, w, c), -3, 3, g)
        wgt = torch.empty(c, 8, 3, 3, device=dev())
        gd = Guarded(1, c * 72)
        wgt._hn_grad_slot = (gd.buf, BAND)                # ops.grad_out hands this slot out as the gradient tensor
        slots.append(gd)
        q.add_gconv(wgt, x, dz, (n, h, w), c)
        wts.append(wgt)
        refs.append(diag_blocks(wgrad_ref(taps_of(5, x, None, (n, h, w)), dz, c)))
    tab = (ctypes.c_long * (9 * len(jobs)))()
    for i, ((n, h, w, c), (_, x, dz, _, _)) in enumerate(zip(jobs, q.gconv)):
        tab[9 * i:9 * i + 9] = [x.data_ptr(), dz.data_ptr(), 1, n, h, w, c, K.ld(x), K.ld(dz)]
    assert K.lib().query("hn_gconv_wgrad_group_ws_bytes", ctypes.addressof(tab), len(jobs)) == gp["ws_bytes"]
    q.weights = tuple(wts)
    got = q.flush()
    torch.cuda.synchronize()
    for i, (gt, r, gd) in enumerate(zip(got, refs, slots)):
        assert gt.data_ptr() == gd.view.data_ptr()
        exact(gt.reshape(r.shape), r, f"gconv group job {i} {jobs[i]} (patch splits {gp['splits'][i]})")
        gd.check(f"gconv group job {i}")


PHASE_CASES = [
    # name, grid (low-res), C0, C1, k (couts per phase), kernel
    ("ph64x64_span64", (2, 9, 13), 64, 0, 64, "patch<64,64,1>"),
    ("ph64x64_span64_skip", (1, 10, 12), 40, 24, 64, "patch<64,64,1>"),
    ("ph128x64_span128", (1, 9, 11), 128, 0, 128, "patch<128,64,1>"),
    ("ph128x64_span128_kp64", (2, 7, 17), 48, 16, 128, "patch<128,64,1>"),
]


def phase_mask(k):
    """[4k][9]: effective tap (dy, dx) is used by phase (py, px) iff dy in {py, py+1} and dx in {px, px+1}"""
    m = torch.zeros(4 * k, 9, dtype=F64, device=dev())
    for py in range(2):
        for px in range(2):
            for dy in (py, py + 1):
                for dx in (px, px + 1):
                    m[(2 * py + px) * k:(2 * py + px + 1) * k, dy * 3 + dx] = 1
    return m


@pytest.mark.parametrize("case", PHASE_CASES, ids=[c[0] for c in PHASE_CASES])
def test_wgrad_phase_exact(K, case):
    """hn_conv_gemm_tn_phase (effective weights [4k][C0][3][3], replicate-padded low-resolution gather, bias per phase) + hn_phase_fold
    (with the skip operand's dw1 of a full-resolution reflect-pad conv) == the weight / bias gradient of the 3x3 reflect-pad conv over
    cat[nearest_up2(x0), x1] (the SegConvUp backward, ops/seg.py)"""
    name, (n, h, w), c0, c1, k, kern = case
    kp = P.kp32(c0)
    q = P.wgrad_plan(4, n, h, w, n * h * w, 4 * k, kp, 9, phase_span=k)
    assert q["kernel"] == kern, q
    s, r, wsb = ctypes.c_int(), ctypes.c_long(), ctypes.c_long()
    K.lib().query("hn_wgrad_plan_phase", n, h, w, 4 * k, kp, k, ctypes.addressof(s), ctypes.addressof(r), ctypes.addressof(wsb))
    assert (s.value, r.value, wsb.value) == (q["splits"], q["rows_per_split"], q["ws_bytes"])
    g = gen(seed_of(name))
    x0 = ints((n, h, w, c0), -3, 3, g, width=c0 + 8)
    x1 = ints((n, 2 * h, 2 * w, c1), -3, 3, g) if c1 else None
    dz = ints((n, 2 * h, 2 * w, k), -3, 3, g)                             # full-resolution output gradient
    dzs = dz.view(n, h, 2, w, 2, k).permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, 4 * k).contiguous()   # space-to-depth, phase-major
    budget(9 * 4 * n * h * w * 4, name)
    ws = torch.empty((wsb.value // 4,), device=dev(), dtype=F32)
    dwe = Guarded(4 * k, c0 * 9)
    dbe = Guarded(1, 4 * k)
    K.lib().call("hn_conv_gemm_tn_phase", K.ptr(x0), n, h, w, c0, K.ld(x0), K.ptr(dzs), K.ld(dzs), 4 * k, kp, k, K.ptr(ws), dwe.ptr(), dbe.ptr())
    torch.cuda.synchronize()
    xs = taps_of(4, x0, None, (n, h, w))
    want_e = wgrad_ref(xs, dzs, 4 * k) * phase_mask(k)[:, None, :]
    got_e = dwe.view.reshape(want_e.shape)
    exact(got_e, want_e, f"{name} effective dW ({kern})", lambda ii: split_blame(q, xs, dzs, ii, got_e, want_e, (n, h, w)))
    exact(dbe.view[0], dzs.double().reshape(-1, 4 * k).sum(0), f"{name} effective db")
    dwe.check(f"{name} dW_eff")
    dbe.check(f"{name} db_eff")
    dw1 = None
    if c1:
        dw1 = K.k_gemm_tn(x1, None, 2, (n, 2 * h, 2 * w), dz, k, P.kp32(c1), 9, c1, kh=3)
    dw = Guarded(k, (c0 + c1) * 9)
    db = Guarded(1, k)
    K.lib().call("hn_phase_fold", dwe.ptr(), K.ptr(dw1), dbe.ptr(), dw.ptr(), db.ptr(), k, c0, c1)
    torch.cuda.synchronize()
    full = taps_of(2, x0, x1, (n, 2 * h, 2 * w), up=1)
    want = wgrad_ref(full, dz, k)
    exact(dw.view.reshape(want.shape), want, f"{name} folded dW")
    exact(db.view[0], dz.double().reshape(-1, k).sum(0), f"{name} folded db")
    dw.check(f"{name} dW")
    db.check(f"{name} db")


def test_wgrad_deferred_exact(K):
    """k_gemm_tn(defer=WgradBatch) + flush(): one to four jobs of mixed reduce kinds (0, 1, 2 and the -1 form launched immediately), each
    exact against float64"""
    specs = [  # mode, grid, C0, Nout, taps, kp, expected kind
        (0, (2, 32, 32), 936, 936, 1, 960, 0),
        (0, (4, 64, 128), 112, 112, 1, 128, 1),
        (5, (2, 13, 21), 152, 152, 9, 64, 2),
        (2, (1, 13, 21), 64, 16, 9, 64, -1),
    ]
    g = gen(91)
    for njobs in (1, 4):
        batch = K.WgradBatch()
        pend = []
        for mode, grid, c0, nout, taps, kp, kind in specs[:njobs] if njobs == 1 else specs:
            n, h, w = grid
            assert P.wgrad_plan(mode, n, h, w, n * h * w, nout, kp, taps)["reduce"] == kind
            x = ints((n, h, w, c0), -3, 3, g, width=c0 + 8)
            dz = ints((n, h, w, nout), -3, 3, g, width=nout + 8)
            q, dw, _, _ = tn_call(K, "deferred", x, None, mode, grid, dz, nout, kp, taps, defer=batch)
            pend.append((q, dw, taps_of(mode, x, None, grid), dz, nout, mode, grid, kind))
        batch.flush()
        for q, dw, xs, dz, nout, mode, grid, kind in pend:
            check_wgrad(q, dw, None, xs, dz, nout, f"deferred x{njobs} kind {kind}", grid=grid, grouped=mode == 5)


# hn_wgrad_group: one launch per tile of the grouped kernel; every launch mixes a split job, an unsplit job (stores straight into dw
# with out_ld = cin), a job narrower than the tile and a stride-2 (mode 1) job
GROUP_TILES = {  # tile -> (max nout, max cin) of the launch
    "tng_regs<128,128>": (376, 232), "tng<128,64>": (152, 40), "tng<128,32>": (232, 24),
    "tng<64,128>": (56, 152), "tng<64,64>": (56, 40), "tng<64,32>": (40, 24),
    "tng<32,128>": (24, 232), "tng<32,64>": (24, 40), "tng<32,32>": (32, 24),
    "tng<16,128>": (16, 152), "tng<16,64>": (16, 24),
}


def _group_jobs(nmax, cmax):
    small_n = max(8, nmax // 2 // 8 * 8)
    small_c = max(8, cmax // 2 // 8 * 8)
    return [  # (mode, n, h, w, cin, nout)
        (0, 4, 32, 40, cmax, nmax),              # split
        (0, 1, 8, 24, small_c, nmax),            # M = 192: unsplit, stores into dw directly
        (1, 2, 16, 20, cmax, small_n),           # stride 2, narrower than the tile
        (0, 1, 4, 20, cmax, small_n),            # unsplit, narrow
    ]


@pytest.mark.parametrize("tile", list(GROUP_TILES), ids=list(GROUP_TILES))
def test_wgrad_group_exact(K, tile):
    nmax, cmax = GROUP_TILES[tile]
    jobs = _group_jobs(nmax, cmax)
    pj = [(mode, n, h, w, cin, nout, n * h * w) for (mode, n, h, w, cin, nout) in jobs]
    gp = P.group_plan(pj)
    assert gp["kernel"] == tile, gp
    assert any(s > 1 for s in gp["splits"]) and any(s == 1 for s in gp["splits"]), f"{tile}: no split / unsplit mix: {gp}"
    q = K.GradQueue()
    g = gen(seed_of(tile))
    wts, refs, slots, tabrows = [], [], [], []
    for (mode, n, h, w, cin, nout) in jobs:
        hi, wi = (2 * h, 2 * w) if mode == 1 else (h, w)
        x = ints((n, hi, wi, cin), -3, 3, g, width=cin + 8)
        dz = ints((n, h, w, nout), -3, 3, g, width=nout + 8)
        wgt = torch.empty(nout, cin, 1, 1, device=dev())
        gd = Guarded(nout, cin)
        wgt._hn_grad_slot = (gd.buf, BAND)
        slots.append(gd)
        q.add(wgt, x, dz, mode, (n, h, w), cin, nout)
        wts.append(wgt)
        refs.append(wgrad_ref(taps_of(mode, x, None, (n, h, w)), dz, nout).reshape(nout, cin, 1, 1))
        tabrows.append([x.data_ptr(), dz.data_ptr(), 1, mode, n, h, w, cin, K.ld(x), dz.stride(2), nout, n * h * w])
    tab = (ctypes.c_long * (12 * len(jobs)))()
    for i, row in enumerate(tabrows):
        tab[12 * i:12 * i + 12] = row
    assert K.lib().query("hn_wgrad_group_ws_bytes", ctypes.addressof(tab), len(jobs)) == gp["ws_bytes"]
    budget(9 * max(j[-1] for j in pj), tile)
    q.weights = tuple(wts)
    got = q.flush()
    torch.cuda.synchronize()
    for i, (gt, r, gd) in enumerate(zip(got, refs, slots)):
        assert gt.data_ptr() == gd.view.data_ptr()
        red = gp["reduce"][i]
        exact(gt, r, f"{tile} job {i} {jobs[i]} splits={gp['splits'][i]} rps={gp['rps'][i]} "
                     f"{'unsplit (direct store, out_ld = cin)' if red is None else P.REDUCE_NAMES[red]}")
        gd.check(f"{tile} job {i}")


DW_CASES = [("dw112", (2, 13, 21), 112, None), ("dw64_levels", 2, 64, ([5, 9, 17], [5, 15, 33])), ("dw112_levels", 1, 112, ([9, 5], [15, 5]))]


@pytest.mark.parametrize("case", DW_CASES, ids=[c[0] for c in DW_CASES])
def test_dwconv_wgrad_exact(K, case):
    """depthwise 3x3 weight gradient: k_dwconv_wgrad (one map) and k_dwconv_wgrad_levels (level-packed det-tower rows, odd level sizes)"""
    name, grid, c, levels = case
    g = gen(seed_of(name))
    if levels is None:
        n, h, w = grid
        x = ints((n, h, w, c), -3, 3, g)
        dz = ints((n, h, w, c), -3, 3, g)
        got = K.k_dwconv_wgrad(x, dz)
        pairs = [(x, dz, (n, h, w))]
    else:
        n = grid
        hs, wsz = levels
        rows = [K.core._pad_rows(n * hh * ww) for hh, ww in zip(hs, wsz)]
        x = torch.zeros((1, 1, sum(rows), c), dtype=BF16, device=dev())
        dz = torch.zeros_like(x)
        pairs, off = [], 0
        for hh, ww, rr in zip(hs, wsz, rows):
            xl = ints((n, hh, ww, c), -3, 3, g)
            dl = ints((n, hh, ww, c), -3, 3, g)
            x[0, 0, off:off + n * hh * ww] = xl.reshape(-1, c)
            dz[0, 0, off:off + n * hh * ww] = dl.reshape(-1, c)
            pairs.append((xl, dl, (n, hh, ww)))
            off += rr
        got = K.k_dwconv_wgrad_levels(x, dz, (n, hs, wsz))
    torch.cuda.synchronize()
    want = torch.zeros(c, 9, dtype=F64, device=dev())
    for xl, dl, gr in pairs:
        xs = taps_of(5, xl, None, gr)                       # zero padding
        d = dl.double().reshape(-1, c)
        want += torch.stack([(d * t).sum(0) for t in xs], -1)
    budget(9 * sum(p[2][0] * p[2][1] * p[2][2] for p in pairs), name)
    exact(got.reshape(c, 9), want, f"{name} depthwise dW")


# ---- random-operand companions: one per family ---------------------------------------------------------------------------------------
def rand_bound(got, want, scale, name):
    r = float(((got.double() - want).abs() / scale.clamp(min=1e-30)).max())
    assert r <= RAND_TOL, f"{name}: max |err| / (|x|^T |dz|) = {r:.3e} > {RAND_TOL:.0e}"
    return r


RAND_CASES = [
    # family, mode, grid, C0, C1, up, Nout, taps
    ("row_gather_512splits", 0, (16, 64, 128), 112, 0, 0, 112, 1),
    ("row_gather_reduce4", 0, (2, 32, 32), 936, 0, 0, 936, 1),
    ("patch_1024slabs", 2, (16, 128, 256), 64, 0, 0, 24, 9),
    ("patch_up_c1", 2, (2, 64, 96), 24, 16, 1, 128, 9),
    ("grouped", 5, (2, 16, 24), 152, 0, 0, 152, 9),
]


@pytest.mark.parametrize("case", RAND_CASES, ids=[c[0] for c in RAND_CASES])
def test_wgrad_random_bound(K, case):
    name, mode, grid, c0, c1, up, nout, taps = case
    n, h, w = grid
    g = gen(seed_of(name))
    s0 = (n, h // 2, w // 2, c0) if up else (n, h, w, c0)
    x0 = randn(s0, g, width=c0 + 8)
    x1 = randn((n, h, w, c1), g) if c1 else None
    dz = randn((n, h, w, nout), g, width=P.cdiv(nout, 8) * 8 + 8)
    kp = 64 if mode == 5 else P.kp32(c0 + c1)
    q, dw, _, _ = tn_call(K, "plain", x0, x1, mode, grid, dz, nout, kp, taps, up=up)
    torch.cuda.synchronize()
    xs = taps_of(mode, x0, x1, grid, up)
    want, scale = wgrad_ref(xs, dz, nout), wgrad_ref(xs, dz, nout, absval=True)
    if mode == 5:
        want, scale = diag_blocks(want), diag_blocks(scale)
    r = rand_bound(dw.view.reshape(want.shape), want, scale, f"{name} ({q['kernel']}, {q['splits']} splits)")
    dw.check(name)
    print(f"{name}: max ratio {r:.3e}")


def test_wgrad_random_bound_group_phase_dw(K):
    """random companions of the grouped 1x1 launch, the phase form and the depthwise gradient"""
    g = gen(4242)
    # grouped 1x1
    jobs = _group_jobs(152, 232)
    q = K.GradQueue()
    wts, refs = [], []
    for (mode, n, h, w, cin, nout) in jobs:
        hi, wi = (2 * h, 2 * w) if mode == 1 else (h, w)
        x = randn((n, hi, wi, cin), g)
        dz = randn((n, h, w, nout), g)
        wgt = torch.empty(nout, cin, 1, 1, device=dev())
        q.add(wgt, x, dz, mode, (n, h, w), cin, nout)
        wts.append(wgt)
        xs = taps_of(mode, x, None, (n, h, w))
        refs.append((wgrad_ref(xs, dz, nout), wgrad_ref(xs, dz, nout, absval=True)))
    q.weights = tuple(wts)
    ratios = []
    for gt, (r, s) in zip(q.flush(), refs):
        ratios.append(rand_bound(gt.reshape(r.shape), r, s, "grouped 1x1"))
    # phase form
    n, h, w, c0, k = 2, 9, 13, 64, 64
    x0 = randn((n, h, w, c0), g)
    dzs = randn((n, h, w, 4 * k), g)
    s, rr, wsb = ctypes.c_int(), ctypes.c_long(), ctypes.c_long()
    K.lib().query("hn_wgrad_plan_phase", n, h, w, 4 * k, 64, k, ctypes.addressof(s), ctypes.addressof(rr), ctypes.addressof(wsb))
    ws = torch.empty((wsb.value // 4,), device=dev(), dtype=F32)
    dwe = torch.empty((4 * k, c0, 3, 3), device=dev(), dtype=F32)
    dbe = torch.empty((4 * k,), device=dev(), dtype=F32)
    K.lib().call("hn_conv_gemm_tn_phase", K.ptr(x0), n, h, w, c0, K.ld(x0), K.ptr(dzs), K.ld(dzs), 4 * k, 64, k, K.ptr(ws), K.ptr(dwe), K.ptr(dbe))
    xs = taps_of(4, x0, None, (n, h, w))
    m = phase_mask(k)[:, None, :]
    ratios.append(rand_bound(dwe.reshape(4 * k, c0, 9), wgrad_ref(xs, dzs, 4 * k) * m, wgrad_ref(xs, dzs, 4 * k, absval=True) * m + 1e-30,
                             "phase form"))
    # depthwise
    n, h, w, c = 2, 13, 21, 112
    x = randn((n, h, w, c), g)
    dz = randn((n, h, w, c), g)
    got = K.k_dwconv_wgrad(x, dz).reshape(c, 9)
    xs = taps_of(5, x, None, (n, h, w))
    d = dz.double().reshape(-1, c)
    want = torch.stack([(d * t).sum(0) for t in xs], -1)
    scale = torch.stack([(d.abs() * t.abs()).sum(0) for t in xs], -1)
    ratios.append(rand_bound(got, want, scale, "depthwise"))
    print("random ratios (group, phase, depthwise):", ["%.3e" % v for v in ratios])


# ---- 3. forward NT / direct 3x3 --------------------------------------------------------------------------------------------------------
def nt_ref(xs, wt, bias, act):
    """out [M][Nout] = act(bias + sum_t X_t @ W_t^T); wt float64 [Nout][C][taps]"""
    out = sum(x @ wt[:, :, t].t() for t, x in enumerate(xs))
    if bias is not None:
        out = out + bias.double()
    if act == 1:
        out = out.clamp(min=0)
    return out


NT_CASES = [
    # name, mode, grid, C0, C1, up, Nout, taps, out_f32, act, stats, expected kernel
    ("nt16_plain_f32", 0, (1, 50, 200), 40, 0, 0, 16, 1, True, 0, False, "nt<16,128>"),
    ("nt32_s2_bf16_relu", 1, (1, 50, 200), 40, 0, 0, 24, 1, False, 1, True, "nt<32,128>"),
    ("nt64_plain_bf16", 0, (1, 50, 200), 64, 0, 0, 56, 1, False, 0, True, "nt<64,128>"),
    ("nt64_least_pad_152", 0, (1, 90, 100), 40, 0, 0, 152, 1, True, 1, False, "nt<64,128>"),
    ("nt128_256", 0, (1, 90, 100), 40, 0, 0, 256, 1, False, 0, True, "nt<128,128>"),
    ("nt_small_M", 1, (1, 40, 100), 40, 0, 0, 96, 1, False, 1, True, "nt<64,64>"),
    ("nt_small_112_131k", 0, (16, 64, 128), 112, 0, 0, 112, 1, False, 0, True, "nt<64,64>"),
    ("nt_small_kg2", 0, (2, 32, 32), 936, 0, 0, 936, 1, True, 0, False, "nt<64,64,kg2>"),
    ("nt_gather_up_c1_stats", 2, (2, 30, 40), 24, 16, 1, 40, 9, False, 1, True, "nt<64,128>"),
    ("nt_gather_clamp_stats", 4, (2, 17, 23), 24, 0, 0, 24, 9, False, 0, True, "nt<32,128>"),
]


def _w_int(nout, cin, taps, g, lo=-2, hi=2, density=1.0):
    v = torch.randint(lo, hi + 1, (nout, cin, taps), generator=g, device=dev()).float()
    if density < 1.0:
        v = v * (torch.rand(v.shape, generator=g, device=dev()) < density).float()
    return v


def _stats_check(out_bf, psum, psq, tile, nout, name):
    o = out_bf.double().reshape(-1, nout)
    m = o.shape[0]
    nt = P.cdiv(m, tile)
    pad = torch.zeros(nt * tile - m, nout, dtype=F64, device=dev())
    op = torch.cat([o, pad]).view(nt, tile, nout)
    budget(float((op * op).sum(1).max()), name + " psq")
    exact(psum, op.sum(1), name + " psum", lambda ii: f"statistics tile {ii[0][0]} of {tile} rows")
    exact(psq, (op * op).sum(1), name + " psq", lambda ii: f"statistics tile {ii[0][0]} of {tile} rows")


@pytest.mark.parametrize("case", NT_CASES, ids=[c[0] for c in NT_CASES])
def test_nt_exact(K, case):
    name, mode, grid, c0, c1, up, nout, taps, out_f32, act, stats, kern = case
    n, h, w = grid
    m = n * h * w
    kp = P.kp32(c0 + c1)
    assert P.nt_kernel(mode, m, nout, kp, taps) == kern, P.nt_kernel(mode, m, nout, kp, taps)
    if stats:
        assert K.lib().query("hn_nt_stat_tile", m, nout) == P.stat_tile(m, nout)
    g = gen(seed_of(name))
    dens = 0.3 if stats else 1.0
    hi_, wi_ = (2 * h, 2 * w) if mode == 1 else ((h // 2, w // 2) if up else (h, w))
    x0 = ints((n, hi_, wi_, c0), -2, 2, g, dens, width=c0 + 8)
    x1 = ints((n, h, w, c1), -2, 2, g, dens) if c1 else None
    w3 = _w_int(nout, c0 + c1, taps, g, density=dens)
    wp = K.pack_conv_weight(w3.view(nout, c0 + c1, *((3, 3) if taps == 9 else (1, 1))).contiguous())[0]
    bias = torch.randint(-4, 5, (nout,), generator=g, device=dev()).float()
    xs = taps_of(mode, x0, x1, grid, up)
    budget(float(sum(x.abs() @ w3[:, :, t].abs().t().double() for t, x in enumerate(xs)).max()) + 4, name)
    want = nt_ref(xs, w3.double(), bias, act)
    ldc = nout + 24
    out = Guarded(m, nout, ldc, F32 if out_f32 else BF16)
    outv = out.view
    pr = K.lib().query("hn_nt_stat_rows", m, nout)
    psum = Guarded(pr, nout) if stats else None
    psq = Guarded(pr, nout) if stats else None
    fn = "hn_conv_gemm_nt"
    K.lib().call(fn, K.ptr(x0), K.ptr(x1), mode, n, h, w, c0, c1, K.ld(x0), K.ld(x1) if x1 is not None else 0, up, m, K.ptr(wp), nout, kp,
                 taps, K.ptr(bias), act, out.ptr(), 1 if out_f32 else 0, ldc, 0, 0, psum.ptr() if stats else None, psq.ptr() if stats else None)
    torch.cuda.synchronize()
    exact(outv, want if out_f32 else want.to(BF16), f"{name} ({kern}) out",
          lambda ii: f"pixel tile {ii[0][0] // P.stat_tile(m, nout) if 'nt<64,64' in kern else ii[0][0] // 128}")
    out.check(f"{name} out")
    if stats:
        # the statistics are those of bf16(conv + bias), taken BEFORE the activation (include/hydranet_hip.h)
        _stats_check(nt_ref(xs, w3.double(), bias, 0).to(BF16), psum.view, psq.view, P.stat_tile(m, nout), nout, name)
        psum.check(f"{name} psum")
        psq.check(f"{name} psq")


DIRECT_CASES = [
    # name, mode, grid (output), C0, C1, up, Nout, out_f32, act, ldc, expected
    ("d16_wpre_f32", 2, (1, 19, 37), 64, 0, 0, 16, True, 0, 16, "direct<16,f32,wpre>"),
    ("d16_wpre_bf16_up_c1", 2, (2, 18, 34), 24, 16, 1, 16, False, 1, 24, "direct<16,bf16,wpre>"),
    ("d32_f32_mode3", 3, (1, 21, 35), 40, 0, 0, 24, True, 0, 24, "direct<32,f32>"),
    ("d32_bf16_clamp", 4, (2, 17, 20), 64, 0, 0, 32, False, 1, 40, "direct<32,bf16>"),
    ("d64_f32", 2, (1, 20, 33), 128, 0, 0, 64, True, 0, 64, "direct<64,f32>"),
    ("d64_bf16_staged", 2, (2, 17, 19), 72, 0, 0, 56, False, 1, 64, "direct<64,bf16>"),
    ("d64_narrow", 2, (2, 23, 29), 24, 0, 0, 64, False, 0, 64, "direct_narrow<64>"),
    ("d128_f32_mode3", 3, (1, 18, 36), 64, 0, 0, 128, True, 1, 128, "direct<128,f32>"),
    ("d128_bf16", 4, (1, 20, 18), 40, 0, 0, 112, False, 0, 120, "direct<128,bf16>"),
    ("d128_fallback32_odd_ldc", 2, (1, 19, 21), 40, 0, 0, 96, False, 0, 100, "direct<32,bf16>"),
    ("d128_fallback32_odd_nout", 2, (1, 17, 23), 40, 0, 0, 66, False, 1, 66, "direct<32,bf16>"),
]


@pytest.mark.parametrize("case", DIRECT_CASES, ids=[c[0] for c in DIRECT_CASES])
def test_direct_exact(K, case):
    name, mode, grid, c0, c1, up, nout, out_f32, act, ldc, kern = case
    n, h, w = grid
    m = n * h * w
    kp = P.kp32(c0 + c1)
    assert P.direct_kernel(mode, nout, kp, out_f32, ldc)[0] == kern
    g = gen(seed_of(name))
    s0 = (n, h - 2, w - 2, c0) if mode == 3 else ((n, h // 2, w // 2, c0) if up else (n, h, w, c0))
    x0 = ints(s0, -2, 2, g, width=c0 + 8)
    x1 = ints((n, h, w, c1), -2, 2, g) if c1 else None
    w3 = _w_int(nout, c0 + c1, 9, g)
    wp = K.pack_conv_weight(w3.view(nout, c0 + c1, 3, 3).contiguous())[0]
    bias = torch.randint(-4, 5, (nout,), generator=g, device=dev()).float()
    xs = taps_of(mode, x0, x1, grid, up)
    want = nt_ref(xs, w3.double(), bias, act)
    out = Guarded(m, nout, ldc, F32 if out_f32 else BF16)
    K.lib().call("hn_conv_gemm_nt", K.ptr(x0), K.ptr(x1), mode, n, h, w, c0, c1, K.ld(x0), K.ld(x1) if x1 is not None else 0, up, m,
                 K.ptr(wp), nout, kp, 9, K.ptr(bias), act, out.ptr(), 1 if out_f32 else 0, ldc, 0, 0, None, None)
    torch.cuda.synchronize()
    exact(out.view, want if out_f32 else want.to(BF16), f"{name} ({kern}) out",
          lambda ii: "16x16 patch %d" % (((ii[0][0] // (h * w)) * P.cdiv(h, 16) + (ii[0][0] % (h * w)) // w // 16) * P.cdiv(w, 16)
                                          + (ii[0][0] % w) // 16))
    out.check(f"{name} out")


@pytest.mark.parametrize("grid,c", [((2, 19, 37), 64), ((1, 17, 33), 152)], ids=["g64", "g152"])
def test_direct_grouped_stats_exact(K, grid, c):
    """mode 5 on the direct kernel with its statistics rows (one per 16 x 16 output patch, hn_direct_stat_rows)"""
    n, h, w = grid
    m = n * h * w
    g = gen(c)
    x = ints((n, h, w, c), -1, 1, g, 0.5, width=c + 8)
    wg = _w_int(c, 8, 9, g, -1, 1)
    wk = K.pack_gconv_diag(wg.view(c, 8, 3, 3).contiguous())[0]
    xs = taps_of(5, x, None, grid)
    want = torch.stack([sum(xs[t][:, 8 * (o // 8):8 * (o // 8) + 8] @ wg[o, :, t].double() for t in range(9)) for o in range(c)], -1)
    out = Guarded(m, c, c + 8, BF16)
    pr = K.lib().query("hn_direct_stat_rows", n, h, w)
    psum, psq = Guarded(pr, c), Guarded(pr, c)
    K.lib().call("hn_conv_gemm_nt", K.ptr(x), None, 5, n, h, w, c, 0, K.ld(x), 0, 0, m, K.ptr(wk), c, 64, 9, None, 0, out.ptr(), 0, c + 8, 0, 0,
                 psum.ptr(), psq.ptr())
    torch.cuda.synchronize()
    exact(out.view, want.to(BF16), f"grouped direct C={c} out")
    out.check("grouped direct out")
    o = want.to(BF16).double().view(n, h, w, c)
    th, tw = P.cdiv(h, 16), P.cdiv(w, 16)
    op = torch.zeros(n, th * 16, tw * 16, c, dtype=F64, device=dev())
    op[:, :h, :w] = o
    op = op.view(n, th, 16, tw, 16, c).permute(0, 1, 3, 2, 4, 5).reshape(n * th * tw, 256, c)
    budget(float((op * op).sum(1).max()), "grouped direct psq")
    exact(psum.view, op.sum(1), "grouped direct psum", lambda ii: f"16x16 patch row {ii[0][0]}")
    exact(psq.view, (op * op).sum(1), "grouped direct psq", lambda ii: f"16x16 patch row {ii[0][0]}")
    psum.check("grouped direct psum")
    psq.check("grouped direct psq")


def test_nt_direct_random_bound(K):
    """random companions of the NT GEMM and the direct kernel (fp32 outputs): |err| <= 2e-5 * (|X| |W|^T)"""
    g = gen(555)
    ratios = []
    for mode, grid, c0, nout in [(0, (1, 90, 100), 936, 152), (2, (2, 37, 41), 64, 128)]:
        n, h, w = grid
        x0 = randn((n, h, w, c0), g)
        w3 = randn((nout, c0, 9 if mode == 2 else 1), g).float()
        taps = 9 if mode == 2 else 1
        wp = K.pack_conv_weight(w3.view(nout, c0, *((3, 3) if taps == 9 else (1, 1))).contiguous())[0]
        out, _, _ = K.k_gemm_nt(x0, None, mode, grid, wp, nout, P.kp32(c0), taps, out_f32=True)
        xs = taps_of(mode, x0, None, grid)
        want = nt_ref(xs, w3.double(), None, 0)
        scale = sum(x.abs() @ w3[:, :, t].abs().t().double() for t, x in enumerate(xs))
        ratios.append(rand_bound(out.reshape(-1, nout), want, scale, f"NT mode {mode}"))
    print("random ratios (NT, direct):", ["%.3e" % v for v in ratios])
