"""The BatchNorm kernels of csrc/hn_norm.hip (round-1 passes, level-packed forms) and csrc/hn_fused.hip (fused passes) held to the
float64 reference of tests/bn_ref.py, pass by pass, through the C entry points.

A. statistics: integer operands, so every fp32 partial sum is exact below 2^24: psum / psq must equal float64 bit for bit.
B. finalize: from exact partial sums, mean / rstd / scale / shift and the running statistics within FIN_ULPS fp32 ulps of float64.
C. apply: every bf16 output must be the bf16 rounding of a value within the fp32 evaluation slack of the float64 value (`slack_fwd`).
D. backward: integer gradients make pg exact for act 0 / 1; pgx, dgamma, dbeta within gamma_n sums; dz and g by the interval check.
E. shapes and edges: C from 8 to 2048 (ragged 128-channel chunks, C8 = 256), M from 7 to 131072, P on both sides of MAX_PROLOGUE_ROWS,
   and the argument checks.
F. accuracy at large per-channel offsets (E[z^2] - mean^2 from fp32 partial sums).
Every output lives between sentinel guard bands (tests/guards.py); a mismatch names the pass, the channel and the row block."""
import ctypes

import pytest
import torch

from tests import bn_ref as B
from tests import exact_checks as X
from tests.exact_checks import BF16, F32, F64, U, EXACT_LIMIT, D, gen, gpu_bf16, exact, within, bf_interval, slack_fwd
from tests.guards import Guarded, dev

pytestmark = pytest.mark.gpu

FIN_ULPS = 4                   # finalize outputs: |err| <= FIN_ULPS * U * (the magnitudes the fp32 expression combines)
SHIFT_ULPS = 2 * FIN_ULPS      # shift = beta - mean * scale also carries the error of scale


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _release():
    yield
    X.release()


def f32(x):
    """the fp32 value a float argument becomes at the C boundary, as a Python float"""
    return float(torch.tensor(x, dtype=F32))


def ints(m, c, lo, hi, g):
    return torch.randint(lo, hi + 1, (m, c), generator=g).to(F64)


def ldof(t):
    return t.stride(0)


def call(K, name, *args):
    K.lib().call(name, *args)


def coef_of(cf):
    """coef [4][C] (scale, shift, mean, rstd) fp32 on the GPU -> float64 CPU dict"""
    c = cf.detach().double().cpu()
    return {"scale": c[0], "shift": c[1], "mean": c[2], "rstd": c[3]}


def fold_depth(rows_per_partial, partials, limit=128):
    """fp32 additions behind one value folded from `partials` partial sums of `rows_per_partial` rows: fold_rows sums groups of
    ceil(partials / 32) of them in fp32 when there are more than `limit` (the rest is double)"""
    return rows_per_partial + ((partials + 31) // 32 if partials > limit else 0) + 2


def host_ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def host_longs(v):
    return (ctypes.c_long * len(v))(*v)


# =====================================================================================================================================
# A. statistics, exact on integer operands
# =====================================================================================================================================
COL_CASES = [
    # name, M, C, ld, align, R (None: hn_colred_rows)
    ("m7_c8", 7, 8, 8, 0, None),
    ("prime_c24_ld32", 1031, 24, 32, 0, None),
    ("prime_c40_r100", 1031, 40, 48, 0, 100),
    ("prime_c152_r13", 1031, 152, 152, 0, 13),
    ("align_c376", 2 * 1221, 376, 384, 1221, None),
    ("prime_c936", 1031, 936, 936, 0, None),
    ("prime_c2048", 1031, 2048, 2048, 0, None),
    ("big_c40", 16 * 64 * 128, 40, 40, 0, None),
    ("big_c8_align", 16 * 64 * 128, 8, 8, 64 * 128, None),
]


@pytest.mark.parametrize("case", COL_CASES, ids=[c[0] for c in COL_CASES])
def test_col_stats_exact(K, case):
    name, m, c, ldx, align, r = case
    plan = K.lib().query("hn_colred_rows", m, align)
    if align:
        assert align % plan == 0, (plan, align)
    r = r or plan
    g = gen("col" + name)
    x = ints(m, c, -4, 4, g)
    xg = gpu_bf16(x, ldx)
    pr = (m + r - 1) // r
    ps, pq = Guarded(pr, c), Guarded(pr, c)
    call(K, "hn_col_stats", xg.data_ptr(), ldof(xg), m, c, r, ps.ptr(), pq.ptr())
    torch.cuda.synchronize()
    s1, s2 = B.block_sums(x, r)
    exact(ps.view, s1, f"hn_col_stats {name} psum (R={r})", f"row block (R={r})")
    exact(pq.view, s2, f"hn_col_stats {name} psq (R={r})", f"row block (R={r})")
    ps.check(f"hn_col_stats {name} psum")
    pq.check(f"hn_col_stats {name} psq")


FSTAT_CASES = [
    # name, M, C, ld, align
    ("m7_c8", 7, 8, 8, 0),
    ("prime_c24", 1031, 24, 40, 0),
    ("prime_c152_chunks", 1031, 152, 160, 0),
    ("align_c376", 4 * 33 * 37, 376, 376, 33 * 37),
    ("c936_align", 2 * 32 * 32, 936, 944, 32 * 32),
    ("c2048", 1031, 2048, 2048, 0),
    ("big_c40_align", 16 * 64 * 128, 40, 40, 64 * 128),
]


@pytest.mark.parametrize("case", FSTAT_CASES, ids=[c[0] for c in FSTAT_CASES])
def test_col_stats_fused_exact(K, case):
    name, m, c, ldx, align = case
    rb = K.lib().query("hn_fused_row_block", m, c, align, 0, 1)
    if align:
        assert align % rb == 0, (rb, align)
    g = gen("fstat" + name)
    x = ints(m, c, -4, 4, g)
    xg = gpu_bf16(x, ldx)
    pr = (m + rb - 1) // rb
    ps, pq = Guarded(pr, c), Guarded(pr, c)
    call(K, "hn_col_stats_fused", xg.data_ptr(), ldof(xg), m, c, rb, ps.ptr(), pq.ptr())
    torch.cuda.synchronize()
    s1, s2 = B.block_sums(x, rb)
    exact(ps.view, s1, f"hn_col_stats_fused {name} psum (RB={rb})", f"row block (RB={rb})")
    exact(pq.view, s2, f"hn_col_stats_fused {name} psq (RB={rb})", f"row block (RB={rb})")
    ps.check(f"hn_col_stats_fused {name} psum")
    pq.check(f"hn_col_stats_fused {name} psq")


@pytest.mark.parametrize("rows,groups,c,two", [(129, 32, 24, True), (1000, 7, 40, True), (4096, 32, 152, False), (33, 32, 8, True)])
def test_rows_reduce2_exact(K, rows, groups, c, two):
    g = gen(f"rr2_{rows}_{groups}_{c}")
    a = ints(rows, c, -1000, 1000, g)
    b = ints(rows, c, 0, 1000, g)
    ag, bg = a.float().to(dev()), b.float().to(dev())
    o1, o2 = Guarded(groups, c), Guarded(groups, c)
    call(K, "hn_rows_reduce2", ag.data_ptr(), bg.data_ptr() if two else None, o1.ptr(), o2.ptr() if two else None, rows, groups, c)
    torch.cuda.synchronize()
    s = (rows + groups - 1) // groups
    exact(o1.view, B.group_sums(a, groups), f"hn_rows_reduce2 out1 (groups of {s})", "group")
    o1.check("hn_rows_reduce2 out1")
    if two:
        exact(o2.view, B.group_sums(b, groups), f"hn_rows_reduce2 out2 (groups of {s})", "group")
    else:
        torch.cuda.synchronize()
        assert bool((o2.buf.view(torch.int32) == 0x7FC00001).all()), "hn_rows_reduce2 wrote out2 without in2"
    o2.check("hn_rows_reduce2 out2")


def test_fold_rows_exact(K):
    g = gen("fold")
    for rows, c in ((128, 24), (129, 24), (600, 40)):
        a = ints(rows, c, -500, 500, g)
        b = ints(rows, c, 0, 500, g)
        f1, f2 = K.fold_rows(a.float().to(dev()), b.float().to(dev()), limit=128)
        torch.cuda.synchronize()
        if rows <= 128:
            exact(f1, a, "fold_rows below the limit (identity)")
            continue
        assert f1.shape == (32, c)
        exact(f1, B.group_sums(a, 32), f"fold_rows {rows} rows psum", "group")
        exact(f2, B.group_sums(b, 32), f"fold_rows {rows} rows psq", "group")


# =====================================================================================================================================
# B. finalize
# =====================================================================================================================================
def bn_params(c, g):
    gamma = (torch.rand(c, generator=g, dtype=F64) + 0.5).float()
    beta = torch.randn(c, generator=g, dtype=F64).float()
    rm = torch.randn(c, generator=g, dtype=F64).float()
    rv = (torch.rand(c, generator=g, dtype=F64) + 0.5).float()
    return gamma, beta, rm, rv


def edge_data(count, c, g, lo=-6, hi=6):
    """integer data with a constant channel (var 0) at 0 and an all-zero channel at c - 1"""
    z = ints(count, c, lo, hi, g)
    z[:, 0] = 3.0
    z[:, c - 1] = 0.0
    return z


def check_finalize(name, st_k, ref, gamma, beta):
    """st_k: float64 dict of the kernel's mean / rstd / scale / shift; ref: bn_ref.finalize of the exact sums"""
    within(st_k["mean"], ref["mean"], FIN_ULPS * U * ref["mean"].abs(), f"{name} mean")
    within(st_k["rstd"], ref["rstd"], FIN_ULPS * U * ref["rstd"], f"{name} rstd")
    within(st_k["scale"], ref["scale"], FIN_ULPS * U * ref["scale"].abs(), f"{name} scale")
    within(st_k["shift"], ref["shift"], SHIFT_ULPS * U * (beta.double().abs() + (ref["mean"] * ref["scale"]).abs()), f"{name} shift")


def check_running(name, rm_k, rv_k, rm0, rv0, ref, count, mom):
    rm_w, rv_w = B.running(rm0, rv0, ref["mean"], ref["var"], count, mom)
    unb = ref["var"] * (count / (count - 1.0)) if count > 1 else ref["var"]
    within(rm_k, rm_w, FIN_ULPS * U * ((1 - mom) * rm0.double().abs() + mom * ref["mean"].abs()) + 1e-30, f"{name} running_mean")
    within(rv_k, rv_w, FIN_ULPS * U * ((1 - mom) * rv0.double().abs() + mom * unb) + 1e-30, f"{name} running_var (unbiased)")


FIN_CASES = [(2, 1e-5, 0.1), (3, 1e-3, 1.0), (120, 1e-5, 1.0), (120, 1e-3, 0.1), (100_003, 1e-5, 1.0), (100_003, 1e-3, 0.1)]


@pytest.mark.parametrize("count,eps,mom", FIN_CASES)
def test_bn_finalize(K, count, eps, mom):
    c = 40
    g = gen(f"fin{count}{eps}{mom}")
    z = edge_data(count, c, g)
    r = K.lib().query("hn_colred_rows", count, 0)
    s1, s2 = B.block_sums(z, r)
    gamma, beta, rm0, rv0 = bn_params(c, g)
    ref = B.finalize(s1.sum(0), s2.sum(0), count, gamma, beta, f32(eps))
    momf = f32(mom)
    dv = lambda t: t.to(dev())
    rm, rv = dv(rm0.clone()), dv(rv0.clone())
    outs = [Guarded(1, c) for _ in range(4)]
    call(K, "hn_bn_finalize", D(s1.float()).data_ptr(), D(s2.float()).data_ptr(), s1.shape[0], c, count, D(gamma).data_ptr(),
         D(beta).data_ptr(), float(eps), float(mom), rm.data_ptr(), rv.data_ptr(), *[o.ptr() for o in outs])
    torch.cuda.synchronize()
    st = {k: o.view[0].double().cpu() for k, o in zip(("scale", "shift", "mean", "rstd"), outs)}
    name = f"hn_bn_finalize count={count} eps={eps} momentum={mom}"
    check_finalize(name, st, ref, gamma, beta)
    assert float(st["rstd"][0]) == pytest.approx(f32(eps) ** -0.5, rel=2 * U), f"{name}: constant channel 0 rstd != eps^-1/2"
    assert float(st["mean"][c - 1]) == 0.0 and float(st["shift"][c - 1]) == float(beta[c - 1]), f"{name}: all-zero channel"
    check_running(name, rm.cpu(), rv.cpu(), rm0, rv0, ref, count, momf)
    for i, o in enumerate(outs):
        o.check(f"{name} output {i}")


@pytest.mark.parametrize("m,c,rb_s", [(1031, 40, 64), (128 * 256, 152, 256), (131072, 24, 128)], ids=["p17", "p128", "p1024_folded"])
@pytest.mark.parametrize("mom", [0.1, 1.0])
def test_apply_fused_prologue_finalize(K, m, c, rb_s, mom):
    """the finalize in hn_bn_apply_fused's prologue (P > 0): P <= 128 partial rows directly, P > 128 after fold_rows (as ops does)"""
    g = gen(f"pro{m}{c}{rb_s}{mom}")
    z = edge_data(m, c, g)
    zg = gpu_bf16(z)
    s1, s2 = B.block_sums(z, rb_s)
    p1, p2 = s1.float().to(dev()), s2.float().to(dev())
    if p1.shape[0] > K.MAX_PROLOGUE_ROWS:
        p1, p2 = K.fold_rows(p1, p2, limit=K.MAX_PROLOGUE_ROWS)
    P = p1.shape[0]
    assert P <= K.MAX_PROLOGUE_ROWS
    gamma, beta, rm0, rv0 = bn_params(c, g)
    eps = 1e-5
    ref = B.finalize(s1.sum(0), s2.sum(0), m, gamma, beta, f32(eps))
    rm, rv = rm0.clone().to(dev()), rv0.clone().to(dev())
    coef = Guarded(4, c)
    out = Guarded(m, c, c + 8, BF16)
    rb = K.lib().query("hn_fused_row_block", m, c, 0, P, 0)
    call(K, "hn_bn_apply_fused", zg.data_ptr(), ldof(zg), m, c, p1.data_ptr(), p2.data_ptr(), P, m, D(gamma).data_ptr(),
         D(beta).data_ptr(), eps, float(mom), rm.data_ptr(), rv.data_ptr(), coef.ptr(), None, 0, 0, out.ptr(), c + 8, None, None, 0, rb)
    torch.cuda.synchronize()
    name = f"hn_bn_apply_fused prologue finalize (P={P} of {s1.shape[0]} partial rows, M={m}, C={c}, momentum={mom})"
    st = coef_of(coef.view)
    check_finalize(name, st, ref, gamma, beta)
    check_running(name, rm.cpu(), rv.cpu(), rm0, rv0, ref, m, f32(mom))
    coef.check(name + " coef")
    out.check(name + " out")


def test_apply_fused_prologue_unfolded_p_above_limit(K):
    """P > MAX_PROLOGUE_ROWS handed to the prologue as is (the kernel walks any P): same finalize"""
    m, c = 300 * 64, 24
    g = gen("unfolded")
    z = edge_data(m, c, g)
    zg = gpu_bf16(z)
    s1, s2 = B.block_sums(z, 64)
    P = s1.shape[0]
    assert P > K.MAX_PROLOGUE_ROWS
    gamma, beta, rm0, rv0 = bn_params(c, g)
    ref = B.finalize(s1.sum(0), s2.sum(0), m, gamma, beta, f32(1e-3))
    coef = Guarded(4, c)
    out = Guarded(m, c, c, BF16)
    rb = K.lib().query("hn_fused_row_block", m, c, 0, P, 0)
    rm, rv = rm0.clone().to(dev()), rv0.clone().to(dev())
    call(K, "hn_bn_apply_fused", zg.data_ptr(), ldof(zg), m, c, D(s1.float()).data_ptr(), D(s2.float()).data_ptr(), P, m,
         D(gamma).data_ptr(), D(beta).data_ptr(), 1e-3, 0.1, rm.data_ptr(), rv.data_ptr(), coef.ptr(), None, 0, 0, out.ptr(), c,
         None, None, 0, rb)
    torch.cuda.synchronize()
    check_finalize(f"hn_bn_apply_fused P={P}", coef_of(coef.view), ref, gamma, beta)
    check_running(f"hn_bn_apply_fused P={P}", rm.cpu(), rv.cpu(), rm0, rv0, ref, m, f32(0.1))
    coef.check("coef")


LEVEL_ROWS = [(128, 50), (256, 256), (384, 300)]         # (rows incl. alignment rows, real rows) per level


def level_data(c, g, rows_cnt, bias_q):
    """level-packed conv output: real rows = bias_q + 0.5 * k (k integer in [-3, 3]), alignment rows = bf16(bias) = bias_q exactly"""
    zs = []
    for rows, cnt in rows_cnt:
        z = bias_q.expand(rows, -1).clone()
        z[:cnt] += 0.5 * ints(cnt, c, -3, 3, g)
        z[:cnt, 1] = bias_q[1]                            # a constant channel over the real rows
        zs.append(z)
    return zs


@pytest.mark.parametrize("mom", [0.1, 1.0])
def test_bn_finalize_levels(K, mom):
    c, div, eps = 24, 64, 1e-3
    g = gen(f"finlev{mom}")
    bias = (torch.rand(c, generator=g, dtype=F64) * 60 + 70).float()      # |bf16(bias)| ~ 100 >> the spread of the real rows (~1)
    bias[c - 1] = 0.0
    bias_q = bias.to(BF16).double()
    zs = level_data(c, g, LEVEL_ROWS, bias_q)
    z = torch.cat(zs)
    s1, s2 = B.block_sums(z, div)
    assert float(s2.max()) < EXACT_LIMIT / 4           # multiples of 1/4: still exact in fp32
    nl = len(LEVEL_ROWS)
    params = [bn_params(c, g) for _ in range(nl)]
    gam = [p[0].to(dev()) for p in params]
    bet = [p[1].to(dev()) for p in params]
    rms = [p[2].clone().to(dev()) for p in params]
    rvs = [p[3].clone().to(dev()) for p in params]
    R = host_longs([r for r, _ in LEVEL_ROWS])
    CNT = host_longs([n for _, n in LEVEL_ROWS])
    ga, ba, rma, rva = host_ptrs(gam), host_ptrs(bet), host_ptrs(rms), host_ptrs(rvs)
    coef = Guarded(nl * 4, c)
    call(K, "hn_bn_finalize_levels", D(s1.float()).data_ptr(), D(s2.float()).data_ptr(), div, c, nl, ctypes.addressof(R),
         ctypes.addressof(CNT), ctypes.addressof(ga), ctypes.addressof(ba), ctypes.addressof(rma), ctypes.addressof(rva), eps, float(mom),
         D(bias).data_ptr(), coef.ptr())
    torch.cuda.synchronize()
    cf = coef.view.view(nl, 4, c)
    for l, ((rows, cnt), zl) in enumerate(zip(LEVEL_ROWS, zs)):
        real = zl[:cnt]
        gamma, beta, rm0, rv0 = params[l]
        ref = B.finalize(real.sum(0), (real * real).sum(0), cnt, gamma, beta, f32(eps))
        name = f"hn_bn_finalize_levels level {l} ({cnt} real of {rows} rows, momentum {mom})"
        check_finalize(name, coef_of(cf[l]), ref, gamma, beta)
        check_running(name, rms[l].cpu(), rvs[l].cpu(), rm0, rv0, ref, cnt, f32(mom))
    coef.check("hn_bn_finalize_levels coef")


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_bn_eval_coeff(K, eps):
    c = 152
    g = gen(f"eval{eps}")
    gamma, beta, rm, rv = bn_params(c, g)
    rv[0] = 0.0                                           # eps alone
    sc, sh = Guarded(1, c), Guarded(1, c)
    call(K, "hn_bn_eval_coeff", D(gamma).data_ptr(), D(beta).data_ptr(), D(rm).data_ptr(), D(rv).data_ptr(), eps,
         c, sc.ptr(), sh.ptr())
    torch.cuda.synchronize()
    # fp32: sqrtf, a division, a product and a difference
    rv_e = (rv + torch.tensor(eps, dtype=F32)).double()   # (rv + eps rounds in fp32 first)
    w_sc = gamma.double() / torch.sqrt(rv_e)
    w_sh = beta.double() - rm.double() * w_sc
    within(sc.view[0], w_sc, FIN_ULPS * U * w_sc.abs(), f"hn_bn_eval_coeff eps={eps} scale")
    within(sh.view[0], w_sh, SHIFT_ULPS * U * (beta.double().abs() + (rm.double() * w_sc).abs()), f"hn_bn_eval_coeff eps={eps} shift")
    sc.check("scale")
    sh.check("shift")


# =====================================================================================================================================
# C. apply
# =====================================================================================================================================
def rand_bf(m, c, g, scale=2.0, offset=None):
    v = torch.randn(m, c, generator=g, dtype=F64) * scale
    if offset is not None:
        v = v + offset
    return v.to(BF16).double()


def rand_coef(c, g):
    sc = (torch.rand(c, generator=g, dtype=F64) * 1.5 + 0.2).float()
    sc[1] = -sc[1]
    sh = (torch.randn(c, generator=g, dtype=F64) * 0.7).float()
    return sc, sh


BNACT_CASES = [
    # name, M, C, ldz, ldo, res, rscale
    ("m7_c8", 7, 8, 8, 16, False, False),
    ("prime_c40_res", 1031, 40, 48, 56, True, False),
    ("prime_c152_res_rscale", 1031, 152, 160, 152, True, True),
    ("c2048_res", 263, 2048, 2048, 2056, True, False),
    ("c936_rscale", 517, 936, 944, 936, True, True),
]


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("case", BNACT_CASES, ids=[c[0] for c in BNACT_CASES])
def test_bn_act_interval(K, case, act):
    name, m, c, ldz, ldo, res, rsc = case
    g = gen(f"bnact{name}{act}")
    z = rand_bf(m, c, g)
    sc, sh = rand_coef(c, g)
    r = rand_bf(m, c, g) if res else None
    rs, rh = rand_coef(c, g) if rsc else (None, None)
    zg = gpu_bf16(z, ldz)
    rg = gpu_bf16(r, ldz + 8) if res else None
    out = Guarded(m, c, ldo, BF16)
    call(K, "hn_bn_act", zg.data_ptr(), ldof(zg), D(sc).data_ptr(), D(sh).data_ptr(), rg.data_ptr() if res else None,
         ldof(rg) if res else 0, D(rs).data_ptr() if rsc else None, D(rh).data_ptr() if rsc else None, act, out.ptr(), ldo, m, c)
    torch.cuda.synchronize()
    x = B.pre_act(z, sc, sh, r, rs, rh)
    y = B.act_fwd(x, act)
    mags = (z * sc.double()).abs() + sh.double().abs()
    if res:
        mags = mags + ((r * rs.double()).abs() + rh.double().abs() if rsc else r.abs()) + x.abs()
    bf_interval(out.view, y, slack_fwd(x, y, mags, act), f"hn_bn_act {name} act {act}")
    out.check(f"hn_bn_act {name} out")


def fused_apply(K, z, c, ldz, P=0, p12=None, count=0, params=None, eps=1e-5, mom=0.1, coef=None, res=None, act=0, want_out=True,
                pool=False, gate=None, hw=0, ldo=None, rb_align=0):
    """one hn_bn_apply_fused launch; returns (out Guarded | None, coef Guarded | None, pool Guarded | None, RB)"""
    m = z.shape[0]
    zg = gpu_bf16(z, ldz)
    rg = gpu_bf16(res, ldz) if res is not None else None
    rb = K.lib().query("hn_fused_row_block", m, c, rb_align or hw, max(P, 0), 0)
    ldo = ldo or c
    out = Guarded(m, c, ldo, BF16) if want_out else None
    pl = Guarded((m + rb - 1) // rb, c) if pool else None
    gamma, beta, rm, rv = [t.to(dev()) if t is not None else None for t in (params or (None,) * 4)]
    call(K, "hn_bn_apply_fused", zg.data_ptr(), ldz, m, c, p12[0].data_ptr() if P > 0 else None, p12[1].data_ptr() if P > 0 else None, P,
         count, gamma.data_ptr() if gamma is not None else None, beta.data_ptr() if beta is not None else None, eps, mom,
         rm.data_ptr() if rm is not None else None, rv.data_ptr() if rv is not None else None, coef.ptr() if coef is not None else None,
         rg.data_ptr() if rg is not None else None, ldof(rg) if rg is not None else 0, act, out.ptr() if want_out else None,
         ldo if want_out else 0, pl.ptr() if pool else None, D(gate).data_ptr() if gate is not None else None, hw, rb)
    torch.cuda.synchronize()
    return out, pl, rb


def expect_apply(z, st, act, res=None):
    x = B.pre_act(z, st["scale"], st["shift"], res)
    y = B.act_fwd(x, act)
    mags = (z * st["scale"]).abs() + st["shift"].abs()
    if res is not None:
        mags = mags + res.abs() + x.abs()
    return y, slack_fwd(x, y, mags, act)


FAPPLY_SHAPES = [(7, 8, 8), (1031, 24, 32), (1031, 152, 160), (2 * 1221, 376, 384), (517, 936, 936), (263, 2048, 2048)]


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("shape", FAPPLY_SHAPES, ids=[f"m{s[0]}_c{s[1]}" for s in FAPPLY_SHAPES])
def test_apply_fused_training(K, shape, act):
    """P > 0: coef from the prologue (checked in B), out by the interval check with the kernel's own coef"""
    m, c, ldz = shape
    g = gen(f"fat{m}{c}{act}")
    z = rand_bf(m, c, g, 2.0, torch.randn(c, generator=g, dtype=F64))
    s1, s2 = B.block_sums(z, 64)
    p12 = (s1.float().to(dev()), s2.float().to(dev()))
    params = bn_params(c, g)
    coef = Guarded(4, c)
    res = rand_bf(m, c, g) if act in (1, 2) else None
    out, _, rb = fused_apply(K, z, c, ldz, P=s1.shape[0], p12=p12, count=m, params=params, coef=coef, act=act, res=res, ldo=c + 8)
    y, s = expect_apply(z, coef_of(coef.view), act, res)
    bf_interval(out.view, y, s, f"hn_bn_apply_fused P>0 M={m} C={c} act {act}{' res' if res is not None else ''}", rb)
    out.check("out")
    coef.check("coef")


@pytest.mark.parametrize("mode", ["coef", "identity", "eval", "res"])
@pytest.mark.parametrize("shape", [(1031, 40, 48), (517, 936, 936)], ids=["c40", "c936"])
def test_apply_fused_modes(K, mode, shape):
    m, c, ldz = shape
    g = gen(f"fam{mode}{m}{c}")
    z = rand_bf(m, c, g)
    act = 2 if mode == "eval" else 1
    gamma, beta, rm, rv = bn_params(c, g)
    res = rand_bf(m, c, g) if mode == "res" else None
    eps = 1e-3
    if mode in ("coef", "res"):
        sc, sh = rand_coef(c, g)
        cf = Guarded(4, c)
        cf.view.copy_(torch.stack([sc, sh, torch.zeros(c), torch.ones(c)]).to(dev()))
        out, _, rb = fused_apply(K, z, c, ldz, P=0, coef=cf, act=act, res=res, ldo=c + 16)
        st = {"scale": sc.double(), "shift": sh.double()}
    elif mode == "identity":
        out, _, rb = fused_apply(K, z, c, ldz, P=0, coef=None, act=act)
        st = {"scale": torch.ones(c, dtype=F64), "shift": torch.zeros(c, dtype=F64)}
    else:
        cf = Guarded(4, c)
        out, _, rb = fused_apply(K, z, c, ldz, P=-1, params=(gamma, beta, rm, rv), eps=eps, coef=cf, act=act)
        rv_e = (rv + torch.tensor(eps, dtype=F32)).double()
        w_rs = 1.0 / torch.sqrt(rv_e)
        k = coef_of(cf.view)
        within(k["rstd"], w_rs, FIN_ULPS * U * w_rs, "eval rstd")
        within(k["scale"], gamma.double() * w_rs, FIN_ULPS * U * gamma.double() * w_rs, "eval scale")
        within(k["shift"], beta.double() - rm.double() * k["scale"], SHIFT_ULPS * U * (beta.double().abs() + (rm.double() * k["scale"]).abs()),
               "eval shift")
        assert torch.equal(k["mean"], rm.double()), "eval mean != running_mean"
        cf.check("eval coef")
        st = k
    y, s = expect_apply(z, st, act, res)
    bf_interval(out.view, y, s, f"hn_bn_apply_fused mode {mode} C={c}", rb)
    out.check(f"{mode} out")


@pytest.mark.parametrize("c,n,hw", [(40, 3, 16 * 24), (152, 2, 33 * 37), (936, 2, 8 * 8)])
def test_apply_fused_gate_pool(K, c, n, hw):
    """SE: gate applied to the bf16 output, pool = per-row-block sums of the gated output; out == null (pool only) gives the same pool"""
    m = n * hw
    g = gen(f"gate{c}{n}{hw}")
    z = rand_bf(m, c, g)
    sc, sh = rand_coef(c, g)
    cf = Guarded(4, c)
    cf.view.copy_(torch.stack([sc, sh, torch.zeros(c), torch.ones(c)]).to(dev()))
    gate = torch.rand(n, c, generator=g, dtype=F64).float() * 0.98 + 0.01
    out, pool, rb = fused_apply(K, z, c, c, P=0, coef=cf, act=1, pool=True, gate=gate, hw=hw, ldo=c + 8)
    assert hw % rb == 0
    x = B.pre_act(z, sc, sh)
    y = B.act_fwd(x, 1)
    s = slack_fwd(x, y, (z * sc.double()).abs() + sh.double().abs(), 1) + 2 * U * y.abs()
    lo = (y - s).float().to(BF16).float()
    hi = (y + s).float().to(BF16).float()
    gr = gate.repeat_interleave(hw, 0)                    # [m][c]: gate of the row's image
    want_lo = (lo * gr).to(BF16).double()                 # fp32 product of the bf16 output and the gate, rounded to bf16: monotone
    want_hi = (hi * gr).to(BF16).double()
    mid = (want_lo + want_hi) / 2
    bf_interval(out.view, mid, (want_hi - want_lo) / 2, f"hn_bn_apply_fused gate C={c}", rb)
    o = out.view.double().cpu()
    nb = (m + rb - 1) // rb
    ps = o.view(nb, rb, c).sum(1)
    bound = rb * U * o.abs().view(nb, rb, c).sum(1)
    within(pool.view, ps, bound, f"hn_bn_apply_fused pool (RB={rb}) C={c}", "row block, channel")
    _, pool2, rb2 = fused_apply(K, z, c, c, P=0, coef=cf, act=1, pool=True, gate=gate, hw=hw, want_out=False)
    assert rb2 == rb
    within(pool2.view, ps, bound, f"hn_bn_apply_fused pool only (out == null) C={c}", "row block, channel")
    out.check("gate out")
    pool.check("pool")
    pool2.check("pool only")


@pytest.mark.parametrize("act", [0, 1, 2])
def test_bn_act_levels_interval(K, act):
    c = 40
    g = gen(f"actlev{act}")
    rows = [128, 256, 384]
    nl = len(rows)
    z = rand_bf(sum(rows), c, g)
    cfs = [torch.stack([*rand_coef(c, g), torch.zeros(c), torch.ones(c)]) for _ in range(nl)]
    coef = torch.stack(cfs).to(dev())
    zg = gpu_bf16(z, c + 8)
    out = Guarded(sum(rows), c, c + 8, BF16)
    R = host_longs(rows)
    call(K, "hn_bn_act_levels", zg.data_ptr(), ldof(zg), coef.data_ptr(), act, out.ptr(), c + 8, c, nl, ctypes.addressof(R))
    torch.cuda.synchronize()
    sc = torch.cat([cfs[l][0].double().expand(rows[l], c) for l in range(nl)])
    sh = torch.cat([cfs[l][1].double().expand(rows[l], c) for l in range(nl)])
    x = z * sc + sh
    y = B.act_fwd(x, act)
    bf_interval(out.view, y, slack_fwd(x, y, (z * sc).abs() + sh.abs(), act), f"hn_bn_act_levels act {act}", 128)
    out.check("levels out")


# =====================================================================================================================================
# D. backward
# =====================================================================================================================================
def unambiguous(z, st, act):
    """move z off the ReLU kink where the fp32 pre-activation's sign is not determined (|sc z + sh| within its rounding): one bf16 step"""
    if act != B.ACT_RELU:
        return z
    x = z * st["scale"] + st["shift"]
    amb = x.abs() <= 8 * U * ((z * st["scale"]).abs() + st["shift"].abs())
    if bool(amb.any()):
        z = z.clone()
        z[amb] = (z[amb] * (1 + 2.0 ** -7) + 2.0 ** -7).to(BF16).double()
    return z


def grad_slack(d, z, st, act):
    """|g_kernel - g_ref| bound: exact for act 0 / 1 (a product by 0 or 1) and the saved-output mask, else the error of act'(pre)"""
    if act in (B.ACT_NONE, B.ACT_RELU):
        return torch.zeros_like(d)
    x = z * st["scale"] + st["shift"]
    dpre = 4 * U * ((z * st["scale"]).abs() + st["shift"].abs())
    return d.abs() * (dpre + 16 * U * (2 + x.abs()))


def check_bwd_sums(name, pg, pgx, g, xhat, dg, rb, integer):
    """partial sums over row blocks of rb rows: pg exact when g is integer, else and pgx within gamma_rb sums"""
    nb = pg.shape[0]
    m, c = g.shape
    padr = nb * rb - m
    blk = lambda t: torch.cat([t, torch.zeros(padr, c, dtype=F64)]).view(nb, rb, c)
    w_pg, w_pgx = blk(g).sum(1), blk(g * xhat).sum(1)
    if integer:
        exact(pg, w_pg, f"{name} pg", f"row block (R={rb})")
    else:
        within(pg, w_pg, B.gamma_n(rb) * blk(g.abs()).sum(1) + blk(dg).sum(1), f"{name} pg", "row block, channel")
    within(pgx, w_pgx, B.gamma_n(rb + 3) * blk((g * xhat).abs()).sum(1) + blk(dg * xhat.abs()).sum(1) + 1e-30, f"{name} pgx",
           "row block, channel")
    return blk(g.abs()).sum(1), blk((g * xhat).abs()).sum(1)


def check_dz(name, dz, gout, g, dg, xhat, st, count, n_sum, rb=None):
    """dz = sc (g - mg - xhat mgx): the interval check, with the slack of the kernel's mg / mgx (gamma_{n_sum} sums) and of the fp32
    expression"""
    bw_mg = g.sum(0) / count
    bw_mgx = (g * xhat).sum(0) / count
    d_mg = (B.gamma_n(n_sum) * g.abs().sum(0) + dg.sum(0)) / count + 2 * U * bw_mg.abs()
    d_mgx = (B.gamma_n(n_sum) * (g * xhat).abs().sum(0) + (dg * xhat.abs()).sum(0)) / count + 2 * U * bw_mgx.abs()
    sc = st["scale"]
    y = sc * (g - bw_mg - xhat * bw_mgx)
    s = sc.abs() * (dg + d_mg + xhat.abs() * d_mgx + 4 * U * (g.abs() + bw_mg.abs() + (xhat * bw_mgx).abs() + 2 * xhat.abs() * bw_mgx.abs()))
    bf_interval(dz, y, s, f"{name} dz", rb)
    if gout is not None:
        bf_interval(gout, g, dg, f"{name} gout", rb)
    return bw_mg, bw_mgx


def fwd_coef(K, z, c, params, eps=1e-5):
    """the kernel's own forward coefficients (hn_bn_apply_fused, P > 0, no output stores but the coef) as float64 dict + GPU tensor"""
    s1, s2 = B.block_sums(z, 64)
    cf = Guarded(4, c)
    fused_apply(K, z, c, c, P=s1.shape[0], p12=(s1.float().to(dev()), s2.float().to(dev())), count=z.shape[0], params=params, eps=eps,
                coef=cf, act=0)
    return coef_of(cf.view), cf


BWD_SHAPES = [(7, 8), (1031, 40), (1031, 152), (2 * 1221, 376), (517, 936), (263, 2048)]


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=[f"m{s[0]}_c{s[1]}" for s in BWD_SHAPES])
def test_bwd_round1(K, shape, act):
    """hn_bn_bwd_reduce (R = hn_colred_rows) -> fold -> hn_bn_bwd_finalize -> hn_bn_bwd_apply"""
    m, c = shape
    g = gen(f"bw1{m}{c}{act}")
    z = rand_bf(m, c, g, 3.0, torch.randn(c, generator=g, dtype=F64))
    params = bn_params(c, g)
    st, cf = fwd_coef(K, z, c, params)
    z = unambiguous(z, st, act)
    d = ints(m, c, -3, 3, g)
    gin = B.grad_in(d, z, st["scale"], st["shift"], act)
    dg = grad_slack(d, z, st, act)
    xhat = (z - st["mean"]) * st["rstd"]
    zg, dgpu = gpu_bf16(z, c + 8), gpu_bf16(d, c + 16)
    r = K.lib().query("hn_colred_rows", m, 0)
    pr = (m + r - 1) // r
    pg, pgx = Guarded(pr, c), Guarded(pr, c)
    cfv = cf.view
    call(K, "hn_bn_bwd_reduce", dgpu.data_ptr(), ldof(dgpu), zg.data_ptr(), ldof(zg), None, 0, cfv[0].data_ptr(), cfv[1].data_ptr(),
         cfv[2].data_ptr(), cfv[3].data_ptr(), act, m, c, r, pg.ptr(), pgx.ptr())
    torch.cuda.synchronize()
    name = f"round-1 backward M={m} C={c} act {act}"
    check_bwd_sums(name + " hn_bn_bwd_reduce", pg.view, pgx.view, gin, xhat, dg, r, act in (0, 1))
    pg.check("pg")
    pgx.check("pgx")
    f1, f2 = K.fold_rows(pg.view, pgx.view)
    n_sum = fold_depth(r, pr)
    outs = [Guarded(1, c) for _ in range(4)]
    call(K, "hn_bn_bwd_finalize", f1.data_ptr(), f2.data_ptr(), f1.shape[0], c, m, *[o.ptr() for o in outs])
    dz, gout = Guarded(m, c, c + 8, BF16), Guarded(m, c, c + 24, BF16)
    call(K, "hn_bn_bwd_apply", dgpu.data_ptr(), ldof(dgpu), zg.data_ptr(), ldof(zg), None, 0, cfv[0].data_ptr(), cfv[1].data_ptr(),
         cfv[2].data_ptr(), cfv[3].data_ptr(), outs[2].ptr(), outs[3].ptr(), act, dz.ptr(), c + 8, gout.ptr(), c + 24, m, c)
    torch.cuda.synchronize()
    w_db, w_dgm = gin.sum(0), (gin * xhat).sum(0)
    if act in (0, 1):
        exact(outs[1].view, w_db[None], name + " hn_bn_bwd_finalize dbeta", "row")
    else:
        within(outs[1].view[0], w_db, B.gamma_n(n_sum) * gin.abs().sum(0) + dg.sum(0) + U * w_db.abs(), name + " dbeta")
    within(outs[0].view[0], w_dgm, B.gamma_n(n_sum) * (gin * xhat).abs().sum(0) + (dg * xhat.abs()).sum(0) + U * w_dgm.abs(),
           name + " hn_bn_bwd_finalize dgamma")
    check_dz(name + " hn_bn_bwd_apply", dz.view, gout.view, gin, dg, xhat, st, m, n_sum)
    for i, o in enumerate(outs):
        o.check(f"finalize output {i}")
    dz.check("dz")
    gout.check("gout")


def fused_backward(K, name, z, d, c, st, cf, act, y=None, gate=None, dpool=None, hw=0, want_g=True, zero_c=True):
    """hn_bn_bwd_reduce_fused -> (fold) -> hn_bn_bwd_apply_fused with guard bands; returns the kernel outputs"""
    m = z.shape[0]
    zg, dgpu = gpu_bf16(z, c + 8), gpu_bf16(d, c + 16)
    yg = gpu_bf16(y, c + 24) if y is not None else None
    gd = gate.to(dev()) if gate is not None else None
    dpd = dpool.to(dev()) if dpool is not None else None
    rb_r = K.lib().query("hn_fused_row_block", m, c, hw, 0, 1)
    pr = (m + rb_r - 1) // rb_r
    pg, pgx = Guarded(pr, c), Guarded(pr, c)
    call(K, "hn_bn_bwd_reduce_fused", dgpu.data_ptr(), ldof(dgpu), zg.data_ptr(), ldof(zg), yg.data_ptr() if y is not None else None,
         ldof(yg) if y is not None else 0, cf.ptr(), act, gd.data_ptr() if gd is not None else None,
         dpd.data_ptr() if dpd is not None else None, hw, m, c, rb_r, pg.ptr(), pgx.ptr())
    torch.cuda.synchronize()
    f1, f2 = pg.view, pgx.view
    if pr > K.MAX_PROLOGUE_ROWS:
        f1, f2 = K.fold_rows(f1.contiguous(), f2.contiguous(), limit=K.MAX_PROLOGUE_ROWS)
    P = f1.shape[0]
    rb_a = K.lib().query("hn_fused_row_block", m, c, hw, P, 0)
    dgam, dbet = Guarded(1, c), Guarded(1, c)
    zc = Guarded(1, c) if zero_c else None
    dz = Guarded(m, c, c + 8, BF16)
    gout = Guarded(m, c, c + 16, BF16) if want_g else None
    call(K, "hn_bn_bwd_apply_fused", dgpu.data_ptr(), ldof(dgpu), zg.data_ptr(), ldof(zg), yg.data_ptr() if y is not None else None,
         ldof(yg) if y is not None else 0, cf.ptr(), act, gd.data_ptr() if gd is not None else None,
         dpd.data_ptr() if dpd is not None else None, hw, f1.data_ptr(), f2.data_ptr(), P, m, dgam.ptr(), dbet.ptr(), dz.ptr(), c + 8,
         gout.ptr() if want_g else None, c + 16 if want_g else 0, m, c, rb_a, zc.ptr() if zc is not None else None)
    torch.cuda.synchronize()
    n_sum = fold_depth(rb_r, pr, K.MAX_PROLOGUE_ROWS)
    return {"pg": pg, "pgx": pgx, "rb_r": rb_r, "P": P, "rb_a": rb_a, "dgamma": dgam, "dbeta": dbet, "zero": zc, "dz": dz, "gout": gout,
            "n_sum": n_sum}


def check_fused_backward(name, o, gin, dg, xhat, st, m, integer):
    check_bwd_sums(name + " hn_bn_bwd_reduce_fused", o["pg"].view, o["pgx"].view, gin, xhat, dg, o["rb_r"], integer)
    n_sum = o["n_sum"]
    w_db, w_dgm = gin.sum(0), (gin * xhat).sum(0)
    if integer:
        exact(o["dbeta"].view, w_db[None], name + " hn_bn_bwd_apply_fused dbeta", "row")
    else:
        within(o["dbeta"].view[0], w_db, B.gamma_n(n_sum) * gin.abs().sum(0) + dg.sum(0) + U * w_db.abs(), name + " dbeta")
    within(o["dgamma"].view[0], w_dgm, B.gamma_n(n_sum) * (gin * xhat).abs().sum(0) + (dg * xhat.abs()).sum(0) + U * w_dgm.abs(),
           name + " hn_bn_bwd_apply_fused dgamma")
    check_dz(name + " hn_bn_bwd_apply_fused", o["dz"].view, o["gout"].view if o["gout"] is not None else None, gin, dg, xhat, st, m, n_sum,
             o["rb_a"])
    if o["zero"] is not None:
        assert bool((o["zero"].view == 0).all()), f"{name}: zero_c not zeroed"
    for k in ("pg", "pgx", "dgamma", "dbeta", "zero", "dz", "gout"):
        if o[k] is not None:
            o[k].check(f"{name} {k}")


FBWD_SHAPES = [(7, 8), (1031, 24), (1031, 152), (2 * 1221, 376), (517, 936), (263, 2048), (16 * 64 * 128, 40)]


# the large shape with the exact activations only (the transcendental ones are covered at the other shapes)
FBWD_CASES = [(s, a) for s in FBWD_SHAPES for a in B.ACTS if s[0] < 100_000 or a in (B.ACT_NONE, B.ACT_RELU)]


@pytest.mark.parametrize("shape,act", FBWD_CASES, ids=[f"m{s[0]}_c{s[1]}-{a}" for s, a in FBWD_CASES])
def test_bwd_fused_act(K, shape, act):
    m, c = shape
    g = gen(f"bwf{m}{c}{act}")
    z = rand_bf(m, c, g, 3.0, torch.randn(c, generator=g, dtype=F64))
    st, cf = fwd_coef(K, z, c, bn_params(c, g))
    z = unambiguous(z, st, act)
    d = ints(m, c, -3, 3, g)
    gin = B.grad_in(d, z, st["scale"], st["shift"], act)
    dg = grad_slack(d, z, st, act)
    xhat = (z - st["mean"]) * st["rstd"]
    o = fused_backward(K, "", z, d, c, st, cf, act, want_g=act != 2, zero_c=act == 1)
    check_fused_backward(f"fused backward M={m} C={c} act {act} (P={o['P']})", o, gin, dg, xhat, st, m, act in (0, 1))


@pytest.mark.parametrize("shape", [(1031, 40), (517, 936)], ids=["c40", "c936"])
def test_bwd_fused_masked(K, shape):
    """the saved block output y: g = dout * [y > 0], y a bf16 tensor with exact zeros and negatives"""
    m, c = shape
    g = gen(f"bwm{m}{c}")
    z = rand_bf(m, c, g, 2.0)
    st, cf = fwd_coef(K, z, c, bn_params(c, g))
    y = rand_bf(m, c, g).clamp(min=0.0)
    y[::3] = -y[::3]
    d = rand_bf(m, c, g)
    gin = B.grad_in(d, z, st["scale"], st["shift"], 0, y=y)
    xhat = (z - st["mean"]) * st["rstd"]
    o = fused_backward(K, "", z, d, c, st, cf, 0, y=y)
    check_fused_backward(f"fused backward masked C={c}", o, gin, torch.zeros_like(gin), xhat, st, m, False)


@pytest.mark.parametrize("c,n,hw", [(40, 3, 16 * 16), (152, 2, 32 * 32), (936, 2, 8 * 8)])
def test_bwd_fused_se(K, c, n, hw):
    """SE form: g = bf16(dout * gate + dpool / HW) * [pre > 0].  Gate k/4, dpool = HW * j / 8 and HW a power of two make g exact"""
    m = n * hw
    g = gen(f"bwse{c}{n}{hw}")
    z = rand_bf(m, c, g, 2.0)
    st, cf = fwd_coef(K, z, c, bn_params(c, g))
    z = unambiguous(z, st, 1)
    d = ints(m, c, -3, 3, g)
    gate = torch.randint(1, 5, (n, c), generator=g).double() / 4
    dpool = torch.randint(-4, 5, (n, c), generator=g).double() * hw / 8
    v = d * gate.repeat_interleave(hw, 0) + (dpool / hw).repeat_interleave(hw, 0)
    assert torch.equal(v.to(BF16).double(), v)
    gin = B.grad_in(v, z, st["scale"], st["shift"], 1)
    xhat = (z - st["mean"]) * st["rstd"]
    o = fused_backward(K, "", z, d, c, st, cf, 1, gate=gate.float(), dpool=dpool.float(), hw=hw)
    assert hw % o["rb_r"] == 0 and hw % o["rb_a"] == 0
    check_fused_backward(f"fused backward SE C={c} HW={hw}", o, gin, torch.zeros_like(gin), xhat, st, m, True)


@pytest.mark.parametrize("act", [0, 1, 2])
def test_bwd_levels(K, act):
    """hn_bn_bwd_reduce_levels -> hn_bn_bwd_finalize_levels -> hn_bn_bwd_apply_levels with the coefficients of
    hn_bn_finalize_levels; dout is zero on the alignment rows (as the heads produce it), count = real rows"""
    c, R = 40, 64
    g = gen(f"bwlev{act}")
    bias = (torch.randn(c, generator=g, dtype=F64) * 0.3).float()
    bias_q = bias.to(BF16).double()
    zs = []
    for rows, cnt in LEVEL_ROWS:
        zl = bias_q.expand(rows, -1).clone()
        zl[:cnt] = rand_bf(cnt, c, g, 2.0)
        zs.append(zl)
    z = torch.cat(zs)
    nl = len(LEVEL_ROWS)
    s1, s2 = B.block_sums(z, R)
    params = [bn_params(c, g) for _ in range(nl)]
    Rr = host_longs([r for r, _ in LEVEL_ROWS])
    CNT = host_longs([n for _, n in LEVEL_ROWS])
    gam = [p[0].to(dev()) for p in params]
    bet = [p[1].to(dev()) for p in params]
    ga, ba = host_ptrs(gam), host_ptrs(bet)
    coef = Guarded(nl * 4, c)
    call(K, "hn_bn_finalize_levels", D(s1.float()).data_ptr(), D(s2.float()).data_ptr(), R, c, nl, ctypes.addressof(Rr),
         ctypes.addressof(CNT), ctypes.addressof(ga), ctypes.addressof(ba), None, None, 1e-5, 0.1, D(bias).data_ptr(), coef.ptr())
    torch.cuda.synchronize()
    cfl = coef.view.view(nl, 4, c).double().cpu()
    per_row = lambda k: torch.cat([cfl[l][k].expand(LEVEL_ROWS[l][0], c) for l in range(nl)])
    st = {"scale": per_row(0), "shift": per_row(1), "mean": per_row(2), "rstd": per_row(3)}
    z = unambiguous(z, st, act)
    d = ints(z.shape[0], c, -3, 3, g)
    off = 0
    for rows, cnt in LEVEL_ROWS:
        d[off + cnt:off + rows] = 0.0
        off += rows
    gin = B.grad_in(d, z, st["scale"], st["shift"], act)
    dg = grad_slack(d, z, st, act)
    xhat = (z - st["mean"]) * st["rstd"]
    zg, dgpu = gpu_bf16(z, c + 8), gpu_bf16(d, c)
    total = z.shape[0]
    pg, pgx = Guarded(total // R, c), Guarded(total // R, c)
    call(K, "hn_bn_bwd_reduce_levels", dgpu.data_ptr(), ldof(dgpu), zg.data_ptr(), ldof(zg), None, 0, coef.ptr(), act, c, R, nl,
         ctypes.addressof(Rr), pg.ptr(), pgx.ptr())
    torch.cuda.synchronize()
    name = f"level-packed backward act {act}"
    check_bwd_sums(name + " hn_bn_bwd_reduce_levels", pg.view, pgx.view, gin, xhat, dg, R, act in (0, 1))
    red = Guarded(nl * 2, c)
    dgs = [Guarded(1, c) for _ in range(nl)]
    dbs = [Guarded(1, c) for _ in range(nl)]
    zc = Guarded(1, c)
    dga = (ctypes.c_void_p * nl)(*[x.ptr() for x in dgs])
    dba = (ctypes.c_void_p * nl)(*[x.ptr() for x in dbs])
    call(K, "hn_bn_bwd_finalize_levels", pg.ptr(), pgx.ptr(), R, c, nl, ctypes.addressof(Rr), ctypes.addressof(CNT), ctypes.addressof(dga),
         ctypes.addressof(dba), red.ptr(), zc.ptr())
    dz = Guarded(total, c, c + 16, BF16)
    call(K, "hn_bn_bwd_apply_levels", dgpu.data_ptr(), ldof(dgpu), zg.data_ptr(), ldof(zg), None, 0, coef.ptr(), red.ptr(), act, dz.ptr(), c + 16,
         c, nl, ctypes.addressof(Rr))
    torch.cuda.synchronize()
    assert bool((zc.view == 0).all()), "zero_c not zeroed"
    off = 0
    rdv = red.view.view(nl, 2, c).double().cpu()
    for l, (rows, cnt) in enumerate(LEVEL_ROWS):
        sl = slice(off, off + rows)
        gl, xl, dgl = gin[sl], xhat[sl], dg[sl]
        w_db, w_dgm = gl.sum(0), (gl * xl).sum(0)
        b_db = B.gamma_n(rows) * gl.abs().sum(0) + dgl.sum(0) + U * w_db.abs()
        b_dgm = B.gamma_n(rows) * (gl * xl).abs().sum(0) + (dgl * xl.abs()).sum(0) + U * w_dgm.abs()
        lname = f"{name} level {l}"
        if act in (0, 1):
            exact(dbs[l].view, w_db[None], lname + " dbeta", "row")
        else:
            within(dbs[l].view[0], w_db, b_db, lname + " dbeta")
        within(dgs[l].view[0], w_dgm, b_dgm, lname + " dgamma")
        within(rdv[l][0], w_db / cnt, b_db / cnt + U * (w_db / cnt).abs(), lname + " mean(g) (count = real rows)")
        within(rdv[l][1], w_dgm / cnt, b_dgm / cnt + U * (w_dgm / cnt).abs(), lname + " mean(g xhat) (count = real rows)")
        stl = {k: v[sl] for k, v in st.items()}
        check_dz(lname + " hn_bn_bwd_apply_levels", dz.view[sl], None, gl, dgl, xl, stl, cnt, rows + 2, 128)
        off += rows
    for x in [pg, pgx, red, zc, dz] + dgs + dbs:
        x.check(name)


# =====================================================================================================================================
# E. argument checks: C8 > 256 and C % 8 != 0 are refused, not run
# =====================================================================================================================================
def test_bad_channel_counts_raise(K):
    from multitask_hydranet_amd._lib import HipKernelError
    m = 8
    for c in (2056, 20):
        ldc = (c + 7) // 8 * 8
        x = torch.zeros(m, ldc, dtype=BF16, device=dev())
        o = torch.zeros(m, ldc, dtype=BF16, device=dev())
        f = torch.zeros(8, ldc, dtype=F32, device=dev())
        cf = torch.zeros(4 * 5 * ldc, dtype=F32, device=dev())
        R = host_longs([128])
        big = torch.zeros(128, ldc, dtype=BF16, device=dev())
        calls = {
            "hn_col_stats": (x.data_ptr(), ldc, m, c, 8, f.data_ptr(), f.data_ptr()),
            "hn_bn_act": (x.data_ptr(), ldc, cf.data_ptr(), cf.data_ptr(), None, 0, None, None, 1, o.data_ptr(), ldc, m, c),
            "hn_bn_bwd_reduce": (x.data_ptr(), ldc, x.data_ptr(), ldc, None, 0, cf.data_ptr(), cf.data_ptr(), cf.data_ptr(), cf.data_ptr(), 0, m,
                                 c, 8, f.data_ptr(), f.data_ptr()),
            "hn_bn_bwd_apply": (x.data_ptr(), ldc, x.data_ptr(), ldc, None, 0, cf.data_ptr(), cf.data_ptr(), cf.data_ptr(), cf.data_ptr(),
                                cf.data_ptr(), cf.data_ptr(), 0, o.data_ptr(), ldc, None, 0, m, c),
            "hn_bn_act_levels": (big.data_ptr(), ldc, cf.data_ptr(), 0, big.data_ptr(), ldc, c, 1, ctypes.addressof(R)),
            "hn_bn_bwd_apply_levels": (big.data_ptr(), ldc, big.data_ptr(), ldc, None, 0, cf.data_ptr(), cf.data_ptr(), 0, big.data_ptr(), ldc,
                                       c, 1, ctypes.addressof(R)),
        }
        if c % 8:
            calls.update({
                "hn_col_stats_fused": (x.data_ptr(), ldc, m, c, 8, f.data_ptr(), f.data_ptr()),
                "hn_bn_apply_fused": (x.data_ptr(), ldc, m, c, None, None, 0, 0, None, None, 1e-5, 0.1, None, None, cf.data_ptr(), None, 0, 0,
                                      o.data_ptr(), ldc, None, None, 0, 8),
                "hn_bn_bwd_reduce_fused": (x.data_ptr(), ldc, x.data_ptr(), ldc, None, 0, cf.data_ptr(), 0, None, None, 0, m, c, 8,
                                           f.data_ptr(), f.data_ptr()),
                "hn_bn_bwd_apply_fused": (x.data_ptr(), ldc, x.data_ptr(), ldc, None, 0, cf.data_ptr(), 0, None, None, 0, f.data_ptr(),
                                          f.data_ptr(), 1, m, cf.data_ptr(), cf.data_ptr(), o.data_ptr(), ldc, None, 0, m, c, 8, None),
            })
        for name, args in calls.items():
            with pytest.raises(HipKernelError):
                K.lib().call(name, *args)
    torch.cuda.synchronize()
    assert bool((o == 0).all()), "a refused call wrote its output"


# =====================================================================================================================================
# F. accuracy at large per-channel offsets (non-integer data)
# =====================================================================================================================================
@pytest.mark.parametrize("path", ["round1", "fused"])
def test_stats_large_offsets(K, path):
    """channels with mean / std up to 32 (fp32 sums of z and z^2, finished as E[z^2] - mean^2 in double): the variance error within
    gamma_R (sum z^2 + 2 |mean| sum |z|) / count (R = rows per partial sum of the plan) and rstd within 1e-3 of float64"""
    m, c = 16 * 64 * 128, 40
    g = gen("large" + path)
    std = torch.tensor([0.125, 1.0, 3.0, 0.5] * 10, dtype=F64)
    ratio = torch.tensor([0.0, 1.0, 8.0, 16.0, 32.0, -32.0, 24.0, -8.0, 32.0, 2.0] * 4, dtype=F64)
    z = (torch.randn(m, c, generator=g, dtype=F64) * std + ratio * std).to(BF16).double()
    zg = gpu_bf16(z)
    gamma, beta, _, _ = bn_params(c, g)
    eps = 1e-5
    if path == "round1":
        r = K.lib().query("hn_colred_rows", m, 0)
        ps, pq, _ = K.k_col_stats(zg.view(1, 1, m, c))
        coef = K.k_bn_finalize(ps, pq, m, gamma.to(dev()), beta.to(dev()), eps, 0.1, None, None)
    else:
        r = K.lib().query("hn_fused_row_block", m, c, 0, 0, 1)
        ps, pq = K.k_col_stats_fused(zg.view(1, 1, m, c))
        _, coef, _, _ = K.k_bn_apply_fused(zg.view(1, 1, m, c), ps, pq, m, gamma.to(dev()), beta.to(dev()), eps, 0.1, None, None, 0,
                                           want_out=True)
    torch.cuda.synchronize()
    st = coef_of(coef)
    ref = B.stats(z, gamma, beta, f32(eps))
    var_k = st["rstd"] ** -2 - f32(eps)
    n = fold_depth(r, (m + r - 1) // r)
    bound = B.gamma_n(n) * ((z * z).sum(0) + 2 * ref["mean"].abs() * z.abs().sum(0)) / m + 4 * U * (ref["var"] + f32(eps))
    within(var_k, ref["var"], bound, f"{path} statistics: variance at mean/std up to 32 (R={r})")
    rel = ((st["rstd"] - ref["rstd"]) / ref["rstd"]).abs()
    worst = int(rel.argmax())
    print(f"{path}: worst rstd rel err {float(rel.max()):.3e} at channel {worst} (mean/std {float(ratio[worst]):.0f}), R={r}")
    assert float(rel.max()) <= 1e-3, f"{path}: rstd rel err {float(rel.max()):.3e} at channel {worst} (mean/std {float(ratio[worst])})"
