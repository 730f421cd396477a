"""The squeeze-excite kernels of csrc/hn_norm.hip (excitation MLP forward / backward, the SEGate path's reductions and row scalings) and of
csrc/hn_fused.hip (hn_se_gate_apply, hn_se_bwd_reduce_fused) held to the float64 reference of tests/se_ref.py, kernel by kernel, through
the C entry points, in two regimes:

exact   operands chosen so that every fp32 sum is exact (small integers, alpha = 1/HW with HW a power of two, gate = k/4, integer hid /
        pooled): the kernel must equal float64 bit for bit whatever its summation order.  Each test first PROVES the regime on the
        reference side: for every output the float64 sum of absolute terms, in units of the operands' common quantum, stays below 2^24.
random  bf16-representable random operands: fp32 outputs within gamma_n(n + S + 8) * sum|terms| of float64 (n the contraction length, S the
        partial rows, 8 the wave / LDS reduction steps) plus the propagated error of their fp32 inputs; sigmoid gates within that bound times
        the slope 1/4 plus slack_fwd's __expf term; bf16 outputs by the interval check.

Shapes are the smallest that reach an edge: the <3>/<7> switch and the rounds of four partial rows of se_fc_parts, the 1024-wide round and
the unpaired last output, empty and two-round partitions of se_fc_cols, ragged 16x16 MFMA tiles and the K tail of se_mlp_wgrad, chunks of
8 / 16 / 24 channels (cln = 3 idles threads), workgroup counts of 1 and of no multiple of 8 under xcd_remap.
Every output lives between sentinel guard bands (tests/guards.py), bf16 outputs with ld > C; a mismatch names the entry point, the image
(or partial row / row block) and the channel or output index."""
import pytest
import torch

from tests import bn_ref as B
from tests import exact_checks as X
from tests import se_ref as R
from tests.exact_checks import BF16, F32, F64, U, EXACT_LIMIT, D, gen, gpu_bf16, exact, within, bf_interval, slack_fwd
from tests.guards import BAND, Guarded, dev

pytestmark = pytest.mark.gpu

REGIMES = ("exact", "random")


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


def call(K, name, *args):
    K.lib().call(name, *args)


def f32(x):
    """the fp32 value a float argument becomes at the C boundary, as a Python float"""
    return float(torch.tensor(x, dtype=F32))


def ints(shape, lo, hi, g, density=1.0):
    """integers in [lo, hi] as float64; density < 1: that share of them kept, the rest zero"""
    v = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density)
    return v


def rand_bf(shape, g, scale=1.0):
    """bf16-representable random float64 values"""
    return (torch.randn(shape, generator=g, dtype=F64) * scale).to(BF16).double()


def fp(t):
    """float64 CPU values (fp32-representable) -> the pointer of an fp32 GPU copy kept alive until the test ends"""
    return D(t.float().contiguous()).data_ptr()


def proves_exact(name, q, **abs_sums):
    """the exact regime's condition, on the reference side: every sum of absolute terms, in units of the quantum q, below 2^24"""
    for k, v in abs_sums.items():
        worst = float(v.max()) / q
        assert worst < EXACT_LIMIT, f"{name}: {k} leaves the exact regime: sum|terms| / quantum = {worst:.0f} >= 2^24"


def sig_bound(pre2, gate, d_pre2):
    """|gate_kernel - gate_ref|: the pre-activation's bound through the slope 1/4 plus slack_fwd's term for __expf"""
    return 0.25 * d_pre2 + slack_fwd(pre2, gate, torch.zeros_like(pre2), B.ACT_SIGMOID)


# =====================================================================================================================================
# A. excitation MLP forward: hn_se_mlp_fwd_parts (S partial rows per image) and hn_se_mlp_fwd (the S-less form, S = 0 below)
# =====================================================================================================================================
FWD_CASES = [
    # C, Cs, S, N, gate
    (24, 6, 1, 1, True),            # one workgroup in both launches
    (152, 38, 2, 3, True),          # 15 workgroups: no multiple of 8
    (936, 234, 4, 5, False),        # S = 4: the last case of se_fc_parts<3>; first layer only
    (936, 234, 5, 3, True),         # S = 5: the first case of se_fc_parts<7>
    (1032, 7, 8, 3, True),          # second round of 1024; Cs = 7: an unpaired last output
    (64, 1, 9, 1, True),            # Cs = 1; S = 9: one full round of four more rows
    (152, 38, 13, 5, False),        # S = 13: a full and a ragged round of four
    (1032, 7, 13, 1, True),
    (24, 6, 0, 3, True),
    (64, 1, 0, 1, True),
    (1032, 7, 0, 5, True),
    (936, 234, 0, 3, True),
]
assert {(c, cs) for c, cs, *_ in FWD_CASES} == set(R.MLP_FWD_SHAPES)


def mlp_weights(c, cs, regime, g, r1=2, r2=1):
    if regime == "exact":
        return ints((cs, c), -r1, r1, g), ints((cs,), -3, 3, g), ints((c, cs), -r2, r2, g), ints((c,), -2, 2, g)
    return (rand_bf((cs, c), g, c ** -0.5), rand_bf((cs,), g, 0.3), rand_bf((c, cs), g, cs ** -0.5), rand_bf((c,), g, 0.3))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", FWD_CASES, ids=[f"c{c}_cs{cs}_s{s}_n{n}{'' if gt else '_nogate'}" for c, cs, s, n, gt in FWD_CASES])
def test_se_mlp_fwd(K, case, regime):
    c, cs, s, n, want_gate = case
    g = gen(f"sefwd{case}{regime}")
    rows = n * max(s, 1)
    if regime == "exact":
        alpha = 1.0 / 64
        parts = ints((rows, c), -3, 3, g) * (1.0 if s else alpha)
    else:
        alpha = f32(1.0 / 60)
        parts = rand_bf((rows, c), g, 2.0 if s else 0.5)
    w1, b1, w2, b2 = mlp_weights(c, cs, regime, g)
    entry = "hn_se_mlp_fwd_parts" if s else "hn_se_mlp_fwd"
    name = f"{entry} C={c} Cs={cs} S={s} N={n} {regime}"
    hid_o = Guarded(n, cs)
    gate_o = Guarded(n, c) if want_gate else None
    if s:
        pooled_o = Guarded(n, c)
        call(K, entry, fp(parts), s, alpha, fp(w1), fp(b1), fp(w2) if want_gate else None, fp(b2) if want_gate else None, pooled_o.ptr(),
             hid_o.ptr(), gate_o.ptr() if want_gate else None, n, c, cs)
        p = R.pooled(parts, s, alpha)
        p_abs = R.pooled(parts.abs(), s, alpha)
    else:
        pooled_o = None
        call(K, entry, fp(parts), fp(w1), fp(b1), fp(w2), fp(b2), hid_o.ptr(), gate_o.ptr(), n, c, cs)
        p, p_abs = parts, parts.abs()
    torch.cuda.synchronize()
    hid, pre2, gate = R.mlp_fwd(p, w1, b1, w2, b2)
    t1 = p_abs @ w1.abs().t() + b1.abs()                                  # sum|terms| of the first layer [N, Cs]
    if regime == "exact":
        proves_exact(name, alpha, pooled=p_abs, hid=t1)
        if s:
            exact(pooled_o.view, p, name + " pooled", "image")
        exact(hid_o.view, hid, name + " hid", "image")
        d_hid = torch.zeros_like(hid)
    else:
        if s:
            within(pooled_o.view, p, B.gamma_n(s + 1) * p_abs, name + " pooled", "image, channel")
        d_hid = B.gamma_n(c + s + 8) * t1
        within(hid_o.view, hid, d_hid, name + " hid", "image, output")
    if want_gate:
        # the second layer reads the kernel's own hid: its error is carried through |w2|
        d_pre2 = B.gamma_n(cs + 8) * ((hid.abs() + d_hid) @ w2.abs().t() + b2.abs()) + d_hid @ w2.abs().t()
        within(gate_o.view, gate, sig_bound(pre2, gate, d_pre2), name + " gate", "image, channel")
        gate_o.check(name + " gate")
    hid_o.check(name + " hid")
    if pooled_o is not None:
        pooled_o.check(name + " pooled")


# =====================================================================================================================================
# B. hn_se_gate_apply: second excitation layer + sigmoid + BatchNorm / activation / product in one launch, held to float64 directly
# =====================================================================================================================================
GATE_APPLY_CASES = [
    # C, Cs, HW, N, coef, act, gate
    (8, 1, 1, 1, False, 0, True),               # one workgroup, one row
    (24, 6, 63, 3, True, 1, True),              # one chunk of 24 channels (cln = 3: an idle thread); 3 workgroups
    (40, 6, 64 * 5, 1, True, 1, False),         # chunks of 32 + 8 channels, 5 row blocks: 10 workgroups
    (152, 234, 33 * 37, 3, True, 1, True),      # last chunk of 24 channels; RB = 111 (the divisor of HW above 64)
    (936, 300, 64 * 5, 3, False, 0, False),     # Cs = 300: a second 256-wide slab of the contraction; last chunk of 8 channels
    (24, 300, 1, 3, True, 0, True),
    (40, 234, 63, 1, False, 1, True),           # last chunk of 8
    (152, 1, 64 * 5, 1, True, 0, True),
]


@pytest.mark.parametrize("case", GATE_APPLY_CASES, ids=[f"c{c}_cs{cs}_hw{hw}_n{n}_coef{int(cf)}_act{a}_gate{int(gt)}"
                                                        for c, cs, hw, n, cf, a, gt in GATE_APPLY_CASES])
def test_se_gate_apply(K, case):
    c, cs, hw, n, has_coef, act, want_gate = case
    g = gen(f"gateapply{case}")
    m = n * hw
    z = rand_bf((m, c), g, 2.0)
    hid = rand_bf((n, cs), g).abs()
    w2, b2 = rand_bf((c, cs), g, cs ** -0.5), rand_bf((c,), g, 0.3)
    sc = (torch.rand(c, generator=g, dtype=F64) * 1.5 + 0.2).float().double()
    sc[1] = -sc[1]
    sh = (torch.randn(c, generator=g, dtype=F64) * 0.7).float().double()
    coef = torch.stack([sc, sh, torch.zeros(c, dtype=F64), torch.ones(c, dtype=F64)])
    zg = gpu_bf16(z, c + 8)
    out = Guarded(m, c, c + 8, BF16)
    gate_o = Guarded(n, c) if want_gate else None
    name = f"hn_se_gate_apply C={c} Cs={cs} HW={hw} N={n} act {act}{' coef' if has_coef else ''}"
    call(K, "hn_se_gate_apply", zg.data_ptr(), zg.stride(0), fp(coef) if has_coef else None, act, fp(hid), fp(w2), fp(b2),
         gate_o.ptr() if want_gate else None, out.ptr(), c + 8, n, hw, c, cs)
    torch.cuda.synchronize()
    pre2 = hid @ w2.t() + b2
    gate = torch.sigmoid(pre2)
    d_gate = sig_bound(pre2, gate, B.gamma_n(cs + 8) * (hid @ w2.abs().t() + b2.abs()))
    if want_gate:
        within(gate_o.view, gate, d_gate, name + " gate", "image, channel")
        gate_o.check(name + " gate")
    if has_coef:
        x = z * sc + sh
        mags = (z * sc).abs() + sh.abs()
    else:
        x, mags = z, torch.zeros_like(z)
    y = B.act_fwd(x, act)
    s = slack_fwd(x, y, mags, act) + 2 * U * y.abs()
    lo, hi = R.bf16_round(y - s), R.bf16_round(y + s)                    # the bf16 activation the kernel may hold
    assert torch.equal(R.gate_apply(z, sc if has_coef else None, sh if has_coef else None, act, gate, hw),
                       R.bf16_round(y) * gate.repeat_interleave(hw, 0))
    g_lo, g_hi = (gate - d_gate).repeat_interleave(hw, 0), (gate + d_gate).repeat_interleave(hw, 0)
    corners = torch.stack([lo * g_lo, lo * g_hi, hi * g_lo, hi * g_hi])
    w_lo, w_hi = corners.min(0).values, corners.max(0).values
    bf_interval(out.view, (w_lo + w_hi) / 2, (w_hi - w_lo) / 2, name + " out")
    out.check(name + " out")


# =====================================================================================================================================
# C. hn_se_bwd_reduce_fused: pdot = per-row-block sums of dbg * b, b = bf16(relu(sc z + sh)); bg = b * gate in bf16
# =====================================================================================================================================
SE_REDUCE_CASES = [
    # C, N, HW, RB (None: hn_fused_row_block(.., kind 1)), bg
    (24, 1, 111, 111, True),        # one workgroup; rln = 85: rows 85..110 are the second of a pair, the others have none
    (24, 1, 111, None, False),      # the policy's RB = 37: HW / RB = 3, 3 workgroups
    (152, 3, 16 * 21, 21, True),    # HW / RB = 16; chunks of 80 and 72 channels
    (936, 2, 192, 64, True),        # HW / RB = 3; rln = 17: a short last pair of rows
    (936, 2, 64 * 5, None, False),
    (152, 3, 33 * 37, None, True),
]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", SE_REDUCE_CASES, ids=[f"c{c}_n{n}_hw{hw}_rb{rb}_bg{int(b)}" for c, n, hw, rb, b in SE_REDUCE_CASES])
def test_se_bwd_reduce_fused(K, case, regime):
    c, n, hw, rb, want_bg = case
    m = n * hw
    rb = rb or K.lib().query("hn_fused_row_block", m, c, hw, 0, 1)
    assert hw % rb == 0, (hw, rb)
    g = gen(f"sered{case}{regime}")
    if regime == "exact":
        z = ints((m, c), -8, 8, g) / 4
        sc = torch.tensor([0.5, 1.0, 2.0, -1.0], dtype=F64)[torch.randint(0, 4, (c,), generator=g)]
        sh = ints((c,), -2, 2, g)
        dbg = ints((m, c), -3, 3, g)
        gate = ints((n, c), 1, 3, g) / 4
    else:
        z = rand_bf((m, c), g, 2.0)
        sc = (torch.rand(c, generator=g, dtype=F64) * 1.5 + 0.2).float().double()
        sc[1] = -sc[1]
        sh = (torch.randn(c, generator=g, dtype=F64) * 0.7).float().double()
        dbg = rand_bf((m, c), g)
        gate = (torch.rand(n, c, generator=g, dtype=F64) * 0.98 + 0.01).float().double()
    coef = torch.stack([sc, sh, torch.zeros(c, dtype=F64), torch.ones(c, dtype=F64)])
    zg, dg = gpu_bf16(z, c + 8), gpu_bf16(dbg, c + 16)
    nb = m // rb
    pdot = Guarded(nb, c)
    bg = Guarded(m, c, c + 8, BF16) if want_bg else None
    name = f"hn_se_bwd_reduce_fused C={c} N={n} HW={hw} RB={rb} {regime}"
    call(K, "hn_se_bwd_reduce_fused", dg.data_ptr(), dg.stride(0), zg.data_ptr(), zg.stride(0), fp(coef), fp(gate), hw,
         bg.ptr() if want_bg else None, c + 8 if want_bg else 0, pdot.ptr(), m, c, rb)
    torch.cuda.synchronize()
    x = z * sc + sh
    y = x.clamp(min=0.0)
    gr = gate.repeat_interleave(hw, 0)
    blk = lambda t: t.view(nb, rb, c).sum(1)
    what = f"row block (RB={rb}, {hw // rb} per image)"
    if regime == "exact":
        assert torch.equal(R.bf16_round(y), y)                            # multiples of 1/8 below 32: b is exact
        proves_exact(name, 1.0 / 8, pdot=blk((dbg * y).abs()))
        exact(pdot.view, R.dgate_parts(dbg, y, rb, hw), name + " pdot", what)
        if want_bg:
            exact(bg.view, R.bf16_round(y * gr), name + " bg (the exact product, rounded once)", "row")
    else:
        s = slack_fwd(x, y, (z * sc).abs() + sh.abs(), B.ACT_RELU) + 2 * U * y.abs()
        lo, hi = R.bf16_round(y - s), R.bf16_round(y + s)                # the bf16 activation the kernel may hold
        bound = B.gamma_n(rb + 8) * blk(dbg.abs() * hi) + blk(dbg.abs() * (hi - lo)) + 1e-30
        within(pdot.view, R.dgate_parts(dbg, R.bf16_round(y), rb, hw), bound, name + " pdot", what + ", channel")
        if want_bg:
            bf_interval(bg.view, (lo + hi) / 2 * gr, (hi - lo) / 2 * gr, name + " bg", rb)
    pdot.check(name + " pdot")
    if want_bg:
        bg.check(name + " bg")


# =====================================================================================================================================
# D. the SEGate path: hn_col_dot (mode 1 of colred_kernel), hn_rows_reduce, hn_scale_rows, hn_se_bwd_apply
# =====================================================================================================================================
SEGATE_CASES = [
    # C, ld, HW, N
    (8, 16, 1, 1),                  # one row, one workgroup
    (24, 32, 60, 3),                # R = 6: 30 workgroups
    (152, 160, 1221, 3),
    (2048, 2056, 60, 1),            # C8 = 256: one row per pass
    (8, 16, 1221, 3),
    (24, 32, 1, 3),
]
SEGATE_IDS = [f"c{c}_ld{ld}_hw{hw}_n{n}" for c, ld, hw, n in SEGATE_CASES]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", SEGATE_CASES, ids=SEGATE_IDS)
def test_col_dot(K, case, regime):
    c, ldx, hw, n = case
    m = n * hw
    r = K.lib().query("hn_colred_rows", m, hw)
    assert hw % r == 0, (hw, r)
    g = gen(f"coldot{case}{regime}")
    if regime == "exact":
        a, b = ints((m, c), -4, 4, g), ints((m, c), 0, 31, g) / 8         # integer dout, a bf16 activation
    else:
        a, b = rand_bf((m, c), g), rand_bf((m, c), g, 2.0).clamp(min=0.0)
    ag, bgp = gpu_bf16(a, ldx), gpu_bf16(b, ldx + 8)
    pr = m // r
    pd, ps = Guarded(pr, c), Guarded(pr, c)
    name = f"hn_col_dot C={c} HW={hw} N={n} R={r} {regime}"
    call(K, "hn_col_dot", ag.data_ptr(), ag.stride(0), bgp.data_ptr(), bgp.stride(0), m, c, r, pd.ptr(), ps.ptr())
    torch.cuda.synchronize()
    blk = lambda t: t.view(pr, r, c).sum(1)
    what = f"row block (R={r}, {hw // r} per image)"
    if regime == "exact":
        proves_exact(name, 1.0 / 8, pdot=blk((a * b).abs()), psum=blk(a.abs()))
        exact(pd.view, R.dgate_parts(a, b, r, hw), name + " pdot", what)
        exact(ps.view, blk(a), name + " psum", what)
    else:
        within(pd.view, R.dgate_parts(a, b, r, hw), B.gamma_n(r + 8) * blk((a * b).abs()) + 1e-30, name + " pdot", what + ", channel")
        within(ps.view, blk(a), B.gamma_n(r + 8) * blk(a.abs()) + 1e-30, name + " psum", what + ", channel")
    pd.check(name + " pdot")
    ps.check(name + " psum")


ROWS_REDUCE_CASES = [(1, 8, 1.0, 3), (15, 33, 1.0 / 64, 2), (16, 152, 1.0, 3), (17, 33, 1.0, 1), (40, 8, 1.0 / 64, 3), (17, 152, 1.0 / 64, 2)]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("s,c,alpha,groups", ROWS_REDUCE_CASES)
def test_rows_reduce(K, s, c, alpha, groups, regime):
    g = gen(f"rowsred{s}{c}{alpha}{groups}{regime}")
    src = ints((groups * s, c), -1000, 1000, g) if regime == "exact" else rand_bf((groups * s, c), g, 3.0)
    out = Guarded(groups, c)
    name = f"hn_rows_reduce S={s} C={c} alpha={alpha} G={groups} {regime}"
    call(K, "hn_rows_reduce", fp(src), out.ptr(), groups, s, c, alpha)
    torch.cuda.synchronize()
    want = R.pooled(src, s, alpha)
    if regime == "exact":
        proves_exact(name, 1.0, out=R.pooled(src.abs(), s, 1.0))
        exact(out.view, want, name, "group")
    else:
        within(out.view, want, B.gamma_n(s + 8) * R.pooled(src.abs(), s, alpha) + 1e-30, name, "group, channel")
    out.check(name)


@pytest.mark.parametrize("case", SEGATE_CASES, ids=SEGATE_IDS)
def test_scale_rows_and_se_bwd_apply(K, case):
    c, ldx, hw, n = case
    m = n * hw
    g = gen(f"scalerows{case}")
    x = rand_bf((m, c), g, 2.0)
    gate = (torch.rand(n, c, generator=g, dtype=F64) * 0.98 + 0.01).float().double()
    dpool = rand_bf((n, c), g, 4.0)
    xg = gpu_bf16(x, ldx)
    out, db = Guarded(m, c, ldx, BF16), Guarded(m, c, ldx + 8, BF16)
    call(K, "hn_scale_rows", xg.data_ptr(), xg.stride(0), fp(gate), hw, out.ptr(), ldx, m, c)
    call(K, "hn_se_bwd_apply", xg.data_ptr(), xg.stride(0), fp(gate), fp(dpool), hw, db.ptr(), ldx + 8, m, c)
    torch.cuda.synchronize()
    gr = gate.repeat_interleave(hw, 0)
    name = f"C={c} HW={hw} N={n}"
    # one fp32 product, rounded once to bf16 (bf_interval's own term covers the fp32 rounding)
    bf_interval(out.view, x * gr, torch.zeros_like(x), f"hn_scale_rows {name}", hw)
    # dout * gate + dpool * fl(1 / HW): the reciprocal, two products and a sum, 4 fp32 operations on these terms
    pterm = (dpool / hw).repeat_interleave(hw, 0)
    bf_interval(db.view, R.data_bwd(x, gate, dpool, hw), 4 * U * ((x * gr).abs() + pterm.abs()), f"hn_se_bwd_apply {name}", hw)
    out.check(f"hn_scale_rows {name}")
    db.check(f"hn_se_bwd_apply {name}")


def test_scale_rows_grid_cap(K):
    """more pieces than the grid cap (8192 workgroups x 256 threads) by a ragged amount: the second trip of the grid-stride loop and its
    tail; gate k/4 and dpool = HW j / 8 on integer rows: both outputs are one exact value rounded once"""
    c, hw, n = 152, 64, 1725
    m = n * hw
    assert 8192 * 256 < m * (c // 8) < 2 * 8192 * 256 and (m * (c // 8)) % 256
    g = gen("scalerowscap")
    xi = torch.randint(-64, 65, (m, c), generator=g, dtype=torch.int16)
    gk = torch.randint(1, 4, (n, c), generator=g, dtype=torch.int16)
    pj = torch.randint(-4, 5, (n, c), generator=g, dtype=torch.int16)
    xg = xi.to(BF16).to(dev())
    out, db = Guarded(m, c, c, BF16), Guarded(m, c, c + 8, BF16)
    call(K, "hn_scale_rows", xg.data_ptr(), c, fp(gk.double() / 4), hw, out.ptr(), c, m, c)
    call(K, "hn_se_bwd_apply", xg.data_ptr(), c, fp(gk.double() / 4), fp(pj.double() * hw / 8), hw, db.ptr(), c + 8, m, c)
    torch.cuda.synchronize()
    prod8 = xi.int() * 2 * gk.int().repeat_interleave(hw, 0)              # x * gate in eighths: |.| <= 384
    for nm, o, w8 in (("hn_scale_rows", out, prod8), ("hn_se_bwd_apply", db, prod8 + pj.int().repeat_interleave(hw, 0))):
        want = (w8.float() / 8).to(BF16)
        bad = (o.view.cpu() != want)
        if bool(bad.any()):
            r, ch = bad.nonzero()[0].tolist()
            pytest.fail(f"{nm} past the grid cap: {int(bad.sum())} values differ, first at row {r} (image {r // hw}, piece {r * (c // 8) + ch // 8}), "
                        f"channel {ch}: got {float(o.view[r, ch])} want {float(want[r, ch])}")
        o.check(nm + " past the grid cap")


# =====================================================================================================================================
# E. excitation MLP backward: hn_se_mlp_bwd (S = 0 below) and hn_se_mlp_bwd_parts; the parameter gradients in the launch (all four
#    pointers) and deferred (all null) through hn_grad_tail kind 2 (ops.GradQueue.add_outer): the same bits
# =====================================================================================================================================
BWD_CASES = [
    # C, Cs, S, N
    (16, 4, 2, 1),                  # one workgroup in every launch, the second (16 outputs x 16 partitions) included
    (24, 6, 0, 1),                  # C = 24: empty partitions among the 64
    (40, 10, 1, 2),
    (152, 38, 3, 3),                # 3 x 3 workgroups in the first launch; N = 3: a K tail of the MFMA
    (936, 234, 4, 4),               # S = 4: the first 1 + 3 rows, no round behind them
    (1032, 17, 5, 5),               # S = 5: one ragged round (one row of two); 1032 / 64 > 16: a partition's second round; Cs = 17: a tile of one output
    (24, 300, 6, 16),               # S = 6: one full round of two; Cs = 300: second round of the second launch's partitions, a ragged tile
    (152, 38, 15, 17),              # S = 15: five rounds of two and a ragged last one; N = 17: K tail of one image
    (936, 234, 16, 3),              # S = 16: six full rounds of two
    (40, 10, 16, 1),
    (1032, 17, 0, 4),
]
assert {(c, cs) for c, cs, *_ in BWD_CASES} == set(R.MLP_BWD_SHAPES)
LADDER = [(3, 1.0), (2, 0.5), (1, 0.25), (1, 0.1), (1, 0.04), (1, 0.015)]      # weight range and density, tried in turn until the regime is exact


def bwd_abs_sums(parts, s, gate, hid, pooled, w1, w2):
    """sum|terms| of every output of the backward pass (each level from the level before's sum of absolute terms)"""
    n = gate.shape[0]
    dg = parts.abs().view(n, max(s, 1), -1).sum(1)
    dpre2 = dg * gate * (1 - gate)
    dpre1 = torch.where(hid > 0, dpre2 @ w2.abs(), torch.zeros_like(hid))
    return {"dgate": dg, "dpre2": dpre2, "dpre1": dpre1, "dpool": dpre1 @ w1.abs(), "dw1": dpre1.t() @ pooled.abs(), "db1": dpre1.sum(0),
            "dw2": dpre2.t() @ hid.abs(), "db2": dpre2.sum(0)}


def bwd_operands(case, regime):
    c, cs, s, n = case
    rows = n * max(s, 1)
    if regime == "random":
        g = gen(f"sebwd{case}random")
        gate = (torch.rand(n, c, generator=g, dtype=F64) * 0.98 + 0.01).float().double()
        hid = rand_bf((n, cs), g).clamp(min=0.0)
        return (rand_bf((rows, c), g), gate, hid, rand_bf((n, c), g), rand_bf((cs, c), g, c ** -0.5), rand_bf((c, cs), g, cs ** -0.5))
    for rng, density in LADDER:
        g = gen(f"sebwd{case}exact{rng}{density}")
        parts = ints((rows, c), -3, 3, g)
        gate = ints((n, c), 1, 3, g) / 4                                  # g (1 - g) is 3/16 or 4/16
        hid = ints((n, cs), -2, 3, g).clamp(min=0.0)                      # integers, half of them zero (the ReLU mask)
        pooled = ints((n, c), -4, 4, g)
        ops = (parts, gate, hid, pooled, ints((cs, c), -rng, rng, g, density), ints((c, cs), -rng, rng, g, density))
        a = bwd_abs_sums(parts, s, gate, hid, pooled, ops[4], ops[5])
        if all(float(v.max()) * 16 < EXACT_LIMIT for v in a.values()):
            break
    return ops                                                            # (the test asserts the regime: no rung is taken on trust)


class _Param:
    """stands for a parameter in ops.GradQueue: its gradient goes to the slot of a guarded buffer"""

    def __init__(self, shape, guarded):
        self.shape, self.grad = shape, None
        self._hn_grad_slot = (guarded.buf, BAND)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", BWD_CASES, ids=[f"c{c}_cs{cs}_s{s}_n{n}" for c, cs, s, n in BWD_CASES])
def test_se_mlp_bwd(K, case, regime):
    c, cs, s, n = case
    parts, gate, hid, pooled, w1, w2 = bwd_operands(case, regime)
    entry = "hn_se_mlp_bwd_parts" if s else "hn_se_mlp_bwd"
    name = f"{entry} C={c} Cs={cs} S={s} N={n} {regime}"
    ins = [fp(t) for t in (parts, gate, hid, pooled, w1, w2)]
    args = lambda o: ([ins[0]] + ([s] if s else []) + ins[1:] + [o[k].ptr() if o[k] is not None else None
                                                                  for k in ("dpre2", "dpre1", "dpool", "dw1", "db1", "dw2", "db2")] + [n, c, cs])
    full = {"dpre2": Guarded(n, c), "dpre1": Guarded(n, cs), "dpool": Guarded(n, c), "dw1": Guarded(cs, c), "db1": Guarded(1, cs),
            "dw2": Guarded(c, cs), "db2": Guarded(1, c)}
    call(K, entry, *args(full))
    # the deferred form: no parameter gradient pointers, the two outer products through hn_grad_tail kind 2
    lean = {"dpre2": Guarded(n, c), "dpre1": Guarded(n, cs), "dpool": Guarded(n, c), "dw1": None, "db1": None, "dw2": None, "db2": None}
    call(K, entry, *args(lean))
    tail = {"dw1": Guarded(cs, c), "db1": Guarded(1, cs), "dw2": Guarded(c, cs), "db2": Guarded(1, c)}
    q = K.GradQueue()
    pw2, pb2 = _Param((c, cs, 1, 1), tail["dw2"]), _Param((c,), tail["db2"])
    pw1, pb1 = _Param((cs, c, 1, 1), tail["dw1"]), _Param((cs,), tail["db1"])
    q.weights = (pw2, pb2, pw1, pb1)
    q.add_outer(pw2, pb2, lean["dpre2"].view, D(hid.float()))
    q.add_outer(pw1, pb1, lean["dpre1"].view, D(pooled.float()))
    grads = q.flush()
    torch.cuda.synchronize()
    for gr, k in zip(grads, ("dw2", "db2", "dw1", "db1")):
        assert gr is not None and gr.data_ptr() == tail[k].ptr(), f"{name}: GradQueue did not write {k} to its slot"

    ref = R.mlp_bwd(parts, gate, hid, pooled, w1, w2, S=s)
    a = bwd_abs_sums(parts, s, gate, hid, pooled, w1, w2)
    what = {"dpre2": "image", "dpre1": "image", "dpool": "image", "dw1": "output (row of w1)", "db1": "row", "dw2": "channel (row of w2)",
            "db2": "row"}
    as2d = lambda t: t if t.dim() == 2 else t[None]
    if regime == "exact":
        proves_exact(name, 1.0 / 16, **a)
        for k, o in full.items():
            exact(o.view, as2d(ref[k]), f"{name} {k}", what[k])
        for k, o in tail.items():
            exact(o.view, as2d(ref[k]), f"hn_grad_tail kind 2 {k} ({name})", what[k])
    else:
        # a level's bound: gamma_n(contraction + S + 8) * sum|terms|, plus the bound of the fp32 input it reads, carried through
        d = {"dpre2": B.gamma_n(s + 3) * a["dpre2"]}
        d["dpre1"] = B.gamma_n(c + s + 8) * a["dpre1"]
        d["dpool"] = B.gamma_n(cs + 8) * a["dpool"] + d["dpre1"] @ w1.abs()
        d["dw2"] = B.gamma_n(n + 8) * a["dw2"] + d["dpre2"].t() @ hid.abs()
        d["db2"] = B.gamma_n(n + 8) * a["db2"] + d["dpre2"].sum(0)
        d["dw1"] = B.gamma_n(n + 8) * a["dw1"] + d["dpre1"].t() @ pooled.abs()
        d["db1"] = B.gamma_n(n + 8) * a["db1"] + d["dpre1"].sum(0)
        for k, o in full.items():
            within(o.view, as2d(ref[k]), as2d(d[k]) + 1e-30, f"{name} {k}", what[k] + ", index")
    for k, o in lean.items():
        if o is not None:
            assert torch.equal(o.view, full[k].view), f"{name}: {k} differs between the forms with and without parameter gradient pointers"
            o.check(f"{name} {k} (no parameter gradients)")
    for k, o in tail.items():
        bad = o.view != full[k].view
        if bool(bad.any()):
            i, j = bad.nonzero()[0].tolist()
            pytest.fail(f"hn_grad_tail kind 2 {k} ({name}): {int(bad.sum())} values differ from the launch's own, first at [{i}][{j}]: "
                        f"got {float(o.view[i, j])!r} want {float(full[k].view[i, j])!r}")
        o.check(f"hn_grad_tail kind 2 {k} ({name})")
    for k, o in full.items():
        o.check(f"{name} {k}")
