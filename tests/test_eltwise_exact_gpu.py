"""The small elementwise kernels of csrc/hn_norm.hip (hn_eltwise ops 0-4, hn_add_n, hn_add_strided2, hn_cast_f32_to_bf16_pad) held to the
float64 reference of tests/se_ref.py through the C entry points.

exact   integer-valued operands (|v| <= 128, alpha a power of two): every fp32 intermediate is exact, so the bf16 output must be the one
        rounding of the float64 value, bit for bit (ops 0, 1 and 4 with ReLU or no activation, op 2, add_n, add_strided2, the cast).
random  bf16-representable random operands: the output must be the bf16 rounding of a value within k * U * sum|terms| of float64, k the
        number of fp32 operations of the expression, plus slack_fwd's term for the __expf activations (the interval check).

Shapes: C from 8 to 2048, M in {1, 7, 1031}, ld = C and C + 8, and for every kernel one case whose piece count passes the grid cap (8192
workgroups x 256 threads) by a ragged amount, so the second trip of the grid-stride loop and its tail both run.  Every output lives between
sentinel guard bands; the HN_CHECK_ARG refusals must return the error code and leave a sentinel-filled output untouched."""
import pytest
import torch

from tests import bn_ref as B
from tests import exact_checks as X
from tests import se_ref as R
from tests.exact_checks import BF16, F32, F64, U, D, gen, gpu_bf16, exact, bf_interval, slack_fwd
from tests.guards import Guarded, SENT16

pytestmark = pytest.mark.gpu

HN_ERR_ARG = 1
GRID_CAP = 8192 * 256               # pieces one trip of the grid-stride loop covers at the capped grid


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


def status(K, name, *args):
    """the entry point's return code (lib().call would raise on a refusal)"""
    return K.lib().raw(name)(*args, torch.cuda.current_stream().cuda_stream)


def ints(shape, g, lim=128):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(F64)


def rand_bf(shape, g, scale=2.0):
    return (torch.randn(shape, generator=g, dtype=F64) * scale).to(BF16).double()


def rounded_once(got, want, name, what="row"):
    """the exact regime: the bf16 output equals the float64 value rounded once"""
    exact(got, R.bf16_round(want), name, what)


def untouched(o, name):
    torch.cuda.synchronize()
    assert bool((o.buf.view(torch.int16) == SENT16).all()), f"{name}: a refused call wrote its output"


def past_cap(pieces):
    return GRID_CAP < pieces < 2 * GRID_CAP and pieces % 256 != 0


def first_diff(got, want, name, c8):
    """bf16 [M, C] tensors, bit for bit (the large cases: no float64 copies); names row, channel and piece of the first mismatch"""
    bad = got.cpu() != want
    if bool(bad.any()):
        r, ch = bad.nonzero()[0].tolist()
        pytest.fail(f"{name}: {int(bad.sum())} of {bad.numel()} values differ, first at row {r}, channel {ch} (piece {r * c8 + ch // 8}): "
                    f"got {float(got[r, ch])} want {float(want[r, ch])}")


# =====================================================================================================================================
# hn_eltwise
# =====================================================================================================================================
OP_ACTS = [(0, 0), (1, B.ACT_RELU), (1, B.ACT_ELU), (2, 0)] + [(3, a) for a in B.ACTS] + [(4, a) for a in B.ACTS]
EW_SHAPES = [(1, 8, 8), (7, 24, 32), (1031, 152, 160), (7, 2048, 2048), (1031, 8, 16), (1, 2048, 2056), (7, 152, 152), (1031, 24, 24)]   # M, C, ld
EXACT_ACTS = (B.ACT_NONE, B.ACT_RELU)


def ew_slack(op, a, b, act, alpha, want):
    """k * U * sum|terms| for the k fp32 operations of the expression (+ the __expf term of the transcendental activations)"""
    if op == 0:
        return U * (a.abs() + b.abs())
    if op == 1:                                                           # ELU: a sum and a product
        return 2 * U * a.abs() * (b.abs() + 1) if act == B.ACT_ELU else torch.zeros_like(a)
    if op == 2:
        return U * (alpha * a).abs()
    if op == 3:
        return slack_fwd(a, want, a.abs() if act > 1 else torch.zeros_like(a), act)
    if act in EXACT_ACTS:                                                 # op 4: a product by 0 or 1
        return torch.zeros_like(a)
    return a.abs() * 16 * U * (2 + b.abs())                               # a * act'(b): the derivative's __expf and its handful of operations


@pytest.mark.parametrize("shape", EW_SHAPES, ids=[f"m{m}_c{c}_ld{ld}" for m, c, ld in EW_SHAPES])
@pytest.mark.parametrize("op,act", OP_ACTS, ids=[f"op{o}_act{a}" for o, a in OP_ACTS])
def test_eltwise(K, op, act, shape):
    m, c, ldx = shape
    binary = op in (0, 1, 4)
    alpha = 0.25 if op == 2 else 1.0
    regimes = ("exact", "random") if (op == 2 or act in EXACT_ACTS) else ("random",)
    for regime in regimes:
        g = gen(f"ew{op}{act}{shape}{regime}")
        a = ints((m, c), g) if regime == "exact" else rand_bf((m, c), g)
        b = (ints((m, c), g) if regime == "exact" else rand_bf((m, c), g)) if binary else None
        if op == 1 and act == B.ACT_ELU:
            b = b.clamp(min=-1.0)                                         # a post-activation of ELU
        ag = gpu_bf16(a, ldx + 8)
        bgp = gpu_bf16(b, ldx) if binary else None
        out = Guarded(m, c, ldx, BF16)
        name = f"hn_eltwise op {op} act {act} M={m} C={c} ld={ldx} {regime}"
        call(K, "hn_eltwise", op, ag.data_ptr(), ag.stride(0), bgp.data_ptr() if binary else None, bgp.stride(0) if binary else 0, out.ptr(),
             ldx, m, c, act, alpha)
        torch.cuda.synchronize()
        want = R.eltwise(op, a, b, act, alpha)
        if regime == "exact":
            rounded_once(out.view, want, name)
        else:
            bf_interval(out.view, want, ew_slack(op, a, b, act, alpha, want), name)
        out.check(name)


def test_eltwise_grid_cap(K):
    m, c = 110400, 152
    assert past_cap(m * (c // 8))
    g = gen("ewcap")
    a = torch.randint(-128, 129, (m, c), generator=g, dtype=torch.int16)
    b = torch.randint(-128, 129, (m, c), generator=g, dtype=torch.int16)
    ag, bgp = D(a.to(BF16)), D(b.to(BF16))
    out = Guarded(m, c, c + 8, BF16)
    call(K, "hn_eltwise", 0, ag.data_ptr(), c, bgp.data_ptr(), c, out.ptr(), c + 8, m, c, 0, 1.0)
    torch.cuda.synchronize()
    first_diff(out.view, (a + b).to(BF16), "hn_eltwise op 0 past the grid cap", c // 8)       # |a + b| <= 256: exact in bf16
    out.check("hn_eltwise past the grid cap")


def test_eltwise_refusals(K):
    m, c = 7, 24
    x = D(torch.ones(m, c + 8, dtype=BF16))
    out = Guarded(m, c, c + 8, BF16)
    p, ldx = x.data_ptr(), c + 8
    bad = {
        "lda not a multiple of 8": (0, p, c + 4, p, ldx, out.ptr(), ldx, m, c, 0, 1.0),
        "ldo not a multiple of 8": (0, p, ldx, p, ldx, out.ptr(), c + 4, m, c, 0, 1.0),
        "ldb not a multiple of 8": (0, p, ldx, p, c + 4, out.ptr(), ldx, m, c, 0, 1.0),
        "op 5": (5, p, ldx, p, ldx, out.ptr(), ldx, m, c, 0, 1.0),
        "op -1": (-1, p, ldx, p, ldx, out.ptr(), ldx, m, c, 0, 1.0),
        "op 0 without b": (0, p, ldx, None, 0, out.ptr(), ldx, m, c, 0, 1.0),
        "op 1 without b": (1, p, ldx, None, 0, out.ptr(), ldx, m, c, 1, 1.0),
        "op 4 without b": (4, p, ldx, None, 0, out.ptr(), ldx, m, c, 2, 1.0),
        "a null": (2, None, ldx, None, 0, out.ptr(), ldx, m, c, 0, 1.0),
        "C = 20": (2, p, ldx, None, 0, out.ptr(), ldx, m, 20, 0, 1.0),
        "M = 0": (2, p, ldx, None, 0, out.ptr(), ldx, 0, c, 0, 1.0),
    }
    for why, args in bad.items():
        assert status(K, "hn_eltwise", *args) == HN_ERR_ARG, f"hn_eltwise accepted {why}"
        untouched(out, f"hn_eltwise ({why})")
    assert status(K, "hn_eltwise", 2, p, ldx, None, 0, out.ptr(), ldx, m, c, 0, 2.0) == 0      # (the same call, well formed, runs)
    torch.cuda.synchronize()
    assert bool((out.view == 2.0).all())
    out.check("hn_eltwise op 2")


# =====================================================================================================================================
# hn_add_n: out += b0 [+ b1] [+ b2], one rounding
# =====================================================================================================================================
@pytest.mark.parametrize("shape", EW_SHAPES[:6], ids=[f"m{m}_c{c}_ld{ld}" for m, c, ld in EW_SHAPES[:6]])
@pytest.mark.parametrize("addends", [1, 2, 3])
@pytest.mark.parametrize("regime", ["exact", "random"])
def test_add_n(K, regime, addends, shape):
    m, c, ldx = shape
    g = gen(f"addn{regime}{addends}{shape}")
    mk = (lambda: ints((m, c), g)) if regime == "exact" else (lambda: rand_bf((m, c), g))
    o0 = mk()
    bs = [mk() for _ in range(addends)]
    out = Guarded(m, c, ldx, BF16)
    out.view.copy_(o0.to(BF16))
    bg = [gpu_bf16(b, ldx + 8 * i) for i, b in enumerate(bs)] + [None, None]
    ptr_ld = []
    for t in bg[:3]:
        ptr_ld += [t.data_ptr() if t is not None else None, t.stride(0) if t is not None else 0]
    name = f"hn_add_n {addends} addends M={m} C={c} ld={ldx} {regime}"
    call(K, "hn_add_n", out.ptr(), ldx, *ptr_ld, m, c)
    torch.cuda.synchronize()
    want = R.add_n(o0, *bs)
    if regime == "exact":
        rounded_once(out.view, want, name)                                # the fp32 sum of up to four integers is exact
    else:
        bf_interval(out.view, want, addends * U * (o0.abs() + sum(b.abs() for b in bs)), name)
    out.check(name)


def test_add_n_grid_cap(K):
    m, c = 110400, 152
    assert past_cap(m * (c // 8))
    g = gen("addncap")
    ts = [torch.randint(-128, 129, (m, c), generator=g, dtype=torch.int16) for _ in range(4)]
    out = Guarded(m, c, c, BF16)
    out.view.copy_(ts[0].to(BF16))
    bg = [D(t.to(BF16)) for t in ts[1:]]
    call(K, "hn_add_n", out.ptr(), c, bg[0].data_ptr(), c, bg[1].data_ptr(), c, bg[2].data_ptr(), c, m, c)
    torch.cuda.synchronize()
    first_diff(out.view, (ts[0].int() + ts[1] + ts[2] + ts[3]).float().to(BF16), "hn_add_n past the grid cap", c // 8)
    out.check("hn_add_n past the grid cap")


def test_add_n_refusals(K):
    m, c = 7, 24
    x = D(torch.ones(m, c + 8, dtype=BF16))
    out = Guarded(m, c, c + 8, BF16)
    p, ldx = x.data_ptr(), c + 8
    bad = {
        "ldo not a multiple of 8": (out.ptr(), c + 4, p, ldx, None, 0, None, 0, m, c),
        "ld0 not a multiple of 8": (out.ptr(), ldx, p, c + 4, None, 0, None, 0, m, c),
        "ld1 not a multiple of 8": (out.ptr(), ldx, p, ldx, p, c + 4, None, 0, m, c),
        "b0 null": (out.ptr(), ldx, None, 0, None, 0, None, 0, m, c),
        "b2 without b1": (out.ptr(), ldx, p, ldx, None, 0, p, ldx, m, c),
        "C = 20": (out.ptr(), ldx, p, ldx, None, 0, None, 0, m, 20),
        "M = 0": (out.ptr(), ldx, p, ldx, None, 0, None, 0, 0, c),
    }
    for why, args in bad.items():
        assert status(K, "hn_add_n", *args) == HN_ERR_ARG, f"hn_add_n accepted {why}"
        untouched(out, f"hn_add_n ({why})")


# =====================================================================================================================================
# hn_add_strided2: dx[n, 2y, 2x, :] += dxs[n, y, x, :]
# =====================================================================================================================================
STRIDED_CASES = [(1, 3, 5, 8, 8, 16), (3, 7, 9, 24, 32, 24), (1, 1, 1, 152, 160, 160), (3, 5, 3, 2048, 2048, 2056), (3, 1, 7, 152, 152, 152)]


@pytest.mark.parametrize("n,ho,wo,c,ldx,lds", STRIDED_CASES)
@pytest.mark.parametrize("regime", ["exact", "random"])
def test_add_strided2(K, regime, n, ho, wo, c, ldx, lds):
    g = gen(f"strided{regime}{n}{ho}{wo}{c}")
    mk = (lambda s: ints(s, g)) if regime == "exact" else (lambda s: rand_bf(s, g))
    dx0, dxs = mk((n, 2 * ho, 2 * wo, c)), mk((n, ho, wo, c))
    m, ms = n * 4 * ho * wo, n * ho * wo
    dx = Guarded(m, c, ldx, BF16)
    dx.view.copy_(dx0.view(m, c).to(BF16))
    sg = gpu_bf16(dxs.view(ms, c), lds)
    name = f"hn_add_strided2 N={n} Ho={ho} Wo={wo} C={c} {regime}"
    call(K, "hn_add_strided2", dx.ptr(), ldx, sg.data_ptr(), sg.stride(0), n, ho, wo, c)
    torch.cuda.synchronize()
    want = R.add_strided2(dx0, dxs).view(m, c)
    if regime == "exact":
        rounded_once(dx.view, want, name, f"row (of {2 * wo} per image row)")
    else:
        bf_interval(dx.view, want, U * want.abs(), name)
    dx.check(name)


def test_add_strided2_grid_cap(K):
    n, ho, wo, c = 1, 837, 837, 24
    assert past_cap(n * ho * wo * (c // 8))
    g = gen("stridedcap")
    dx0 = torch.randint(-128, 129, (n, 2 * ho, 2 * wo, c), generator=g, dtype=torch.int16)
    dxs = torch.randint(-128, 129, (n, ho, wo, c), generator=g, dtype=torch.int16)
    m = n * 4 * ho * wo
    dx = Guarded(m, c, c, BF16)
    dx.view.copy_(dx0.view(m, c).to(BF16))
    sg = D(dxs.view(-1, c).to(BF16))
    call(K, "hn_add_strided2", dx.ptr(), c, sg.data_ptr(), c, n, ho, wo, c)
    torch.cuda.synchronize()
    dx0[:, ::2, ::2, :] += dxs                                            # |.| <= 256: exact in bf16
    first_diff(dx.view, dx0.view(m, c).to(BF16), "hn_add_strided2 past the grid cap", c // 8)
    dx.check("hn_add_strided2 past the grid cap")


def test_add_strided2_refusals(K):
    n, ho, wo, c = 1, 2, 2, 24
    x = D(torch.ones(n * ho * wo, c + 8, dtype=BF16))
    dx = Guarded(n * 4 * ho * wo, c, c + 8, BF16)
    p, ldx = x.data_ptr(), c + 8
    bad = {
        "ldx not a multiple of 8": (dx.ptr(), c + 4, p, ldx, n, ho, wo, c),
        "lds not a multiple of 8": (dx.ptr(), ldx, p, c + 4, n, ho, wo, c),
        "dxs null": (dx.ptr(), ldx, None, ldx, n, ho, wo, c),
        "C = 20": (dx.ptr(), ldx, p, ldx, n, ho, wo, 20),
        "N = 0": (dx.ptr(), ldx, p, ldx, 0, ho, wo, c),
        "Ho = 0": (dx.ptr(), ldx, p, ldx, n, 0, wo, c),
    }
    for why, args in bad.items():
        assert status(K, "hn_add_strided2", *args) == HN_ERR_ARG, f"hn_add_strided2 accepted {why}"
        untouched(dx, f"hn_add_strided2 ({why})")


# =====================================================================================================================================
# hn_cast_f32_to_bf16_pad: fp32 [M][C] (row stride lds) -> bf16 [M][ldo], the columns from C on zero
# =====================================================================================================================================
CAST_CASES = [(1, 3, 5, 8), (7, 19, 24, 24), (1031, 152, 160, 160), (7, 2040, 2048, 2048), (1031, 8, 16, 16), (7, 24, 40, 32)]   # M, C, lds, ldo


@pytest.mark.parametrize("m,c,lds,ldo", CAST_CASES)
@pytest.mark.parametrize("regime", ["exact", "random"])
def test_cast_pad(K, regime, m, c, lds, ldo):
    assert ldo > c and lds > c
    g = gen(f"cast{regime}{m}{c}")
    src = ints((m, c), g) if regime == "exact" else torch.randn(m, c, generator=g, dtype=F64).float().double()
    wide = torch.full((m, lds), 7.0, dtype=F32)                           # the columns behind C hold values that must not come through
    wide[:, :c] = src.float()
    sg = D(wide)
    dst = Guarded(m, ldo, ldo, BF16)
    name = f"hn_cast_f32_to_bf16_pad M={m} C={c} lds={lds} ldo={ldo} {regime}"
    call(K, "hn_cast_f32_to_bf16_pad", sg.data_ptr(), lds, dst.ptr(), ldo, m, c)
    torch.cuda.synchronize()
    want = R.cast_pad(src, ldo)
    assert bool((dst.view[:, c:] == 0).all()), f"{name}: the padding columns are not zero"
    if regime == "exact":
        exact(dst.view, want, name, "row")
    else:
        bf_interval(dst.view, want, torch.zeros_like(want), name)         # one rounding
    dst.check(name)


def test_cast_pad_grid_cap(K):
    m, c, ldo = 1031, 2040, 2056
    assert GRID_CAP < m * ldo < 2 * GRID_CAP and (m * ldo) % 256
    g = gen("castcap")
    src = ints((m, c), g)
    sg = D(src.float())
    dst = Guarded(m, ldo, ldo, BF16)
    call(K, "hn_cast_f32_to_bf16_pad", sg.data_ptr(), c, dst.ptr(), ldo, m, c)
    torch.cuda.synchronize()
    exact(dst.view, R.cast_pad(src, ldo), "hn_cast_f32_to_bf16_pad past the grid cap", "row")
    dst.check("hn_cast_f32_to_bf16_pad past the grid cap")


def test_cast_pad_refusals(K):
    m, c = 7, 24
    src = D(torch.ones(m, c, dtype=F32))
    dst = Guarded(m, c + 8, c + 8, BF16)
    bad = {
        "ldo < C": (src.data_ptr(), c, dst.ptr(), c - 8, m, c),
        "src null": (None, c, dst.ptr(), c + 8, m, c),
        "M = 0": (src.data_ptr(), c, dst.ptr(), c + 8, 0, c),
        "C = 0": (src.data_ptr(), c, dst.ptr(), c + 8, m, 0),
    }
    for why, args in bad.items():
        assert status(K, "hn_cast_f32_to_bf16_pad", *args) == HN_ERR_ARG, f"hn_cast_f32_to_bf16_pad accepted {why}"
        untouched(dst, f"hn_cast_f32_to_bf16_pad ({why})")
