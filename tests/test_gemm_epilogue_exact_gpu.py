"""The epilogue and operand options of gemm_nt_kernel (csrc/hn_gemm.hip) held to EXACT references, option by option: per-image weights
(hn_scale_weight_gate + hn_conv_gemm_nt_imgw), per-level coefficients (hn_conv_gemm_nt_lvl), the level-mapped output
(hn_conv_gemm_nt_lvlout), the rpi / img_stride output mapping, the three addend modes of hn_conv_gemm_nt_ex and the statistics
epilogues emode 1, 2 (hn_conv_gemm_nt_stat, GEMM and grouped direct kernel) and 3 (hn_conv_gemm_nt_stat3), on both tilings
(nt<*,128> and nt<64,64>, asserted per case through tests/gemm_plans.py).

The method of tests/test_gemm_exact_gpu.py: integer operands and weights, every fp32 accumulation exact below 2^24 (budget()); an fp32
output equals the float64 reference bit for bit, a bf16 output equals it rounded once.  Coefficients keep the products exact: level and
BatchNorm scales are signed powers of two, shifts / means / biases integers, rs a power of two, gates from {0, 0.5, 1, 2}.  Where the
header documents two roundings (the post-rounding addend: out = bf16(bf16(acc) + addend); emode 3 sums that FINAL value) the reference
restates them in order with float64 in between.  Swish alone is held to the two bf16 neighbours of the float64 value: the sigmoid of an
integer is not exactly determinable (the interval rule of test_batchnorm_exact_gpu.py::test_bn_act_interval).  Outputs lie between
guard bands (for the mapped outputs: every element the mapping does not name, alignment and inter-image gaps included, must keep its
sentinel), and a mismatch names image, level, pixel tile or statistics row."""
import ctypes

import pytest
import torch

from tests import gemm_plans as P
from tests import seg_conv_ref as R
from tests.guards import BAND, SENT16, SENT32, Guarded, dev
from tests.test_gemm_exact_gpu import BF16, F32, F64, RAND_TOL, _w_int, budget, exact, gen, ints, nt_ref, randn, seed_of, taps_of

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_RELU, ACT_SWISH = 0, 1, 2
HN_ERR_ARG, HN_ERR_UNSUPPORTED = 1, 3


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops
    return ops


def rc_of(K, name, *args):
    return K.lib().raw(name)(*args, torch.cuda.current_stream().cuda_stream)


def pack1x1(K, w2):
    """integer [Nout, C] -> packed forward operand [Nout][KP]"""
    return K.pack_conv_weight(w2.view(w2.shape[0], w2.shape[1], 1, 1).contiguous())[0]


def pow2(shape, g, exps=(-1, 0, 1, 2), signed=True):
    e = torch.tensor(exps, device=dev(), dtype=F32)[torch.randint(0, len(exps), shape, generator=g, device=dev())]
    s = (torch.randint(0, 2, shape, generator=g, device=dev()).float() * 2 - 1) if signed else 1.0
    return torch.exp2(e) * s


def intf(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g, device=dev()).float()


def tile_rows(kern):
    return 64 if kern.startswith("nt<64,64") else 128


class Flat:
    """a sentinel-filled flat output that a kernel addresses through a row mapping: check() holds the mapped elements to the reference and
    every other element (row-stride gaps, alignment gaps, inter-image gaps, the bands) to its sentinel"""

    def __init__(self, numel, dtype):
        self.dtype, self.numel = dtype, numel
        self.idt, self.sent = (torch.int32, SENT32) if dtype == F32 else (torch.int16, SENT16)
        self.buf = torch.full((2 * BAND + numel,), self.sent, dtype=self.idt, device=dev()).view(dtype)

    def ptr(self):
        return self.buf[BAND:].data_ptr()

    def check(self, offs, ncols, want, name, why=None, locate=None):
        """offs [M]: element offset of every GEMM row (-1: a row that must not be stored); want [M, ncols]; locate(element offset) names
        the place of a stray store"""
        real = offs >= 0
        idx = offs[real][:, None] + torch.arange(ncols, device=dev())[None, :] + BAND
        assert int(idx.max()) < BAND + self.numel
        rows = real.nonzero()[:, 0]
        exact(self.buf[idx], want[real], name, (lambda ii: why([(int(rows[i[0]]), i[1]) for i in ii])) if why else None)
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=dev())
        keep[idx.reshape(-1)] = False
        bad = (self.buf.view(self.idt) != self.sent) & keep
        if int(bad.sum()):
            first = [int(i) - BAND for i in bad.nonzero()[:6, 0]]
            pytest.fail(f"{name}: {int(bad.sum())} elements outside the mapping were written (first at element offsets {first}): gap, alignment-row "
                        f"or guard-band stores" + (f"\n  first: {locate(first[0])}" if locate else ""))


def bf16_step(r, d):
    """the next bf16 value above (d = +1) / below (d = -1) r"""
    b = r.view(torch.int16).int() & 0xFFFF
    key = torch.where(b < 0x8000, b, -(b & 0x7FFF)) + d
    nb = torch.where(key >= 0, key, (-key) | 0x8000)
    return torch.where(nb >= 0x8000, nb - 0x10000, nb).to(torch.int16).view(BF16)


def bf16_neighbours(got, y, name):
    """got (bf16) is one of the two bf16 values that bracket the float64 value y (y itself when it is representable)"""
    r = y.to(BF16)
    rd = r.double()
    lo = torch.where(rd <= y, rd, bf16_step(r, -1).double())
    hi = torch.where(rd >= y, rd, bf16_step(r, +1).double())
    g = got.double()
    bad = ~((g >= lo) & (g <= hi))
    if int(bad.sum()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        pytest.fail(f"{name}: {int(bad.sum())} bf16 outputs are not a bf16 neighbour of the float64 value; at {i}: got {float(g[i])!r}, "
                    f"allowed [{float(lo[i])!r}, {float(hi[i])!r}] (value {float(y[i])!r})")


# ---- 7. per-image weights ------------------------------------------------------------------------------------------------------------
IMGW_CASES = [  # name, rows per image, C, Cout, expected tiling   (n = 3)
    ("rpi128_c40", 128, 40, 56, "nt<64,128>"), ("rpi384_c40", 384, 40, 56, "nt<64,128>"),
    ("rpi128_c152", 128, 152, 152, "nt<64,64>"), ("rpi384_c152", 384, 152, 152, "nt<64,64>"),
    ("rpi128_c936", 128, 936, 376, "nt<64,64,kg2>"), ("rpi384_c936", 384, 936, 376, "nt<64,64,kg2>"),
]
GATES = (0.0, 0.5, 1.0, 2.0)


def scaled_weights(K, wp, gate, n, cout, c, kp):
    wn = Guarded(n * cout, kp, kp, BF16)
    K.lib().call("hn_scale_weight_gate", K.ptr(wp), K.ptr(gate), wn.ptr(), n, cout, c, kp)
    torch.cuda.synchronize()
    wn.check("hn_scale_weight_gate out")
    return wn


@pytest.mark.parametrize("case", IMGW_CASES, ids=[c[0] for c in IMGW_CASES])
def test_imgw_exact(K, case):
    name, rpi, c, cout, kern = case
    n = 3
    m, kp = n * rpi, P.kp32(c)
    assert P.nt_entry_kernel("imgw", m, cout, kp) == kern
    g = gen(seed_of(name))
    x = ints((1, 1, m, c), -2, 2, g, width=c + 8)
    w2 = _w_int(cout, c, 1, g)[:, :, 0].contiguous()
    wp = pack1x1(K, w2)
    gate = torch.tensor(GATES, device=dev())[torch.randint(0, 4, (n, c), generator=g, device=dev())].contiguous()
    assert all(not torch.equal(gate[i], gate[j]) for i in range(n) for j in range(i)), "two images share their gates"
    wn = scaled_weights(K, wp, gate, n, cout, c, kp)
    wn_ref = w2.double()[None] * gate.double()[:, None, :]                     # exact: gates are 0 or powers of two
    wv = wn.view.view(n, cout, kp)
    exact(wv[:, :, :c], wn_ref, f"{name} scaled weights", lambda ii: f"image {ii[0][0]} cout {ii[0][1]}")
    assert bool((wv[:, :, c:] == 0).all()), "the K padding of the scaled weights is not zero"
    bias = intf((cout,), -4, 4, g)
    img = R.image_of_rows(m, rpi, dev())
    xd = x.double().reshape(m, c)
    acc = torch.cat([xd[img == i] @ wn_ref[i].t() for i in range(n)])          # (per image: the mapping itself is pinned on the CPU)
    budget(float((xd.abs() @ w2.double().abs().t()).max()) * 2 + 4 + 8, name)
    add = ints((1, 1, m, cout), -8, 8, g, width=cout + 8)
    for with_add in (False, True):
        for act in (ACT_RELU, ACT_NONE):
            pre = acc + bias.double() + (add.double().reshape(m, cout) if with_add else 0)
            want = (pre.clamp(min=0) if act == ACT_RELU else pre).to(BF16)
            out = Guarded(m, cout, cout + 8, BF16)
            K.lib().call("hn_conv_gemm_nt_imgw", K.ptr(x), x.stride(2), m, c, wn.ptr(), cout * kp, rpi, cout, kp, K.ptr(bias), act, out.ptr(), cout + 8,
                         K.ptr(add) if with_add else None, add.stride(2) if with_add else 0)
            torch.cuda.synchronize()
            exact(out.view, want, f"{name} addend={with_add} act={act} ({kern})",
                  lambda ii: f"image {ii[0][0] // rpi} (its weight matrix), pixel tile {ii[0][0] // tile_rows(kern)}, cout tile {ii[0][1] // 64}")
            out.check(f"{name} out")


def test_scale_weight_gate_arbitrary_gates(K):
    """arbitrary fp32 gates: one correctly rounded multiply on both sides, bf16(fp32(w) * fp32(gate))"""
    n, cout, c = 3, 152, 152
    kp = P.kp32(c)
    g = gen(seed_of("arbitrary gates"))
    wp = K.pack_conv_weight((torch.randn(cout, c, 1, 1, generator=g, device=dev()) * 0.3).contiguous())[0]
    gate = torch.rand(n, c, generator=g, device=dev()).contiguous()
    wn = scaled_weights(K, wp, gate, n, cout, c, kp)
    want = (wp.view(cout, kp)[:, :c].float()[None] * gate[:, None, :]).to(BF16)
    wv = wn.view.view(n, cout, kp)
    exact(wv[:, :, :c], want, "scaled weights, arbitrary gates", lambda ii: f"image {ii[0][0]} cout {ii[0][1]}")
    assert bool((wv[:, :, c:] == 0).all())


# ---- 8. per-level coefficients --------------------------------------------------------------------------------------------------------------
LVL_CASES = [  # name, rows per level, Nout, expected tiling
    ("lvl5_n64", (256, 128, 128, 128, 128), 64, "nt<64,128>"), ("lvl5_n88", (256, 128, 128, 128, 128), 88, "nt<64,64>"),
    ("lvl2_n64", (1280, 128), 64, "nt<64,128>"), ("lvl2_n88", (1280, 128), 88, "nt<64,64>"),
]


@pytest.mark.parametrize("case", LVL_CASES, ids=[c[0] for c in LVL_CASES])
def test_lvl_exact(K, case):
    name, rows, nout, kern = case
    c, m, nl = 64, sum(rows), len(rows)
    assert P.nt_entry_kernel("lvl", m, nout, P.kp32(c)) == kern
    g = gen(seed_of(name))
    x = ints((1, 1, m, c), -1, 1, g, width=c + 8)
    w2 = _w_int(nout, c, 1, g)[:, :, 0].contiguous()
    wp = pack1x1(K, w2)
    bias = intf((nout,), -4, 4, g)
    coef = torch.zeros(nl, 4, nout, device=dev())
    coef[:, 0] = pow2((nl, nout), g, exps=(-2, -1, 0))
    coef[:, 1] = intf((nl, nout), -6, 6, g)
    assert all(not torch.equal(coef[i], coef[j]) for i in range(nl) for j in range(i)), "two levels share their coefficients"
    lev = R.level_of_rows(rows, dev())
    acc = x.double().reshape(m, c) @ w2.double().t() + bias.double()
    budget(float((x.double().reshape(m, c).abs() @ w2.double().abs().t()).max()) * 2 + 16, name)
    y = coef[:, 0].double()[lev] * acc + coef[:, 1].double()[lev]
    rows_c = (ctypes.c_long * nl)(*rows)
    for act in (ACT_RELU, ACT_NONE, ACT_SWISH):
        out = Guarded(m, nout, nout + 8, BF16)
        K.lib().call("hn_conv_gemm_nt_lvl", K.ptr(x), x.stride(2), m, c, K.ptr(wp), nout, P.kp32(c), K.ptr(bias), act, out.ptr(), nout + 8,
                     K.ptr(coef), nl, ctypes.addressof(rows_c))
        torch.cuda.synchronize()
        why = lambda ii: f"level {int(lev[ii[0][0]])} (its coefficients), pixel tile {ii[0][0] // tile_rows(kern)}"
        if act == ACT_SWISH:
            # y sigmoid(y) must stay a NORMAL fp32 number for the neighbour rule to hold a device that flushes subnormals: sigmoid(-80) =
            # 1.8e-35 is normal (the smallest normal fp32 is 1.2e-38 = sigmoid(-87.3)), so the case keeps |y| <= 80
            assert float(y.abs().max()) <= 80
            bf16_neighbours(out.view, y * torch.sigmoid(y), f"{name} swish ({kern})")
        else:
            exact(out.view, (y.clamp(min=0) if act == ACT_RELU else y).to(BF16), f"{name} act={act} ({kern})", why)
        out.check(f"{name} out")


# ---- 9. level-mapped output -------------------------------------------------------------------------------------------------------------------
LVLOUT_CASES = [  # name, n, level heights, level widths, row_align
    ("n2_5levels", 2, (8, 4, 2, 1, 1), (16, 8, 4, 2, 1), 128),
    ("n3_2levels_a128", 3, (7, 3), (13, 5), 128),
    ("n3_2levels_a256", 3, (7, 3), (13, 5), 256),
]


def lvlout_kernel(case, nout):
    name, n, hs, ws, align = case
    m = R.lvlout_rows(n, hs, ws, align, "cpu")[0]
    return P.nt_entry_kernel("lvlout", m, nout, 64)


@pytest.mark.parametrize("nout", [36, 81])
@pytest.mark.parametrize("case", LVLOUT_CASES, ids=[c[0] for c in LVLOUT_CASES])
def test_lvlout_exact(K, case, nout):
    name, n, hs, ws, align = case
    c = 64
    kern = lvlout_kernel(case, nout)
    assert kern == ("nt<64,128>" if nout == 36 else "nt<64,64>")
    m, lev, img, pix, real = R.lvlout_rows(n, hs, ws, align, dev())
    g = gen(seed_of(name) + nout)
    x = ints((1, 1, m, c), -2, 2, g, width=c + 8)                              # alignment rows hold integers too: they must not leak
    w2 = _w_int(nout, c, 1, g)[:, :, 0].contiguous()
    wp = pack1x1(K, w2)
    bias = intf((nout,), -4, 4, g)
    want = x.double().reshape(m, c) @ w2.double().t() + bias.double()
    budget(float((x.double().reshape(m, c).abs() @ w2.double().abs().t()).max()) + 4, name)
    tot = sum(h * w for h, w in zip(hs, ws))
    ldc = nout + 3
    img_stride = tot * ldc + 29                                               # larger than the packed image
    offs = R.lvlout_offsets(n, hs, ws, align, img_stride, ldc, dev())
    assert int(real.sum()) == n * tot and int((~real).sum()) > 0
    # the buffer also covers where the alignment rows WOULD land if the kernel stored them by the same formula ("image" index >= n): a
    # kernel that stores one writes into watched sentinels, not into somebody else's memory
    spill = max(P.cdiv(P.cdiv(n * h * w, align) * align, h * w) for h, w in zip(hs, ws))
    out = Flat(max(n, spill) * img_stride, F32)
    hc, wc = (ctypes.c_int * len(hs))(*hs), (ctypes.c_int * len(ws))(*ws)
    K.lib().call("hn_conv_gemm_nt_lvlout", K.ptr(x), x.stride(2), m, c, K.ptr(wp), nout, 64, K.ptr(bias), 0, out.ptr(), ldc, img_stride, n, len(hs),
                 ctypes.addressof(hc), ctypes.addressof(wc), align)
    torch.cuda.synchronize()
    starts = [sum(h * w for h, w in zip(hs[:l], ws[:l])) for l in range(len(hs) + 1)]

    def locate(o):
        slot, r = divmod(o, img_stride)
        px, col = divmod(r, ldc)
        lv = max((l for l in range(len(hs)) if starts[l] <= px), default=0)
        what = (f"image slot {slot} >= n = {n}: an ALIGNMENT ROW of level {lv} was stored" if 0 <= slot and slot >= n and px < tot and col < nout
                else ("the inter-image gap" if px >= tot else ("the row-stride gap" if col >= nout else "a guard band")))
        return f"image slot {slot}, concatenated pixel {px} (level {lv}), column {col}: {what}"

    out.check(offs, nout, want, f"{name} nout={nout} ({kern})",
              lambda ii: f"level {int(lev[ii[0][0]])} image {int(img[ii[0][0]])} (packed row {ii[0][0]}, pixel tile {ii[0][0] // tile_rows(kern)})", locate)


# ---- 10. rpi / img_stride ---------------------------------------------------------------------------------------------------------------------
RPI_CASES = [  # name, mode, image grid (h, w) with h * w = rpi, Nout, out_f32, expected tiling      (n = 3)
    ("1x1_rpi35_f32", 0, (5, 7), 40, True, "nt<64,128>"), ("1x1_rpi128_bf16", 0, (8, 16), 40, False, "nt<64,128>"),
    ("1x1_rpi35_bf16_n88", 0, (5, 7), 88, False, "nt<64,64>"), ("1x1_rpi128_f32_n88", 0, (8, 16), 88, True, "nt<64,64>"),
    ("3x3_rpi35_bf16", 2, (5, 7), 40, False, "nt<64,128>"), ("3x3_rpi128_f32", 2, (8, 16), 40, True, "nt<64,128>"),
    ("3x3_rpi35_f32_n88", 2, (5, 7), 88, True, "nt<64,64>"), ("3x3_rpi128_bf16_n88", 2, (8, 16), 88, False, "nt<64,64>"),
]


@pytest.mark.parametrize("case", RPI_CASES, ids=[c[0] for c in RPI_CASES])
def test_rpi_mapping_exact(K, case):
    name, mode, (h, w), nout, out_f32, kern = case
    n, c = 3, 24
    rpi, m, taps = h * w, 3 * h * w, (9 if mode == 2 else 1)
    assert P.nt_kernel(mode, m, nout, P.kp32(c), taps) == kern           # (a 3x3 call with rpi goes through the gather GEMM, not the direct kernel)
    g = gen(seed_of(name))
    x = ints((n, h, w, c), -2, 2, g, width=c + 8)
    w3 = _w_int(nout, c, taps, g)
    wp = K.pack_conv_weight(w3.view(nout, c, *((3, 3) if taps == 9 else (1, 1))).contiguous())[0]
    bias = intf((nout,), -4, 4, g)
    xs = taps_of(mode, x, None, (n, h, w))
    budget(float(sum(t.abs() @ w3[:, :, i].abs().t().double() for i, t in enumerate(xs)).max()) + 4, name)
    want = nt_ref(xs, w3.double(), bias, 1)
    ldc = nout + 8
    img_stride = rpi * ldc + (40 if not out_f32 else 13)                   # bf16: a multiple of 8 keeps the staged epilogue
    offs = R.rpi_offsets(m, rpi, img_stride, ldc, dev())
    out = Flat(n * img_stride, F32 if out_f32 else BF16)
    K.lib().call("hn_conv_gemm_nt", K.ptr(x), None, mode, n, h, w, c, 0, x.stride(2), 0, 0, m, K.ptr(wp), nout, P.kp32(c), taps, K.ptr(bias), 1,
                 out.ptr(), 1 if out_f32 else 0, ldc, rpi, img_stride, None, None)
    torch.cuda.synchronize()
    out.check(offs, nout, want if out_f32 else want.to(BF16), f"{name} ({kern})",
              lambda ii: f"image {ii[0][0] // rpi} row {ii[0][0] % rpi}, pixel tile {ii[0][0] // tile_rows(kern)}")


# ---- 11. addend modes ---------------------------------------------------------------------------------------------------------------------------
ADD_CASES = [  # name, kind (post | pre | s2), grid, Nout, expected tiling
    ("post_n56", "post", (2, 6, 10), 56, "nt<64,128>"), ("post_n152", "post", (1, 16, 24), 152, "nt<64,64>"),
    ("pre_n56", "pre", (2, 6, 10), 56, "nt<64,128>"), ("pre_n152", "pre", (1, 16, 24), 152, "nt<64,64>"),
    ("s2_n56", "s2", (2, 6, 10), 56, "nt<64,128>"), ("s2_n152", "s2", (1, 16, 24), 152, "nt<64,64>"),
    ("s2_n56_16x24", "s2", (1, 16, 24), 56, "nt<64,128>"), ("s2_n152_6x10", "s2", (2, 6, 10), 152, "nt<64,64>"),
]


def addend_ref(kind, acc_b, add, grid, act):
    """acc_b = acc + bias in float64 [M, Nout]; the header's order of roundings, float64 in between"""
    n, h, w = grid
    relu = (lambda v: v.clamp(min=0)) if act == ACT_RELU else (lambda v: v)
    if kind == "pre":
        return relu(acc_b + add.double().reshape(acc_b.shape)).to(BF16)
    first = relu(acc_b).to(BF16).double()                                     # the staged tile: bf16(act(acc + bias))
    if kind == "post":
        return (first + add.double().reshape(acc_b.shape)).to(BF16)
    full = torch.zeros(n, h, w, acc_b.shape[1], dtype=F64, device=dev())
    full[:, ::2, ::2] = add.double()                                          # the stride-2 sub-grid addend, at even (y, x) only
    hit = torch.zeros(n, h, w, 1, dtype=torch.bool, device=dev())
    hit[:, ::2, ::2] = True
    v = first.view(n, h, w, -1)
    return torch.where(hit, (v + full).to(BF16).double(), v).reshape(acc_b.shape).to(BF16)


def ex_call(K, x, grid, wp, nout, kp, bias, act, out, ldc, add, kind, psum=None, psq=None, xscale=None, xshift=None):
    n, h, w = grid
    ld_add = 0 if add is None else (-add.stride(2) if kind == "pre" else add.stride(2))
    return ("hn_conv_gemm_nt_ex", K.ptr(x), None, 0, n, h, w, x.shape[3], 0, x.stride(2), 0, 0, n * h * w, K.ptr(wp), nout, kp, 1, K.ptr(bias), act,
            out.ptr(), 0, ldc, 0, 0, psum, psq, K.ptr(xscale), K.ptr(xshift), None, 0, 0, K.ptr(add), ld_add, 1 if kind == "s2" else 0)


@pytest.mark.parametrize("case", ADD_CASES, ids=[c[0] for c in ADD_CASES])
def test_addend_modes_exact(K, case):
    name, kind, grid, nout, kern = case
    n, h, w = grid
    c, m = 40, n * h * w
    assert P.nt_kernel(0, m, nout, P.kp32(c), 1) == kern
    g = gen(seed_of(name))
    x = ints((n, h, w, c), -8, 8, g, width=c + 8)                          # accumulators well beyond +-256: the first rounding is no identity
    w2 = _w_int(nout, c, 1, g, -8, 8)[:, :, 0].contiguous()
    wp = pack1x1(K, w2)
    bias = intf((nout,), -4, 4, g)
    acc_b = x.double().reshape(m, c) @ w2.double().t() + bias.double()
    budget(float((x.double().reshape(m, c).abs() @ w2.double().abs().t()).max()) + 4 + 300, name)
    assert float(acc_b.abs().max()) > 256, "no accumulator beyond the bf16-exact integers: the first rounding would be an identity"
    ag = (n, h // 2, w // 2) if kind == "s2" else grid
    add = ints((*ag, nout), -300, 300, g, width=nout + 8)
    for act in ((ACT_RELU, ACT_NONE) if kind == "pre" else (ACT_NONE, ACT_RELU)):
        want = addend_ref(kind, acc_b, add, grid, act)
        out = Guarded(m, nout, nout + 8, BF16)
        K.lib().call(*ex_call(K, x, grid, wp, nout, P.kp32(c), bias, act, out, nout + 8, add, kind))
        torch.cuda.synchronize()
        exact(out.view, want, f"{name} act={act} ({kern})",
              lambda ii: f"pixel tile {ii[0][0] // tile_rows(kern)}, pixel (y, x) = ({ii[0][0] % (h * w) // w}, {ii[0][0] % w})"
                         + (" [even (y, x): takes the addend]" if kind == "s2" and not ((ii[0][0] % (h * w) // w) | (ii[0][0] % w)) & 1 else ""))
        out.check(f"{name} out")


def test_operand_transform_is_refused_by_the_product_library(K):
    g = gen(7)
    grid, c, nout = (1, 8, 16), 40, 56
    x = ints((*grid, c), -2, 2, g)
    wp = pack1x1(K, _w_int(nout, c, 1, g)[:, :, 0].contiguous())
    sc, sh = torch.ones(c, device=dev()), torch.zeros(c, device=dev())
    out = Guarded(128, nout, nout + 8, BF16)
    call = ex_call(K, x, grid, wp, nout, P.kp32(c), None, 0, out, nout + 8, None, "post", xscale=sc, xshift=sh)
    assert rc_of(K, *call) == HN_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    out.check("refused xscale call")
    assert bool((out.buf.view(torch.int16) == SENT16).all()), "the refused call wrote to the output"


# ---- 12. statistics epilogues emode 1 / 2 ---------------------------------------------------------------------------------------------------------
STAT_CASES = [  # name, mode, grid (output), C, Nout, addend kind (None | post | s2), expected tiling
    ("m0_n56", 0, (2, 13, 16), 40, 56, None, "nt<64,128>"), ("m0_n152", 0, (2, 13, 16), 40, 152, None, "nt<64,64>"),
    ("m0_n56_post", 0, (1, 10, 14), 40, 56, "post", "nt<64,128>"), ("m0_n152_s2", 0, (2, 6, 10), 40, 152, "s2", "nt<64,64>"),
    ("m0_n56_s2", 0, (1, 16, 24), 40, 56, "s2", "nt<64,128>"), ("m0_n152_post", 0, (1, 16, 24), 40, 152, "post", "nt<64,64>"),
    ("m1_n56", 1, (2, 9, 13), 40, 56, None, "nt<64,128>"), ("m1_n152", 1, (1, 17, 11), 40, 152, None, "nt<64,64>"),
    ("m5_c64", 5, (2, 19, 37), 64, 64, None, "direct<64,bf16>"), ("m5_c152", 5, (1, 17, 33), 152, 152, None, "direct<64,bf16>"),
]


def stat_coef(nout, g):
    return torch.stack([pow2((nout,), g), intf((nout,), -2, 2, g), intf((nout,), -2, 2, g), pow2((nout,), g, signed=False)]).contiguous()


@pytest.mark.parametrize("emode", [1, 2])
@pytest.mark.parametrize("case", STAT_CASES, ids=[c[0] for c in STAT_CASES])
def test_stat_epilogue_exact(K, case, emode):
    name, mode, grid, c, nout, kind, kern = case
    n, h, w = grid
    m = n * h * w
    g = gen(seed_of(name) + emode)
    if mode == 5:
        assert P.direct_kernel(5, nout, 64, False, nout + 8)[0] == kern
        x = ints((n, h, w, c), -1, 1, g, 0.5, width=c + 8)
        wg = _w_int(c, 8, 9, g, -1, 1)
        wp, kp, taps = K.pack_gconv_diag(wg.view(c, 8, 3, 3).contiguous())[0], 64, 9
        xs = taps_of(5, x, None, grid)
        acc = torch.stack([sum(xs[t][:, 8 * (o // 8):8 * (o // 8) + 8] @ wg[o, :, t].double() for t in range(9)) for o in range(c)], -1)
        bias = None
        prows = K.lib().query("hn_direct_stat_rows", n, h, w)
    else:
        kp, taps = P.kp32(c), 1
        assert P.nt_kernel(mode, m, nout, kp, 1) == kern
        x = ints((n, 2 * h, 2 * w, c) if mode == 1 else (n, h, w, c), -2, 2, g, width=c + 8)
        w2 = _w_int(nout, c, 1, g)
        wp = pack1x1(K, w2[:, :, 0].contiguous())
        bias = intf((nout,), -3, 3, g)
        xs = taps_of(mode, x, None, grid)
        acc = nt_ref(xs, w2.double(), bias, 0)
        prows = K.lib().query("hn_nt_stat_rows", m, nout)
        assert prows == P.cdiv(m, tile_rows(kern)) and K.lib().query("hn_nt_stat_tile", m, nout) == tile_rows(kern)
    # a statistics row sums <= 256 pixels of |q| * |bf16(relu(sc z + sh))| <= |q| * 14 or |q| * |z - mu| * rs <= |q| * 20
    budget(float(acc.abs().max()) * 20 * 256 + 1, name)
    q = acc.to(BF16).double()                                                # the statistics see bf16(acc + bias), BEFORE a post-rounding addend
    ez = ints((n, h, w, nout), -3, 3, g, width=nout + 4)
    coef = stat_coef(nout, g)
    pre = coef[0].double() * ez.double().reshape(m, nout) + coef[1].double()
    assert int((pre == 0).sum()) > 0 and int((pre > 0).sum()) > 0 and int((pre < 0).sum()) > 0, "the mask's boundary value 0 does not occur"
    t1, t2 = R.estat_terms(emode, q, ez.reshape(m, nout), coef)
    assert bool(t1[pre == 0].eq(0).all())                                    # values exactly 0 are not counted
    sums = (lambda t: R.patch_sums(t.view(n, h, w, nout))) if mode == 5 else (lambda t: R.tile_sums(t, tile_rows(kern)))
    ag = (n, h // 2, w // 2) if kind == "s2" else grid
    add = ints((*ag, nout), -300, 300, g, width=nout + 8) if kind else None
    want = addend_ref(kind, acc, add, grid, ACT_NONE) if kind else q.to(BF16)
    out = Guarded(m, nout, nout + 8, BF16)
    psum, psq = Guarded(prows, nout), Guarded(prows, nout)
    K.lib().call("hn_conv_gemm_nt_stat", K.ptr(x), None, mode, n, h, w, c, 0, x.stride(2), 0, 0, m, K.ptr(wp), nout, kp, taps, K.ptr(bias), 0, out.ptr(),
                 0, nout + 8, 0, 0, psum.ptr(), psq.ptr(), K.ptr(add), add.stride(2) if kind else 0, 1 if kind == "s2" else 0, emode, K.ptr(ez),
                 ez.stride(2), K.ptr(coef))
    torch.cuda.synchronize()
    unit = "16x16 patch" if mode == 5 else f"pixel tile of {tile_rows(kern)} rows"
    exact(out.view, want, f"{name} emode {emode} out ({kern})")
    out.check(f"{name} out")
    exact(psum.view, sums(t1), f"{name} emode {emode} psum ({kern})", lambda ii: f"statistics row {ii[0][0]} ({unit}) of {prows}, channel {ii[0][1]}")
    psum.check(f"{name} psum")
    if emode == 1:
        psq.check(f"{name} psq")
        assert bool((psq.buf.view(torch.int32) == SENT32).all()), f"{name}: emode 1 wrote psq (the header: psq is not written)"
    else:
        exact(psq.view, sums(t2), f"{name} emode 2 psq ({kern})", lambda ii: f"statistics row {ii[0][0]} ({unit}) of {prows}, channel {ii[0][1]}")
        psq.check(f"{name} psq")


# ---- 13. emode 3 -----------------------------------------------------------------------------------------------------------------------------------
STAT3_CASES = [("m2048_c152", 2048, 152, 152), ("m520_c72_ragged", 520, 72, 72)]


def stat3_call(K, x, m, c, wp, nout, out, psum, psq, add, ez, ey, coef):
    return ("hn_conv_gemm_nt_stat3", K.ptr(x), x.stride(2), m, c, K.ptr(wp), nout, P.kp32(c), out.ptr(), out.ld, psum.ptr(), psq.ptr(), K.ptr(add),
            add.stride(2), K.ptr(ez), ez.stride(2), K.ptr(ey), ey.stride(2), K.ptr(coef))


@pytest.mark.parametrize("case", STAT3_CASES, ids=[c[0] for c in STAT3_CASES])
def test_stat3_exact(K, case):
    name, m, c, nout = case
    assert P.nt_entry_kernel("stat3", m, nout, P.kp32(c)) == "nt<64,64>"
    if "ragged" in name:
        assert m % 64
    g = gen(seed_of(name))
    x = ints((1, 1, m, c), -8, 8, g, width=c + 8)
    w2 = _w_int(nout, c, 1, g, -8, 8)[:, :, 0].contiguous()
    wp = pack1x1(K, w2)
    add = ints((1, 1, m, nout), -300, 300, g, width=nout + 8)
    ez = ints((1, 1, m, nout), -3, 3, g, width=nout + 8)
    ey = ints((1, 1, m, nout), -1, 1, g, width=nout + 8)
    assert int((ey == 0).sum()) > 0
    coef = stat_coef(nout, g)
    acc = x.double().reshape(m, c) @ w2.double().t()
    budget(float((x.double().reshape(m, c).abs() @ w2.double().abs().t()).max()), name)
    assert float(acc.abs().max()) > 256
    final = (acc.to(BF16).double() + add.double().reshape(m, nout)).to(BF16)     # two roundings: the staged accumulator, then the sum
    t1, t2 = R.estat_terms(3, final, ez.reshape(m, nout), coef, ey.reshape(m, nout))
    budget(float(R.tile_sums(t2.abs(), 64).max()) + 1, name + " psq")
    prows = P.cdiv(m, 64)
    assert K.lib().query("hn_nt_stat_rows", m, nout) == prows
    out, psum, psq = Guarded(m, nout, nout + 8, BF16), Guarded(prows, nout), Guarded(prows, nout)
    K.lib().call(*stat3_call(K, x, m, c, wp, nout, out, psum, psq, add, ez, ey, coef))
    torch.cuda.synchronize()
    why = lambda ii: f"statistics row {ii[0][0]} of {prows} (64-row pixel tile{', the ragged last one' if ii[0][0] == prows - 1 and m % 64 else ''}), channel {ii[0][1]}"
    exact(out.view, final, f"{name} out", lambda ii: f"pixel tile {ii[0][0] // 64}")
    exact(psum.view, R.tile_sums(t1, 64), f"{name} psum", why)
    exact(psq.view, R.tile_sums(t2, 64), f"{name} psq", why)
    for gb, nm in ((out, "out"), (psum, "psum"), (psq, "psq")):
        gb.check(f"{name} {nm}")


def test_stat3_outside_the_64x64_tiling_is_refused(K):
    m, c, nout = 256, 40, 56
    assert P.nt_entry_kernel("stat3", m, nout, P.kp32(c)) is None
    g = gen(11)
    x = ints((1, 1, m, c), -1, 1, g)
    wp = pack1x1(K, _w_int(nout, c, 1, g)[:, :, 0].contiguous())
    add, ez, ey = (ints((1, 1, m, nout), -1, 1, g) for _ in range(3))
    out, psum, psq = Guarded(m, nout, nout + 8, BF16), Guarded(4, nout), Guarded(4, nout)
    assert rc_of(K, *stat3_call(K, x, m, c, wp, nout, out, psum, psq, add, ez, ey, stat_coef(nout, g))) == HN_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out.buf.view(torch.int16) == SENT16).all()) and bool((psum.buf.view(torch.int32) == SENT32).all())


# ---- random-operand companion -------------------------------------------------------------------------------------------------------------------
def test_mapped_outputs_random_bound(K):
    """random companions on the fp32-observable outputs of this file (the rpi mapping and the level-mapped output, both tilings):
    |err| <= 2e-5 * (|x| . |w|) elementwise"""
    g = gen(777)
    ratios = []
    for nout in (36, 88):
        n, c, hs, ws, align = 3, 64, (7, 3), (13, 5), 128
        m, lev, img, pix, real = R.lvlout_rows(n, hs, ws, align, dev())
        x = randn((1, 1, m, c), g)
        w2 = randn((nout, c), g).float()
        wp = pack1x1(K, w2)
        tot, ldc = 91 + 15, nout + 3
        stride = tot * ldc + 5
        out = Flat(max(n, max(P.cdiv(P.cdiv(n * h * w, align) * align, h * w) for h, w in zip(hs, ws))) * stride, F32)   # (as in test_lvlout_exact)
        hc, wc = (ctypes.c_int * 2)(*hs), (ctypes.c_int * 2)(*ws)
        K.lib().call("hn_conv_gemm_nt_lvlout", K.ptr(x), x.stride(2), m, c, K.ptr(wp), nout, 64, None, 0, out.ptr(), ldc, stride, n, 2,
                     ctypes.addressof(hc), ctypes.addressof(wc), align)
        offs = R.lvlout_offsets(n, hs, ws, align, stride, ldc, dev())
        for which in ("lvlout", "rpi"):
            if which == "rpi":
                m, stride = 3 * 35, 35 * ldc + 5
                x = randn((3, 5, 7, c), g)
                out = Flat(3 * stride, F32)
                K.lib().call("hn_conv_gemm_nt", K.ptr(x), None, 0, 3, 5, 7, c, 0, x.stride(2), 0, 0, m, K.ptr(wp), nout, 64, 1, None, 0, out.ptr(), 1, ldc,
                             35, stride, None, None)
                offs = R.rpi_offsets(m, 35, stride, ldc, dev())
            torch.cuda.synchronize()
            xd = x.double().reshape(-1, c)
            want, scale = xd @ w2.double().t(), xd.abs() @ w2.double().abs().t()
            rl = offs >= 0
            got = out.buf[offs[rl][:, None] + torch.arange(nout, device=dev())[None, :] + BAND].double()
            r = float(((got - want[rl]).abs() / scale[rl].clamp(min=1e-30)).max())
            print(f"{which} nout={nout}: max |err| / (|x| . |w|) = {r:.3e}")
            assert r <= RAND_TOL, f"{which} nout={nout}: max |err| / (|x| . |w|) = {r:.3e} > {RAND_TOL:.0e}"
            ratios.append(r)
    print("random ratios:", ["%.3e" % v for v in ratios])
