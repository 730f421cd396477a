"""The kernels of csrc/hn_stencil.hip held to the float64 index-form references of tests/stencil_ref.py, kernel by kernel, through the C
entry points.

All of them read bf16, accumulate in fp32 and do little else, so small-integer operands make every result an exact integer (or half):
bf16 holds integers exactly up to 256 and fp32 up to 2^24.  Every case states that budget (`budget`), asserts the kernel / partial-row
count it claims through the dispatch restatements of stencil_ref.py, keeps every output between sentinel guard bands (tests/guards.py,
row stride > C at least once per entry point), feeds inputs as channel slices of wider tensors, and compares with == in float64.  A
mismatch names the entry point, the case, the first positions with got / want and a hint (border, last strip, last channel group, level,
alignment row).

The swish parts of the BiFPN fusion node are not exact: they use the interval check of tests/test_batchnorm_exact_gpu.py (a bf16 output
must be the bf16 rounding of some value within `slack` of the float64 value), with that file's `slack_fwd` derivation:
  forward   slack = 4 U mags * 1.0999 + 8 U (2 + |x|) (|y| + 1)            (mags = sum |w_i v_i|, the __expf term as there)
  g         the same expression for y = swish'(x), times |dout| (swish' = s (1 + x (1 - s)): |d swish'/ds| <= 1 + |x|, so the sigmoid's
            (2 + |x|) ulps stay under the 8 (|y| + 1) factor for |x| <= 7; the cases assert |x| <= 6)
  w * g     the slack of g times |w| (+ the accumulated value's own rounding is inside the interval check)
  pw / dp   n_terms * 2^-24 * sum |g v| (fp32 running sums) on top of the slack of g times |v|
  wn        2 fp32 ulps;  sigmoid' of hn_head_grad: 3 fp32 ulps of |dy| / 4."""
import ctypes
import zlib

import pytest
import torch

from tests import bn_ref as B
from tests import stencil_ref as R
from tests.guards import Guarded, dev

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
BF16_EXACT = 256
F32_EXACT = 1 << 24


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops
    return ops


_LIVE = []


@pytest.fixture(autouse=True)
def _release():
    yield
    if _LIVE:
        torch.cuda.synchronize()
        _LIVE.clear()


def D(t):
    """t on the GPU, kept alive until the test ends (see test_batchnorm_exact_gpu.D)"""
    t = t.to(dev())
    _LIVE.append(t)
    return t


def gen(name):
    g = torch.Generator(device=dev())
    g.manual_seed(zlib.crc32(name.encode()) & 0xFFFFFF)
    return g


def ints(shape, lo, hi, g):
    """integers in [lo, hi] drawn on the device, as float64"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, device=dev()).to(F64)


def ints8(shape, lo, hi, g):
    """the same drawn as int8 (the large cap-crossing cases: a float64 copy of their operands would be gigabytes)"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, device=dev(), dtype=torch.int8)


class ArgBytes:
    """arg-max scratch of nbytes (prefilled with 77) between two 64-byte bands of a value no arg byte takes"""
    PAD, SENT = 64, 0xA5

    def __init__(self, nbytes, init=None):
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * self.PAD,), self.SENT, dtype=torch.uint8, device=dev())
        self.view = self.buf[self.PAD:self.PAD + nbytes]
        self.view.copy_(init.reshape(-1)) if init is not None else self.view.fill_(77)
        _LIVE.append(self)

    def ptr(self):
        return self.view.data_ptr()

    def check(self, name):
        bands = torch.cat([self.buf[:self.PAD], self.buf[self.PAD + self.n:]])
        bad = int((bands != self.SENT).sum())
        if bad:
            pytest.fail(f"{name}: {bad} bytes written outside the {self.n}-byte arg scratch")


def budget(name, terms, amax, bmax=1, extra=0, limit=BF16_EXACT):
    """the largest magnitude a result can reach stays exactly representable"""
    worst = terms * amax * bmax + extra
    assert worst <= limit, f"{name}: worst case {worst} exceeds the exactness limit {limit}"


def bf_in(v, extra=0, c0=0):
    """float64 [..., C] -> bf16 [rows, C] on the GPU; extra > 0: a channel slice (from column c0) of a tensor `extra` columns wider whose
    other columns hold other integers"""
    c = v.shape[-1]
    rows = v.numel() // c
    assert extra % 8 == 0 and c0 % 8 == 0 and c0 <= extra
    wide = torch.full((rows, c + extra), 5.0, dtype=BF16, device=dev())
    wide[:, c0:c0 + c] = v.reshape(rows, c).to(BF16)
    _LIVE.append(wide)
    return wide[:, c0:c0 + c]


def ld(t):
    return t.stride(0)


def out_bf(rows, c, extra=0, prev=None):
    g = Guarded(rows, c, c + extra, BF16)
    if prev is not None:
        g.view.copy_(prev.reshape(rows, c).to(BF16))
    _LIVE.append(g)
    return g


def out_f32(rows, c):
    g = Guarded(rows, c, c, F32)
    _LIVE.append(g)
    return g


def dscalar(v):
    return D(torch.tensor([v], dtype=F32))


def c_ints(v):
    return (ctypes.c_int * len(v))(*v)


def c_ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else (t if isinstance(t, int) else t.data_ptr()) for t in ts])


def call(K, name, *args):
    K.lib().call(name, *args)


def conv_hint(H, W, C):
    def h(idx):
        n, y, x, c = idx
        out = ["border pixel" if y in (0, H - 1) or x in (0, W - 1) else "interior"]
        if x >= (W - 1) // 4 * 4:
            out.append("last 4-pixel strip of the row")
        if c >= C - 8:
            out.append("last channel group")
        return ", ".join(out)
    return h


def level_hint(N, Hs, Ws, row_align):
    off = R.row_offsets(N, Hs, Ws, row_align)

    def h(idx):
        r = idx[0]
        l = max(i for i in range(len(Hs)) if off[i] <= r)
        real = N * Hs[l] * Ws[l]
        if r - off[l] >= real:
            return f"level {l}, alignment row"
        p = (r - off[l]) % (Hs[l] * Ws[l])
        y, x = p // Ws[l], p % Ws[l]
        return f"level {l} ({Hs[l]}x{Ws[l]}), pixel ({y}, {x}), tile ({y // 8}, {x // 16})" + (", border" if y in (0, Hs[l] - 1) or x in (0, Ws[l] - 1) else "")
    return h


def exact(got, want, name, hint=None, what="(n, y, x, c)"):
    """got == want in float64, bit for bit"""
    g = got.detach().to(want.dtype if want.dtype == F32 else F64).reshape(want.shape)       # (float32 references: the large cases)
    bad = ~(g == want.to(g.device))
    n = int(bad.sum())
    if n:
        lines = []
        for idx in bad.nonzero()[:6].tolist():
            t = tuple(idx)
            lines.append(f"  {what} {t}: got {float(g[t])!r} want {float(want[t])!r}" + (f"  [{hint(t)}]" if hint else ""))
        pytest.fail(f"{name}: {n} of {g.numel()} values differ\n" + "\n".join(lines))


def exact_bytes(got, want, name):
    g, w = got.to(torch.int64), want.to(torch.int64).to(got.device)
    bad = g != w
    n = int(bad.sum())
    if n:
        lines = [f"  (n, y, x, c) {tuple(i)}: got arg {int(g[tuple(i)])} want {int(w[tuple(i)])}" for i in bad.nonzero()[:6].tolist()]
        pytest.fail(f"{name}: {n} of {g.numel()} arg bytes differ\n" + "\n".join(lines))


def partial_rows(part, want, name, what="(c, tap)"):
    """fp32 partial rows [P, K]: every value an integer, the float64 column sum equal to the reference"""
    p = part.detach().double()
    frac = ~(p == p.round())                              # (a row the kernel never wrote holds the NaN sentinel and fails here)
    if int(frac.sum()):
        r, k = frac.nonzero()[0].tolist()
        pytest.fail(f"{name}: partial row {r}, column {k} holds {float(p[r, k])!r}, not an integer ({int(frac.sum())} such values of {p.numel()})")
    exact(p.sum(0).reshape(want.shape), want, name + " (column sums of the partial rows)", what=what)


def bf_interval(got, y, s, name):
    """every bf16 value of got is the bf16 rounding of some value in [y - s, y + s] (test_batchnorm_exact_gpu.bf_interval, on the device)"""
    s = s + 2 * U * y.abs() + 1e-38
    lo = (y - s).float().to(BF16).double()
    hi = (y + s).float().to(BF16).double()
    g = got.detach().double().reshape(y.shape)
    bad = ~((g >= lo) & (g <= hi))
    n = int(bad.sum())
    if n:
        lines = [f"  (n, y, x, c) {tuple(i)}: got {float(g[tuple(i)])!r}, allowed [{float(lo[tuple(i)])!r}, {float(hi[tuple(i)])!r}] "
                 f"(float64 value {float(y[tuple(i)])!r})" for i in bad.nonzero()[:6].tolist()]
        pytest.fail(f"{name}: {n} of {g.numel()} bf16 outputs outside their interval\n" + "\n".join(lines))


def swish_slack(x, y, mags):
    """slack_fwd of test_batchnorm_exact_gpu.py for the swish family (y = swish(x) or swish'(x))"""
    return 4 * U * mags * B.act_slope(B.ACT_SWISH) + 8 * U * (2 + x.abs()) * (y.abs() + 1)


# =====================================================================================================================================
# grouped 3x3
# =====================================================================================================================================
def gconv_weights(K, name, w, flip, c):
    """hn_gconv_pack on integer weights [C][8][3][3]; both packs are compared with the reference layout before they are used"""
    g8 = c // 8
    wg = D(w.float().contiguous())
    wk, wd = out_bf(72 * g8, 8), out_bf(72 * g8, 8)
    call(K, "hn_gconv_pack", wg.data_ptr(), wk.ptr(), wd.ptr(), c, flip)
    torch.cuda.synchronize()
    w4 = w.reshape(g8, 8, 8, 9)                                               # [g][o][i][tap]
    want_k = w4.permute(3, 2, 0, 1)                                           # wk[tap][i][g][o]
    want_d = w4.permute(3, 1, 0, 2)                                           # wd[tap'][o][g][i], tap' = 8 - tap when flipped
    if flip:
        want_d = want_d.flip(0)
    exact(wk.view, want_k.reshape(72 * g8, 8), f"hn_gconv_pack {name} wk", what="(piece, lane)")
    exact(wd.view, want_d.reshape(72 * g8, 8), f"hn_gconv_pack {name} wd (flip={flip})", what="(piece, lane)")
    wk.check(f"hn_gconv_pack {name} wk")
    wd.check(f"hn_gconv_pack {name} wd")
    return wk, wd


GCONV_S1 = [
    # name, N, H, W, C, extra columns of the input, of the output
    ("c8_3x5", 1, 3, 5, 8, 0, 8),
    ("c24_9x8", 2, 9, 8, 24, 8, 0),
    ("c176_3x17", 1, 3, 17, 176, 16, 8),
    ("c24_9x17_n3", 3, 9, 17, 24, 0, 0),
    ("c8_9x5", 2, 9, 5, 8, 8, 8),
]


@pytest.mark.parametrize("case", GCONV_S1, ids=[c[0] for c in GCONV_S1])
def test_gconv_stride1_fwd_and_dgrad(K, case):
    name, n, h, w, c, xi, xo = case
    budget(name, 72, 3, 1)
    g = gen("gconv1" + name)
    x, dz, wt = ints((n, h, w, c), -3, 3, g), ints((n, h, w, c), -3, 3, g), ints((c, 8, 3, 3), -1, 1, g)
    wk, wd = gconv_weights(K, name, wt, 1, c)
    xg, zg = bf_in(x, xi, xi), bf_in(dz, xi)
    y, dx = out_bf(n * h * w, c, xo), out_bf(n * h * w, c, xo)
    call(K, "hn_gconv_fwd", xg.data_ptr(), ld(xg), wk.ptr(), y.ptr(), y.ld, n, h, w, c, 1)
    call(K, "hn_gconv_fwd", zg.data_ptr(), ld(zg), wd.ptr(), dx.ptr(), dx.ld, n, h, w, c, 1)
    torch.cuda.synchronize()
    y.check(f"hn_gconv_fwd {name}")
    dx.check(f"hn_gconv_fwd (dgrad) {name}")
    exact(y.view, R.gconv(x, wt, 1), f"hn_gconv_fwd stride 1 {name}", conv_hint(h, w, c))
    exact(dx.view, R.gconv_dgrad(dz, wt, 1, h, w), f"hn_gconv_fwd stride 1 on dz with the flipped pack {name}", conv_hint(h, w, c))


GCONV_S2 = [
    # name, N, Hi, Wi, C, lds form, extra in, extra out
    ("c168_4x6", 1, 4, 6, 168, True, 8, 0),
    ("c168_10x14", 2, 10, 14, 168, True, 0, 8),
    ("c176_4x6", 2, 4, 6, 176, False, 0, 8),
    ("c176_10x14", 1, 10, 14, 176, False, 16, 0),
]


@pytest.mark.parametrize("case", GCONV_S2, ids=[c[0] for c in GCONV_S2])
def test_gconv_stride2_fwd(K, case):
    name, n, h, w, c, lds, xi, xo = case
    assert R.gconv_s2_lds(c) == lds
    budget(name, 72, 3, 1)
    g = gen("gconv2" + name)
    x, wt = ints((n, h, w, c), -3, 3, g), ints((c, 8, 3, 3), -1, 1, g)
    _, wd = gconv_weights(K, name, wt, 0, c)
    xg = bf_in(x, xi, xi)
    ho, wo = h // 2, w // 2
    y = out_bf(n * ho * wo, c, xo)
    call(K, "hn_gconv_fwd", xg.data_ptr(), ld(xg), wd.ptr(), y.ptr(), y.ld, n, h, w, c, 2)
    torch.cuda.synchronize()
    y.check(f"hn_gconv_fwd stride 2 {name}")
    exact(y.view, R.gconv(x, wt, 2), f"hn_gconv_fwd stride 2 {name} ({'LDS' if lds else 'global'} weights)", conv_hint(ho, wo, c))


GCONV_D2 = [
    ("c168_4x4", 2, 4, 4, 168, True, 8, 0),
    ("c168_10x12", 1, 10, 12, 168, True, 0, 8),
    ("c176_4x4", 1, 4, 4, 176, False, 0, 8),
    ("c176_10x12", 3, 10, 12, 176, False, 8, 0),
]


@pytest.mark.parametrize("case", GCONV_D2, ids=[c[0] for c in GCONV_D2])
def test_gconv_stride2_dgrad(K, case):
    name, n, h, w, c, lds, xi, xo = case
    assert R.gconv_s2_lds(c) == lds
    budget(name, 4 * 8, 3, 1)
    g = gen("gconvd2" + name)
    dz, wt = ints((n, h // 2, w // 2, c), -3, 3, g), ints((c, 8, 3, 3), -1, 1, g)
    wk, _ = gconv_weights(K, name, wt, 0, c)
    zg = bf_in(dz, xi, xi)
    dx = out_bf(n * h * w, c, xo)
    call(K, "hn_gconv_dgrad_s2", zg.data_ptr(), ld(zg), wk.ptr(), dx.ptr(), dx.ld, n, h, w, c)
    torch.cuda.synchronize()
    dx.check(f"hn_gconv_dgrad_s2 {name}")
    exact(dx.view, R.gconv_dgrad(dz, wt, 2, h, w), f"hn_gconv_dgrad_s2 {name} ({'LDS' if lds else 'global'} weights)", conv_hint(h, w, c))


GCONV_WG = [
    # name, N, Hi, Wi, C, stride, kernel, chunks, extra
    ("strip_c8_4x4", 1, 4, 4, 8, 1, "strip", 1, 8),
    ("strip_c8_8x8_s2", 1, 8, 8, 8, 2, "strip", 1, 0),
    ("sub_c24_32x32", 2, 32, 32, 24, 1, "sub", 32, 8),          # G * 9 = 27 items: one ragged block of 32
    ("sub_c24_64x32_s2", 2, 64, 32, 24, 2, "sub", 16, 0),
    ("sub_c24_33x31_short", 1, 33, 31, 24, 1, "sub", 16, 0),    # 1023 pixels in 16 chunks of 64: the last is short
    ("sub_c8_9x9_short", 1, 9, 9, 8, 1, "sub", 2, 8),           # 81 pixels in 2 chunks of 41, eight sub-chunks of 6
    ("sub_c176_16x8", 1, 16, 8, 176, 1, "sub", 2, 0),           # 198 items: 7 blocks of 32, the last ragged
]


@pytest.mark.parametrize("case", GCONV_WG, ids=[c[0] for c in GCONV_WG])
def test_gconv_wgrad(K, case):
    name, n, h, w, c, s, kern, chunks, xi = case
    plan = R.gconv_wgrad_plan(n, h, w, c, s)
    assert plan[:2] == (kern, chunks), plan
    ho, wo = R.out_hw(h, w, s)
    pixels = n * ho * wo
    assert chunks == K.lib().query("hn_wgrad_chunks", pixels, c // 8 * 9)
    if "short" in name:
        assert pixels % chunks != 0 and plan[2] * chunks > pixels
    budget(name, pixels, 3, 3, limit=F32_EXACT)
    g = gen("gwgrad" + name)
    x, dz = ints((n, h, w, c), -3, 3, g), ints((n, ho, wo, c), -3, 3, g)
    xg, zg = bf_in(x, xi, xi), bf_in(dz, xi)
    part = out_f32(chunks, c * 72)
    call(K, "hn_gconv_wgrad", xg.data_ptr(), ld(xg), zg.data_ptr(), ld(zg), part.ptr(), n, h, w, c, s)
    torch.cuda.synchronize()
    part.check(f"hn_gconv_wgrad {name}")
    partial_rows(part.view, R.gconv_wgrad(x, dz, s).reshape(c * 8, 9), f"hn_gconv_wgrad {name} ({kern} kernel, {chunks} chunks of {plan[2]})",
                 what="(o * 8 + i, tap)")


def plant(x, y0, x0, base, centre):
    """a 3x3 neighbourhood of constant `base` whose centre pixel holds `centre` (a list over channels, cycled)"""
    x[:, y0 - 1:y0 + 2, x0 - 1:x0 + 2, :] = base
    x[:, y0, x0, :] = torch.tensor(centre, dtype=F64, device=x.device).repeat(x.shape[-1] // len(centre))


def test_gconv_rounding_ties(K):
    """sums above 256 leave as round-to-nearest-even bf16: 257 -> 256 and 259 -> 260 (planted), and whatever else the map holds"""
    n, h, w, c = 1, 5, 9, 16
    g = gen("gconv_round")
    x = ints((n, h, w, c), 0, 7, g)
    plant(x, 1, 1, 3, [9, 8, 8, 8, 8, 8, 8, 8])                  # 72 * 3 + 40 + 1 = 257
    plant(x, 3, 5, 3, [11, 8, 8, 8, 8, 8, 8, 8])                 # 72 * 3 + 40 + 3 = 259
    wt = torch.ones((c, 8, 3, 3), dtype=F64, device=dev())
    budget("gconv_round", 72, 11, 1, limit=F32_EXACT)
    want = R.gconv(x, wt, 1)
    assert float(want[0, 1, 1, 0]) == 257 and float(want[0, 3, 5, 0]) == 259 and float(want.max()) > 256
    wk, wd = gconv_weights(K, "round", wt, 0, c)
    xg = bf_in(x, 8)
    y = out_bf(n * h * w, c)
    call(K, "hn_gconv_fwd", xg.data_ptr(), ld(xg), wk.ptr(), y.ptr(), y.ld, n, h, w, c, 1)
    torch.cuda.synchronize()
    y.check("hn_gconv_fwd rounding")
    rounded = R.bf16_rne(want)
    assert float(rounded[0, 1, 1, 0]) == 256 and float(rounded[0, 3, 5, 0]) == 260
    exact(y.view, rounded, "hn_gconv_fwd stride 1, sums above 256 (round to nearest even)", conv_hint(h, w, c))
    x2 = ints((n, 4, 8, c), 2, 7, g)                             # the packed-dot stride-2 form
    want2 = R.gconv(x2, wt, 2)
    assert float(want2.max()) > 256
    xg2 = bf_in(x2)
    y2 = out_bf(n * 2 * 4, c, 8)
    call(K, "hn_gconv_fwd", xg2.data_ptr(), ld(xg2), wd.ptr(), y2.ptr(), y2.ld, n, 4, 8, c, 2)
    torch.cuda.synchronize()
    y2.check("hn_gconv_fwd stride 2 rounding")
    exact(y2.view, R.bf16_rne(want2), "hn_gconv_fwd stride 2, sums above 256 (round to nearest even)", conv_hint(2, 4, c))


# =====================================================================================================================================
# depthwise 3x3
# =====================================================================================================================================
def dw_weights(K, name, w, c):
    """hn_dw_pack on integer weights [C][3][3]: wk[tap][c] and the flipped wkf[8 - tap][c], both compared with the reference layout"""
    wg = D(w.float().contiguous())
    wk, wf = out_bf(9, c), out_bf(9, c)
    call(K, "hn_dw_pack", wg.data_ptr(), wk.ptr(), wf.ptr(), c)
    torch.cuda.synchronize()
    w9 = w.reshape(c, 9).t()
    exact(wk.view, w9, f"hn_dw_pack {name} wk", what="(tap, c)")
    exact(wf.view, w9.flip(0), f"hn_dw_pack {name} flipped pack", what="(tap, c)")
    wk.check(f"hn_dw_pack {name} wk")
    wf.check(f"hn_dw_pack {name} wkf")
    return wk, wf


DW_FWD = [
    ("c8_1x1", 1, 1, 1, 8, 0, 8),
    ("c16_2x3", 2, 2, 3, 16, 8, 0),
    ("c88_5x5", 2, 5, 5, 88, 0, 8),
    ("c112_8x12", 1, 8, 12, 112, 16, 0),
    ("c256_7x18", 2, 7, 18, 256, 8, 8),
]


@pytest.mark.parametrize("case", DW_FWD, ids=[c[0] for c in DW_FWD])
def test_dwconv_fwd_dgrad_wgrad(K, case):
    name, n, h, w, c, xi, xo = case
    budget(name, 9, 7, 3)
    budget(name + " accumulate", 9, 7, 3, extra=20)
    g = gen("dw" + name)
    x, dz, wt = ints((n, h, w, c), -7, 7, g), ints((n, h, w, c), -3, 3, g), ints((c, 3, 3), -3, 3, g)
    prev = ints((n, h, w, c), -20, 20, g)
    wk, wf = dw_weights(K, name, wt, c)
    xg, zg = bf_in(x, xi, xi), bf_in(dz, xi)
    rows = n * h * w
    y, dx, ya = out_bf(rows, c, xo), out_bf(rows, c, xo), out_bf(rows, c, xo, prev)
    call(K, "hn_dwconv_fwd", xg.data_ptr(), ld(xg), wk.ptr(), y.ptr(), y.ld, n, h, w, c)
    call(K, "hn_dwconv_fwd", zg.data_ptr(), ld(zg), wf.ptr(), dx.ptr(), dx.ld, n, h, w, c)
    call(K, "hn_dwconv_fwd_levels", xg.data_ptr(), ld(xg), wk.ptr(), ya.ptr(), ya.ld, n, c, 1, c_ints([h]), c_ints([w]), 1, 1)
    strips = R.strips_of(n, [h], [w])
    blocks = R.dwconv_wgrad_blocks(strips, c)
    assert blocks == K.lib().query("hn_dwconv_wgrad_blocks", strips, c)
    budget(name + " wgrad", rows, 7, 3, limit=F32_EXACT)
    part = out_f32(blocks, c * 9)
    call(K, "hn_dwconv_wgrad", xg.data_ptr(), ld(xg), zg.data_ptr(), ld(zg), part.ptr(), n, h, w, c)
    torch.cuda.synchronize()
    for o, what in ((y, "fwd"), (dx, "fwd on dz"), (ya, "fwd accumulate"), (part, "wgrad")):
        o.check(f"hn_dwconv {what} {name}")
    hint = conv_hint(h, w, c)
    exact(y.view, R.dwconv(x, wt), f"hn_dwconv_fwd {name}", hint)
    exact(dx.view, R.dwconv_dgrad(dz, wt), f"hn_dwconv_fwd on dz with the flipped pack {name}", hint)
    exact(ya.view, R.dwconv(x, wt) + prev, f"hn_dwconv_fwd_levels (one level, accumulate) {name}", hint)
    partial_rows(part.view, R.dwconv_wgrad(x, dz).reshape(c, 9), f"hn_dwconv_wgrad {name} ({blocks} partial rows)")


def test_dwconv_wgrad_accepts_c2048(K):
    n, h, w, c = 1, 2, 3, 2048
    g = gen("dw2048")
    x, dz = ints((n, h, w, c), -7, 7, g), ints((n, h, w, c), -3, 3, g)
    xg, zg = bf_in(x), bf_in(dz)
    blocks = R.dwconv_wgrad_blocks(R.strips_of(n, [h], [w]), c)
    assert blocks == K.lib().query("hn_dwconv_wgrad_blocks", R.strips_of(n, [h], [w]), c)
    part = out_f32(blocks, c * 9)
    call(K, "hn_dwconv_wgrad", xg.data_ptr(), ld(xg), zg.data_ptr(), ld(zg), part.ptr(), n, h, w, c)
    torch.cuda.synchronize()
    part.check("hn_dwconv_wgrad c2048")
    partial_rows(part.view, R.dwconv_wgrad(x, dz).reshape(c, 9), "hn_dwconv_wgrad C = 2048")


def test_dwconv_rounding_ties(K):
    n, h, w, c = 1, 5, 9, 8
    g = gen("dw_round")
    x = ints((n, h, w, c), 20, 36, g)
    plant(x, 1, 1, 28, [33])                                      # 9 * 28 + 5 = 257
    plant(x, 3, 5, 28, [35])                                      # 9 * 28 + 7 = 259
    wt = torch.ones((c, 3, 3), dtype=F64, device=dev())
    budget("dw_round", 9, 36, 1, limit=F32_EXACT)
    want = R.dwconv(x, wt)
    assert float(want[0, 1, 1, 0]) == 257 and float(want[0, 3, 5, 3]) == 259 and float(want.max()) > 256
    wk, _ = dw_weights(K, "round", wt, c)
    xg = bf_in(x, 8, 8)
    y = out_bf(n * h * w, c, 8)
    call(K, "hn_dwconv_fwd", xg.data_ptr(), ld(xg), wk.ptr(), y.ptr(), y.ld, n, h, w, c)
    torch.cuda.synchronize()
    y.check("hn_dwconv_fwd rounding")
    rounded = R.bf16_rne(want)
    assert float(rounded[0, 1, 1, 0]) == 256 and float(rounded[0, 3, 5, 3]) == 260
    exact(y.view, rounded, "hn_dwconv_fwd, sums above 256 (round to nearest even)", conv_hint(h, w, c))


def packed_ints(n, hs, ws, c, align, lo, hi, g, junk):
    """level-packed integers [rows, C]; the alignment rows hold `junk`"""
    rows = R.row_offsets(n, hs, ws, align)[-1]
    v = ints((rows, c), lo, hi, g)
    v[R.alignment_rows(n, hs, ws, align).to(dev())] = junk
    return v


PYRAMID = ((20, 10, 5, 3, 2), (20, 10, 5, 3, 2))


@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("align", [1, 128])
def test_dwconv_levels_fwd_wgrad(K, align, acc):
    from multitask_hydranet_amd.ops import core
    hs, ws = PYRAMID
    n, c = 1, 16
    name = f"pyramid_align{align}_acc{acc}"
    off = R.row_offsets(n, hs, ws, align)
    if align > 1:
        assert off == [sum(core._pad_rows(n * h * w) for h, w in zip(hs[:l], ws[:l])) for l in range(6)] and align == core.LEVEL_ALIGN
    budget(name, 9, 7, 3, extra=20)
    g = gen("dwl" + name)
    x, dz = packed_ints(n, hs, ws, c, align, -7, 7, g, 99.0), packed_ints(n, hs, ws, c, align, -3, 3, g, -77.0)
    wt = ints((c, 3, 3), -3, 3, g)
    prev = ints((off[-1], c), -20, 20, g)
    wk, _ = dw_weights(K, name, wt, c)
    xg, zg = bf_in(x, 8, 8), bf_in(dz, 8)
    y = out_bf(off[-1], c, 8, prev if acc else None)
    H, W = c_ints(hs), c_ints(ws)
    call(K, "hn_dwconv_fwd_levels", xg.data_ptr(), ld(xg), wk.ptr(), y.ptr(), y.ld, n, c, 5, H, W, align, acc)
    strips = R.strips_of(n, hs, ws)
    blocks = R.dwconv_wgrad_blocks(strips, c)
    assert blocks == K.lib().query("hn_dwconv_wgrad_blocks", strips, c)
    part = out_f32(blocks, c * 9)
    call(K, "hn_dwconv_wgrad_levels", xg.data_ptr(), ld(xg), zg.data_ptr(), ld(zg), part.ptr(), n, c, 5, H, W, align)
    torch.cuda.synchronize()
    y.check(f"hn_dwconv_fwd_levels {name}")
    part.check(f"hn_dwconv_wgrad_levels {name}")
    exact(y.view, R.dwconv_levels(x, wt, n, hs, ws, align, prev if acc else None), f"hn_dwconv_fwd_levels {name}",
          level_hint(n, hs, ws, align), what="(row, c)")
    partial_rows(part.view, R.dwconv_wgrad_levels(x, dz, n, hs, ws, align).reshape(c, 9), f"hn_dwconv_wgrad_levels {name}")


DW_BWD = [
    # name, N, Hs, Ws, C, row_align, want dx, accumulate, form, extra columns
    ("strip_c8_5x5", 2, (5,), (5,), 8, 1, True, 0, "strip", 8),
    ("strip_c8_1x1", 1, (1,), (1,), 8, 1, True, 0, "strip", 0),
    ("strip_c112_7x18_acc", 2, (7,), (18,), 112, 1, True, 1, "strip", 8),
    ("strip_c112_2x3_nodx", 2, (2,), (3,), 112, 1, False, 0, "strip", 0),
    ("strip_c736_5x6", 1, (5,), (6,), 736, 1, True, 0, "strip", 0),
    ("strip_c776_5x6", 1, (5,), (6,), 776, 1, True, 0, "strip", 8),           # (256 * 37 + 9 C) * 4 > 64 KiB from C = 776: the LDS opt-in
    ("strip_c1024_3x9_acc", 1, (3,), (9,), 1024, 1, True, 1, "strip", 0),
    ("strip_c16_pyramid_align128", 1, PYRAMID[0], PYRAMID[1], 16, 128, True, 0, "strip", 8),
    ("strip_c16_pyramid_acc", 1, PYRAMID[0], PYRAMID[1], 16, 128, True, 1, "strip", 0),
    ("strip_c136_pyramid_nodx", 2, PYRAMID[0], PYRAMID[1], 136, 1, False, 0, "strip", 0),
    ("strip_c8_510tiles", 3, (80,), (272,), 8, 1, True, 0, "strip", 0),       # 510 tiles: just under the tiled form's 512
    ("tiled_c8_60x90", 11, (60,), (90,), 8, 1, True, 0, "tiled", 8),          # 528 ragged tiles (60 = 7.5 x 8, 90 = 5.6 x 16), 2 per workgroup
    ("tiled_c24_60x90_acc", 11, (60,), (90,), 24, 1, True, 1, "tiled", 0),
    ("tiled_c88_60x90_nodx", 11, (60,), (90,), 88, 1, False, 0, "tiled", 8),
    ("tiled_c112_60x90", 11, (60,), (90,), 112, 1, True, 0, "tiled", 0),
    ("tiled_c128_60x90", 11, (60,), (90,), 128, 1, True, 0, "tiled", 0),
    ("tiled_c24_levels_n7", 7, (64, 32, 16, 8, 4), (128, 64, 32, 16, 8), 24, 128, True, 0, "tiled", 0),   # 602 tiles, workgroups straddle levels
    ("tiled_c24_levels_n7_acc", 7, (64, 32, 16, 8, 4), (128, 64, 32, 16, 8), 24, 128, True, 1, "tiled", 8),
    ("tiled_c8_tpw3", 22, (60,), (90,), 8, 1, True, 0, "tiled", 0),           # 1056 tiles: three per workgroup
]


@pytest.mark.parametrize("case", DW_BWD, ids=[c[0] for c in DW_BWD])
def test_dwconv_bwd_levels(K, case):
    name, n, hs, ws, c, align, want_dx, acc, form, xi = case
    plan = R.dwconv_bwd_plan(n, c, hs, ws)
    assert plan[0] == form, plan
    blocks = plan[1]
    assert blocks == K.lib().query("hn_dwconv_bwd_blocks_levels", n, c, len(hs), c_ints(hs), c_ints(ws))
    strip_blocks = R.dwconv_bwd_strip_blocks(R.strips_of(n, hs, ws), c)
    if form == "tiled":
        assert blocks != strip_blocks, "the two forms give the same number of partial rows: the case cannot tell them apart"
        tiles = R.tiles_of(n, hs, ws)
        tpw = R.dwconv_bwd_tiled_plan(n, c, hs, ws)[0]
        if "tpw3" in name:
            assert tpw == 3
        if "levels" in name:
            assert any(sum(tiles[:l]) % tpw for l in range(1, len(tiles))), "no workgroup straddles two levels"
    if "510tiles" in name:
        assert sum(R.tiles_of(n, hs, ws)) == 510
    if "c776" in name:
        assert R.dwconv_bwd_strip_lds(c) > 65536 >= R.dwconv_bwd_strip_lds(c - 8)
    off = R.row_offsets(n, hs, ws, align)
    budget(name, 9, 3, 3, extra=20)
    budget(name + " wgrad", off[-1], 7, 3, limit=F32_EXACT)
    g = gen("dwb" + name)
    x, dz = packed_ints(n, hs, ws, c, align, -7, 7, g, 99.0), packed_ints(n, hs, ws, c, align, -3, 3, g, -77.0)
    wt = ints((c, 3, 3), -3, 3, g)
    prev = ints((off[-1], c), -20, 20, g)
    _, wf = dw_weights(K, name, wt, c)
    xg, zg = bf_in(x, xi, xi), bf_in(dz, xi)
    dx = out_bf(off[-1], c, xi, prev if acc else None) if want_dx else None
    part = out_f32(blocks, c * 9)
    call(K, "hn_dwconv_bwd_levels", zg.data_ptr(), ld(zg), xg.data_ptr(), ld(xg), wf.ptr(), dx.ptr() if dx else None, dx.ld if dx else 0,
         part.ptr(), n, c, len(hs), c_ints(hs), c_ints(ws), align, acc)
    torch.cuda.synchronize()
    part.check(f"hn_dwconv_bwd_levels {name} partial rows")
    where = f"hn_dwconv_bwd_levels {name} ({form} form, {blocks} partial rows)"
    if dx:
        dx.check(f"hn_dwconv_bwd_levels {name} dx")
        exact(dx.view, R.dwconv_dgrad_levels(dz, wt, n, hs, ws, align, prev if acc else None), where + " dx", level_hint(n, hs, ws, align),
              what="(row, c)")
    partial_rows(part.view, R.dwconv_wgrad_levels(x, dz, n, hs, ws, align).reshape(c, 9), where)


# =====================================================================================================================================
# pools and resamplers
# =====================================================================================================================================
POOL = [(n, h, w, c) for (n, h, w) in [(2, 2, 2), (1, 4, 6), (2, 16, 10)] for c in (8, 40)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", POOL, ids=[f"n{n}_{h}x{w}_c{c}" for n, h, w, c in POOL])
def test_maxpool_fwd_and_three_backward_routes(K, shape, mode):
    n, h, w, c = shape
    name = f"n{n}_{h}x{w}_c{c}_mode{mode}"
    ho, wo = h // 2, w // 2
    budget(name, 4, 3, 1, extra=20)                                     # a pixel collects at most four windows' gradients
    g = gen("pool" + name)
    x, dout = ints((n, h, w, c), -2, 2, g), ints((n, ho, wo, c), -3, 3, g)
    x[..., 0] = -1                                                      # all negative: in mode 0 the border windows pick the zero pad
    prev = ints((n, h, w, c), -20, 20, g)
    val, arg = R.maxpool(x, mode)
    if mode == 0:
        assert int((arg == 9).sum()) > 0, "no window picks the zero pad"
    xg, dg = bf_in(x, 8, 8), bf_in(dout, 8)
    y = out_bf(n * ho * wo, c, 8)
    call(K, "hn_maxpool_fwd", xg.data_ptr(), ld(xg), y.ptr(), y.ld, n, h, w, c, mode)
    half = dscalar(0.5)
    outs = []
    for ws, wsv in ((None, None), (half, 0.5)):
        d1, d2, d3, d4 = out_bf(n * h * w, c, 8), out_bf(n * h * w, c), out_bf(n * h * w, c, 8), out_bf(n * h * w, c, 0, prev)
        d5 = out_bf(n * h * w, c, 8, prev)
        a2 = ArgBytes(n * ho * wo * c)
        a3 = ArgBytes(n * ho * wo * c, arg)
        wp = ws.data_ptr() if ws is not None else None
        call(K, "hn_maxpool_bwd", xg.data_ptr(), ld(xg), dg.data_ptr(), ld(dg), d1.ptr(), d1.ld, wp, n, h, w, c, mode)
        call(K, "hn_maxpool_bwd2", xg.data_ptr(), ld(xg), dg.data_ptr(), ld(dg), d2.ptr(), d2.ld, wp, a2.ptr(), n, h, w, c, mode, 0)
        call(K, "hn_maxpool_bwd_from_arg", a3.ptr(), dg.data_ptr(), ld(dg), d3.ptr(), d3.ld, wp, n, h, w, c, mode, 0)
        call(K, "hn_maxpool_bwd_from_arg", a3.ptr(), dg.data_ptr(), ld(dg), d5.ptr(), d5.ld, wp, n, h, w, c, mode, 1)
        call(K, "hn_maxpool_bwd2", xg.data_ptr(), ld(xg), dg.data_ptr(), ld(dg), d4.ptr(), d4.ld, wp, a2.ptr(), n, h, w, c, mode, 1)
        outs.append((wsv, d1, d2, d3, d4, d5, a2, a3))
    torch.cuda.synchronize()
    y.check(f"hn_maxpool_fwd {name}")
    exact(y.view, val, f"hn_maxpool_fwd {name}", conv_hint(ho, wo, c))
    for wsv, d1, d2, d3, d4, d5, a2, a3 in outs:
        want = R.maxpool_bwd(arg, dout, wsv, h, w, mode)
        a2.check(f"hn_maxpool_bwd2 {name} arg scratch")
        a3.check(f"hn_maxpool_bwd_from_arg {name} arg bytes")
        exact_bytes(a2.view.reshape(n, ho, wo, c), arg, f"hn_maxpool_bwd2 {name} arg scratch")
        exact_bytes(a3.view.reshape(n, ho, wo, c), arg, f"hn_maxpool_bwd_from_arg {name} arg bytes (read only)")
        for o, route in ((d1, "hn_maxpool_bwd"), (d2, "hn_maxpool_bwd2"), (d3, "hn_maxpool_bwd_from_arg")):
            o.check(f"{route} {name}")
            exact(o.view, want, f"{route} {name} wscale {wsv}", conv_hint(h, w, c))
        for o, route in ((d4, "hn_maxpool_bwd2"), (d5, "hn_maxpool_bwd_from_arg")):
            o.check(f"{route} accumulate {name}")
            exact(o.view, want + prev, f"{route} accumulate {name} wscale {wsv}", conv_hint(h, w, c))


RESAMPLE = [("n2_1x1_c8", 2, 1, 1, 8), ("n1_3x5_c40", 1, 3, 5, 40), ("n2_8x6_c16", 2, 8, 6, 16)]


@pytest.mark.parametrize("case", RESAMPLE, ids=[c[0] for c in RESAMPLE])
def test_up2_and_sum2x2(K, case):
    name, n, h, w, c = case
    budget(name, 4, 3, 1, extra=20)
    g = gen("res" + name)
    x, gr = ints((n, h, w, c), -100, 100, g), ints((n, 2 * h, 2 * w, c), -3, 3, g)
    prev = ints((n, h, w, c), -20, 20, g)
    xg, gg = bf_in(x, 8, 8), bf_in(gr, 8)
    up = out_bf(n * 4 * h * w, c, 8)
    s0, s1, s2 = out_bf(n * h * w, c, 8), out_bf(n * h * w, c), out_bf(n * h * w, c, 8, prev)
    half = dscalar(0.5)
    call(K, "hn_up2_fwd", xg.data_ptr(), ld(xg), up.ptr(), up.ld, n, h, w, c)
    call(K, "hn_sum2x2", gg.data_ptr(), ld(gg), s0.ptr(), s0.ld, None, n, h, w, c, 0)
    call(K, "hn_sum2x2", gg.data_ptr(), ld(gg), s1.ptr(), s1.ld, half.data_ptr(), n, h, w, c, 0)
    call(K, "hn_sum2x2", gg.data_ptr(), ld(gg), s2.ptr(), s2.ld, half.data_ptr(), n, h, w, c, 1)
    torch.cuda.synchronize()
    for o, what in ((up, "hn_up2_fwd"), (s0, "hn_sum2x2"), (s1, "hn_sum2x2 wscale"), (s2, "hn_sum2x2 accumulate")):
        o.check(f"{what} {name}")
    exact(up.view, R.up2(x), f"hn_up2_fwd {name}")
    exact(s0.view, R.sum2x2(gr), f"hn_sum2x2 {name}")
    exact(s1.view, R.sum2x2(gr, 0.5), f"hn_sum2x2 {name} wscale 0.5")
    exact(s2.view, R.sum2x2(gr, 0.5) + prev, f"hn_sum2x2 {name} wscale 0.5, accumulate")


def second_pass(items):
    """the launch is capped at 8192 blocks of 256: more items than that run the grid-stride loop a second time"""
    assert R.ew_grid(items) == 8192 and items > 8192 * 256
    return f"item {8192 * 256} onwards is the second pass of the grid-stride loop"


def test_up2_past_the_grid_cap(K):
    n, h, w, c = 1, 512, 1030, 8
    hint = second_pass(n * 4 * h * w * (c // 8))
    x = ints8((n, h, w, c), -100, 100, gen("up2big"))
    xg = bf_in(x)
    up = out_bf(n * 4 * h * w, c, 8)
    call(K, "hn_up2_fwd", xg.data_ptr(), ld(xg), up.ptr(), up.ld, n, h, w, c)
    torch.cuda.synchronize()
    up.check("hn_up2_fwd past the cap")
    exact(up.view, R.up2(x, F32), "hn_up2_fwd past the cap: " + hint)


def test_sum2x2_past_the_grid_cap(K):
    n, h, w, c = 1, 1024, 2056, 8
    hint = second_pass(n * h * w * (c // 8))
    g = gen("sumbig")
    gr, prev = ints8((n, 2 * h, 2 * w, c), -3, 3, g), ints8((n, h, w, c), -20, 20, g)
    gg = bf_in(gr)
    s = out_bf(n * h * w, c, 8, prev)
    half = dscalar(0.5)
    call(K, "hn_sum2x2", gg.data_ptr(), ld(gg), s.ptr(), s.ld, half.data_ptr(), n, h, w, c, 1)
    torch.cuda.synchronize()
    s.check("hn_sum2x2 past the cap")
    exact(s.view, R.sum2x2(gr, 0.5, F32) + prev.to(F32), "hn_sum2x2 (wscale, accumulate) past the cap: " + hint)


def test_maxpool_fwd_past_the_grid_cap(K):
    n, h, w, c = 1, 2048, 4112, 8
    hint = second_pass(n * (h // 2) * (w // 2) * (c // 8))
    x = ints8((n, h, w, c), -2, 2, gen("poolbig"))
    xg = bf_in(x)
    y = out_bf(n * (h // 2) * (w // 2), c, 8)
    call(K, "hn_maxpool_fwd", xg.data_ptr(), ld(xg), y.ptr(), y.ld, n, h, w, c, 0)
    torch.cuda.synchronize()
    y.check("hn_maxpool_fwd past the cap")
    exact(y.view, R.maxpool(x, 0, F32)[0], "hn_maxpool_fwd past the cap: " + hint)


# =====================================================================================================================================
# seg fold, pixel shuffles, head gradient
# =====================================================================================================================================
FOLD = [(hw, up, c0, yp) for hw in [(4, 4), (5, 7), (16, 12)] for up in (0, 1, 2) for c0, yp in ((0, False), (24, True))
        if not (up == 1 and (hw[0] % 2 or hw[1] % 2))]


@pytest.mark.parametrize("case", FOLD, ids=[f"{h}x{w}_up{up}_c0_{c0}_{'elu' if yp else 'plain'}" for (h, w), up, c0, yp in FOLD])
def test_seg_fold(K, case):
    (h, w), up, c0, yp = case
    n, c, ldv = 2, 16, 48
    name = f"{h}x{w} up={up} c0={c0} yprev={yp}"
    budget(name, 4 * 4, 3, 1)                                           # a corner collects 4 padded positions, times the 2x2 block; halves are exact
    g = gen("fold" + name)
    dvp = ints((n, h + 2, w + 2, ldv), -3, 3, g)
    ho, wo = (h // 2, w // 2) if up == 1 else (h, w)
    yprev = None
    if yp:
        yprev = torch.tensor([-0.5, 0.0, 2.0], dtype=F64, device=dev())[torch.randint(0, 3, (n, ho, wo, c), generator=g, device=dev())]
    vg = bf_in(dvp)
    yg = bf_in(yprev, 8, 8) if yp else None
    out = out_bf(n * ho * wo, c, 8)
    call(K, "hn_seg_fold", vg.data_ptr(), ld(vg), c0, out.ptr(), out.ld, yg.data_ptr() if yp else None, ld(yg) if yp else 0, n, h, w, c, up)
    torch.cuda.synchronize()
    out.check(f"hn_seg_fold {name}")
    exact(out.view, R.seg_fold(dvp, c0, c, h, w, up, yprev), f"hn_seg_fold {name}", conv_hint(ho, wo, c))


def test_seg_fold_past_the_grid_cap(K):
    n, h, w, c = 2, 1024, 1100, 8
    hint = second_pass(n * h * w * (c // 8))
    dvp = ints8((n, h + 2, w + 2, c), -3, 3, gen("foldbig"))
    vg = bf_in(dvp)
    out = out_bf(n * h * w, c, 8)
    call(K, "hn_seg_fold", vg.data_ptr(), ld(vg), 0, out.ptr(), out.ld, None, 0, n, h, w, c, 0)
    torch.cuda.synchronize()
    out.check("hn_seg_fold past the cap")
    exact(out.view, R.seg_fold(dvp, 0, c, h, w, 0, None, F32), "hn_seg_fold past the cap: " + hint, conv_hint(h, w, c))


@pytest.mark.parametrize("k,ldo", [(5, 24), (64, 256)])
def test_space_to_depth(K, k, ldo):
    n, h, w = 2, 3, 5
    dy = ints((n, 2 * h, 2 * w, k), -200, 200, gen(f"s2d{k}"))
    dg = D(dy.float().contiguous())
    out = out_bf(n * h * w, ldo)
    call(K, "hn_space_to_depth", dg.data_ptr(), out.ptr(), ldo, n, h, w, k)
    torch.cuda.synchronize()
    out.check(f"hn_space_to_depth k={k}")
    exact(out.view, R.space_to_depth(dy, k, ldo), f"hn_space_to_depth k={k} ldo={ldo} (columns >= {4 * k} are zero fill)")


@pytest.mark.parametrize("psum", [False, True], ids=["plain", "psum"])
@pytest.mark.parametrize("k", [64, 128])
def test_space_to_depth_bf16(K, k, psum):
    n, h, w = 2, 5, 7
    budget(f"s2d16 k={k}", n * 4 * h * w, 100, 1, limit=F32_EXACT)
    x = ints((n, 2 * h, 2 * w, k), -100, 100, gen(f"s2d16{k}"))
    xg = bf_in(x, 8, 8)
    out = out_bf(n * h * w, 4 * k)
    blocks = R.space_to_depth_blocks(n, h, w, k)
    assert blocks == K.lib().query("hn_space_to_depth_blocks", n, h, w, k)
    ps = out_f32(blocks, k)
    call(K, "hn_space_to_depth_bf16", xg.data_ptr(), ld(xg), out.ptr(), n, h, w, k, ps.ptr() if psum else None)
    torch.cuda.synchronize()
    out.check(f"hn_space_to_depth_bf16 k={k}")
    ps.check(f"hn_space_to_depth_bf16 k={k} psum")
    want, sums = R.space_to_depth_sums(x, k)
    exact(out.view, want, f"hn_space_to_depth_bf16 k={k}")
    if psum:
        partial_rows(ps.view, sums.reshape(1, k), f"hn_space_to_depth_bf16 k={k} psum ({blocks} rows)", what="(0, channel)")
    else:
        assert bool((ps.buf.view(torch.int32) == 0x7FC00001).all()), "hn_space_to_depth_bf16 wrote psum without being given one"


def test_head_grad_gather(K):
    n, hs, ws, lds, nout, ldz, align = 2, (5, 3, 2), (4, 3, 1), 12, 5, 8, 16
    rows = sum(h * w for h, w in zip(hs, ws))
    g = gen("headgrad")
    dy = ints((n, rows, lds), -200, 200, g)
    dg = D(dy.float().contiguous())
    dz = out_bf(n * rows, ldz)
    call(K, "hn_head_grad", dg.data_ptr(), None, rows, rows * lds, lds, nout, dz.ptr(), ldz, n * rows, 0)
    off = R.row_offsets(n, hs, ws, align)
    prev = ints((off[-1], ldz), -20, 20, g)
    dl = out_bf(off[-1], ldz, 0, prev)
    call(K, "hn_head_grad_levels", dg.data_ptr(), None, rows * lds, lds, nout, dl.ptr(), ldz, n, 3, c_ints(hs), c_ints(ws), align, 0)
    torch.cuda.synchronize()
    dz.check("hn_head_grad")
    dl.check("hn_head_grad_levels")
    exact(dz.view, R.head_grad(dy, None, rows, rows * lds, lds, nout, ldz, n * rows), "hn_head_grad (no sigmoid)", what="(row, c)")
    exact(dl.view, R.head_grad_levels(dy, None, rows * lds, lds, nout, ldz, n, hs, ws, align, False, prev),
          "hn_head_grad_levels (no sigmoid; alignment rows untouched)", level_hint(n, hs, ws, align), what="(row, c)")


def test_head_grad_sigmoid(K):
    n, rows, lds, nout, ldz = 2, 37, 8, 5, 8
    g = gen("headsig")
    dy = ints((n, rows, lds), -200, 200, g)
    y = torch.rand((n, rows, lds), generator=g, device=dev(), dtype=F32)
    dg, yg = D(dy.float().contiguous()), D(y)
    dz = out_bf(n * rows, ldz)
    call(K, "hn_head_grad", dg.data_ptr(), yg.data_ptr(), rows, rows * lds, lds, nout, dz.ptr(), ldz, n * rows, 1)
    torch.cuda.synchronize()
    dz.check("hn_head_grad sigmoid")
    want = R.head_grad(dy, y, rows, rows * lds, lds, nout, ldz, n * rows, True)
    slack = 3 * 2.0 ** -23 * R.head_grad(dy, None, rows, rows * lds, lds, nout, ldz, n * rows).abs() / 4         # dy * s * (1 - s) <= |dy| / 4
    bf_interval(dz.view, want, slack, "hn_head_grad with sigmoid'")


# =====================================================================================================================================
# BiFPN fusion node
# =====================================================================================================================================
def fuse_shapes(n, h, w, c):
    return {1: (n, h, w, c), 2: (n, h // 2, w // 2, c), 3: (n, 2 * h, 2 * w, c)}


class FuseCase:
    """one node: integer inputs, power-of-two weights, everything both sides need"""

    def __init__(self, name, modes, n, h, w, c, wv=(0.5, 0.25, 0.25)):
        g = gen("fuse" + name)
        self.name, self.modes, self.n, self.h, self.w, self.c = name, modes, n, h, w, c
        sh = fuse_shapes(n, h, w, c)
        self.ins = [None if m == 0 else ints(sh[m], -3, 3, g) for m in modes]
        self.wv = [wv[i] if m else 0.0 for i, m in enumerate(modes)]
        self.dout = ints(sh[1], -3, 3, g)
        self.prev = [None if m == 0 else ints(sh[m], -20, 20, g) for m in modes]
        self.gin = [None if x is None else bf_in(x, 8, 8) for x in self.ins]
        self.gd = bf_in(self.dout, 8)
        self.wg = D(torch.tensor(self.wv, dtype=F32))
        self.IN = c_ptrs(self.gin)
        self.LD = c_ints([0 if t is None else ld(t) for t in self.gin])
        self.MODE = c_ints(modes)
        self.rows = n * h * w

    def backward(self, K, dst, acc, with_arg):
        """launch hn_fuse_bwd / hn_fuse_bwd_arg; dst[i]: give input i a destination.  Returns the guarded outputs."""
        sh = fuse_shapes(self.n, self.h, self.w, self.c)
        g = out_bf(self.rows, self.c, 8)
        din = []
        for i, m in enumerate(self.modes):
            if m in (1, 2) and dst[i]:
                r = sh[m][0] * sh[m][1] * sh[m][2]
                din.append(out_bf(r, self.c, 8, self.prev[i] if acc[i] else None))
            else:
                din.append(None)
        blocks = R.fuse_bwd_blocks(self.n, self.h, self.w, self.c)
        assert blocks == K.lib().query("hn_fuse_bwd_blocks", self.n, self.h, self.w, self.c)
        pw = out_f32(blocks, 3)
        args = [ArgBytes(self.rows * self.c) if m == 3 and with_arg else None for m in self.modes]
        DIN = c_ptrs([None if d is None else d.ptr() for d in din])
        LDIN = c_ints([0 if d is None else d.ld for d in din])
        head = (self.IN, self.LD, self.MODE, self.wg.data_ptr(), self.gd.data_ptr(), ld(self.gd), g.ptr(), g.ld, DIN, LDIN, c_ints(acc), pw.ptr())
        _LIVE.append((DIN, LDIN))
        if with_arg:
            A = c_ptrs([None if a is None else a.ptr() for a in args])
            _LIVE.append(A)
            call(K, "hn_fuse_bwd_arg", *head, A, self.n, self.h, self.w, self.c)
        else:
            call(K, "hn_fuse_bwd", *head, self.n, self.h, self.w, self.c)
        return g, din, pw, args


FUSE = [
    # name, modes, N, H, W, C
    ("td_120", (1, 2, 0), 2, 6, 10, 16),
    ("td_102", (1, 0, 2), 1, 4, 4, 40),
    ("td_210", (2, 1, 0), 1, 4, 8, 24),            # the identity input behind the up-sampled one
    ("bu_121", (1, 2, 1), 2, 4, 6, 8),
    ("bu_113", (1, 1, 3), 2, 3, 5, 16),
    ("bu_130", (1, 3, 0), 1, 5, 3, 24),
    ("big_113", (1, 1, 3), 2, 96, 96, 128),        # 294912 work items: the 1024-block cap makes the loop stride
]


ACC_ALL = ("td_120", "td_210", "bu_113", "big_113")       # cases whose every destination, the identity in slot 0 included, accumulates


@pytest.mark.parametrize("case", FUSE, ids=[c[0] for c in FUSE])
def test_fuse_fwd(K, case):
    name, modes, n, h, w, c = case
    f = FuseCase(name, modes, n, h, w, c)
    out = out_bf(f.rows, c, 8)
    call(K, "hn_fuse_fwd", f.IN, f.LD, f.MODE, f.wg.data_ptr(), out.ptr(), out.ld, n, h, w, c)
    # the raw form: p = (2, 1, 1) -> (0.5, 0.25, 0.25) up to eps; one case with a negative parameter (its weight is exactly 0)
    nw = max(i for i, m in enumerate(modes) if m) + 1                    # the kernel takes praw[i] by slot: every active slot gets its parameter
    praw = [2.0, 1.0, 1.0]
    if name == "bu_121":
        praw = [2.0, -1.0, 2.0]
    eps = 1e-4
    pr = D(torch.tensor(praw, dtype=F32))
    wn = out_f32(1, 3)
    out2 = out_bf(f.rows, c, 8)
    call(K, "hn_fuse_fwd_raw", f.IN, f.LD, f.MODE, pr.data_ptr(), nw, eps, wn.ptr(), out2.ptr(), out2.ld, n, h, w, c)
    torch.cuda.synchronize()
    for o, what in ((out, "hn_fuse_fwd"), (out2, "hn_fuse_fwd_raw"), (wn, "hn_fuse_fwd_raw wn")):
        o.check(f"{what} {name}")
    pre, y = R.fuse_fwd(f.ins, modes, f.wv)
    assert float(pre.abs().max()) <= 6
    bf_interval(out.view, y, swish_slack(pre, y, 0 * pre), f"hn_fuse_fwd {name}")          # integer inputs, power-of-two weights: pre is exact
    eps32 = float(torch.tensor(eps, dtype=F32))
    want_w = R.fuse_weights(torch.tensor(praw, dtype=F64), nw, eps32)
    got_w = wn.view.detach().double().cpu().reshape(3)
    assert bool(((got_w - want_w).abs() <= 2 * 2.0 ** -23 * want_w.abs()).all()), f"hn_fuse_fwd_raw {name}: wn {got_w.tolist()} want {want_w.tolist()}"
    if name == "bu_121":
        assert float(got_w[1]) == 0.0
    terms, _ = R._fuse_terms(f.ins, modes)
    mags = sum(abs(float(got_w[i])) * t.abs() for i, t in enumerate(terms) if t is not None)
    pre2 = sum(float(got_w[i]) * t for i, t in enumerate(terms) if t is not None)           # the kernel's own (checked) weights
    bf_interval(out2.view, pre2 * torch.sigmoid(pre2), swish_slack(pre2, pre2 * torch.sigmoid(pre2), mags), f"hn_fuse_fwd_raw {name}")


@pytest.mark.parametrize("case", FUSE, ids=[c[0] for c in FUSE])
def test_fuse_bwd(K, case):
    name, modes, n, h, w, c = case
    f = FuseCase(name, modes, n, h, w, c)
    dst_all = [m in (1, 2) for m in modes]
    # accumulate on every destination (ACC_ALL), or on every destination but the one in slot 0
    acc = [1 if (m in (1, 2) and (i != 0 or name in ACC_ALL)) else 0 for i, m in enumerate(modes)]
    expect = R.fuse_bwd_kernel(modes, dst_all, h, w)
    assert expect == ("quads" if name.startswith("td") else "generic")
    g1, din1, pw1, args1 = f.backward(K, dst_all, acc, True)                                # hn_fuse_bwd_arg (no pooled input: an array of nulls)
    g0, din0, pw0, _ = f.backward(K, dst_all, acc, False)                                   # hn_fuse_bwd: the same kernel; pooled inputs by fuse_gather
    runs = [(expect, g1, din1, pw1)]
    if expect == "quads":                                                                   # the same node without a destination for the up-sampled input
        dst2 = [m == 1 for m in modes]
        assert R.fuse_bwd_kernel(modes, dst2, h, w) == "generic"
        g2, din2, pw2, _ = f.backward(K, dst2, acc, False)
        runs.append(("generic", g2, din2, pw2))
    torch.cuda.synchronize()
    for o in [g0, pw0] + [d for d in din0 if d is not None]:
        o.check(f"hn_fuse_bwd {name} (plain entry)")
    same = [(g0, g1, "g"), (pw0, pw1, "pw")] + [(a, b, f"din[{i}]") for i, (a, b) in enumerate(zip(din0, din1)) if a is not None]
    for a, b, what in same:
        it = torch.int16 if a.dtype == BF16 else torch.int32
        assert torch.equal(a.view.contiguous().view(it), b.view.contiguous().view(it)), \
            f"hn_fuse_bwd {name}: {what} differs between hn_fuse_bwd and hn_fuse_bwd_arg ({expect} kernel)"
    ref = R.fuse_bwd(f.ins, modes, f.wv, f.dout)
    assert float(ref["pre"].abs().max()) <= 6
    sg = f.dout.abs() * swish_slack(ref["pre"], R.swish_grad(ref["pre"]), 0 * ref["pre"])
    blocks = pw1.rows
    items = f.rows * (c // 8)
    for kern, g, din, pw in runs:
        where = f"hn_fuse_bwd {name} ({kern} kernel)"
        g.check(where + " g")
        pw.check(where + " pw")
        bf_interval(g.view, ref["g"], sg, where + " g")
        gk = g.view.detach().double().reshape(n, h, w, c)                                   # the kernel's own g
        for i, m in enumerate(modes):
            if din[i] is None:
                continue
            din[i].check(where + f" din[{i}]")
            base = f.prev[i] if acc[i] else 0
            if m == 1:
                bf_interval(din[i].view, f.wv[i] * ref["g"] + base, f.wv[i] * sg, where + f" din[{i}] (identity)")
            else:                                                                           # w * 2x2 sums of the bf16-rounded g: exact
                exact(din[i].view, R.bf16_rne(R.sum2x2(gk, f.wv[i]) + base), where + f" din[{i}] (2x2 sums of the kernel's g)")
        # pw: fp32 sums of g * T_i(in_i) over each block's items (8 channels, 4 pixels in the quads form)
        n_terms = 32 * -(-items // (blocks * 256)) + 6 + 4                                  # a thread's chain, the wave sum, the four waves
        got = pw.view.detach().double().sum(0).cpu()
        for i, m in enumerate(modes):
            if not m:
                assert float(got[i]) == 0.0
                continue
            mag = float((ref["g"] * ref["terms"][i]).abs().sum())
            bound = n_terms * U * mag + float((sg * ref["terms"][i].abs()).sum())
            assert abs(float(got[i]) - float(ref["dw"][i])) <= bound, \
                f"{where} pw column {i}: got {float(got[i])!r} want {float(ref['dw'][i])!r} (bound {bound:.3e})"
    if len(runs) == 2:                                                                      # "same arithmetic in the same order"
        (_, ga, da, _), (_, gb, db, _) = runs
        assert torch.equal(ga.view.contiguous().view(torch.int16), gb.view.contiguous().view(torch.int16)), f"hn_fuse_bwd {name}: g differs between the quads and the generic kernel"
        for i, m in enumerate(modes):
            if m == 1:
                assert torch.equal(da[i].view.contiguous().view(torch.int16), db[i].view.contiguous().view(torch.int16)), \
                    f"hn_fuse_bwd {name}: din[{i}] differs between the quads and the generic kernel"
    if name == "big_113":
        assert blocks == 1024 and f.rows * (c // 8) > 262144
    # pooled inputs: the arg bytes, and the routing of the kernel's own g through them
    for i, m in enumerate(modes):
        if m != 3:
            continue
        args1[i].check(f"hn_fuse_bwd_arg {name} arg bytes of input {i}")
        exact_bytes(args1[i].view.reshape(n, h, w, c), ref["arg"][i], f"hn_fuse_bwd_arg {name} arg bytes of input {i}")
        gk = g1.view.detach().double().reshape(n, h, w, c)
        wsc = dscalar(f.wv[i])
        gcont = D(g1.view.contiguous())
        dxp = out_bf(n * 4 * h * w, c, 8)
        call(K, "hn_maxpool_bwd_from_arg", args1[i].ptr(), gcont.data_ptr(), c, dxp.ptr(), dxp.ld, wsc.data_ptr(), n, 2 * h, 2 * w, c, 0, 0)
        torch.cuda.synchronize()
        dxp.check(f"hn_maxpool_bwd_from_arg after hn_fuse_bwd_arg {name}")
        # up to four bf16 values summed in fp32 and scaled by a power of two: the sum of four 8-bit mantissas within 2^16 of each other is
        # exact in fp32 unless their exponents differ by more than 16, which the interval check allows for
        a4 = args1[i].view.reshape(n, h, w, c)
        routed = R.maxpool_bwd(a4, gk, f.wv[i], 2 * h, 2 * w, 0)
        absr = R.maxpool_bwd(a4, gk.abs(), f.wv[i], 2 * h, 2 * w, 0)
        bf_interval(dxp.view, routed, 4 * U * absr, f"hn_maxpool_bwd_from_arg on the arg bytes and g of hn_fuse_bwd_arg {name}")


def test_fuse_dweights(K):
    g = gen("fusedw")
    blocks = 300
    pw = torch.rand((blocks, 3), generator=g, device=dev(), dtype=F32) * 2 - 1
    for praw, nw in (([2.0, 1.0, 1.0], 3), ([2.0, -1.0, 2.0], 3), ([0.5, 1.5, 0.0], 2)):
        eps = 1e-4
        pr = D(torch.tensor(praw, dtype=F32))
        pg = D(pw.clone())
        dp = out_f32(1, 3)
        call(K, "hn_fuse_dweights", pg.data_ptr(), blocks, pr.data_ptr(), nw, eps, dp.ptr())
        torch.cuda.synchronize()
        dp.check("hn_fuse_dweights")
        dw = pw.double().sum(0).cpu()
        want = R.fuse_dweights(dw, torch.tensor(praw, dtype=F64), nw, float(torch.tensor(eps, dtype=F32)))
        mag = float(pw.double().abs().sum(0).max())
        s = float(sum(max(p, 0.0) for p in praw[:nw])) + eps
        bound = (blocks // 256 + 2 + 8 + 8) * U * mag * 2 / s                               # fp32 running sums of the columns, then a handful of fp32 operations
        got = dp.view.detach().double().cpu().reshape(3)[:nw]
        assert bool(((got - want).abs() <= bound).all()), f"hn_fuse_dweights praw={praw}: got {got.tolist()} want {want.tolist()} (bound {bound:.3e})"
        for i in range(nw):
            if praw[i] <= 0:
                assert float(got[i]) == 0.0


# =====================================================================================================================================
# stem: dense 3x3 / stride 2 from the fp32 NCHW frame, with its bf16 im2col rows
# =====================================================================================================================================
STEM = [
    # name, N, H, W, store paths the case takes
    ("partial_block", 2, 16, 24, "rows"),                  # 96 pixel pairs: thread-owned rows only
    ("whole_blocks", 2, 64, 128, "lds"),                   # 2048 pairs: eight whole blocks through LDS
    ("block_and_tail", 1, 34, 68, "both"),                 # 289 pairs: one whole block and a tail of 33
    ("odd_wo", 3, 18, 22, "rows"),                         # Wo = 11: every row ends in a lone pixel
    ("one_pixel", 1, 2, 2, "rows"),
]


def stem_hint(n, h, w):
    lds = R.stem_lds_path(n, h, w)
    wo = w >> 1

    def hint(idx):
        b, y, x = idx[:3]
        out = ["XOR-swizzled LDS store path" if bool(lds[b, y, x]) else "thread-owned rows store path"]
        out.append("second pixel of its thread" if x & 1 else ("lone pixel ending an odd row" if x == wo - 1 else "first pixel of its thread"))
        if y in (0, (h >> 1) - 1) or x in (0, wo - 1):
            out.append("border")
        return ", ".join(out)
    return hint


@pytest.mark.parametrize("with_patches", [False, True], ids=["patches_null", "patches"])
@pytest.mark.parametrize("case", STEM, ids=[c[0] for c in STEM])
def test_stem_fwd(K, case, with_patches):
    name, n, h, w, paths = case
    budget(name, 27, 3, 3)                                  # 27 taps of |x| <= 3 times |w| <= 3: 243 <= 256, z is exact in bf16
    lds = R.stem_lds_path(n, h, w)
    assert {"rows": not bool(lds.any()), "lds": bool(lds.all()), "both": bool(lds.any()) and not bool(lds.all())}[paths]
    ho, wo = R.stem_out_hw(h, w)
    g = gen("stem" + name)
    x, wt = ints((n, 3, h, w), -3, 3, g), ints((32, 3, 3, 3), -3, 3, g)
    xg, wg = D(x.float().contiguous()), D(wt.float().contiguous())
    z = out_bf(n * ho * wo, 32)
    p = out_bf(n * ho * wo, 32)
    call(K, "hn_stem_fwd", xg.data_ptr(), wg.data_ptr(), z.ptr(), p.ptr() if with_patches else None, n, h, w)
    torch.cuda.synchronize()
    z.check(f"hn_stem_fwd {name} z")
    p.check(f"hn_stem_fwd {name} patches")
    hint = stem_hint(n, h, w)
    exact(z.view, R.stem(x, wt), f"hn_stem_fwd {name} z (patches {'on' if with_patches else 'null'})", hint)
    if with_patches:
        want = R.stem_patches(x)
        exact(p.view, want, f"hn_stem_fwd {name} patches", hint, what="(n, y, x, tap)")
        assert float(p.view.detach().double()[:, 27:].abs().sum()) == 0, f"hn_stem_fwd {name}: columns 27..31 of the patch rows are not zero"
    else:
        assert bool((p.buf.view(torch.int16) == 0x7FC1).all()), f"hn_stem_fwd {name} wrote patches without being given a buffer"


def test_stem_refuses_an_odd_frame(K):
    """`H >> 1` on an odd frame would drop conv2d's last output row (stencil_ref.stem_out_hw): the entry point refuses it, nothing is written"""
    xg, wg = D(torch.zeros(1, 3, 17, 24)), D(torch.zeros(32, 3, 3, 3))
    z, p = out_bf(8 * 12, 32), out_bf(8 * 12, 32)
    raw = K.lib().raw("hn_stem_fwd")
    st = torch.cuda.current_stream().cuda_stream
    assert raw(xg.data_ptr(), wg.data_ptr(), z.ptr(), p.ptr(), 1, 17, 24, st) == 1
    assert raw(xg.data_ptr(), wg.data_ptr(), z.ptr(), p.ptr(), 1, 16, 23, st) == 1
    torch.cuda.synchronize()
    for o in (z, p):
        assert bool((o.buf.view(torch.int16) == 0x7FC1).all())
