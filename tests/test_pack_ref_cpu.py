"""CPU: the weight-pack references of tests/pack_ref.py pinned to plain torch, so that a reference cannot share a misreading of a layout
with the kernel it judges (tests/test_pack_exact_gpu.py).  Integer data: every contraction below is exact in float64 and compared with ==.

An operand is pinned by USING it the way its consumer does: pixel rows (zero / clamp padded, channels padded to the operand's K) are
contracted with it tap by tap, and the result must be the convolution, or the gradient, the operand stands for."""
import pytest
import torch
import torch.nn.functional as F

from tests import pack_ref as P
from tests import seg_conv_ref as S
from tests.exact_checks import gen

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F64)


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def zero_pad(x, k):
    """[n, H, W, C] -> [n, H + 2, W + 2, k]: one pixel of zeros around the map, channels zero-extended to k"""
    n, h, w, c = x.shape
    out = torch.zeros(n, h + 2, w + 2, k, dtype=F64)
    out[:, 1:-1, 1:-1, :c] = x
    return out


def contract(xp, op, h, w, c_off=None):
    """out[n, y, x, r] = sum_{tap, k} xp[n, y + ky, x + kx, c_off[r] + k] * op[r][tap][k]; op [rows][taps][K].  taps == 1: the centre.
    c_off (per operand row): first channel of the K window (block-diagonal tiles); None: 0"""
    rows, taps, kk = op.shape
    out = torch.zeros(xp.shape[0], h, w, rows, dtype=F64)
    for tap in range(taps):
        ky, kx = (tap // 3, tap % 3) if taps == 9 else (1, 1)
        win = xp[:, ky:ky + h, kx:kx + w]
        if c_off is None:
            out += win[..., :kk] @ op[:, tap, :].t()
        else:
            for r in range(rows):
                out[..., r] += win[..., c_off[r]:c_off[r] + kk] @ op[r, tap, :]
    return out


DENSE = [(1, 1, 1), (5, 3, 9), (33, 31, 1), (7, 13, 9), (40, 33, 9)]


@pytest.mark.parametrize("cout,cin,taps", DENSE)
def test_dense_operands_are_the_conv_and_its_data_gradient(cout, cin, taps):
    g = gen(f"dense{cout}x{cin}x{taps}")
    w = ints((cout, cin, taps), -4, 4, g)
    x = ints((2, 4, 5, cin), -3, 3, g)
    dz = ints((2, 4, 5, cout), -3, 3, g)
    wp, wt = P.dense(w)
    assert wp.shape == (cout, taps, P.kp(cin)) and wt.shape == (cin, taps, P.kp(cout))
    k = 3 if taps == 9 else 1
    xt = nchw(x).requires_grad_()
    y = F.conv2d(xt, w.reshape(cout, cin, k, k), padding=k // 2)
    (dx,) = torch.autograd.grad(y, xt, nchw(dz))
    assert torch.equal(contract(zero_pad(x, P.kp(cin)), wp, 4, 5), nhwc(y.detach()))
    # data gradient: dx[p][ci] = sum_{tap, co} dz[p - (tap - centre)][co] * wt[ci][tap][co]: the taps mirrored
    assert torch.equal(contract(zero_pad(dz, P.kp(cout)), wt.flip(1), 4, 5), nhwc(dx))
    # padding: +0.0 everywhere beyond the channel counts
    assert not wp[:, :, cin:].any() and not wt[:, :, cout:].any()
    assert not torch.signbit(wp[:, :, cin:]).any() and not torch.signbit(wt[:, :, cout:]).any()


def test_slice_is_dense_of_the_channel_range():
    w = P.coded(6, 20, 9)
    for ci0, cin in ((3, 13), (8, 12), (0, 20)):
        wp, wt = P.slice_(w, ci0, cin)
        assert wp.shape == (6, 9, 32) and wt.shape == (cin, 9, 32)
        for ci in range(cin):
            assert torch.equal(wp[:, :, ci], w[:, ci0 + ci, :].double()) and torch.equal(wt[ci, :, :6], w[:, ci0 + ci, :].double().t())


@pytest.mark.parametrize("c", [8, 24, 64, 72, 152])
def test_diag_operands_are_the_grouped_conv_and_its_data_gradient(c):
    g = gen(f"diag{c}")
    w = ints((c, 8, 3, 3), -4, 4, g)
    x = ints((1, 4, 5, c), -3, 3, g)
    dz = ints((1, 4, 5, c), -3, 3, g)
    wk, wd = P.diag(w)
    xt = nchw(x).requires_grad_()
    y = F.conv2d(xt, w, padding=1, groups=c // 8)
    (dx,) = torch.autograd.grad(y, xt, nchw(dz))
    ctile = (c + 63) // 64 * 64                                              # the last tile's missing channels read as zero
    off = [ch // 64 * 64 for ch in range(c)]
    assert torch.equal(contract(zero_pad(x, ctile), wk, 4, 5, off), nhwc(y.detach()))
    assert torch.equal(contract(zero_pad(dz, ctile), wd, 4, 5, off), nhwc(dx))   # (wd carries the mirrored taps itself)
    m = P.diag_mask(c)
    assert int(m.sum()) == c * 72 and not wk[~m].any() and not wd[~m].any()


def test_gconv_and_dw_operands():
    g = gen("gconv-dw")
    c = 24
    w = ints((c, 8, 3, 3), -4, 4, g)
    for flip in (0, 1):
        wk, wd = P.gconv(w, flip)
        for tap in range(9):
            for grp in range(c // 8):
                blk = w[grp * 8:grp * 8 + 8, :, tap // 3, tap % 3]             # [o][i]
                assert torch.equal(wk[tap, :, grp, :], blk.t())                # wk[tap][i][G][o]
                assert torch.equal(wd[8 - tap if flip else tap, :, grp, :], blk)   # wd[tap'][o][G][i]
    wdw = ints((c, 1, 3, 3), -4, 4, g)
    wk, wkf = P.dw(wdw)
    x = ints((1, 4, 5, c), -3, 3, g)
    y = F.conv2d(nchw(x), wdw, padding=1, groups=c)
    xp = zero_pad(x, c)
    acc = sum(xp[:, t // 3:t // 3 + 4, t % 3:t % 3 + 5] * wk[t] for t in range(9))
    assert torch.equal(acc, nhwc(y))
    assert all(torch.equal(wkf[8 - t], wk[t]) for t in range(9))


@pytest.mark.parametrize("k,ctot,ci0,c0", [(5, 3, 0, 3), (2, 12, 0, 8), (3, 12, 4, 8)])
def test_phase_form_is_upsample_reflect_pad_conv(k, ctot, ci0, c0):
    g = gen(f"phase{k}x{ctot}")
    w = ints((k, ctot, 3, 3), -4, 4, g)
    bias = ints((k,), -5, 5, g)
    x = ints((2, 5, 6, c0), -3, 3, g)
    wp, wt, be = P.phase(w, c0, bias, ci0)
    assert wp.shape == (4 * k, 9, P.kp(c0)) and wt.shape == (c0, 9, P.kp(4 * k)) and be.shape == (4 * k,)
    up = F.interpolate(nchw(x), scale_factor=2, mode="nearest")
    want = nhwc(F.conv2d(F.pad(up, (1, 1, 1, 1), mode="reflect"), w[:, ci0:ci0 + c0], bias))          # [2, 10, 12, k]
    clamp = torch.zeros(2, 7, 8, P.kp(c0), dtype=F64)
    clamp[..., :c0] = S.pad1(x, "clamp")
    got = S.depth_to_space(contract(clamp, wp, 5, 6) + be)
    assert torch.equal(got, want)
    # wt is the same effective tensor transposed
    assert torch.equal(wt[:, :, :4 * k], wp[:, :, :c0].permute(2, 1, 0)) and not wt[:, :, 4 * k:].any()


def test_levels_layout():
    n, hs, ws = 2, (5, 3, 2, 1), (7, 4, 2, 1)
    srcs = [torch.arange(n * h * w * 8, dtype=torch.int16).reshape(-1, 8) + 1000 * l for l, (h, w) in enumerate(zip(hs, ws))]
    for align in (1, 128):
        out = P.levels(srcs, n, hs, ws, align, -1, ldd=16)
        rows = [n * h * w for h, w in zip(hs, ws)]
        assert out.shape[0] == sum((r + align - 1) // align * align for r in rows)
        at = 0
        for l, r in enumerate(rows):
            assert at % align == 0 and torch.equal(out[at:at + r, :8], srcs[l]) and bool((out[at:at + r, 8:] == -1).all())
            pad = (r + align - 1) // align * align
            assert bool((out[at + r:at + pad] == -1).all())
            at += pad


def test_rounding_restatement_is_torch_bf16():
    rs = P.rounding_set()
    assert rs.numel() == 2 * 3 * 5 * 6 + 2 and bool(torch.isfinite(rs).all())
    want = rs.to(BF16).view(torch.int16)
    assert torch.equal(P.rne_bits(rs), want)
    assert torch.equal(P.bits(rs.double()), want)
    # the set takes every branch: exact, round down, tie to even both ways, round up, and a carry into the exponent
    b = rs.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    hi, lo, out = b >> 16, b & 0xFFFF, want.to(torch.int64) & 0xFFFF
    assert bool(((lo == 0x8000) & (hi & 1 == 0) & (out == hi)).any())                  # tie, even stays
    assert bool(((lo == 0x8000) & (hi & 1 == 1) & (out == hi + 1)).any())              # tie, odd goes up
    assert bool(((lo == 0x7FFF) & (out == hi)).any()) and bool(((lo == 0x8001) & (out == hi + 1)).any())
    assert bool((((hi & 0x7F) == 0x7F) & (out == hi + 1)).any())                       # mantissa overflow -> next exponent
    assert bool((b == 0x80000000).any()) and int(want[b == 0x80000000][0]) == -0x8000  # -0 keeps its sign
    # random normals as well
    x = torch.randn(4096, generator=gen("rne"))
    assert torch.equal(P.rne_bits(x), x.to(BF16).view(torch.int16))
    # coded integers and dyadic phase sums need / survive rounding as the GPU test assumes
    assert torch.equal(P.coded(9, 7, 9).to(BF16).float(), P.coded(9, 7, 9))
