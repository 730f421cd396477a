"""The float64 oracle of the seg-head conv forms and NT epilogue options (tests/seg_conv_ref.py) held to plain torch at tiny shapes, bit for
bit on integer data (every sum is far below 2^53: float64 is exact in any order).  Pins the oracle the exact GPU files use without a
GPU."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests import seg_conv_ref as R

F64 = torch.float64


def ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def up_conv(x, w, b):
    """Conv3x3(ReflectionPad2d(1)(nearest_up2(x))), x NHWC -> NHWC"""
    u = F.interpolate(nchw(x), scale_factor=2, mode="nearest")
    return nhwc(F.conv2d(F.pad(u, [1, 1, 1, 1], mode="reflect"), w, b))


SHAPES = [(1, 1, 1), (2, 3, 5), (1, 4, 4), (2, 2, 7)]


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_phase_forward_is_the_upsampled_reflect_conv(n, h, w):
    k, c = 3, 4
    x, wt, b = ints((n, h, w, c), -3, 3, 1), ints((k, c, 3, 3), -2, 2, 2), ints((k,), -4, 4, 3)
    assert torch.equal(R.phase_forward_pre(x, wt, b), up_conv(x, wt, b))
    add = ints((n, 2 * h, 2 * w, k), -5, 5, 4)
    assert torch.equal(R.phase_forward_pre(x, wt, b, addend=add), up_conv(x, wt, b) + add)
    # a channel slice (the skip operand's channels are not part of the phase form)
    assert torch.equal(R.phase_forward_pre(x[..., :2], wt, b, c0=2), up_conv(x[..., :2], wt[:, :2].contiguous(), b))
    we, be = R.phase_weights(wt, b)
    assert we.shape == (4 * k, c, 3, 3) and torch.equal(be, b.repeat(4))
    # every effective weight is a sum of at most 4 taps, and every tap lands on exactly one effective tap per phase
    assert torch.equal(we.view(4, k, c, 9).sum(3), wt.view(k, c, 9).sum(2).expand(4, k, c))
    z = ints((n, h, w, 4 * k), -3, 3, 5)
    assert torch.equal(R.space_to_depth(R.depth_to_space(z)), z)
    assert torch.equal(R.elu(torch.tensor([-2.0, 0.0, 3.0], dtype=F64)), F.elu(torch.tensor([-2.0, 0.0, 3.0], dtype=F64)))


@pytest.mark.parametrize("kind", ["reflect", "clamp"])
def test_conv3x3_is_the_padded_conv(kind):
    x, wt = ints((2, 4, 5, 3), -3, 3, 6), ints((5, 3, 3, 3), -2, 2, 7)
    ref = nhwc(F.conv2d(F.pad(nchw(x), [1, 1, 1, 1], mode="reflect" if kind == "reflect" else "replicate"), wt))
    assert torch.equal(R.conv3x3(x, wt, kind), ref)


@pytest.mark.parametrize("n,h,w", [(1, 4, 4), (2, 4, 6), (1, 5, 7)])
def test_folds_are_the_autograd_gradients(n, h, w):
    k, c = 2, 3
    wt, b = ints((k, c, 3, 3), -2, 2, 8), ints((k,), -1, 1, 9)
    # clamp = 0: the gradient of the reflect-padded conv at this resolution
    x = ints((n, h, w, c), -3, 3, 10).requires_grad_(True)
    dz = ints((n, h, w, k), -3, 3, 11)
    y = nhwc(F.conv2d(F.pad(nchw(x), [1, 1, 1, 1], mode="reflect"), wt, b))
    gx, = torch.autograd.grad(y, x, dz)
    dvp = R.dgrad_padded(dz, wt)
    assert dvp.shape == (n, h + 2, w + 2, c)
    assert torch.equal(R.fold(dvp, 0), gx)
    # clamp = 1: the phase form -- the gradient of the up-sampled reflect conv w.r.t. the LOW-resolution input
    xl = ints((n, h, w, c), -3, 3, 12).requires_grad_(True)
    dzf = ints((n, 2 * h, 2 * w, k), -3, 3, 13)
    gl, = torch.autograd.grad(up_conv(xl, wt, b), xl, dzf)
    we, _ = R.phase_weights(wt, b)
    dvl = R.dgrad_padded(R.space_to_depth(dzf), we)
    assert torch.equal(R.fold(dvl, 1), gl)
    # ... and of the replicate-padded low-resolution conv with the effective weights
    xr = xl.detach().clone().requires_grad_(True)
    yr = nhwc(F.conv2d(F.pad(nchw(xr), [1, 1, 1, 1], mode="replicate"), we))
    gr, = torch.autograd.grad(yr, xr, R.space_to_depth(dzf))
    assert torch.equal(R.fold(dvl, 1), gr)
    # with the producer's ELU: gradient through y = elu(x'), ELU' taken from the output
    yprev = torch.tensor([2, 0.5, 0, -0.25, -0.5, -0.75, -1], dtype=F64)[ints((n, h, w, c), 0, 6, 14).long()]
    for clamp, d in ((0, dvp), (1, dvl)):
        dx, stages = R.fold_staged(d, clamp, yprev)
        assert torch.equal(dx, R.fold(d, clamp) * R.elu_grad_factor(yprev))
        assert [s[0] for s in stages] == ["accumulator", "interior * ELU'", "ring sum * ELU'", "folded value"]
        dx0, st0 = R.fold_staged(d, clamp)
        assert torch.equal(dx0, R.fold(d, clamp)) and len(st0) == 2
    pre = torch.tensor([3.0, 0.0, -1.5], dtype=F64, requires_grad=True)
    out = F.elu(pre)
    assert torch.allclose(R.elu_grad_factor(out.detach()), torch.autograd.grad(out.sum(), pre)[0], rtol=0, atol=1e-15)
    # space-to-depth order of the folded gradient
    if h % 2 == 0 and w % 2 == 0:
        s = R.space_to_depth(gx)
        for yy, xx in itertools.product(range(h), range(w)):
            ch = ((yy & 1) * 2 + (xx & 1)) * c
            assert torch.equal(s[:, yy // 2, xx // 2, ch:ch + c], gx[:, yy, xx])


def test_ring_layout_and_counts():
    n, h, w, c = 2, 4, 5, 2
    dvp = ints((n, h + 2, w + 2, c), -3, 3, 15)
    ring = R.ring_rows(dvp)
    assert ring.shape == (n, 2 * (w + 2) + 2 * h, c)
    assert torch.equal(ring[:, 3], dvp[:, 0, 3]) and torch.equal(ring[:, (w + 2) + 6], dvp[:, h + 1, 6])
    assert torch.equal(ring[:, 2 * (w + 2) + 2], dvp[:, 3, 0]) and torch.equal(ring[:, 2 * (w + 2) + h + 1], dvp[:, 2, w + 1])
    for clamp in (0, 1):
        cnt = R.ring_count(h, w, clamp, dvp.device)
        assert int(cnt.sum()) == 2 * (w + 2) + 2 * h                      # every ring position lands on exactly one pixel
        r0, r1, c0, c1 = (0, h - 1, 0, w - 1) if clamp else (1, h - 2, 1, w - 2)
        assert int(cnt[r0, c0]) == 3 and int(cnt[r1, c1]) == 3 and int(cnt[r0, 2]) == 1
        assert int((cnt > 0).sum()) == 2 * w + 2 * (h - 2)                 # the border targets of seg_ring_fix_kernel
    # 4 x 4: 12 of the 16 pixels are border targets either way (clamp: all but the inner 2 x 2; reflect: all but the four image corners)
    assert R.ring_count(4, 4, 1, dvp.device).tolist() == [[3, 1, 1, 3], [1, 0, 0, 1], [1, 0, 0, 1], [3, 1, 1, 3]]
    assert R.ring_count(4, 4, 0, dvp.device).tolist() == [[0, 1, 1, 0], [1, 3, 3, 1], [1, 3, 3, 1], [0, 1, 1, 0]]


def test_row_mappings_are_the_concatenation_of_per_level_results():
    n, c, nout = 3, 4, 5
    wt = ints((nout, c), -2, 2, 16)
    # lvl: per-level coefficients
    rows = (8, 4, 4)
    x = ints((sum(rows), c), -3, 3, 17)
    coef = ints((len(rows), nout), 1, 3, 18)
    lev = R.level_of_rows(rows, x.device)
    got = (x @ wt.t()) * coef[lev]
    want = torch.cat([(xl @ wt.t()) * coef[l] for l, xl in enumerate(x.split(rows))])
    assert torch.equal(got, want)
    # imgw: one weight matrix per image
    wn = ints((n, nout, c), -2, 2, 19)
    xi = ints((n * 4, c), -3, 3, 20)
    img = R.image_of_rows(n * 4, 4, xi.device)
    got = torch.einsum("mc,moc->mo", xi, wn[img])
    assert torch.equal(got, torch.cat([xi[4 * i:4 * i + 4] @ wn[i].t() for i in range(n)]))
    # rpi / img_stride: image i's rows at i * img_stride
    ldc, stride = nout + 2, 4 * (nout + 2) + 7
    buf = torch.full((n * stride,), -99.0, dtype=F64)
    off = R.rpi_offsets(n * 4, 4, stride, ldc, xi.device)
    for j in range(nout):
        buf[off + j] = got[:, j]
    for i in range(n):
        assert torch.equal(buf[i * stride:i * stride + 4 * ldc].view(4, ldc)[:, :nout], xi[4 * i:4 * i + 4] @ wn[i].t())
    # lvlout: level-packed rows with alignment rows -> per-image concatenation of the levels
    hs, ws, align = (2, 1), (3, 2), 4
    m, lv, im, px, real = R.lvlout_rows(n, hs, ws, align, xi.device)
    assert m == 20 + 8 and int(real.sum()) == n * (6 + 2)
    xs = ints((m, c), -3, 3, 21)
    res = xs @ wt.t()
    per_level = [res[:20][:18].view(n, 6, nout), res[20:][:6].view(n, 2, nout)]
    want = torch.cat(per_level, 1)                                         # [n][sum_l H_l W_l][nout]
    ldc, stride = nout + 1, 8 * (nout + 1) + 3
    off = R.lvlout_offsets(n, hs, ws, align, stride, ldc, xi.device)
    buf = torch.full((n * stride,), -99.0, dtype=F64)
    for j in range(nout):
        buf[off[real] + j] = res[real][:, j]
    assert torch.equal(buf.view(n, stride)[:, :8 * ldc].reshape(n, 8, ldc)[:, :, :nout], want)
    assert int((buf != -99).sum()) == want.numel() and bool((off[~real] == -1).all())


def test_statistics_epilogues_are_the_comment_blocks_definitions():
    m, c, tile = 11, 3, 4
    q, z, ey = ints((m, c), -3, 3, 22), ints((m, c), -2, 2, 23), ints((m, c), -1, 1, 24)
    coef = torch.stack([torch.tensor([2.0, -0.5, 1.0]), ints((c,), -1, 1, 25), ints((c,), -1, 1, 26), torch.tensor([0.5, 2.0, 4.0])]).double()
    for emode in range(4):
        t1, t2 = R.estat_terms(emode, q, z, coef, ey)
        for r in range(R.cdiv(m, tile)):
            s1, s2 = torch.zeros(c, dtype=F64), torch.zeros(c, dtype=F64)
            for i in range(r * tile, min(m, (r + 1) * tile)):
                for j in range(c):
                    pre = float(coef[0, j] * z[i, j] + coef[1, j])
                    xh = float((z[i, j] - coef[2, j]) * coef[3, j])
                    qq = float(q[i, j])
                    if emode == 0:
                        a, b = qq, qq * qq
                    elif emode == 1:
                        a, b = qq * max(pre, 0.0), 0.0
                    elif emode == 2:
                        a, b = (qq, qq * xh) if pre > 0 else (0.0, 0.0)
                    else:
                        a, b = (qq, qq * xh) if float(ey[i, j]) > 0 else (0.0, 0.0)
                    s1[j] += a
                    s2[j] += b
            assert torch.equal(R.tile_sums(t1, tile)[r], s1)
            if t2 is not None:
                assert torch.equal(R.tile_sums(t2, tile)[r], s2)
        assert (t2 is None) == (emode == 1)
    v = ints((2, 17, 18, 2), -3, 3, 27)
    ps = R.patch_sums(v)
    assert ps.shape == (2 * 2 * 2, 2)
    assert torch.equal(ps[0], v[0, :16, :16].sum((0, 1))) and torch.equal(ps[3], v[0, 16:, 16:].sum((0, 1))) and torch.equal(ps[5], v[1, :16, 16:].sum((0, 1)))


def test_elu_of_negative_integers_is_far_from_a_bf16_rounding_boundary():
    """the phase-forward cases demand bit equality through ELU: pre-activations are integers, the negative branch takes only the values
    expm1(-j), and the device's __expf(x) - 1 is accurate to ~1e-7 there -- so every such value must lie at least 2^-12 away (relative
    to its own magnitude: a bf16 ulp at [0.5, 1) is 2^-8) from the midpoint of two bf16 neighbours"""
    j = torch.arange(1, 200, dtype=F64)
    assert R.elu_margin(-j) >= 2.0 ** -12
