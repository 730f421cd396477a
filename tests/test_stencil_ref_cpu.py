"""Holds tests/stencil_ref.py (the float64 reference of the exact stencil tests) to torch's own float64 operators on the CPU, the max-pool
tie rule to a brute-force loop, the dispatch restatements to the library's host-side queries, and a few argument refusals of the stencil
entry points (they return before any launch, so no device is needed)."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests import stencil_ref as R

F64 = torch.float64
RTOL = 1e-12


def rnd(*shape, seed=0):
    g = torch.Generator()
    g.manual_seed(seed + sum(shape) * 131 + len(shape))
    return torch.randn(*shape, generator=g, dtype=F64)


def close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max()) if got.numel() else 0.0
    scale = max(float(want.abs().max()), 1e-300) if want.numel() else 1.0
    assert err <= RTOL * scale, f"{what}: max |err| {err:.3e} against max |ref| {scale:.3e}"


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


SIZES = [(2, 2), (2, 3), (3, 2), (3, 3), (4, 4), (4, 5), (5, 4), (5, 5), (7, 9), (1, 1), (6, 10)]


STEM_SIZES = [(2, 2), (2, 4), (4, 2), (16, 24), (18, 22), (34, 68), (7, 10), (10, 7), (5, 5), (3, 2)]


@pytest.mark.parametrize("hw", STEM_SIZES)
def test_stem_against_torch(hw):
    """even sizes: conv2d(stride 2, padding 1) itself.  Odd sizes: `H >> 1` drops conv2d's last row / column, keeps the others unchanged
    and never reads the frame's last row / column (stencil_ref.stem_out_hw)"""
    h, w = hw
    n = 2
    x, wt = rnd(n, 3, h, w), rnd(32, 3, 3, 3, seed=1)
    y = F.conv2d(x, wt, stride=2, padding=1)
    ho, wo = R.stem_out_hw(h, w)
    assert (ho, wo) == (h // 2, w // 2) and y.shape[2:] == ((h + 1) // 2, (w + 1) // 2)
    z = R.stem(x, wt)
    assert z.shape == (n, ho, wo, 32)
    close(z, nhwc(y[:, :, :ho, :wo]), "stem")
    if h % 2 or w % 2:
        x2 = x.clone()
        if h % 2:
            x2[:, :, h - 1, :] = 1e6
        if w % 2:
            x2[:, :, :, w - 1] = 1e6
        assert torch.equal(R.stem(x2, wt), z), "the last row / column of an odd frame is read"
    # patches: the unfold of the frame, tap ci * 9 + ky * 3 + kx, and z = patches . w
    p = R.stem_patches(x)
    u = F.unfold(x, 3, padding=1, stride=2).reshape(n, 27, (h + 1) // 2, (w + 1) // 2)[:, :, :ho, :wo]
    assert torch.equal(p[..., :27], u.permute(0, 2, 3, 1)) and float(p[..., 27:].abs().sum()) == 0
    close(p[..., :27] @ wt.reshape(32, 27).t(), z, "patches . w")


def test_stem_store_paths():
    """which pixels leave through LDS, for the shapes of the GPU test"""
    assert not bool(R.stem_lds_path(2, 16, 24).any())                     # 96 pixel pairs: a partial block only
    assert bool(R.stem_lds_path(2, 64, 128).all())                        # 2048 pairs: eight whole blocks
    m = R.stem_lds_path(1, 34, 68)                                        # 289 pairs: one whole block and a tail of 33
    assert int(m.sum()) == 512 and int((~m).sum()) == 17 * 34 - 512 and bool(m.reshape(-1)[:512].all())
    assert not bool(R.stem_lds_path(3, 18, 22).any())                     # odd Wo = 11: thread-owned rows, every row ends in a lone pixel
    assert R.stem_lds_path(1, 2, 2).shape == (1, 1, 1)
    assert not bool(R.stem_lds_path(6, 32, 22).any()) and 6 * 16 * 6 >= 512   # odd Wo with whole blocks: still thread-owned


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("c", [8, 24])
def test_gconv_against_torch(hw, c, stride):
    h, w = hw
    if stride == 2 and (h % 2 or w % 2):
        h, w = h + h % 2, w + w % 2                                  # the stride-2 kernels take even maps
    n = 2
    x = rnd(n, h, w, c).requires_grad_()
    wt = rnd(c, 8, 3, 3, seed=1).requires_grad_()
    y = F.conv2d(nchw(x), wt, stride=stride, padding=1, groups=c // 8)
    if stride == 2:
        y = y[:, :, :h // 2, :w // 2]
    dz = rnd(*nhwc(y).shape, seed=2)
    gx, gw = torch.autograd.grad(y, (x, wt), nchw(dz))
    close(R.gconv(x.detach(), wt.detach(), stride), nhwc(y.detach()), "gconv")
    close(R.gconv_dgrad(dz, wt.detach(), stride, h, w), gx, "gconv_dgrad")
    close(R.gconv_wgrad(x.detach(), dz, stride), gw, "gconv_wgrad")


@pytest.mark.parametrize("hw", SIZES)
def test_dwconv_against_torch(hw):
    h, w = hw
    n, c = 2, 16
    x = rnd(n, h, w, c).requires_grad_()
    wt = rnd(c, 1, 3, 3, seed=1).requires_grad_()
    y = F.conv2d(nchw(x), wt, padding=1, groups=c)
    dz = rnd(n, h, w, c, seed=2)
    gx, gw = torch.autograd.grad(y, (x, wt), nchw(dz))
    close(R.dwconv(x.detach(), wt.detach()), nhwc(y.detach()), "dwconv")
    close(R.dwconv_dgrad(dz, wt.detach()), gx, "dwconv_dgrad")
    close(R.dwconv_wgrad(x.detach(), dz), gw[:, 0], "dwconv_wgrad")


@pytest.mark.parametrize("row_align", [1, 7, 128])
def test_level_wrappers(row_align):
    n, c, hs, ws = 2, 8, (5, 3, 2, 1), (4, 3, 5, 1)
    off = R.row_offsets(n, hs, ws, row_align)
    assert all(o % row_align == 0 for o in off) and off[1] >= n * 20
    pad = R.alignment_rows(n, hs, ws, row_align)
    assert pad.numel() == off[-1] and int((~pad).sum()) == sum(n * h * w for h, w in zip(hs, ws))
    x, dz, wt = rnd(off[-1], c), rnd(off[-1], c, seed=1), rnd(c, 3, 3, seed=2)
    prev = rnd(off[-1], c, seed=3)
    for acc in (False, True):
        y = R.dwconv_levels(x, wt, n, hs, ws, row_align, prev if acc else None)
        dx = R.dwconv_dgrad_levels(dz, wt, n, hs, ws, row_align, prev if acc else None)
        for l, (h, w) in enumerate(zip(hs, ws)):
            rows = slice(off[l], off[l] + n * h * w)
            base = prev[rows].reshape(n, h, w, c) if acc else 0
            close(y[rows].reshape(n, h, w, c), R.dwconv(x[rows].reshape(n, h, w, c), wt) + base, f"dwconv_levels level {l}")
            close(dx[rows].reshape(n, h, w, c), R.dwconv_dgrad(dz[rows].reshape(n, h, w, c), wt) + base, f"dwconv_dgrad_levels level {l}")
        assert torch.equal(y[pad], prev[pad] if acc else torch.zeros_like(y[pad]))
        assert torch.equal(dx[pad], prev[pad] if acc else torch.zeros_like(dx[pad]))
    dw = R.dwconv_wgrad_levels(x, dz, n, hs, ws, row_align)
    want = sum(R.dwconv_wgrad(x[off[l]:off[l] + n * h * w].reshape(n, h, w, c), dz[off[l]:off[l] + n * h * w].reshape(n, h, w, c))
               for l, (h, w) in enumerate(zip(hs, ws)))
    close(dw, want, "dwconv_wgrad_levels")
    # junk in the alignment rows of the inputs changes nothing
    x2, dz2 = x.clone(), dz.clone()
    x2[pad] = 1e6
    dz2[pad] = -1e6
    assert torch.equal(R.dwconv_levels(x2, wt, n, hs, ws, row_align), R.dwconv_levels(x, wt, n, hs, ws, row_align))
    assert torch.equal(R.dwconv_wgrad_levels(x2, dz2, n, hs, ws, row_align), dw)


def torch_pool(x, mode):
    xc = nchw(x)
    if mode == 0:
        return F.max_pool2d(F.pad(xc, (0, 1, 0, 1)), 3, 2)
    return F.max_pool2d(xc, 3, 2, 1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hw", [(2, 2), (2, 4), (4, 2), (4, 6), (6, 4), (8, 10)])
def test_maxpool_against_torch(hw, mode):
    h, w = hw
    x = rnd(2, h, w, 8).requires_grad_()
    y = torch_pool(x, mode)
    dout = rnd(2, h // 2, w // 2, 8, seed=1)
    gx, = torch.autograd.grad(y, x, nchw(dout))
    v, a = R.maxpool(x.detach(), mode)
    close(v, nhwc(y.detach()), "maxpool values")
    assert a.dtype == torch.uint8 and int(a.max()) <= 9
    close(R.maxpool_bwd(a, dout, None, h, w, mode), gx, "maxpool_bwd")
    close(R.maxpool_bwd(a, dout, 0.5, h, w, mode), 0.5 * gx, "maxpool_bwd wscale")


def brute_pool(x, mode):
    n, h, w, c = x.shape
    val = torch.zeros(n, h // 2, w // 2, c, dtype=F64)
    arg = torch.zeros(n, h // 2, w // 2, c, dtype=torch.uint8)
    for b, oy, ox, ch in itertools.product(range(n), range(h // 2), range(w // 2), range(c)):
        best, at = float("-inf"), 255
        for t in range(9):
            iy, ix = 2 * oy + t // 3 - mode, 2 * ox + t % 3 - mode
            ins = 0 <= iy < h and 0 <= ix < w
            if not ins and mode == 1:
                continue
            f = float(x[b, iy, ix, ch]) if ins else 0.0
            if f > best:
                best, at = f, (t if ins else 9)
        val[b, oy, ox, ch], arg[b, oy, ox, ch] = best, at
    return val, arg


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hw", [(2, 2), (4, 6), (6, 4)])
def test_maxpool_ties_against_brute_force(hw, mode):
    g = torch.Generator()
    g.manual_seed(hw[0] * 10 + hw[1] + mode)
    x = torch.randint(-1, 2, (2, hw[0], hw[1], 3), generator=g).to(F64)
    x[0, :, :, 0] = -1                                               # all negative: in mode 0 the border windows pick the zero pad
    v, a = R.maxpool(x, mode)
    bv, ba = brute_pool(x, mode)
    assert torch.equal(v, bv)
    assert torch.equal(a, ba)
    if mode == 0:
        assert int((a == 9).sum()) > 0, "no window picked the zero pad: the case does not exercise arg 9"
    dout = torch.randint(-3, 4, v.shape, generator=g).to(F64)
    dx = R.maxpool_bwd(a, dout, None, hw[0], hw[1], mode)
    want = torch.zeros_like(x)
    for b, oy, ox, ch in itertools.product(range(2), range(hw[0] // 2), range(hw[1] // 2), range(3)):
        t = int(ba[b, oy, ox, ch])
        if t < 9:
            want[b, 2 * oy + t // 3 - mode, 2 * ox + t % 3 - mode, ch] += dout[b, oy, ox, ch]
    assert torch.equal(dx, want)


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 4)])
def test_up2_sum2x2_against_torch(hw):
    x = rnd(2, hw[0], hw[1], 8).requires_grad_()
    y = F.interpolate(nchw(x), scale_factor=2, mode="nearest")
    g = rnd(2, 2 * hw[0], 2 * hw[1], 8, seed=1)
    gx, = torch.autograd.grad(y, x, nchw(g))
    close(R.up2(x.detach()), nhwc(y.detach()), "up2")
    close(R.sum2x2(g), gx, "sum2x2")
    close(R.sum2x2(g, 0.25), 0.25 * gx, "sum2x2 wscale")


@pytest.mark.parametrize("modes", [(1, 2, 0), (1, 0, 2), (1, 2, 1), (1, 1, 3), (1, 3, 0), (3, 1, 2)])
def test_fuse_against_torch(modes):
    n, h, w, c = 2, 4, 6, 8
    shape = {1: (n, h, w, c), 2: (n, h // 2, w // 2, c), 3: (n, 2 * h, 2 * w, c)}
    ins = [None if m == 0 else rnd(*shape[m], seed=i).requires_grad_() for i, m in enumerate(modes)]
    wv = torch.tensor([0.5, 0.3, 0.2], dtype=F64).requires_grad_()
    terms = []
    for x, m in zip(ins, modes):
        terms.append(None if m == 0 else x if m == 1 else nhwc(F.interpolate(nchw(x), scale_factor=2, mode="nearest")) if m == 2
                     else nhwc(torch_pool(x, 0)))
    pre = sum(wv[i] * t for i, t in enumerate(terms) if t is not None)
    out = pre * torch.sigmoid(pre)
    dout = rnd(n, h, w, c, seed=9)
    live = [x for x in ins if x is not None]
    grads = torch.autograd.grad(out, live + [wv, pre], dout)
    det = [None if x is None else x.detach() for x in ins]
    p, o = R.fuse_fwd(det, modes, wv.detach())
    close(p, pre.detach(), "fuse_fwd pre")
    close(o, out.detach(), "fuse_fwd out")
    b = R.fuse_bwd(det, modes, wv.detach(), dout)
    close(b["g"], grads[-1], "fuse_bwd g")
    k = 0
    for i, m in enumerate(modes):
        if m == 0:
            assert b["din"][i] is None
            continue
        close(b["din"][i], grads[k], f"fuse_bwd din[{i}] (mode {m})")
        k += 1
    close(b["dw"], grads[-2], "fuse_bwd dw")


def test_swish_grad_against_autograd():
    x = rnd(1000).requires_grad_()
    g, = torch.autograd.grad((x * torch.sigmoid(x)).sum(), x)
    close(R.swish_grad(x.detach()), g, "swish'")


@pytest.mark.parametrize("praw,nw", [([1.0, 0.5, 2.0], 3), ([1.0, -0.5, 2.0], 3), ([0.7, 1.3, 5.0], 2)])
def test_fuse_weights_against_autograd(praw, nw):
    eps = 1e-4
    p = torch.tensor(praw, dtype=F64).requires_grad_()
    r = torch.relu(p[:nw])
    wn = r / (r.sum() + eps)
    dw = torch.tensor([0.3, -1.1, 0.8], dtype=F64)
    gp, = torch.autograd.grad((wn * dw[:nw]).sum(), p)
    close(R.fuse_weights(p.detach(), nw, eps)[:nw], wn.detach(), "fuse_weights")
    assert float(R.fuse_weights(p.detach(), nw, eps)[nw:].abs().sum()) == 0
    close(R.fuse_dweights(dw, p.detach(), nw, eps), gp[:nw], "fuse_dweights")


FOLD_CASES = [(hw, up) for up in (0, 1, 2) for hw in [(4, 4), (5, 7), (4, 6), (6, 5), (16, 12)]
              if not (up == 1 and (hw[0] % 2 or hw[1] % 2))]                # the 2x2-summed fold needs an even map


@pytest.mark.parametrize("hw,up", FOLD_CASES)
def test_seg_fold_against_torch(hw, up):
    h, w = hw
    n, c, c0, ldv = 2, 8, 8, 24
    dvp = rnd(n, h + 2, w + 2, ldv)
    pad = torch.nn.ReplicationPad2d(1) if up == 2 else torch.nn.ReflectionPad2d(1)
    if up == 1:
        src = rnd(n, h // 2, w // 2, c, seed=1).requires_grad_()
        y = pad(F.interpolate(nchw(src), scale_factor=2, mode="nearest"))
    else:
        src = rnd(n, h, w, c, seed=1).requires_grad_()
        y = pad(nchw(src))
    g, = torch.autograd.grad(y, src, nchw(dvp[..., c0:c0 + c]))
    close(R.seg_fold(dvp, c0, c, h, w, up), g, f"seg_fold up={up}")
    pre = rnd(*g.shape, seed=3).requires_grad_()
    e = F.elu(pre)
    ge, = torch.autograd.grad(e, pre, g)
    close(R.seg_fold(dvp, c0, c, h, w, up, e.detach()), ge, f"seg_fold up={up} with ELU'")


def test_pad_index():
    assert R.pad_index(4, False).tolist() == [1, 0, 1, 2, 3, 2]
    assert R.pad_index(4, True).tolist() == [0, 0, 1, 2, 3, 3]


@pytest.mark.parametrize("k,ldo", [(5, 24), (8, 32), (3, 16)])
def test_space_to_depth_against_torch(k, ldo):
    n, h, w = 2, 3, 5
    dy = rnd(n, 2 * h, 2 * w, k)
    # pixel_unshuffle gives channel o*4 + py*2 + px; the kernels' layout is (py*2+px)*k + o
    pu = F.pixel_unshuffle(nchw(dy), 2).reshape(n, k, 4, h, w).permute(0, 3, 4, 2, 1).reshape(n, h, w, 4 * k)
    got = R.space_to_depth(dy, k, ldo)
    close(got[..., :4 * k], pu, "space_to_depth")
    assert float(got[..., 4 * k:].abs().sum()) == 0
    s2, sums = R.space_to_depth_sums(dy, k)
    close(s2, pu, "space_to_depth (bf16 form)")
    close(sums, pu.reshape(-1, 4, k).sum((0, 1)), "per-channel sums")


def test_head_grad_against_indexing():
    n, hs, ws, lds, nout, ldz = 2, (3, 2), (4, 1), 12, 5, 8
    rows = sum(h * w for h, w in zip(hs, ws))
    dy, y = rnd(n, rows, lds), torch.sigmoid(rnd(n, rows, lds, seed=1))
    for sig in (False, True):
        full = dy * (y * (1 - y)) if sig else dy
        got = R.head_grad(dy, y, rows, rows * lds, lds, nout, ldz, n * rows, sig)
        close(got[:, :nout], full.reshape(n * rows, lds)[:, :nout], "head_grad")
        assert float(got[:, nout:].abs().sum()) == 0
        prev = rnd(R.row_offsets(n, hs, ws, 16)[-1], ldz, seed=2)
        lv = R.head_grad_levels(dy, y, rows * lds, lds, nout, ldz, n, hs, ws, 16, sig, prev)
        off, p0 = R.row_offsets(n, hs, ws, 16), 0
        for l, (h, w) in enumerate(zip(hs, ws)):
            want = full[:, p0:p0 + h * w, :nout].reshape(n * h * w, nout)
            close(lv[off[l]:off[l] + n * h * w, :nout], want, f"head_grad_levels level {l}")
            p0 += h * w
        pad = R.alignment_rows(n, hs, ws, 16)
        assert torch.equal(lv[pad], prev[pad])


def test_bf16_rne_ties():
    v = torch.tensor([255.0, 256.0, 257.0, 258.0, 259.0, 261.0, -257.0, -259.0], dtype=F64)
    assert R.bf16_rne(v).tolist() == [255.0, 256.0, 256.0, 258.0, 260.0, 260.0, -256.0, -260.0]


# ---- dispatch restatements against the library's own host-side queries ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib.lib()


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def test_wgrad_chunks_mirror(lib):
    for pixels, items in itertools.product((1, 16, 63, 64, 65, 2048, 2049, 100000, 1 << 20, 1 << 26), (9, 27, 189, 198, 1053, 300000)):
        assert R.wgrad_chunks(pixels, items) == lib.query("hn_wgrad_chunks", pixels, items), (pixels, items)
    assert R.gconv_wgrad_plan(1, 4, 4, 8, 1) == ("strip", 1, 16)
    assert R.gconv_wgrad_plan(2, 32, 32, 24, 1)[0] == "sub"
    assert R.gconv_s2_lds(168) and not R.gconv_s2_lds(176)


def test_dwconv_block_mirrors(lib):
    for strips, c in itertools.product((1, 2, 7, 100, 513, 4096, 70000, 1 << 20), (8, 16, 88, 112, 256, 736, 1024, 2048)):
        assert R.dwconv_wgrad_blocks(strips, c) == lib.query("hn_dwconv_wgrad_blocks", strips, c), (strips, c)
        if c <= 1024:
            assert R.dwconv_bwd_strip_blocks(strips, c) == lib.query("hn_dwconv_bwd_blocks", strips, c), (strips, c)
    geoms = [(4, (60,), (90,)), (4, (64, 32, 16, 8, 4), (128, 64, 32, 16, 8)), (1, (20, 10, 5, 3, 2), (20, 10, 5, 3, 2)), (16, (64,), (128,)),
             (4, (60,), (66,)), (7, (64,), (144,)), (3, (5,), (5,)), (4, (57,), (256,)), (2, (128,), (256,))]
    forms = set()
    for (n, hs, ws), c in itertools.product(geoms, (8, 24, 88, 112, 128, 136, 256, 736)):
        form, blocks = R.dwconv_bwd_plan(n, c, hs, ws)
        forms.add(form)
        assert blocks == lib.query("hn_dwconv_bwd_blocks_levels", n, c, len(hs), ints(hs), ints(ws)), (n, hs, ws, c, form)
    assert forms == {"strip", "tiled"}
    assert R.dwconv_bwd_tiled_lds(128) <= 80 * 1024 and R.dwconv_bwd_strip_lds(768) <= 65536 < R.dwconv_bwd_strip_lds(776)
    assert lib.query("hn_dwconv_bwd_blocks_levels", 1, 12, 1, ints((4,)), ints((4,))) == -1
    assert lib.query("hn_dwconv_bwd_blocks_levels", 1, 8, 6, ints((4,) * 6), ints((4,) * 6)) == -1


def test_elementwise_block_mirrors(lib):
    for n, h, w, c in [(1, 1, 1, 8), (2, 16, 16, 64), (2, 64, 64, 64), (2, 64, 64, 128), (16, 64, 128, 64), (1, 3, 5, 40)]:
        assert R.fuse_bwd_blocks(n, h, w, c) == lib.query("hn_fuse_bwd_blocks", n, h, w, c)
    for n, h, w, k in [(1, 1, 1, 8), (2, 3, 5, 64), (2, 64, 64, 128), (4, 256, 256, 64)]:
        assert R.space_to_depth_blocks(n, h, w, k) == lib.query("hn_space_to_depth_blocks", n, h, w, k)
    assert R.ew_grid(0) == 1 and R.ew_grid(256 * 8192 + 1) == 8192 and R.ew_grid(256 * 8191 + 1) == 8192 and R.ew_grid(257) == 2
    assert R.fuse_bwd_kernel((1, 2, 0), (1, 1, 0), 4, 4) == "quads" and R.fuse_bwd_kernel((1, 2, 0), (1, 0, 0), 4, 4) == "generic"
    assert R.fuse_bwd_kernel((1, 2, 1), (1, 1, 1), 4, 4) == "generic" and R.fuse_bwd_kernel((1, 0, 2), (0, 0, 1), 4, 4) == "quads"


def test_argument_refusals(lib):
    """HN_CHECK_ARG returns 1 before any launch: the pointers are never dereferenced (1 stands for 'not null')"""
    P = 1
    r = lib.raw
    assert r("hn_stem_fwd")(P, P, P, P, 1, 17, 24, None) == 1                                  # odd H: `H >> 1` would drop conv2d's last row
    assert r("hn_stem_fwd")(P, P, P, None, 2, 16, 23, None) == 1                               # odd W
    assert r("hn_stem_fwd")(P, P, P, P, 1, 1, 2, None) == 1                                    # H < 2
    assert r("hn_maxpool_fwd")(P, 8, P, 8, 1, 5, 4, 8, 0, None) == 1                           # odd H
    assert r("hn_maxpool_bwd")(P, 8, P, 8, P, 8, None, 1, 4, 5, 8, 0, None) == 1               # odd W
    assert r("hn_maxpool_bwd2")(P, 8, P, 8, P, 8, None, P, 1, 3, 4, 8, 0, 0, None) == 1
    assert r("hn_maxpool_bwd_from_arg")(P, P, 8, P, 8, None, 1, 4, 3, 8, 0, 0, None) == 1
    assert r("hn_maxpool_fwd")(P, 8, P, 8, 1, 4, 4, 8, 2, None) == 1                           # mode
    assert r("hn_gconv_fwd")(P, 16, P, P, 16, 1, 4, 4, 12, 1, None) == 1                       # C % 8
    assert r("hn_gconv_fwd")(P, 16, P, P, 16, 1, 4, 4, 8, 3, None) == 1                        # stride
    assert r("hn_gconv_dgrad_s2")(P, 8, P, P, 8, 1, 5, 4, 8, None) == 1                        # odd Hi
    assert r("hn_gconv_wgrad")(P, 8, P, 12, P, 1, 4, 4, 8, 1, None) == 1                       # ld % 8
    assert r("hn_gconv_pack")(P, P, P, 20, 0, None) == 1
    assert r("hn_dwconv_fwd")(P, 12, P, P, 12, 1, 4, 4, 12, None) == 1
    assert r("hn_dwconv_fwd")(P, 8, P, P, 12, 1, 4, 4, 8, None) == 1                           # ldo % 8
    assert r("hn_dwconv_wgrad")(P, 2056, P, 2056, P, 1, 4, 4, 2056, None) == 1                 # C > 2048
    six = ints((4,) * 6)
    assert r("hn_dwconv_fwd_levels")(P, 8, P, P, 8, 1, 8, 6, six, six, 1, 0, None) == 1        # nlev > HN_MAX_LEVELS
    assert r("hn_dwconv_wgrad_levels")(P, 8, P, 8, P, 1, 8, 6, six, six, 1, None) == 1
    assert r("hn_dwconv_bwd_levels")(P, 8, P, 8, P, P, 8, P, 1, 8, 6, six, six, 1, 0, None) == 1
    assert r("hn_dwconv_bwd_levels")(P, 1032, P, 1032, P, P, 1032, P, 1, 1032, 1, six, six, 1, 0, None) == 1   # C > 1024
    assert r("hn_dwconv_bwd_levels")(P, 8, P, 8, None, P, 8, P, 1, 8, 1, six, six, 1, 0, None) == 1   # dx without the flipped pack
    assert r("hn_dwconv_fwd_levels")(P, 8, P, P, 8, 1, 8, 1, six, six, 0, 0, None) == 1        # row_align 0
    assert r("hn_head_grad_levels")(P, None, 64, 8, 5, P, 8, 1, 6, six, six, 1, 0, None) == 1
    assert r("hn_up2_fwd")(P, 8, P, 12, 1, 4, 4, 8, None) == 1
    assert r("hn_sum2x2")(P, 8, P, 8, None, 1, 4, 4, 12, 0, None) == 1
    assert r("hn_seg_fold")(P, 8, 0, P, 8, None, 0, 1, 3, 4, 8, 0, None) == 1                  # H < 4
    assert r("hn_seg_fold")(P, 8, 0, P, 8, None, 0, 1, 4, 3, 8, 0, None) == 1                  # W < 4
    assert r("hn_seg_fold")(P, 8, 4, P, 8, None, 0, 1, 4, 4, 8, 0, None) == 1                  # c0 % 8
    assert r("hn_seg_fold")(P, 8, 0, P, 8, None, 0, 1, 4, 4, 8, 3, None) == 1                  # up
    assert r("hn_space_to_depth")(P, P, 16, 1, 2, 2, 5, None) == 1                             # ldo < 4k
    assert r("hn_space_to_depth")(P, P, 28, 1, 2, 2, 5, None) == 1                             # ldo % 8
    assert r("hn_space_to_depth_bf16")(P, 24, P, 1, 2, 2, 24, P, None) == 1                    # psum with 256 % (k/2) != 0
    assert r("hn_space_to_depth_bf16")(P, 12, P, 1, 2, 2, 8, None, None) == 1                  # ldi % 8
    assert r("hn_head_grad")(P, None, 4, 32, 8, 5, P, 8, 4, 1, None) == 1                      # sigmoid without y
    assert r("hn_head_grad")(P, None, 4, 32, 8, 9, P, 8, 4, 0, None) == 1                      # ldz < Nout
    m3 = ints((1, 2, 0))
    ld3 = ints((8, 8, 8))
    ptr3 = (ctypes.c_void_p * 3)(1, 1, None)
    assert r("hn_fuse_fwd")(ptr3, ld3, m3, P, P, 8, 1, 3, 4, 8, None) == 1                     # nearest x2 into an odd map
    assert r("hn_fuse_fwd")(ptr3, ld3, ints((1, 4, 0)), P, P, 8, 1, 4, 4, 8, None) == 1        # mode
    assert r("hn_fuse_fwd_raw")(ptr3, ld3, m3, P, 4, 1e-4, P, P, 8, 1, 4, 4, 8, None) == 1     # nw
    assert r("hn_fuse_dweights")(P, 0, P, 2, 1e-4, P, None) == 1                               # blocks
