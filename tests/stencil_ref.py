"""Plain float64 references of the stencil kernels (csrc/hn_stencil.hip), written from the definitions in that file's header comments and
include/hydranet_hip.h: index arithmetic on NHWC tensors [N, H, W, C], no F.conv2d / F.max_pool2d.  They run on CPU or GPU tensors.
tests/test_stencil_ref_cpu.py holds every function here to torch's own float64 operators; tests/test_stencil_exact_gpu.py holds the kernels to
these.  The second half restates the launch decisions (which kernel, how many partial rows) the GPU tests assert before they compare."""
import torch

F64 = torch.float64
GW = 8                                   # group width of the grouped conv
MAX_LEVELS = 5                           # HN_MAX_LEVELS


def _z(shape, like, dtype=F64):
    return torch.zeros(shape, dtype=dtype, device=like.device)


def out_hw(Hi, Wi, stride):
    """output size of the 3x3 / pad 1 convs: stride 2 halves an even map"""
    if stride == 1:
        return Hi, Wi
    assert stride == 2 and Hi % 2 == 0 and Wi % 2 == 0
    return Hi // 2, Wi // 2


def _pad1(x):
    n, h, w, c = x.shape
    xp = _z((n, h + 2, w + 2, c), x)
    xp[:, 1:h + 1, 1:w + 1] = x
    return xp


def _tap(xp, ky, kx, s, Ho, Wo):
    """view of the zero-padded map at input pixel (oy*s + ky - 1, ox*s + kx - 1) for every output pixel (padded index oy*s + ky)"""
    return xp[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s]


# ---- stem: dense 3x3 / stride 2 / zero pad 1 from the NCHW frame; x [N][3][H][W], w [32][3][3][3] = w[co][ci][ky][kx] ----------------------
def stem_out_hw(H, W):
    """the kernel's `Ho = H >> 1, Wo = W >> 1`.  For an even size that is conv2d(stride 2, padding 1)'s (H + 1) // 2.  For an odd size it
    is one less: output row oy reads input rows 2 oy - 1 .. 2 oy + 1 <= H - 2, so the rows 0 .. (H >> 1) - 1 are conv2d's first rows
    unchanged, conv2d's last row (centred on input row H - 1) is not computed, and input row H - 1 is never read (the same for columns).
    hn_stem_fwd refuses odd sizes (HN_ERR_ARG), so that truncation is never launched."""
    return H >> 1, W >> 1


def _stem_taps(x):
    """(t, view [N, Ho, Wo]) for t = ci * 9 + ky * 3 + kx: input pixel (2 oy + ky - 1, 2 ox + kx - 1) of channel ci, 0 outside the frame"""
    n, c, H, W = x.shape
    assert c == 3
    Ho, Wo = stem_out_hw(H, W)
    xp = _z((n, 3, H + 2, W + 2), x)
    xp[:, :, 1:H + 1, 1:W + 1] = x.to(F64)
    for ci in range(3):
        for ky in range(3):
            for kx in range(3):
                yield ci * 9 + ky * 3 + kx, xp[:, ci, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2]


def stem(x, w):
    """z [N, Ho, Wo, 32]: z[n, oy, ox, co] = sum over (ci, ky, kx) of x[n, ci, 2 oy + ky - 1, 2 ox + kx - 1] * w[co, ci, ky, kx]"""
    n, _, H, W = x.shape
    Ho, Wo = stem_out_hw(H, W)
    wt = w.to(F64).reshape(32, 27)
    out = _z((n, Ho, Wo, 32), x)
    for t, v in _stem_taps(x):
        out += v.unsqueeze(-1) * wt[:, t]
    return out


def stem_patches(x):
    """the im2col rows the kernel leaves for the weight gradient: [N, Ho, Wo, 32], column ci * 9 + ky * 3 + kx = that tap, columns 27..31 zero"""
    n, _, H, W = x.shape
    Ho, Wo = stem_out_hw(H, W)
    out = _z((n, Ho, Wo, 32), x)
    for t, v in _stem_taps(x):
        out[..., t] = v
    return out


def stem_lds_path(N, H, W):
    """bool [N, Ho, Wo]: True where the pixel leaves through the XOR-swizzled LDS rows (`!(Wo & 1) && (bidx + 1) * 256 <= total`: a whole
    256-thread block of an even-width grid), False where its thread stores its own rows.  A thread owns the pixel pair (2 p, 2 p + 1) of
    a row, `Wp = (Wo + 1) >> 1` pairs per row; the last pair of an odd row is a lone pixel."""
    Ho, Wo = stem_out_hw(H, W)
    Wp = (Wo + 1) >> 1
    total = N * Ho * Wp
    n, oy, ox = torch.meshgrid(torch.arange(N), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    bidx = ((n * Ho + oy) * Wp + ox // 2) // 256
    return ((bidx + 1) * 256 <= total) & (Wo % 2 == 0)


# ---- grouped 3x3, group width 8, zero pad 1; w [C][8][3][3] = w[o][i][ky][kx] -------------------------------------------------------------
def gconv(x, w, stride):
    n, Hi, Wi, c = x.shape
    Ho, Wo = out_hw(Hi, Wi, stride)
    g = c // GW
    xp = _pad1(x.to(F64))
    out = _z((n, Ho, Wo, g, GW), x)
    for ky in range(3):
        for kx in range(3):
            xt = _tap(xp, ky, kx, stride, Ho, Wo).reshape(n, Ho, Wo, g, GW)
            wt = w[:, :, ky, kx].to(F64).reshape(g, GW, GW)                     # [g][o][i]
            out += (xt.unsqueeze(4) * wt).sum(-1)                              # [n,h,w,g,1,i] * [g,o,i]
    return out.reshape(n, Ho, Wo, c)


def gconv_dgrad(dz, w, stride, Hi, Wi):
    n, Ho, Wo, c = dz.shape
    assert (Ho, Wo) == out_hw(Hi, Wi, stride)
    g = c // GW
    dxp = _z((n, Hi + 2, Wi + 2, c), dz)
    z = dz.to(F64).reshape(n, Ho, Wo, g, GW)
    for ky in range(3):
        for kx in range(3):
            wt = w[:, :, ky, kx].to(F64).reshape(g, GW, GW)                     # [g][o][i]
            contrib = (z.unsqueeze(5) * wt).sum(4)                             # [n,h,w,g,o,1] * [g,o,i] summed over o
            _tap(dxp, ky, kx, stride, Ho, Wo).add_(contrib.reshape(n, Ho, Wo, c))
    return dxp[:, 1:Hi + 1, 1:Wi + 1].contiguous()


def gconv_wgrad(x, dz, stride):
    n, Hi, Wi, c = x.shape
    Ho, Wo = out_hw(Hi, Wi, stride)
    g = c // GW
    xp = _pad1(x.to(F64))
    z = dz.to(F64).reshape(n * Ho * Wo, g, GW)
    dw = _z((c, GW, 3, 3), x)
    for ky in range(3):
        for kx in range(3):
            xt = _tap(xp, ky, kx, stride, Ho, Wo).reshape(n * Ho * Wo, g, GW)
            dw[:, :, ky, kx] = (z.unsqueeze(3) * xt.unsqueeze(2)).sum(0).reshape(c, GW)      # [p,g,o,1] * [p,g,1,i]
    return dw


# ---- depthwise 3x3, stride 1, zero pad 1; w [C][3][3] (or [C][1][3][3]) -------------------------------------------------------------------
def dwconv(x, w):
    n, h, wd, c = x.shape
    w = w.to(F64).reshape(c, 3, 3)
    xp = _pad1(x.to(F64))
    out = _z((n, h, wd, c), x)
    for ky in range(3):
        for kx in range(3):
            out += _tap(xp, ky, kx, 1, h, wd) * w[:, ky, kx]
    return out


def dwconv_dgrad(dz, w):
    n, h, wd, c = dz.shape
    w = w.to(F64).reshape(c, 3, 3)
    dxp = _z((n, h + 2, wd + 2, c), dz)
    for ky in range(3):
        for kx in range(3):
            _tap(dxp, ky, kx, 1, h, wd).add_(dz.to(F64) * w[:, ky, kx])
    return dxp[:, 1:h + 1, 1:wd + 1].contiguous()


def dwconv_wgrad(x, dz):
    n, h, wd, c = x.shape
    xp = _pad1(x.to(F64))
    dw = _z((c, 3, 3), x)
    for ky in range(3):
        for kx in range(3):
            dw[:, ky, kx] = (_tap(xp, ky, kx, 1, h, wd) * dz.to(F64)).sum((0, 1, 2))
    return dw


# ---- level-packed tensors [rows, C]: level l = [N, Hs[l], Ws[l], C] at row_off[l], every level on a multiple of row_align rows ------------
def row_offsets(N, Hs, Ws, row_align=1):
    off = [0]
    for h, w in zip(Hs, Ws):
        real = N * h * w
        off.append(off[-1] + (real + row_align - 1) // row_align * row_align)
    return off


def level_views(packed, N, Hs, Ws, row_align=1):
    """the levels of a packed tensor as NHWC views (alignment rows are in none of them)"""
    off = row_offsets(N, Hs, Ws, row_align)
    return [packed[off[l]:off[l] + N * h * w].reshape(N, h, w, packed.shape[1]) for l, (h, w) in enumerate(zip(Hs, Ws))]


def alignment_rows(N, Hs, Ws, row_align=1):
    """bool [rows]: True on the rows behind each level's real ones"""
    off = row_offsets(N, Hs, Ws, row_align)
    m = torch.ones(off[-1], dtype=torch.bool)
    for l, (h, w) in enumerate(zip(Hs, Ws)):
        m[off[l]:off[l] + N * h * w] = False
    return m


def _levels_map(fn, packed, N, Hs, Ws, row_align, prev):
    """fn per level into a packed output: alignment rows zero when not accumulating, untouched (prev) when accumulating"""
    out = _z(packed.shape, packed) if prev is None else prev.to(F64).clone()
    ov = level_views(out, N, Hs, Ws, row_align)
    for l, xv in enumerate(level_views(packed, N, Hs, Ws, row_align)):
        y = fn(xv)
        ov[l].copy_(y if prev is None else ov[l] + y)
    return out


def dwconv_levels(xp, w, N, Hs, Ws, row_align=1, prev=None):
    return _levels_map(lambda v: dwconv(v, w), xp, N, Hs, Ws, row_align, prev)


def dwconv_dgrad_levels(dzp, w, N, Hs, Ws, row_align=1, prev=None):
    return _levels_map(lambda v: dwconv_dgrad(v, w), dzp, N, Hs, Ws, row_align, prev)


def dwconv_wgrad_levels(xp, dzp, N, Hs, Ws, row_align=1):
    xs, zs = level_views(xp, N, Hs, Ws, row_align), level_views(dzp, N, Hs, Ws, row_align)
    return sum(dwconv_wgrad(a, b) for a, b in zip(xs, zs))


# ---- 3x3 / stride-2 max pools --------------------------------------------------------------------------------------------------------------
def _pool_taps(mode):
    """padded-array offset of the window: mode 0 rows 2o .. 2o+2 of a map padded right / bottom, mode 1 rows 2o-1 .. 2o+1 of one padded left / top"""
    return (0, 0) if mode == 0 else (1, 1)


def maxpool(x, mode, dtype=F64):
    """(dtype: float32 is as exact for the small integers of the large cases and a quarter of the memory)
    values [N, H/2, W/2, C] and arg bytes (uint8): tap ky*3+kx of the FIRST maximum in row-major tap order; mode 0: an out-of-range tap is
    a candidate of value 0 and arg 9; mode 1: out-of-range taps are skipped"""
    n, h, w, c = x.shape
    assert h % 2 == 0 and w % 2 == 0
    ho, wo = h // 2, w // 2
    py, px = _pool_taps(mode)
    fill = 0.0 if mode == 0 else float("-inf")
    xp = torch.full((n, h + 1, w + 1, c), fill, dtype=dtype, device=x.device)
    inside = torch.zeros((1, h + 1, w + 1, 1), dtype=torch.bool, device=x.device)
    xp[:, py:py + h, px:px + w] = x.to(dtype)
    inside[:, py:py + h, px:px + w] = True
    best = torch.full((n, ho, wo, c), float("-inf"), dtype=dtype, device=x.device)
    arg = torch.full((n, ho, wo, c), 255, dtype=torch.uint8, device=x.device)
    for ky in range(3):
        for kx in range(3):
            cand = xp[:, ky:ky + 2 * ho - 1:2, kx:kx + 2 * wo - 1:2]
            ins = inside[:, ky:ky + 2 * ho - 1:2, kx:kx + 2 * wo - 1:2]                       # [1, ho, wo, 1]: broadcasts
            upd = cand > best
            best = torch.where(upd, cand, best)
            tap = torch.where(ins, ky * 3 + kx, 9).to(torch.uint8)
            arg = torch.where(upd, tap, arg)
    return best, arg


def maxpool_bwd(arg, dout, wscale, H, W, mode):
    """dx [N, H, W, C] = wscale * (dout scattered to each window's arg tap); arg 9 (the zero pad) drops its gradient"""
    n, ho, wo, c = dout.shape
    py, px = _pool_taps(mode)
    dxp = _z((n, H + 1, W + 1, c), dout)
    a = arg.to(torch.int64)
    for ky in range(3):
        for kx in range(3):
            dxp[:, ky:ky + 2 * ho - 1:2, kx:kx + 2 * wo - 1:2] += dout.to(F64) * (a == ky * 3 + kx)
    return dxp[:, py:py + H, px:px + W] * (1.0 if wscale is None else float(wscale))


def up2(x, dtype=F64):
    n, h, w, c = x.shape
    iy = torch.arange(2 * h, device=x.device) // 2
    ix = torch.arange(2 * w, device=x.device) // 2
    return x.to(dtype)[:, iy][:, :, ix]


def sum2x2(g, wscale=None, dtype=F64):
    g = g.to(dtype)
    s = g[:, 0::2, 0::2] + g[:, 0::2, 1::2] + g[:, 1::2, 0::2] + g[:, 1::2, 1::2]
    return s * (1.0 if wscale is None else float(wscale))


# ---- BiFPN fusion node: out = swish(sum_i w[i] * T_i(in_i)); mode 0 absent, 1 identity, 2 nearest x2, 3 zero-pad max pool -----------------
def _fuse_terms(ins, modes):
    vs, args = [], []
    for x, m in zip(ins, modes):
        if m == 0:
            vs.append(None), args.append(None)
        elif m == 1:
            vs.append(x.to(F64)), args.append(None)
        elif m == 2:
            vs.append(up2(x)), args.append(None)
        else:
            v, a = maxpool(x, 0)
            vs.append(v), args.append(a)
    return vs, args


def fuse_fwd(ins, modes, w):
    """(pre-activation, swish of it)"""
    vs, _ = _fuse_terms(ins, modes)
    pre = sum(float(w[i]) * v for i, v in enumerate(vs) if v is not None)
    return pre, pre * torch.sigmoid(pre)


def swish_grad(pre):
    s = torch.sigmoid(pre)
    return s * (1 + pre * (1 - s))


def fuse_bwd(ins, modes, w, dout):
    """g = dout * swish'(pre); the gradient of every input (identity: w g, nearest x2: w * 2x2 sums of g, pooled: w * g routed to the
    arg-max tap); dw[i] = sum g * T_i(in_i); the arg bytes of the mode-3 inputs.  Also returns pre and the terms T_i."""
    vs, args = _fuse_terms(ins, modes)
    pre = sum(float(w[i]) * v for i, v in enumerate(vs) if v is not None)
    g = dout.to(F64) * swish_grad(pre)
    dins, dw = [], torch.zeros(3, dtype=F64)
    for i, (x, m) in enumerate(zip(ins, modes)):
        if m == 0:
            dins.append(None)
            continue
        dw[i] = float((g * vs[i]).sum())
        if m == 1:
            dins.append(float(w[i]) * g)
        elif m == 2:
            dins.append(sum2x2(g, float(w[i])))
        else:
            dins.append(maxpool_bwd(args[i], g, float(w[i]), x.shape[1], x.shape[2], 0))
    return {"g": g, "din": dins, "dw": dw, "arg": args, "pre": pre, "terms": vs}


def fuse_weights(praw, nw, eps):
    """w = relu(p) / (sum relu(p) + eps) over the first nw raw parameters (the rest 0)"""
    r = torch.zeros(3, dtype=F64)
    r[:nw] = torch.clamp(praw.to(F64).cpu()[:nw], min=0)
    return r / (r.sum() + eps)


def fuse_dweights(dw, praw, nw, eps):
    """dp_i = [p_i > 0] * (dw_i - sum_j w_j dw_j) / (sum relu(p) + eps)"""
    p = praw.to(F64).cpu()[:nw]
    r = torch.zeros(3, dtype=F64)
    r[:nw] = torch.clamp(p, min=0)
    s = r.sum() + eps
    dot = (dw.to(F64).cpu() * r / s).sum()
    return torch.where(p > 0, (dw.to(F64).cpu()[:nw] - dot) / s, torch.zeros(nw, dtype=F64))


# ---- fold of a padded-domain gradient [N, H+2, W+2, ldv] back to the map: the adjoint of the padding gather -----------------------------------
def pad_index(L, clamp):
    """source index of every padded coordinate 0 .. L+1: the interior is itself; the border is the reflection (1, L-2) or the clamp (0, L-1)"""
    idx = [q - 1 for q in range(L + 2)]
    idx[0] = 0 if clamp else 1
    idx[L + 1] = L - 1 if clamp else L - 2
    return torch.tensor(idx, dtype=torch.int64)


def elu_grad_from_output(y):
    y = y.to(F64)
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def seg_fold(dvp, c0, C, H, W, up, yprev=None, dtype=F64):
    """up = 0: reflect fold, up = 1: reflect fold summed over 2x2, up = 2: clamp (replicate) fold; optionally times ELU'(yprev)"""
    n = dvp.shape[0]
    clamp = up == 2
    v = dvp[..., c0:c0 + C].to(dtype)
    rows = _z((n, H, W + 2, C), dvp, dtype).index_add_(1, pad_index(H, clamp).to(dvp.device), v)
    out = _z((n, H, W, C), dvp, dtype).index_add_(2, pad_index(W, clamp).to(dvp.device), rows)
    if up == 1:
        out = sum2x2(out, None, dtype)
    if yprev is not None:
        out = out * elu_grad_from_output(yprev)
    return out


# ---- pixel shuffles and the head-gradient gather -------------------------------------------------------------------------------------------
def space_to_depth(dy, k, ldo=None):
    """dy [N, 2h, 2w, k] -> [N, h, w, ldo]: channel (py*2+px)*k + o of (y, x) = dy(2y+py, 2x+px, o); columns >= 4k are zero"""
    n, h2, w2, kk = dy.shape
    assert kk == k
    ldo = ldo or 4 * k
    out = _z((n, h2 // 2, w2 // 2, ldo), dy)
    for py in range(2):
        for px in range(2):
            ph = py * 2 + px
            out[..., ph * k:(ph + 1) * k] = dy.to(F64)[:, py::2, px::2]
    return out


def space_to_depth_sums(x, k):
    """the bf16 form: the same shuffle (no padding columns) and the per-channel sums [k] of the tensor that passes through"""
    return space_to_depth(x, k), x.to(F64).sum((0, 1, 2))


def head_grad(dy, y, rpi, img_stride, lds, Nout, ldz, M, sigmoid=False):
    """dy (flat) -> dz [M, ldz]: dz[m, c] = dy[(m // rpi) * img_stride + (m % rpi) * lds + c] for c < Nout (times y (1 - y) with sigmoid),
    else 0"""
    m = torch.arange(M, device=dy.device)
    o = ((m // rpi) * img_stride + (m % rpi) * lds).unsqueeze(1) + torch.arange(Nout, device=dy.device)
    v = dy.to(F64).reshape(-1)[o]
    if sigmoid:
        s = y.to(F64).reshape(-1)[o]
        v = v * (s * (1 - s))
    dz = _z((M, ldz), dy)
    dz[:, :Nout] = v
    return dz


def head_grad_levels(dy, y, img_stride, lds, Nout, ldz, N, Hs, Ws, row_align, sigmoid=False, prev=None):
    """level-packed form: image n's rows of dy are the levels' pixels one after the other; alignment rows of dz are not written (prev)"""
    off = row_offsets(N, Hs, Ws, row_align)
    dz = _z((off[-1], ldz), dy) if prev is None else prev.to(F64).clone()
    pix0 = 0
    for l, (h, w) in enumerate(zip(Hs, Ws)):
        hw = h * w
        flat = dy.to(F64).reshape(-1)[pix0 * lds:]
        fy = None if y is None else y.to(F64).reshape(-1)[pix0 * lds:]
        dz[off[l]:off[l] + N * hw] = head_grad(flat, fy, hw, img_stride, lds, Nout, ldz, N * hw, sigmoid)
        pix0 += hw
    return dz


def bf16_rne(v):
    """round-to-nearest-even bf16 of exact float64 values below 2^24 (they pass through fp32 unchanged), as float64"""
    return v.to(torch.float32).to(torch.bfloat16).to(F64)


# =============================================================================================================================================
# launch decisions of hn_stencil.hip's host side, restated
# =============================================================================================================================================
def cdiv(a, b):
    return (a + b - 1) // b


def ew_grid(items):
    """blocks of the grid-stride elementwise launches: capped at 8192"""
    return max(1, min(8192, cdiv(items, 256)))


def wgrad_chunks(pixels, items):
    chunks = cdiv(262144, items)
    chunks = min(chunks, cdiv(pixels, 64), 4096)
    return max(chunks, 1)


def gconv_wgrad_plan(N, Hi, Wi, C, stride):
    """(kernel, chunks, pixels per chunk): the sub-chunked kernel takes chunks of >= 32 pixels"""
    Ho, Wo = out_hw(Hi, Wi, stride)
    pixels = N * Ho * Wo
    chunks = wgrad_chunks(pixels, C // 8 * 9)
    ppc = cdiv(pixels, chunks)
    return ("sub" if ppc >= 32 and pixels < 1 << 32 else "strip"), chunks, ppc


def gconv_s2_lds(C):
    """stride-2 forward / dgrad: the packed weights (1152 B per group) are staged in LDS up to 24 KiB"""
    return C // 8 * 1152 <= 24576


def strips_of(N, Hs, Ws):
    return sum(N * h * cdiv(w, 4) for h, w in zip(Hs, Ws))


def dwconv_wgrad_blocks(strips, C):
    lanes = 256 // (C // 8)
    spl = max(2, (strips + 2047 * lanes) // (2048 * lanes))
    return cdiv(strips, spl * lanes)


def dwconv_bwd_strip_blocks(strips, C):
    lanes = 256 // (C // 4)
    spl = max(2, (strips + 767 * lanes) // (768 * lanes))
    return cdiv(strips, spl * lanes)


def dwconv_bwd_strip_lds(C):
    return (256 * 37 + 9 * C) * 4


def dwconv_bwd_tiled_lds(C):
    c8 = C // 8
    return (cdiv(10 * 18 * c8, 64) + cdiv(8 * 16 * c8, 64)) * 1024


def tiles_of(N, Hs, Ws):
    return [N * cdiv(h, 8) * cdiv(w, 16) for h, w in zip(Hs, Ws)]


def dwconv_bwd_tiled_plan(N, C, Hs, Ws):
    """None (strip form) or (tiles per workgroup, workgroups): the LDS-tiled form takes >= 512 8x16 tiles at C <= 128 within its LDS limit"""
    total = sum(tiles_of(N, Hs, Ws))
    if C > 128 or dwconv_bwd_tiled_lds(C) > 80 * 1024 or total < 512:
        return None
    tpw = cdiv(total, 512)
    return tpw, cdiv(total, tpw)


def dwconv_bwd_plan(N, C, Hs, Ws):
    """(form, partial rows) of hn_dwconv_bwd_levels"""
    t = dwconv_bwd_tiled_plan(N, C, Hs, Ws)
    if t:
        return "tiled", t[1]
    return "strip", dwconv_bwd_strip_blocks(strips_of(N, Hs, Ws), C)


def fuse_bwd_blocks(N, H, W, C):
    return max(1, min(1024, cdiv(N * H * W * (C // 8), 256)))


def fuse_bwd_kernel(modes, has_dst, H, W):
    """'quads' for a top-down node (one identity, one nearest-x2 input WITH a destination, no pooled input, even map), else 'generic'"""
    n_id = sum(m == 1 for m in modes)
    n_up = sum(m == 2 for m in modes)
    n_pool = sum(m == 3 for m in modes)
    up_dst = sum(m == 2 and bool(d) for m, d in zip(modes, has_dst))
    return "quads" if n_id == 1 and n_up == 1 and up_dst == 1 and n_pool == 0 and H % 2 == 0 and W % 2 == 0 else "generic"


def space_to_depth_blocks(N, h, w, k):
    return ew_grid(N * h * w * 4 * (k // 8))
