"""Float64 statements of the seg-head conv forms and of the NT GEMM's row mappings and statistics epilogues (csrc/hn_gemm.hip), written
from their definitions and device-agnostic: tests/test_seg_conv_ref_cpu.py holds them to plain torch (F.conv2d, autograd, torch.cat) bit
for bit on integer data without a GPU; tests/test_gemm_forms_exact_gpu.py and tests/test_gemm_epilogue_exact_gpu.py hold the kernels to
them.  Activations are NHWC ([n, H, W, C]), weights [Cout][Cin][3][3], everything float64."""
import torch

F64 = torch.float64
BF16 = torch.bfloat16


def cdiv(a, b):
    return -(-a // b)


# ---- padding -----------------------------------------------------------------------------------------------------------------------
def pad_index(L, kind, device):
    """source index (in [0, L)) of the padded positions 0 .. L + 1 of a one-pixel reflect (ReflectionPad2d(1)) / clamp (replicate) pad"""
    v = torch.arange(-1, L + 1, device=device)
    if kind == "reflect":
        return torch.where(v < 0, -v, torch.where(v >= L, 2 * L - 2 - v, v))
    assert kind == "clamp"
    return v.clamp(0, L - 1)


def pad1(x, kind):
    """[n, H, W, C] -> [n, H + 2, W + 2, C]"""
    return x[:, pad_index(x.shape[1], kind, x.device)][:, :, pad_index(x.shape[2], kind, x.device)]


def conv3x3(x, w, kind):
    """3x3 conv of the padded map: out[n, y, x, o] = sum_{c, ky, kx} pad(x)[n, y + ky, x + kx, c] * w[o, c, ky, kx]"""
    n, h, wd, c = x.shape
    xp = pad1(x.double(), kind)
    out = torch.zeros(n, h, wd, w.shape[0], dtype=F64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + h, kx:kx + wd] @ w[:, :, ky, kx].double().t()
    return out


# ---- phase form ----------------------------------------------------------------------------------------------------------------------
def phase_mask(k, device):
    """[4k][9]: effective tap (dy, dx) is used by phase (py, px) iff dy in {py, py+1} and dx in {px, px+1} (the statement of
    tests/test_gemm_exact_gpu.py::phase_mask)"""
    m = torch.zeros(4 * k, 9, dtype=F64, device=device)
    for py in range(2):
        for px in range(2):
            for dy in (py, py + 1):
                for dx in (px, px + 1):
                    m[(2 * py + px) * k:(2 * py + px + 1) * k, dy * 3 + dx] = 1
    return m


def _d(p, k):
    """low-resolution offset (+1) the up-sampled tap k of output phase p falls on: phase 0: k = 0 -> 0, k = 1, 2 -> 1; phase 1: k = 0, 1 -> 1,
    k = 2 -> 2  (output row 2y + p reads up-sampled rows 2y + p + k - 1 = low-resolution rows y + floor((p + k - 1) / 2))"""
    return (p + k - 1) // 2 + 1


def phase_weights(w, bias, c0=None):
    """effective weights of Conv3x3(ReflectionPad2d(1)(nearest_up2(x))) on the low-resolution grid: w [k][C][3][3] (first c0 input
    channels) -> (w_eff [4k][c0][3][3], b_eff [4k]); cout (2 py + px) k + o is output phase (py, px), channel o"""
    k, c = w.shape[0], (c0 or w.shape[1])
    we = torch.zeros(4 * k, c, 3, 3, dtype=F64, device=w.device)
    for py in range(2):
        for px in range(2):
            ph = 2 * py + px
            for ky in range(3):
                for kx in range(3):
                    we[ph * k:(ph + 1) * k, :, _d(py, ky), _d(px, kx)] += w[:, :c, ky, kx].double()
    assert bool((we.reshape(4 * k, c, 9) * (1 - phase_mask(k, w.device))[:, None, :] == 0).all())
    return we, (bias.double().repeat(4) if bias is not None else None)


def depth_to_space(z):
    """[n, H, W, 4k] (phase-major channels) -> [n, 2H, 2W, k]: channel (2 py + px) k + o of (y, x) is channel o of (2y + py, 2x + px)"""
    n, h, w, c = z.shape
    k = c // 4
    return z.reshape(n, h, w, 2, 2, k).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, k)


def space_to_depth(v):
    """[n, 2H, 2W, k] -> [n, H, W, 4k], the inverse of depth_to_space"""
    n, h2, w2, k = v.shape
    return v.reshape(n, h2 // 2, 2, w2 // 2, 2, k).permute(0, 1, 3, 2, 4, 5).reshape(n, h2 // 2, w2 // 2, 4 * k)


def elu(z):
    return torch.where(z > 0, z, torch.expm1(z.clamp(max=0)))


def elu_margin(z):
    """smallest absolute distance of elu(z) (z <= 0, non-zero results) from a bf16 rounding boundary (the midpoint of two neighbouring
    bf16 values of its binade)"""
    v = torch.expm1(z.double()).abs()
    v = v[v > 0]
    ulp = torch.exp2(torch.frexp(v)[1].double() - 8)                  # v = m 2^e, m in [0.5, 1): 8 significant bits -> ulp 2^(e - 8)
    t = v / ulp
    return float((((t - t.floor()) - 0.5).abs() * ulp).min())


def phase_forward_pre(x, w, bias, c0=None, addend=None):
    """pre-activation of the phase-form forward, full resolution [n, 2H, 2W, k]: replicate-padded low-resolution conv with the effective
    weights, depth-to-space store, + bias (+ the pre-activation addend at the output's layout)"""
    we, be = phase_weights(w, bias, c0)
    z = depth_to_space(conv3x3(x, we, "clamp") + (be if be is not None else 0))
    return z + addend.double() if addend is not None else z


def dgrad_padded(dz, w):
    """data gradient on the padded (H + 2) x (W + 2) grid (mode 3, full correlation): dz [n, H, W, Cout], w [Cout][Cin][3][3] ->
    dvp[n, y + ky, x + kx, c] += dz[n, y, x, o] * w[o, c, ky, kx]"""
    n, h, wd, _ = dz.shape
    out = torch.zeros(n, h + 2, wd + 2, w.shape[1], dtype=F64, device=dz.device)
    for ky in range(3):
        for kx in range(3):
            out[:, ky:ky + h, kx:kx + wd] += dz.double() @ w[:, :, ky, kx].double()
    return out


# ---- the fold -------------------------------------------------------------------------------------------------------------------------
def fold(dvp, clamp):
    """padded-grid gradient [n, H + 2, W + 2, C] -> gradient of the unpadded input [n, H, W, C]: every padded position is added to the
    pixel it reflects (clamp = 0) / clamps (clamp = 1) onto"""
    n, hp, wp, c = dvp.shape
    kind = "clamp" if clamp else "reflect"
    t = torch.zeros(n, hp - 2, wp, c, dtype=F64, device=dvp.device).index_add_(1, pad_index(hp - 2, kind, dvp.device), dvp.double())
    return torch.zeros(n, hp - 2, wp - 2, c, dtype=F64, device=dvp.device).index_add_(2, pad_index(wp - 2, kind, dvp.device), t)


def ring_count(h, w, clamp, device):
    """[H, W]: padded RING positions (row 0 / H + 1, column 0 / W + 1) that fold onto each pixel (0: interior; corners of the target
    frame collect 3)"""
    one = torch.ones(1, h + 2, w + 2, 1, dtype=F64, device=device)
    one[:, 1:-1, 1:-1] = 0
    return fold(one, clamp)[0, :, :, 0].long()


def ring_rows(dvp):
    """the ring scratch of hn_conv3x3_dgrad_fold: [n][2 (W + 2) + 2 H][C] = padded row 0, padded row H + 1, padded column 0 (rows 1 .. H),
    padded column W + 1 (rows 1 .. H)"""
    return torch.cat([dvp[:, 0], dvp[:, -1], dvp[:, 1:-1, 0], dvp[:, 1:-1, -1]], 1)


def elu_grad_factor(y):
    """ELU'(x) from the ELU OUTPUT y: 1 where y > 0, else y + 1"""
    y = y.double()
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def fold_staged(dvp, clamp, yprev=None):
    """the folded gradient with the values at the documented rounding points of the two-launch form: the conv epilogue stores
    bf16(bf16(acc) * ELU') for the interior of the padded grid and bf16(acc) for the ring; the fix-up stores bf16(interior + ring sum * ELU').
    -> (dx, stages): dx = fold(dvp) * ELU' in float64, stages = [(name, tensor)] every one of which the caller asserts to be bf16-exact,
    which makes all those roundings identities and dx the bit-exact result"""
    f = elu_grad_factor(yprev) if yprev is not None else None
    inner = dvp[:, 1:-1, 1:-1].double()
    ringsum = fold(dvp, clamp) - inner
    stages = [("accumulator", dvp.double())]
    if f is not None:
        inner, ringsum = inner * f, ringsum * f
        stages += [("interior * ELU'", inner), ("ring sum * ELU'", ringsum)]
    dx = inner + ringsum
    stages.append(("folded value", dx))
    return dx, stages


def bf16_exact(v):
    return bool((v.to(BF16).double() == v).all())


# ---- row mappings of the NT GEMM ----------------------------------------------------------------------------------------------------------
def level_of_rows(rows, device):
    """hn_conv_gemm_nt_lvl: level index of every packed row, rows = rows per level"""
    return torch.repeat_interleave(torch.arange(len(rows), device=device), torch.tensor(list(rows), device=device))


def image_of_rows(m, rows_per_image, device):
    """hn_conv_gemm_nt_imgw: rows [i * rows_per_image, (i + 1) * rows_per_image) use weight matrix i"""
    return torch.arange(m, device=device) // rows_per_image


def rpi_offsets(m, rpi, img_stride, ldc, device):
    """hn_conv_gemm_nt rpi / img_stride: element offset of output row r = (r / rpi) * img_stride + (r % rpi) * ldc"""
    r = torch.arange(m, device=device)
    return (r // rpi) * img_stride + (r % rpi) * ldc


def lvlout_rows(n, hs, ws, row_align, device):
    """hn_conv_gemm_nt_lvlout: the level-packed rows ([image][pixel] per level, every level padded to a multiple of row_align) ->
    (M, level [M], image [M], pixel [M] (the image's concatenated pixel index), real [M] (False: an alignment row, never stored))"""
    lev, img, pix, real = [], [], [], []
    base = 0
    for l, (h, w) in enumerate(zip(hs, ws)):
        hw = h * w
        rows = cdiv(n * hw, row_align) * row_align
        r = torch.arange(rows, device=device)
        lev.append(torch.full((rows,), l, device=device))
        img.append(r // hw)
        pix.append(base + r % hw)
        real.append(r < n * hw)
        base += hw
    return sum(len(v) for v in lev), torch.cat(lev), torch.cat(img), torch.cat(pix), torch.cat(real)


def lvlout_offsets(n, hs, ws, row_align, img_stride, ldc, device):
    """element offset of every packed row in the per-image concatenated output (-1: alignment row)"""
    m, lev, img, pix, real = lvlout_rows(n, hs, ws, row_align, device)
    return torch.where(real, img * img_stride + pix * ldc, torch.full_like(img, -1))


# ---- statistics epilogues (GemmNT::emode) -------------------------------------------------------------------------------------------------
def tile_sums(v, tile):
    """[M, C] -> [ceil(M / tile), C]: one partial row per pixel tile (the last may be ragged)"""
    m, c = v.shape
    nt = cdiv(m, tile)
    vp = torch.cat([v.double(), torch.zeros(nt * tile - m, c, dtype=F64, device=v.device)])
    return vp.view(nt, tile, c).sum(1)


def patch_sums(v):
    """[n, H, W, C] -> [n * ceil(H / 16) * ceil(W / 16), C]: one partial row per 16 x 16 output patch (the direct kernel)"""
    n, h, w, c = v.shape
    th, tw = cdiv(h, 16), cdiv(w, 16)
    vp = torch.zeros(n, th * 16, tw * 16, c, dtype=F64, device=v.device)
    vp[:, :h, :w] = v.double()
    return vp.view(n, th, 16, tw, 16, c).permute(0, 1, 3, 2, 4, 5).reshape(n * th * tw, 256, c).sum(1)


def estat_terms(emode, q, z, coef, ey=None):
    """per-element terms (t1, t2 | None) of the statistics rows; q = the bf16-rounded output the mode sums over (emode 0..2: bf16(acc +
    bias), BEFORE a post-rounding addend; emode 3: the FINAL stored value), z = ez, coef = [4][C] (sc, sh, mu, rs):
      0: q, q^2        1: q * bf16(relu(sc z + sh)), -        2: g = q [sc z + sh > 0]: g, g (z - mu) rs        3: g = q [ey > 0]: g, g (z - mu) rs"""
    q = q.double()
    if emode == 0:
        return q, q * q
    z = z.double()
    sc, sh, mu, rs = (coef[i].double() for i in range(4))
    pre = sc * z + sh
    if emode == 1:
        return q * pre.clamp(min=0).to(BF16).double(), None
    g = torch.where((pre if emode == 2 else ey.double()) > 0, q, torch.zeros_like(q))
    return g, g * (z - mu) * rs
