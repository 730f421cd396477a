"""References of the weight packs (hn_pack_weight, hn_pack_weight_ex, hn_pack_weights_batched, hn_pack_small_batched, hn_gconv_pack,
hn_gconv_pack_diag, hn_dw_pack, hn_pack_levels), written from the comments of include/hydranet_hip.h and the kind list above
pack_small_batched_kernel, in torch on the CPU.  tests/test_pack_ref_cpu.py pins every layout to plain torch (F.conv2d and its autograd
gradients, Upsample + ReflectionPad2d + Conv2d) on integer data, so that a reference cannot share a misreading with the kernel it judges;
tests/test_pack_exact_gpu.py holds the kernels to them bit for bit.

Layout functions return the UNROUNDED operand as float64 (every value an fp32 number, padding +0.0); bits() rounds it to bf16 with
stencil_ref.bf16_rne and returns the int16 bit patterns the kernel must have written.  Rounding domain: normal finite values below 2^127
and +-0 (overflow, NaN and denormals are out of scope)."""
import torch

from tests import seg_conv_ref as S
from tests import stencil_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
I16, I32, I64 = torch.int16, torch.int32, torch.int64


def kp(c):
    """KP(c): c rounded up to 32"""
    return (c + 31) // 32 * 32


# ---- rounding ------------------------------------------------------------------------------------------------------------------------------
def bits(v):
    """bf16 bit patterns (int16) of the round-to-nearest-even rounding of fp32 values held in float64 (or fp32) tensors"""
    assert bool((v.to(F32).to(v.dtype) == v).all()), "the unrounded operand must consist of fp32 numbers"
    return R.bf16_rne(v).to(BF16).view(I16)


def rne_bits(x):
    """the same rounding restated on the fp32 bit pattern: add 0x7FFF + (bit 16), keep the high half.  fp32 tensor -> int16"""
    assert x.dtype == F32
    b = x.contiguous().view(I32).to(I64) & 0xFFFFFFFF
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(I16)


def f32_from_bits(b):
    """int64 bit patterns -> fp32"""
    b = torch.as_tensor(b, dtype=I64)
    return torch.where(b >= 0x80000000, b - 0x100000000, b).to(I32).view(F32)


def rounding_set():
    """fp32 values whose bf16 rounding takes every branch: high halves with even and odd last bit (0x7F: the carry runs into the
    exponent), low halves below, at and above the tie, both signs, exponents near 1.0, 2^-100 and 2^100, and +-0"""
    out = []
    for sign in (0, 1):
        for expo in (127, 27, 227):
            for mant in (0x00, 0x01, 0x2A, 0x7E, 0x7F):
                for low in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
                    out.append((sign << 31) | (expo << 23) | (mant << 16) | low)
    out += [0x00000000, 0x80000000]
    return f32_from_bits(out)


def plant(flat, values):
    """spread `values` (as many as fit) over the 1-D fp32 tensor `flat`, in place"""
    step = max(1, flat.numel() // values.numel())
    m = min(values.numel(), (flat.numel() + step - 1) // step)
    flat[::step][:m] = values[:m]
    return flat


def coded(cout, cin, taps):
    """position-coded integers ((31 co + 7 ci + 3 tap) mod 251) - 125: bf16-exact, neighbours along every axis distinct"""
    co, ci, t = torch.meshgrid(torch.arange(cout), torch.arange(cin), torch.arange(taps), indexing="ij")
    return (((31 * co + 7 * ci + 3 * t) % 251) - 125).to(F32)


def randw(shape, g):
    """random normals with the rounding set planted (a different rotation of the set per generator state, so that small tensors do not
    all carry its first values)"""
    w = torch.randn(shape, generator=g, dtype=F32)
    rs = rounding_set()
    rs = rs.roll(int(torch.randint(0, rs.numel(), (1,), generator=g)))
    plant(w.reshape(-1), rs)
    return w


# ---- dense operands ---------------------------------------------------------------------------------------------------------------------------
def dense(w):
    """w [Cout][Cin][taps] -> wp [Cout][taps][KP(Cin)], wt [Cin][taps][KP(Cout)], zero filled"""
    cout, cin, taps = w.shape
    w = w.to(F64)
    wp = torch.zeros(cout, taps, kp(cin), dtype=F64)
    wt = torch.zeros(cin, taps, kp(cout), dtype=F64)
    wp[:, :, :cin] = w.permute(0, 2, 1)
    wt[:, :, :cout] = w.permute(1, 2, 0)
    return wp, wt


def slice_(w, ci0, cin):
    """dense() of the input channels [ci0, ci0 + cin) of w [Cout][Cin_total][taps]"""
    assert 0 <= ci0 and ci0 + cin <= w.shape[1]
    return dense(w[:, ci0:ci0 + cin])


def phase(w, c0, bias=None, ci0=0):
    """phase form of w [k][C][3][3] over the input channels [ci0, ci0 + c0): Conv3x3(ReflectionPad2d(1)(nearest_up2(x))) evaluated per
    output phase on the low-resolution grid (seg_conv_ref.phase_weights): (wp [4k][9][KP(c0)], wt [c0][9][KP(4k)], b_eff [4k])"""
    we, be = S.phase_weights(w[:, ci0:ci0 + c0], bias, c0)
    wp, wt = dense(we.reshape(we.shape[0], c0, 9))
    return wp, wt, be


# ---- stencil operands -------------------------------------------------------------------------------------------------------------------------
def dw(w):
    """depthwise w [C][1][3][3] (or [C][3][3]) -> wk [tap][C], wkf [8 - tap][C]"""
    wk = w.reshape(w.shape[0], 9).to(F64).t().contiguous()
    return wk, wk.flip(0).contiguous()


def gconv(w, flip):
    """grouped w [C][8][3][3] -> wk [tap][i][G][o], wd [tap'][o][G][i] (tap' = 8 - tap when flipped)"""
    g8 = w.shape[0] // 8
    w4 = w.to(F64).reshape(g8, 8, 8, 9)                                       # [g][o][i][tap]
    wk = w4.permute(3, 2, 0, 1).contiguous()
    wd = w4.permute(3, 1, 0, 2)
    return wk, (wd.flip(0) if flip else wd).contiguous()


def diag(w):
    """grouped w [C][8][3][3] -> block-diagonal operands [C][9][64] of the 64-channel tiles: row = channel c, column j = channel
    64 (c // 64) + j of the same tile.  wk: row = output channel co, the columns of its group's input channels hold w[co][i][tap];
    wd (stride-1 data gradient): row = input channel ci, the columns of its group's output channels hold w[co][ci % 8][8 - tap]"""
    c = w.shape[0]
    w9 = w.to(F64).reshape(c, 8, 9)
    wk = torch.zeros(c, 9, 64, dtype=F64)
    wd = torch.zeros(c, 9, 64, dtype=F64)
    for ch in range(c):
        g = ch // 8
        j0 = g * 8 - (ch // 64) * 64                                          # first column of the channel's group inside its tile
        wk[ch, :, j0:j0 + 8] = w9[ch].t()                                     # [tap][i]
        wd[ch, :, j0:j0 + 8] = w9[g * 8:g * 8 + 8, ch % 8, :].flip(1).t()     # [tap][o] = w[8 g + o][ch % 8][8 - tap]
    return wk, wd


def diag_mask(c):
    """bool [C][9][64]: the elements of the 8 x 8 diagonal blocks"""
    m = torch.zeros(c, 9, 64, dtype=torch.bool)
    for ch in range(c):
        j0 = (ch // 8) * 8 - (ch // 64) * 64
        m[ch, :, j0:j0 + 8] = True
    return m


# ---- level packing ----------------------------------------------------------------------------------------------------------------------------
def levels(srcs, N, Hs, Ws, align, fill, ldd=None):
    """srcs[l] [N * Hs[l] * Ws[l]][C] (any dtype; bit patterns) -> packed [rows][ldd]: level l's rows from row_offsets()[l]; alignment
    rows and the columns beyond C hold `fill`"""
    c = srcs[0].shape[1]
    off = R.row_offsets(N, Hs, Ws, align)
    out = torch.full((off[-1], ldd or c), fill, dtype=srcs[0].dtype)
    for l, s in enumerate(srcs):
        assert s.shape == (N * Hs[l] * Ws[l], c)
        out[off[l]:off[l] + s.shape[0], :c] = s
    assert bool((out[R.alignment_rows(N, Hs, Ws, align)] == fill).all())
    return out
