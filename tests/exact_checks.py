"""Checks shared by the exact kernel tests (test_batchnorm_exact_gpu.py, test_se_exact_gpu.py, test_eltwise_exact_gpu.py): bit-exact
comparison with float64, elementwise error bounds, the bf16 interval check, the fp32 evaluation slack of the activations, and the
deterministic generators / GPU staging helpers.  A failure names the entry point (the `name` the caller passes), the row (image, partial
row or row block) and the channel or output index."""
import zlib

import pytest
import torch

from tests import bn_ref as B
from tests.guards import dev

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24                 # fp32 unit roundoff
EXACT_LIMIT = 1 << 24          # integers below it are exact in fp32

_LIVE = []


def release():
    """end of a test: wait for the launches that read the tensors D() kept alive, then let them go"""
    if _LIVE:
        torch.cuda.synchronize()
        _LIVE.clear()


def D(t):
    """t on the GPU, kept alive until the test ends (a temporary whose data_ptr() is passed to a launch could be freed, and its block
    handed to the next allocation, before the kernel runs)"""
    t = t.to(dev())
    _LIVE.append(t)
    return t


def gen(name):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(name.encode()) & 0xFFFFFF)
    return g


def gpu_bf16(v, width=None):
    """float64 CPU values (bf16-representable) -> bf16 [M, C] on the GPU; width > C: a channel slice of a wider buffer whose other
    columns hold unrelated values"""
    m, c = v.shape
    if width and width > c:
        full = torch.full((m, width), 3.0, dtype=F64)
        full[:, :c] = v
        return full.to(BF16).to(dev())[:, :c]
    return v.to(BF16).to(dev())


def rows_blame(rb):
    return lambda r: f"row block {r // rb} (rows {r // rb * rb}..{r // rb * rb + rb - 1})" if rb else ""


def exact(got, want, name, what="partial row"):
    """fp32 [P, C] == float64 bit for bit; a mismatch names the partial row (row block) and channel"""
    g = got.detach().double().cpu()
    bad = ~(g == want)
    n = int(bad.sum())
    if n:
        idx = bad.nonzero()[:6].tolist()
        lines = [f"  {what} {r}, channel {c}: got {float(g[r, c])!r} want {float(want[r, c])!r}" for r, c in idx]
        pytest.fail(f"{name}: {n} of {g.numel()} values differ\n" + "\n".join(lines))


def same_bits(got, want, name, what="index"):
    """integer views of two tensors (bf16 as int16, fp32 as int32, bytes as uint8) equal bit for bit -- -0 is not +0, and a NaN sentinel
    a kernel left in place is a mismatch; names the first bad indices with both patterns in hex"""
    g = got.detach().cpu()
    w = want.reshape(g.shape)
    assert g.dtype == w.dtype and not g.dtype.is_floating_point, f"{name}: same_bits compares integer views ({g.dtype} against {w.dtype})"
    bad = g != w
    n = int(bad.sum())
    if n:
        mask = (1 << (8 * g.element_size())) - 1
        lines = [f"  {what} {tuple(i)}: got 0x{int(g[tuple(i)]) & mask:0{2 * g.element_size()}x} want 0x{int(w[tuple(i)]) & mask:0{2 * g.element_size()}x}"
                 for i in bad.nonzero()[:6].tolist()]
        pytest.fail(f"{name}: {n} of {g.numel()} values differ bit for bit\n" + "\n".join(lines))


def within(got, want, bound, name, what="channel"):
    """|got - want| <= bound elementwise (1-D per-channel vectors or [rows, C])"""
    g = got.detach().double().cpu()
    err = (g - want).abs()
    bad = ~(err <= bound)
    n = int(bad.sum())
    if n:
        idx = bad.nonzero()[:6].tolist()
        lines = []
        for ii in idx:
            t = tuple(ii)
            lines.append(f"  {what} {t[0] if len(t) == 1 else t}: got {float(g[t])!r} want {float(want[t])!r} "
                         f"(err {float(err[t]):.3e} > bound {float(bound[t] if torch.is_tensor(bound) else bound):.3e})")
        pytest.fail(f"{name}: {n} of {g.numel()} values outside the bound\n" + "\n".join(lines))


def bf_interval(got, y, s, name, rb=None):
    """every bf16 value of got [M, C] must be the bf16 rounding of some value in [y - s, y + s] (rounding is monotone: the set is the bf16
    values between the roundings of the two ends).  Names channel and row block of the first failures."""
    s = s + 2 * U * y.abs() + 1e-38                     # (the ends pass through fp32 on their way to bf16)
    lo = (y - s).float().to(BF16).double()
    hi = (y + s).float().to(BF16).double()
    g = got.detach().double().cpu()
    bad = ~((g >= lo) & (g <= hi))
    n = int(bad.sum())
    if n:
        idx = bad.nonzero()[:6].tolist()
        blame = rows_blame(rb)
        lines = [f"  row {r} {blame(r)}, channel {c}: got {float(g[r, c])!r}, allowed [{float(lo[r, c])!r}, {float(hi[r, c])!r}] "
                 f"(float64 value {float(y[r, c])!r})" for r, c in idx]
        pytest.fail(f"{name}: {n} of {g.numel()} bf16 outputs outside their interval\n" + "\n".join(lines))


def slack_fwd(x, y, mags, act):
    """fp32 evaluation slack of y = act(x), x = sc*z + sh [+ res terms]: a few ulps of the magnitudes the pre-activation combines, times
    the activation's slope, plus the error of __expf-based activations (relative (2 + |x|) ulps, absolute for ELU's exp(x) - 1)"""
    s = 4 * U * mags * B.act_slope(act)
    if act in (B.ACT_SWISH, B.ACT_ELU, B.ACT_SIGMOID):
        s = s + 8 * U * (2 + x.abs()) * (y.abs() + 1)
    return s
