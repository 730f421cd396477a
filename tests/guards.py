"""Sentinel guard bands around kernel outputs, shared by the exact kernel tests (test_gemm_exact_gpu.py, test_batchnorm_exact_gpu.py, test_loss_exact_gpu.py,
test_se_exact_gpu.py, test_eltwise_exact_gpu.py, test_gemm_forms_exact_gpu.py, test_gemm_epilogue_exact_gpu.py, test_post_exact_gpu.py,
test_pack_exact_gpu.py, test_adam_exact_gpu.py, test_copy_many_exact_gpu.py, test_grad_tail_exact_gpu.py, test_lovasz_exact_gpu.py).

An output is a view into a larger buffer filled with a NaN bit pattern that no kernel produces: BAND elements before and after the output
and, when the row stride ld exceeds the column count, the ld - cols columns between its rows.  check() fails on any guard element a
kernel wrote."""
import pytest
import torch

F32 = torch.float32
SENT32 = 0x7FC00001            # NaN bit pattern no kernel produces
SENT16 = 0x7FC1
BAND = 256                     # guard elements before and after every output


def dev():
    return torch.device("cuda:0")


class GuardedBytes:
    """a byte-granular guard for outputs Guarded does not hold (uint8 masks and frames, uint64 counters; ArgBytes of
    test_stencil_exact_gpu.py, generalised): nbytes of payload between two PAD-byte bands of SENT.  The payload starts as `fill` (one
    byte value; SENT by default, so `untouched()` can tell that a refused call wrote nothing) or as a copy of `init` (any tensor of
    nbytes bytes).  as_(dtype, *shape) views the payload; PAD keeps it 256-byte aligned."""
    PAD, SENT = 256, 0xA5

    def __init__(self, nbytes, fill=None, init=None):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * self.PAD,), self.SENT, dtype=torch.uint8, device=dev())
        self.view = self.buf[self.PAD:self.PAD + self.n]
        if init is not None:
            self.view.copy_(init.contiguous().reshape(-1).view(torch.uint8).to(dev()))
        elif fill is not None:
            self.view.fill_(fill)

    def ptr(self):
        return self.view.data_ptr()

    def as_(self, dtype, *shape):
        return self.view.view(dtype).reshape(*shape)

    def untouched(self):
        """the payload still holds SENT everywhere (for payloads that started as SENT)"""
        return bool((self.view == self.SENT).all())

    def check(self, name):
        bands = torch.cat([self.buf[:self.PAD], self.buf[self.PAD + self.n:]])
        bad = (bands != self.SENT).nonzero()
        if bad.numel():
            first = [int(i) - self.PAD if int(i) < self.PAD else int(i) - self.PAD + self.n for i in bad[:4, 0]]
            pytest.fail(f"{name}: {bad.shape[0]} guard bytes overwritten (first at byte offsets {first} from the start of the {self.n}-byte output)")


class Guarded:
    """an output tensor [rows, cols] with row stride ld >= cols inside a sentinel-filled buffer: BAND elements before and after, and
    the ld - cols columns between rows"""

    def __init__(self, rows, cols, ld=None, dtype=F32):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.dtype = dtype
        n = 2 * BAND + rows * self.ld
        idt = torch.int32 if dtype == F32 else torch.int16
        self.buf = torch.full((n,), SENT32 if dtype == F32 else SENT16, dtype=idt, device=dev()).view(dtype)
        self.view = self.buf[BAND:BAND + rows * self.ld].view(rows, self.ld)[:, :cols]

    def ptr(self):
        return self.view.data_ptr()

    def check(self, name):
        idt = torch.int32 if self.dtype == F32 else torch.int16
        bits = self.buf.view(idt)
        mask = torch.ones(bits.numel(), dtype=torch.bool, device=dev())
        mask[BAND:BAND + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = False
        bad = (bits != (SENT32 if self.dtype == F32 else SENT16)) & mask
        nb = int(bad.sum())
        if nb:
            first = [int(i) - BAND for i in bad.nonzero()[:4, 0]]
            pytest.fail(f"{name}: {nb} guard-band elements overwritten (first at offsets {first} from the output's start, "
                        f"rows {self.rows} x cols {self.cols}, ld {self.ld})")
