"""Sentinel guard bands around kernel outputs, shared by the exact kernel tests (test_gemm_exact_gpu.py, test_batchnorm_exact_gpu.py, test_loss_exact_gpu.py,
test_se_exact_gpu.py, test_eltwise_exact_gpu.py, test_gemm_forms_exact_gpu.py, test_gemm_epilogue_exact_gpu.py).

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
