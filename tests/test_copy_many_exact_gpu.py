"""hn_copy_many -- the gather of gradient buckets, their rounding to a bf16 payload and the way back, for the data-parallel step -- through
the C entry point on tables built here from the header ({src, dst, numel, first_block}, blocks of 1024 elements, block_job), never through
ddp.GradReducer.  Kind 0 moves fp32 values (finite payloads, equal bits demanded), kind 1 is the round-to-nearest-even of
tests/pack_ref.py on its rounding set, kind 2 is exact widening.  Sources and destinations each 16-byte aligned and one element (4 bytes,
or 2 for bf16) off: kind 0 takes its float4 path only when both are aligned.  Every destination sits between guard bands."""
import pytest
import torch

from tests import pack_ref as P
from tests.exact_checks import D, gen, release, same_bits
from tests.guards import GuardedBytes

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
I16, I32, I64 = torch.int16, torch.int32, torch.int64
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4099)


@pytest.fixture(scope="module")
def built():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    return lib()


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


class Slot:
    """n elements of `width` bytes in a GuardedBytes payload, `off` elements past a 16-byte boundary; sentinel unless `values` are given"""

    def __init__(self, n, width, off, values=None):
        self.n, self.skip = n, width * off
        self.g = GuardedBytes(width * (n + off))
        self.bytes = self.g.view[self.skip:]
        if values is not None:
            self.bytes.copy_(values.contiguous().view(torch.uint8).reshape(-1))
        assert self.ptr() % 16 == self.skip

    def ptr(self):
        return self.bytes.data_ptr()

    def check(self, name):
        assert bool((self.g.view[:self.skip] == GuardedBytes.SENT).all()), f"{name}: the bytes before the misaligned tensor were written"
        self.g.check(name)


def payload(n, name):
    """finite fp32 values with the rounding set (ties, carries, both signs, +-0, exponents near 2^-100 and 2^100) planted"""
    return P.randw((n,), gen(name))


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_copy_many(built, kind, src_off, dst_off):
    sw, dw = (2 if kind == 2 else 4), (2 if kind == 1 else 4)
    srcs, dsts, wants, rows, owner, blk = [], [], [], [], [], 0
    for i, n in enumerate(SIZES):
        x = payload(n, f"copy{kind}-{i}")
        if kind == 0:
            src, want = x, x.view(I32)
        elif kind == 1:
            src, want = x, P.rne_bits(x)
            assert torch.equal(want, P.bits(x.double()))
        else:
            src = P.rne_bits(x).view(BF16)
            want = (src.view(I16).to(I32) << 16)                            # widening: the bf16 pattern is the fp32 pattern's high half
            assert torch.equal(want.view(F32), src.float())
        s, d = Slot(n, sw, src_off, src), Slot(n, dw, dst_off)
        srcs.append(s), dsts.append(d), wants.append(want)
        nb = (n + 1023) // 1024
        rows.append([s.ptr(), d.ptr(), n, blk])
        owner += [i] * nb
        blk += nb
    jobs, own = D(torch.tensor(rows, dtype=I64)), D(torch.tensor(owner, dtype=I32))
    built.call("hn_copy_many", jobs.data_ptr(), own.data_ptr(), blk, kind)
    for i, (d, want) in enumerate(zip(dsts, wants)):
        name = f"hn_copy_many kind {kind} (source {'off' if src_off else 'aligned'}, destination {'off' if dst_off else 'aligned'}), tensor {i} ({SIZES[i]} elements)"
        same_bits(d.bytes.view(want.dtype), want, name, "element")
        d.check(name)


def test_copy_many_refuses(built):
    f = built.raw("hn_copy_many")
    s, d = Slot(8, 4, 0, torch.ones(8)), Slot(8, 4, 0)
    jobs, own = D(torch.tensor([[s.ptr(), d.ptr(), 8, 0]], dtype=I64)), D(torch.zeros(1, dtype=I32))
    st = torch.cuda.current_stream().cuda_stream
    assert f(jobs.data_ptr(), own.data_ptr(), 1, 3, st) == 1 and f(jobs.data_ptr(), own.data_ptr(), 1, -1, st) == 1
    assert f(jobs.data_ptr(), own.data_ptr(), 0, 0, st) == 1 and f(None, own.data_ptr(), 1, 0, st) == 1
    torch.cuda.synchronize()
    assert d.g.untouched(), "a refused hn_copy_many call wrote"
    d.check("hn_copy_many (refused calls)")
