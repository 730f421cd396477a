"""hn_state_pack / hn_state_verify / hn_state_unpack through the C ABI on the device, against tests/ckpt_ref.py: one table with jobs of
1 .. 131 072 words, sources 16-byte aligned and one word further, sentinels around every source and in every pad word, arbitrary bit
patterns.  Every comparison is of whole buffers, bit for bit."""
import numpy as np
import pytest
import torch

from tests import ckpt_ref as ref

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4099, 131072)
SENTINEL = 0xA5C3F00D
GUARD = 8                                                                          # sentinel words before the first and after the last slot


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    return lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def host(t):
    return t.cpu().numpy().view(np.uint32)


def contents(seed):
    """arbitrary bit patterns per job: random words, with NaN payloads, infinities, -0, denormals and all-ones planted"""
    g = np.random.default_rng(seed)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0xFFFFFFFF, 0x7FFFFFFF, 0],
                       dtype=np.uint32)
    out = []
    for n in SIZES:
        w = g.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        at = g.integers(0, n, size=min(n, 16))
        w[at] = special[g.integers(0, special.size, size=at.size)]
        out.append(w)
    out[-1][:] = 0xFFFFFFFF                                                         # 131 072 all-ones words: s2 wraps modulo 2^64
    return out


def arena(words, shift):
    """every job's words in one buffer of sentinels: job k starts `shift` words past a 16-byte boundary, >= 4 sentinels on either side
    -> (buffer, [start of every job])"""
    starts, off = [], GUARD
    for w in words:
        starts.append(off + shift)
        off += (shift + w.size + 3) // 4 * 4 + 4
    buf = np.full(off + GUARD, SENTINEL, dtype=np.uint32)
    for s, w in zip(starts, words):
        buf[s:s + w.size] = w
    return buf, starts


def tables(src_ptrs, dst_ptrs):
    rows, owner, blk = [], [], 0
    for i, (s, d, n) in enumerate(zip(src_ptrs, dst_ptrs, SIZES)):
        nb = (n + 1023) // 1024
        rows.append([s, d, n, blk])
        owner += [i] * nb
        blk += nb
    return torch.tensor(rows, dtype=torch.int64).to("cuda:0"), torch.tensor(owner, dtype=torch.int32).to("cuda:0"), blk


class Setup:
    """sources (shifted by `shift` words), a staging buffer whose slots follow the layout rule, and the pack tables"""

    def __init__(self, shift, seed=0):
        self.words = contents(seed)
        self.src_host, self.src_at = arena(self.words, shift)
        self.src = dev(self.src_host)
        offs, total = ref.slots(SIZES)
        self.slot_at = [GUARD + o for o in offs]
        self.stage_host = np.full(GUARD + total + GUARD, SENTINEL, dtype=np.uint32)   # pads hold sentinels: pack must not write them
        self.stage = dev(self.stage_host)
        assert self.src.data_ptr() % 16 == 0 and self.stage.data_ptr() % 16 == 0 and all(o % 4 == 0 for o in self.slot_at)
        assert all((self.src.data_ptr() + 4 * s) % 16 == 4 * shift for s in self.src_at)
        self.jobs, self.owner, self.blocks = tables([self.src.data_ptr() + 4 * s for s in self.src_at],
                                                    [self.stage.data_ptr() + 4 * s for s in self.slot_at])
        self.ws = torch.full((self.blocks * 2,), -1, dtype=torch.int64, device="cuda:0")       # never zeroed: every block writes its own
        self.sums = torch.full((len(SIZES) * 2,), -1, dtype=torch.int64, device="cuda:0")
        self.want_sums = np.array([ref.sums(w) for w in self.words], dtype=np.uint64).reshape(-1)
        self.want_stage = self.stage_host.copy()
        for s, w in zip(self.slot_at, self.words):
            self.want_stage[s:s + w.size] = w

    def pack(self, K):
        K.call("hn_state_pack", self.jobs.data_ptr(), self.owner.data_ptr(), self.blocks, len(SIZES), self.ws.data_ptr(), self.sums.data_ptr())

    def got_sums(self, t=None):
        return (self.sums if t is None else t).cpu().numpy().view(np.uint64)

    def back_tables(self, dst, dst_at):
        return tables([self.stage.data_ptr() + 4 * s for s in self.slot_at], [dst.data_ptr() + 4 * s for s in dst_at])


@pytest.mark.parametrize("shift", [0, 1])
def test_pack(K, shift):
    s = Setup(shift)
    s.pack(K)
    assert np.array_equal(host(s.stage), s.want_stage)                              # slots, pads and the guard zones, as one buffer
    assert np.array_equal(host(s.src), s.src_host)                                  # src is only read
    assert np.array_equal(s.got_sums(), s.want_sums), [(i, n) for i, n in enumerate(SIZES) if tuple(s.got_sums()[2 * i:2 * i + 2]) != tuple(s.want_sums[2 * i:2 * i + 2])]
    assert int(s.want_sums[-1]) == (0xFFFFFFFF * (131072 * 131073 // 2)) % 2 ** 64  # (the wrapped one)


def test_sums_do_not_depend_on_alignment(K):
    a, b = Setup(0), Setup(1)
    a.pack(K)
    b.pack(K)
    assert np.array_equal(a.got_sums(), b.got_sums()) and np.array_equal(host(a.stage), host(b.stage))


@pytest.mark.parametrize("shift", [0, 1])
def test_verify(K, shift):
    s = Setup(shift)
    s.pack(K)
    expect = s.sums.clone()
    verdict = torch.tensor([123456, 77, -9, 0x7FFFFFFF], dtype=torch.int32, device="cuda:0")   # garbage: a clean verify overwrites all of it
    out = torch.full_like(s.sums, -1)
    # the src column of the SOURCE tables (aligned or one word further), then of the staging slots
    for jobs in (s.jobs, s.back_tables(s.src, s.src_at)[0]):
        verdict.copy_(torch.tensor([123456, 77, -9, 0x7FFFFFFF], dtype=torch.int32))
        K.call("hn_state_verify", jobs.data_ptr(), s.owner.data_ptr(), s.blocks, len(SIZES), expect.data_ptr(), s.ws.data_ptr(), out.data_ptr(),
               verdict.data_ptr())
        assert verdict.tolist() == [0, -1, 0, 0]
        assert np.array_equal(s.got_sums(out), s.want_sums)
    assert np.array_equal(host(s.stage), s.want_stage) and np.array_equal(host(s.src), s.src_host)     # no copy
    # one word flipped in job 3 and one in job 7 of the staging buffer
    back = s.back_tables(s.src, s.src_at)[0]
    s.stage[s.slot_at[3] + 2] ^= 0x00010000
    s.stage[s.slot_at[7] + 1024] ^= 1                                              # (the single word of job 7's second block)
    K.call("hn_state_verify", back.data_ptr(), s.owner.data_ptr(), s.blocks, len(SIZES), expect.data_ptr(), s.ws.data_ptr(), out.data_ptr(),
           verdict.data_ptr())
    assert verdict.tolist() == [2, 3, 0, 0]
    got = s.got_sums(out).reshape(-1, 2)
    differ = [i for i in range(len(SIZES)) if tuple(got[i]) != tuple(s.want_sums.reshape(-1, 2)[i])]
    assert differ == [3, 7]
    # only the last job damaged: the index is that job's
    s.stage[s.slot_at[3] + 2] ^= 0x00010000
    s.stage[s.slot_at[7] + 1024] ^= 1
    s.stage[s.slot_at[9] + 131071] ^= -0x80000000
    K.call("hn_state_verify", back.data_ptr(), s.owner.data_ptr(), s.blocks, len(SIZES), expect.data_ptr(), s.ws.data_ptr(), out.data_ptr(),
           verdict.data_ptr())
    assert verdict.tolist() == [1, 9, 0, 0]


@pytest.mark.parametrize("dst_shift", [1, 3])
def test_unpack(K, dst_shift):
    s = Setup(0, seed=4)
    s.pack(K)
    empty = [np.full(n, SENTINEL, dtype=np.uint32) for n in SIZES]
    dst_host, dst_at = arena(empty, dst_shift)                                      # destinations pre-filled with sentinels, misaligned
    want, _ = arena(s.words, dst_shift)
    for verdict_words, copied in (([1, 0, 0, 0], False), ([-1, 5, 0, 0], False), ([0, -1, 0, 0], True), (None, True)):
        dst = dev(dst_host)
        jobs, owner, blocks = s.back_tables(dst, dst_at)
        assert all((dst.data_ptr() + 4 * a) % 16 == 4 * dst_shift for a in dst_at)
        verdict = None if verdict_words is None else torch.tensor(verdict_words, dtype=torch.int32, device="cuda:0")
        K.call("hn_state_unpack", jobs.data_ptr(), owner.data_ptr(), blocks, None if verdict is None else verdict.data_ptr())
        assert np.array_equal(host(dst), want if copied else dst_host), verdict_words
        assert verdict is None or verdict.tolist() == verdict_words                 # the verdict is only read
    assert np.array_equal(host(s.stage), s.want_stage)


def test_captured_pack_replayed_twice_equals_two_eager_ones(K):
    eager, cap = Setup(1, seed=9), Setup(1, seed=9)
    second = contents(10)

    def rewrite(s):                                                                 # new contents at the same addresses
        for at, w in zip(s.src_at, second):
            s.src[at:at + w.size] = dev(w)
    eager.pack(K)
    first_stage, first_sums = host(eager.stage).copy(), eager.got_sums().copy()
    rewrite(eager)
    eager.pack(K)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        cap.pack(K)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(host(cap.stage), first_stage) and np.array_equal(cap.got_sums(), first_sums)
    rewrite(cap)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(host(cap.stage), host(eager.stage)) and np.array_equal(cap.got_sums(), eager.got_sums())
    assert not np.array_equal(first_sums, eager.got_sums())
    want = np.array([ref.sums(w) for w in second], dtype=np.uint64).reshape(-1)
    assert np.array_equal(cap.got_sums(), want)
