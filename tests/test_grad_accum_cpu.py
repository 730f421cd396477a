"""CPU: the host side of gradient accumulation (hn_grad_accum, train.accum_options / optimizer_steps_per_epoch): the symbol is declared
and exported, bad arguments are rejected before any HIP call, the trainer key's accepted and rejected values, and the test suite's own
yardstick (tests/grad_accum_ref.py).  No kernel is launched here."""
import ctypes

import numpy as np
import pytest

from tests import grad_accum_ref as ref


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_entry_point(built):
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    assert "hn_grad_accum" in sig and hasattr(dll, "hn_grad_accum") and "hn_grad_accum" in built.lib().symbols()
    ret, args, has_stream = sig["hn_grad_accum"]
    assert ret is ctypes.c_int and has_stream                                      # a launcher: a status, and the stream last
    # (jobs, block_job, total_blocks, j, losses, n_losses, loss_mean, words, n_words, sticky, stream): hn_swap_many's tables first
    assert args[:3] == sig["hn_swap_many"][1][:3]
    assert args[3:] == [ctypes.c_long, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                        ctypes.c_void_p]
    assert "hn_accum.hip" in built.SOURCES


def test_bad_arguments_are_rejected_before_any_hip_call(built):
    f = built.lib().raw("hn_grad_accum")
    buf = (ctypes.c_long * 64)()                           # host memory standing in for every pointer: a rejected call touches none of it
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 8)(*([p] * 8))               # a host array of (stand-in) device pointers, as losses / words are
    a = ctypes.addressof(ptrs)
    for j in (1, 2):
        assert f(None, p, 1, j, a, 1, p, a, 1, p, None) == 1
        assert f(p, None, 1, j, a, 1, p, a, 1, p, None) == 1
        for blocks in (0, -1, -2 ** 40, 2 ** 31, 2 ** 40):
            assert f(p, p, blocks, j, a, 1, p, a, 1, p, None) == 1, blocks
            assert f(p, p, blocks, j, None, 0, None, None, 0, None, None) == 1, blocks
        for n in (-1, 9, 2 ** 31 - 1, -2 ** 31):
            assert f(p, p, 1, j, a, n, p, a, 1, p, None) == 1, n
        for n in (-1, 5, 2 ** 31 - 1, -2 ** 31):
            assert f(p, p, 1, j, a, 1, p, a, n, p, None) == 1, n
        assert f(p, p, 1, j, a, 1, None, a, 0, p, None) == 1                       # losses without a place for their means
        assert f(p, p, 1, j, a, 8, None, None, 0, p, None) == 1
        assert f(p, p, 1, j, a, 0, p, a, 1, None, None) == 1                       # words without a sticky word
        assert f(p, p, 1, j, a, 1, p, a, 4, None, None) == 1
    for j in (0, -1, -2 ** 40):
        assert f(p, p, 1, j, a, 1, p, a, 1, p, None) == 1, j
        assert f(p, p, 1, j, None, 0, None, None, 0, None, None) == 1, j
    assert all(v == 0 for v in buf) and all(v == p for v in ptrs)


def test_accum_options_and_steps_per_epoch():
    from multitask_hydranet_amd.train import accum_options, optimizer_steps_per_epoch
    for adam in (True, False):
        assert accum_options({}, adam) == 1
        assert accum_options(dict(accum_steps=1), adam) == 1
        assert accum_options(dict(accum_steps=None), adam) == 1
    for k in (2, 3, 8, 128):
        assert accum_options(dict(accum_steps=k), True) == k
        with pytest.raises(ValueError):
            accum_options(dict(accum_steps=k), False)                              # the mean is handed to the HIP Adam
    for bad in (True, False, 0, -1, -8, 2.0, 1.5, "2", float("nan"), [2]):
        for adam in (True, False):
            with pytest.raises(ValueError):
                accum_options(dict(accum_steps=bad), adam)
    for (n, k), want in {(5, 2): 3, (4, 2): 2, (1, 2): 1, (7, 1): 7, (8, 8): 1, (9, 8): 2, (3, 128): 1, (0, 4): 0, (6, 3): 2}.items():
        assert optimizer_steps_per_epoch(n, k) == want, (n, k)


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def test_yardstick():
    g = np.random.default_rng(0)
    gs = [g.standard_normal(37).astype(np.float32) * np.float32(10.0 ** e) for e in (0, -3, 2, 1, -1)]
    frozen = [x.copy() for x in gs]
    # j == 1 ignores acc: garbage, NaNs or nothing at all give the same bits -- g's
    for acc in (None, np.full(37, np.nan, dtype=np.float32), g.standard_normal(37).astype(np.float32)):
        assert np.array_equal(bits(ref.accumulate(acc, gs[0], 1)), bits(gs[0]))
    special = np.array([-0.0, 1e-45, -1e-40, np.inf, -np.inf, np.nan], dtype=np.float32)
    assert np.array_equal(bits(ref.accumulate(None, special, 1)), bits(special))
    # one rounded operation per line, restated here
    a1 = ref.accumulate(None, gs[0], 1)
    a2 = ref.accumulate(a1, gs[1], 2)
    w = np.float32(0.5)
    assert np.array_equal(bits(a2), bits(a1 + w * (gs[1] - a1)))
    a3 = ref.accumulate(a2, gs[2], 3)
    w = np.float32(1.0 / 3.0)
    assert np.array_equal(bits(a3), bits(a2 + (w * (gs[2] - a2)).astype(np.float32)))
    assert np.array_equal(bits(ref.mean_of(gs[:3])), bits(a3))
    # close to the float64 mean (a sanity bound, not the contract: a few roundings of the largest term per step)
    m = ref.mean_of(gs)
    exact = np.mean(np.stack(gs).astype(np.float64), axis=0)
    scale = np.max(np.abs(np.stack(gs)), axis=0)
    assert np.all(np.abs(m - exact) <= 8 * 2.0 ** -24 * scale)
    # the mean of k identical arrays is that array exactly
    for k in (1, 2, 3, 7, 16):
        assert np.array_equal(bits(ref.mean_of([gs[0]] * k)), bits(gs[0])), k
    # a NaN or +-Inf anywhere in any micro-batch ends non-finite at that position and nowhere else
    for bad in (np.nan, np.inf, -np.inf):
        for at in range(4):
            for pos in (0, 17, 36):
                run = [x.copy() for x in gs[:4]]
                run[at][pos] = bad
                out = ref.mean_of(run)
                fin = np.isfinite(out)
                assert not fin[pos] and fin.sum() == 36, (bad, at, pos)
                clean = ref.mean_of(gs[:4])
                keep = np.arange(37) != pos
                assert np.array_equal(bits(out)[keep], bits(clean)[keep])
    # inputs are never modified
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(gs, frozen))


def test_yardstick_sticky_word():
    nan, inf = float("nan"), float("inf")
    assert ref.sticky(99, 1, [1.0, 2.0], [0, 0]) == 0                              # j == 1 resets, whatever the word held
    assert ref.sticky(0, 2, [1.0, nan], [0]) == 2
    assert ref.sticky(0, 2, [-inf], []) == 2 and ref.sticky(0, 2, [inf], []) == 2
    assert ref.sticky(0, 2, [], [0, 7]) == 4 and ref.sticky(0, 2, [1.0], [-1]) == 4
    assert ref.sticky(0, 3, [nan], [1]) == 6
    assert ref.sticky(4, 2, [1.0], [0]) == 4 and ref.sticky(2, 3, [1.0], [1]) == 6 # sticks
    assert ref.sticky(6, 1, [], []) == 0 and ref.sticky(6, 2, [], []) == 6
