"""CPU: the host side of the BatchNorm-statistics guard and average (hn_state_guard, bn_state.options / BufferKeeper): the symbol is
declared and exported, bad arguments are rejected before any HIP call, the trainer keys' prerequisites, and the test suite's own
yardstick (tests/state_guard_ref.py).  No kernel is launched here."""
import ctypes

import numpy as np
import pytest

from tests import ema_ref, state_guard_ref as ref


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_entry_point(built):
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    assert "hn_state_guard" in sig and hasattr(dll, "hn_state_guard") and "hn_state_guard" in built.lib().symbols()
    ret, args, has_stream = sig["hn_state_guard"]
    assert ret is ctypes.c_int and has_stream                                      # a launcher: a status, and the stream last
    # (jobs, block_job, total_blocks, mode, record, ema_decay, stream): hn_swap_many's tables first
    assert args[:3] == sig["hn_swap_many"][1][:3]
    assert args[3:] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p]
    assert "hn_state.hip" in built.SOURCES


def test_bad_arguments_are_rejected_before_any_hip_call(built):
    f = built.lib().raw("hn_state_guard")
    buf = (ctypes.c_long * 64)()                           # host memory standing in for every pointer: a rejected call touches none of it
    p = ctypes.addressof(buf)
    for mode in (0, 1, 2):
        assert f(None, p, 1, mode, p, 0.5, None) == 1, mode
        assert f(p, None, 1, mode, p, 0.5, None) == 1, mode
        for blocks in (0, -1, -2 ** 40):
            assert f(p, p, blocks, mode, p, 0.5, None) == 1, (mode, blocks)
    for mode in (-1, 3, 4, 2 ** 31 - 1, -2 ** 31):
        assert f(p, p, 1, mode, p, 0.5, None) == 1, mode
        assert f(p, p, 1, mode, None, 0.5, None) == 1, mode
    for decay in (1.0, -0.1, float("nan"), 1.5, float("inf"), -float("inf")):
        assert f(p, p, 1, 2, p, decay, None) == 1, decay
        assert f(p, p, 1, 2, None, decay, None) == 1, decay
    assert all(v == 0 for v in buf)


def test_options():
    from multitask_hydranet_amd.bn_state import options
    guards = (dict(skip_nonfinite=True), dict(grad_clip_norm=1.0), dict(grad_clip_norm=0.5, skip_nonfinite=True))
    for adam in (True, False):
        assert options({}, adam) == (False, False)
        assert options(dict(protect_bn_stats=False, ema_buffers=False), adam) == (False, False)
        assert options(dict(protect_bn_stats=False, ema_buffers=False, ema_decay=0.9, skip_nonfinite=True), adam) == (False, False)
    for g in guards:
        assert options(dict(protect_bn_stats=True, **g), True) == (True, False)
        assert options(dict(protect_bn_stats=True, ema_buffers=True, ema_decay=0.9, **g), True) == (True, True)
        with pytest.raises(ValueError):
            options(dict(protect_bn_stats=True, **g), False)                       # needs the HIP Adam
        with pytest.raises(ValueError):
            options(dict(protect_bn_stats=True, ema_buffers=True, **g), True)      # the average's prerequisite is missing
    assert options(dict(ema_buffers=True, ema_decay=0.9), True) == (False, True)
    # no record to obey: neither guard key, or a clip norm that means "off"
    for t in (dict(protect_bn_stats=True), dict(protect_bn_stats=True, grad_clip_norm=0.0), dict(protect_bn_stats=True, grad_clip_norm=-1.0),
              dict(protect_bn_stats=True, grad_clip_norm=None, skip_nonfinite=False), dict(protect_bn_stats=True, ema_decay=0.9)):
        with pytest.raises(ValueError):
            options(t, True)
    # no weight average to ride along with
    for t in (dict(ema_buffers=True), dict(ema_buffers=True, ema_decay=None), dict(ema_buffers=True, ema_decay=0.0),
              dict(ema_buffers=True, ema_decay=-1.0), dict(ema_buffers=True, skip_nonfinite=True)):
        with pytest.raises(ValueError):
            options(t, True)
    with pytest.raises(ValueError):
        options(dict(ema_buffers=True, ema_decay=0.9), False)


def words(g, n):
    return g.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.int32)


def make_jobs(seed):
    """kinds 0 and 1, with and without shadow / average; kind 0 averaging inputs are ordinary floats"""
    g = np.random.default_rng(seed)
    jobs = []
    for i, n in enumerate((1, 2, 5, 1025)):
        for kind in (0, 1):
            for has_shadow, has_avg in ((True, True), (True, False), (False, True), (False, False)):
                fl = lambda: g.standard_normal(n).astype(np.float32).view(np.int32)
                jobs.append(dict(live=fl() if kind == 0 and has_avg else words(g, n), shadow=words(g, n) if has_shadow else None,
                                 avg=(fl() if kind == 0 else words(g, n)) if has_avg else None, kind=kind))
    return jobs


def same(a, b, keys=("live", "shadow", "avg")):
    return all((x[k] is None and y[k] is None) or np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in keys)


def test_yardstick():
    jobs = make_jobs(0)
    frozen = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in j.items()} for j in jobs]
    snap = ref.snapshot(jobs)
    assert same(jobs, frozen)                                                      # inputs are never modified
    assert same(snap, jobs, ("live", "avg"))
    assert all(np.array_equal(s["shadow"], j["live"]) for s, j in zip(snap, jobs) if j["shadow"] is not None)
    assert any(not np.array_equal(s["shadow"], j["shadow"]) for s, j in zip(snap, jobs) if j["shadow"] is not None)
    # a forward scribbles over live; a skipped settle after the snapshot is the identity on live, in both modes, for every skip mask
    g = np.random.default_rng(7)
    dirty = [dict(s, live=words(g, s["live"].size) if s["kind"] == 1 or s["avg"] is None else
                  g.standard_normal(s["live"].size).astype(np.float32).view(np.int32)) for s in snap]
    for decay in (None, 0.9):
        for skip in (1, 2, 4, 7):
            back = ref.settle(dirty, skip, decay)
            for b, j, d in zip(back, jobs, dirty):
                assert np.array_equal(b["live"], j["live"] if j["shadow"] is not None else d["live"])
            assert same(back, dirty, ("shadow", "avg"))                            # nothing else is written: the averages stay
    # skip == 0 (or no record): nothing is written to live or shadow; mode 1 writes nothing at all
    for skip in (0, None):
        assert same(ref.settle(dirty, skip), dirty)
        out = ref.settle(dirty, skip, 0.9)
        assert same(out, dirty, ("live", "shadow"))
        for o, d in zip(out, dirty):
            if d["avg"] is None:
                assert o["avg"] is None
            elif d["kind"] == 1:
                assert np.array_equal(o["avg"], d["live"])                         # the average of a counter is the counter
            else:
                want = ema_ref.ema_step(d["avg"].view(np.float32), d["live"].view(np.float32), 0.9)
                assert np.array_equal(o["avg"], want.view(np.int32))
    assert same(dirty, [dict(s, live=d["live"]) for s, d in zip(snap, dirty)])
