"""CPU: the host side of the weight average (hn_adam_step_ema / hn_swap_many, optim.Adam(ema_decay=, ema_warmup=), optim.ema_decay_at):
the symbols are declared and exported, bad arguments are rejected before any HIP call, the decay schedule, and the test suite's own
yardstick (tests/ema_ref.py).  No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ema_ref


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_average(built):
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    for name in ("hn_adam_step_ema", "hn_swap_many"):
        assert name in sig and hasattr(dll, name) and name in built.lib().symbols()
        assert sig[name][2] and sig[name][0] is ctypes.c_int                       # launchers: a status, and the stream last
    # (jobs, block_job, total_blocks, ema, <hn_adam_step's scalars>, ema_decay, record, stream)
    ema, adam = sig["hn_adam_step_ema"][1], sig["hn_adam_step"][1]
    assert ema[:3] == adam[:3] and ema[3] is ctypes.c_void_p and ema[4:10] == adam[3:9]
    assert ema[10] is ctypes.c_double and ema[11] is ctypes.c_void_p and len(ema) == 13
    # hn_copy_many's tables without the kind
    assert sig["hn_swap_many"][1] == sig["hn_copy_many"][1][:3] + sig["hn_copy_many"][1][4:]


def test_bad_arguments_are_rejected_before_any_hip_call(built):
    l = built.lib()
    ema, swap = l.raw("hn_adam_step_ema"), l.raw("hn_swap_many")
    buf = (ctypes.c_long * 64)()                           # host memory standing in for every pointer: a rejected call touches none of it
    p = ctypes.addressof(buf)
    # (jobs, block_job, total_blocks, ema, lr, beta1, beta2, eps, weight_decay, step, ema_decay, record, stream)
    for decay in (1.0, -0.1, float("nan"), 1.5, float("inf")):
        assert ema(p, p, 1, p, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, decay, None, None) == 1, decay
        assert ema(p, p, 1, p, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, decay, p, None) == 1, decay
    assert ema(p, p, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.5, None, None) == 1              # no table of averages
    assert ema(None, p, 1, p, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.5, None, None) == 1
    assert ema(p, None, 1, p, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.5, None, None) == 1
    assert ema(p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.5, None, None) == 1
    assert ema(p, p, 1, p, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0.5, None, None) == 1                 # steps count from 1
    assert ema(p, p, 1, p, 1e-3, 1.0, 0.999, 1e-8, 0.0, 1, 0.5, None, None) == 1
    assert swap(None, p, 1, None) == 1 and swap(p, None, 1, None) == 1 and swap(p, p, 0, None) == 1
    assert all(v == 0 for v in buf)


DECAYS = (0.9, 0.999, 0.9998)


def test_decay_schedule():
    from multitask_hydranet_amd.optim import ema_decay_at
    for decay in DECAYS:
        assert ema_decay_at(0, decay, True) == 0.1
        got = [ema_decay_at(n, decay, True) for n in range(100001)]
        assert all(isinstance(v, float) for v in got[:4])
        assert all(a <= b for a, b in zip(got, got[1:]))                            # monotone
        first = next(n for n in range(100001) if (1.0 + n) / (10.0 + n) >= decay)
        assert first > 0 and all(v < decay for v in got[:first]) and all(v == decay for v in got[first:]), (decay, first)
        assert got == [ema_ref.ema_decay_at(n, decay, True) for n in range(100001)]
        assert all(ema_decay_at(n, decay, False) == decay == ema_ref.ema_decay_at(n, decay, False) for n in (0, 1, 9, 100, 10 ** 5))
    assert ema_decay_at(0, 0.05, True) == 0.05                                      # a decay below the ramp's start is simply the decay


def test_reference_recurrence():
    g = np.random.default_rng(0)
    p = g.standard_normal(1000).astype(np.float32)
    for decay in (0.1, 0.5, 0.9998):
        assert np.array_equal(ema_ref.ema_step(p, p, decay).view(np.int32), p.view(np.int32))    # e == p stays e
    e0 = g.standard_normal(1000).astype(np.float32)
    for decay in (0.5, 0.9, 0.9998):
        e = e0
        for _ in range(10):
            e = ema_ref.ema_step(e, p, decay)
            assert e.dtype == np.float32
        w = float(np.float32(1.0 - decay))
        want = p.astype(np.float64) - (p.astype(np.float64) - e0.astype(np.float64)) * (1.0 - w) ** 10
        assert float(np.abs(e - want).max()) <= 1e-6 * float(np.abs(want).max()), decay


def test_off_values_are_off_and_bad_decays_raise():
    from multitask_hydranet_amd.optim import Adam
    w = torch.nn.Parameter(torch.zeros(3))
    for kw in ({}, dict(ema_decay=None), dict(ema_decay=None, ema_warmup=False)):
        o = Adam([w], 1e-3, **kw)
        assert o.ema_decay is None and o.ema_named([("w", w)]) == {}
        with pytest.raises(RuntimeError):
            o.swap_ema()                                   # nothing to exchange
    for bad in (1.0, -0.1, float("nan"), 2):
        with pytest.raises(ValueError):
            Adam([w], 1e-3, ema_decay=bad)
    o = Adam([w], 1e-3, ema_decay=0.9998, ema_warmup=False)
    assert o.ema_decay == 0.9998 and o.ema_warmup is False
    sd = o.state_dict()                                    # torch's layout, nothing added outside `state`
    assert set(sd) == {"state", "param_groups"} and set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "params"}
