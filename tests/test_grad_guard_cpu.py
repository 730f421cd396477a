"""CPU: the host side of the gradient guard (hn_grad_guard / hn_adam_step_guarded, optim.Adam(max_grad_norm=, skip_nonfinite=)): the
symbols are declared and exported, the workspace query states its range, bad arguments are rejected before any HIP call, and the
options' off values really are off.  No kernel is launched here."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_guard(built):
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    for name in ("hn_grad_guard_ws_bytes", "hn_grad_guard", "hn_adam_step_guarded"):
        assert name in sig and hasattr(dll, name) and name in built.lib().symbols()
    assert sig["hn_grad_guard"][2] and sig["hn_adam_step_guarded"][2] and not sig["hn_grad_guard_ws_bytes"][2]   # launchers take the stream
    assert sig["hn_grad_guard_ws_bytes"][0] is ctypes.c_long
    # hn_adam_step's arguments, then the record
    assert sig["hn_adam_step_guarded"][1][:-2] == sig["hn_adam_step"][1][:-1] and len(sig["hn_grad_guard"][1]) == 15


def test_workspace_query_range(built):
    q = lambda b, j: built.lib().query("hn_grad_guard_ws_bytes", b, j)
    for blocks, jobs in ((1, 1), (5, 2), (1173, 10), (171 * 1024, 693), (2 ** 31 - 1, 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        n = q(blocks, jobs)
        assert n > 0 and n % 16 == 0 and n >= 4 * blocks + 8 * jobs, (blocks, jobs, n)
    for blocks, jobs in ((-1, 1), (4, -1), (-3, -3), (2 ** 31, 1), (2 ** 40, 7), (4, 2 ** 40)):
        assert q(blocks, jobs) == -1, (blocks, jobs)
    assert q(4, 5) == -1                                   # a job owns at least one block


def test_bad_arguments_are_rejected_before_any_hip_call(built):
    l = built.lib()
    guard, adam = l.raw("hn_grad_guard"), l.raw("hn_adam_step_guarded")
    buf = (ctypes.c_long * 64)()                           # host memory standing in for every pointer: a rejected call touches none of it
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 9)(*([p] * 9))
    pa = ctypes.addressof(ptrs)
    ws = l.query("hn_grad_guard_ws_bytes", 1, 1)
    # (jobs, block_job, total_blocks, n_jobs, max_norm, flags, losses, n_losses, words, n_words, ws, ws_bytes, job_sq, record, stream)
    assert guard(None, None, 1, 1, 1.0, 1, None, 0, None, 0, None, 0, None, None, None) == 1
    assert guard(None, p, 1, 1, 1.0, 1, None, 0, None, 0, p, ws, None, p, None) == 1            # no job table
    assert guard(p, None, 1, 1, 1.0, 1, None, 0, None, 0, p, ws, None, p, None) == 1            # no block table
    assert guard(p, p, 1, 1, 1.0, 1, None, 0, None, 0, None, ws, None, p, None) == 1            # no workspace
    assert guard(p, p, 1, 1, 1.0, 1, None, 0, None, 0, p, ws, None, None, None) == 1            # no record
    assert guard(p, p, 1, 1, 1.0, 1, None, 0, None, 0, p, ws - 1, None, p, None) == 1           # workspace too small
    assert guard(p, p, 0, 1, 1.0, 1, None, 0, None, 0, p, ws, None, p, None) == 1               # tables out of range
    assert guard(p, p, 1, 2, 1.0, 1, None, 0, None, 0, p, ws, None, p, None) == 1
    assert guard(p, p, 1, 1, 1.0, 1, pa, 9, None, 0, p, ws, None, p, None) == 1                 # more than 8 losses
    assert guard(p, p, 1, 1, 1.0, 1, None, 0, pa, 5, p, ws, None, p, None) == 1                 # more than 4 words
    assert guard(p, p, 1, 1, 1.0, 1, None, 1, None, 0, p, ws, None, p, None) == 1               # a count without its array
    assert guard(p, p, 1, 1, 1.0, 1, None, 0, None, 1, p, ws, None, p, None) == 1
    assert guard(p, p, 1, 1, 1.0, 1, pa, -1, None, 0, p, ws, None, p, None) == 1
    assert guard(p, p, 1, 1, float("nan"), 1, None, 0, None, 0, p, ws, None, p, None) == 1
    null = (ctypes.c_void_p * 2)(p, None)
    assert guard(p, p, 1, 1, 1.0, 1, ctypes.addressof(null), 2, None, 0, p, ws, None, p, None) == 1   # a null loss pointer
    # (jobs, block_job, total_blocks, lr, beta1, beta2, eps, weight_decay, step, record, stream)
    assert adam(None, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None) == 1
    assert adam(p, p, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None) == 1                       # no record
    assert adam(None, p, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, p, None) == 1
    assert adam(p, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, p, None) == 1
    assert adam(p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, p, None) == 1
    assert adam(p, p, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, p, None) == 1                          # steps count from 1
    assert adam(p, p, 1, 1e-3, 1.0, 0.999, 1e-8, 0.0, 1, p, None) == 1


def test_off_values_are_off():
    from multitask_hydranet_amd.optim import Adam
    w = torch.nn.Parameter(torch.zeros(3))
    for kw in ({}, dict(max_grad_norm=None), dict(max_grad_norm=-1), dict(max_grad_norm=0), dict(max_grad_norm=0.0, skip_nonfinite=False)):
        o = Adam([w], 1e-3, **kw)
        assert not o.guarded and o.max_grad_norm is None and o.guard_record is None, kw
        with pytest.raises(ValueError):
            o.step(losses=[torch.zeros(())])               # nothing would look at them
        with pytest.raises(RuntimeError):
            o.grad_guard_record()
    assert Adam([w], 1e-3, max_grad_norm=2).max_grad_norm == 2.0 and Adam([w], 1e-3, max_grad_norm=2).guarded
    assert Adam([w], 1e-3, skip_nonfinite=True).guarded and Adam([w], 1e-3, skip_nonfinite=True).max_grad_norm is None
    with pytest.raises(ValueError):
        Adam([w], 1e-3, max_grad_norm=float("nan"))
    # the guard's counters are not optimizer state: torch's layout, nothing added
    sd = Adam([w], 1e-3, max_grad_norm=2, skip_nonfinite=True).state_dict()
    assert set(sd) == {"state", "param_groups"} and set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "params"}
