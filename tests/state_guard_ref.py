"""numpy yardstick of hn_state_guard's three modes (include/hydranet_hip.h) on int32 word arrays.

A job is a dict(live=, shadow=, avg=, kind=): int32 arrays of the same length, shadow / avg possibly None ("the job has none"); kind 0:
the words are fp32 values, kind 1: raw words.  Every function returns NEW jobs and leaves its inputs unchanged.  Restores and snapshots
copy words; the kind 0 average goes through tests.ema_ref.ema_step (three individually rounded float32 operations)."""
import numpy as np

from tests import ema_ref


def _copy(job, **new):
    out = {k: (None if v is None else (v.copy() if isinstance(v, np.ndarray) else v)) for k, v in job.items()}
    for k, v in new.items():
        assert v.dtype == np.int32 and v.shape == job["live"].shape
        out[k] = v.copy()
    return out


def snapshot(jobs):
    """mode 0: shadow = live for every job that has a shadow"""
    return [_copy(j, shadow=j["live"]) if j["shadow"] is not None else _copy(j) for j in jobs]


def settle(jobs, skip, ema_decay=None):
    """mode 1 (ema_decay None) / mode 2: skip (the record's word; None = no record = 0) != 0: live = shadow where there is a shadow,
    nothing else; else, in mode 2, every job that has an average: kind 0 avg = ema_step(avg, live, ema_decay), kind 1 avg = live"""
    if skip:
        return [_copy(j, live=j["shadow"]) if j["shadow"] is not None else _copy(j) for j in jobs]
    if ema_decay is None:
        return [_copy(j) for j in jobs]
    out = []
    for j in jobs:
        if j["avg"] is None:
            out.append(_copy(j))
        elif j["kind"] == 1:
            out.append(_copy(j, avg=j["live"]))
        else:
            new = ema_ref.ema_step(j["avg"].view(np.float32), j["live"].view(np.float32), ema_decay)
            out.append(_copy(j, avg=new.view(np.int32)))
    return out
