"""numpy reference of the weight average kept inside the HIP Adam (hn_adam_step_ema, optim.Adam(ema_decay=)): the recurrence in float32
arrays, every numpy operation rounding once (numpy fuses nothing across calls), and the decay schedule restated independently of
multitask_hydranet_amd.optim.ema_decay_at."""
import numpy as np


def ema_step(e, p_new, decay):
    """e + float32(1 - decay) * (p_new - e): the weight is formed in double and rounded once, then three rounded float32 operations"""
    e = np.asarray(e, dtype=np.float32)
    p_new = np.asarray(p_new, dtype=np.float32)
    w = np.float32(1.0 - float(decay))
    d = np.subtract(p_new, e, dtype=np.float32)
    return np.add(e, np.multiply(w, d, dtype=np.float32), dtype=np.float32)


def ema_decay_at(n, decay, warmup=True):
    """decay of EMA step number n (0-based), in double: the warm-up ramp (1 + n) / (10 + n) until it reaches `decay`"""
    if not warmup:
        return float(decay)
    ramp = (1.0 + float(n)) / (10.0 + float(n))
    return ramp if ramp < float(decay) else float(decay)
