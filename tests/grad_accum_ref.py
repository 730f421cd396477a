"""numpy reference of gradient accumulation (hn_grad_accum, optim.GradAccumulator): the running mean in float32 arrays, every numpy
operation rounding once (numpy fuses nothing across calls), and the sticky word's rule.  Inputs are never modified."""
import numpy as np


def accumulate(acc, g, j):
    """the accumulator after micro-batch j (1-based) of a group: j == 1: a copy of g, bit for bit (acc is not looked at, it may be None);
    j > 1: acc + float32(1 / j) * (g - acc), the weight formed in double and rounded once, then three rounded float32 operations"""
    g = np.asarray(g, dtype=np.float32)
    if j < 1:
        raise ValueError("j is 1-based")
    if j == 1:
        return g.copy()
    acc = np.asarray(acc, dtype=np.float32)
    w = np.float32(1.0 / float(j))
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.subtract(g, acc, dtype=np.float32)
        t = np.multiply(w, d, dtype=np.float32)
        return np.add(acc, t, dtype=np.float32)


def mean_of(list_of_g):
    """the accumulator after the micro-batches of list_of_g, in order"""
    acc = None
    for j, g in enumerate(list_of_g, start=1):
        acc = accumulate(acc, g, j)
    return acc


def sticky(prev, j, losses, words):
    """the sticky word after micro-batch j: bits = 2 if any loss is not finite, | 4 if any word is non-zero; j == 1: bits (prev is not
    looked at), else prev | bits"""
    bits = 0
    if any(not np.isfinite(np.float32(l)) for l in losses):
        bits |= 2
    if any(int(w) != 0 for w in words):
        bits |= 4
    return bits if j == 1 else (int(prev) | bits)
