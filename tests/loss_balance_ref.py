"""numpy restatement of hn_balanced_sum (csrc/hn_loss.hip), in two forms.

(a) exact_*: the kernel's own sequence of individually rounded fp32 operations.  The multipliers e_i = expf(-s~_i) are an INPUT here (the
    device's expf is held to exp() separately, at the bound the project gives it), so everything else can be compared with ==.
(b) f64_*: the same quantities in float64 from s, with the analytic gradients.

Terms are given as parallel sequences: x (losses), w (term weights), grp (non-decreasing group id per term), gw (weight per group id),
slot (the entry of s / ds a term owns, strictly increasing).  A term is active when x != 0.
"""
import numpy as np

F = np.float32


def clamp_s(s, clamp, dtype=F):
    """min(max(s, -S), S) with fminf / fmaxf's handling of NaN (the other operand)"""
    s = np.asarray(s, dtype)
    return np.fmin(np.fmax(s, dtype(-clamp)), dtype(clamp))


def weighted_forward(x, w, grp, gw):
    """hn_weighted_sum's forward: the parent's association order, every operation rounded to fp32"""
    tot, i, n = F(0), 0, len(x)
    while i < n:
        g = grp[i]
        s = F(x[i]) * F(w[i])
        i += 1
        while i < n and grp[i] == g:
            s = F(s + F(x[i]) * F(w[i]))
            i += 1
        tot = F(tot + F(s * F(gw[g])))
    return tot


def weighted_backward(w, grp, gw, gout):
    return np.array([F(F(F(gout) * F(gw[grp[i]])) * F(w[i])) for i in range(len(w))], F)


def exact_forward(x, w, grp, gw, slot, s, clamp, e):
    """-> (total, active [n] bool); e [n] fp32: the multipliers the device formed"""
    n = len(x)
    x = np.asarray(x, F)
    act = x != 0
    sc = clamp_s(np.asarray(s, F)[list(slot)], clamp)
    tot, i = F(0), 0
    while i < n:
        g, sg, first = grp[i], F(0), True
        while i < n and grp[i] == g:
            if act[i]:
                t = F(F(x[i] * F(w[i])) * F(e[i]))
                sg = t if first else F(sg + t)
                first = False
            i += 1
        tot = F(tot + F(sg * F(gw[g])))
    for i in range(n):
        if act[i]:
            tot = F(tot + sc[i])
    return tot, act


def exact_backward(x, w, grp, gw, slot, s, clamp, e, gout, n_slots):
    """-> (seeds [n], ds [2 * n_slots]: the gradient by slot, then the activity by slot)"""
    n = len(x)
    x, s, go, S = np.asarray(x, F), np.asarray(s, F), F(gout), F(clamp)
    seeds, ds = np.zeros(n, F), np.zeros(2 * n_slots, F)
    for i in range(n):
        gwi = F(gw[grp[i]])
        seeds[i] = F(F(F(go * gwi) * F(w[i])) * F(e[i]))
        if x[i] == 0:
            continue
        t = F(F(x[i] * F(w[i])) * F(e[i]))
        d = F(go * F(F(1) - F(t * gwi)))
        sv = s[slot[i]]
        keep = (-S < sv < S) or (sv >= S and d > 0) or (sv <= -S and d < 0)
        ds[slot[i]] = d if keep else F(0)
        ds[n_slots + slot[i]] = F(1)
    return seeds, ds


def f64_forward(x, w, grp, gw, slot, s, clamp):
    """-> (total, e [n]) in float64"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    sc = clamp_s(np.asarray(s, np.float64)[list(slot)], clamp, np.float64)
    e = np.exp(-sc)
    act = x != 0
    gwt = np.asarray([gw[g] for g in grp], np.float64)
    return float(np.sum(np.where(act, x * w * e * gwt + sc, 0.0))), e


def f64_backward(x, w, grp, gw, slot, s, clamp, gout, n_slots):
    """analytic d total / d x [n] and d total / d s [n_slots] in float64 (the clamp's rule as the kernel's; inactive terms: ds = 0)"""
    x, w, s = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(s, np.float64)
    _, e = f64_forward(x, w, grp, gw, slot, s, clamp)
    gwt = np.asarray([gw[g] for g in grp], np.float64)
    dx = gout * gwt * w * e
    ds = np.zeros(n_slots)
    for i in range(len(x)):
        if x[i] == 0:
            continue
        d = gout * (1.0 - x[i] * w[i] * e[i] * gwt[i])
        sv = s[slot[i]]
        if (-clamp < sv < clamp) or (sv >= clamp and d > 0) or (sv <= -clamp and d < 0):
            ds[slot[i]] = d
    return dx, ds


def forward_bound(x, w, grp, gw, slot, s, clamp, e_rtol=2e-6):
    """|fp32 total (a) - float64 total (b)| is at most this.  Every magnitude below is of the float64 values.  A product of k factors,
    each rounded, is off by (1 + u)^k - 1 <= 1.01 k u relative (u = 2^-24); e_i carries the device expf's relative error e_rtol on
    top.  A term |t_i| gw passes through 3 products (x w, x e, x gw) and through at most 7 + 8 further additions of the running sums
    (<= 8 terms, then <= 8 regulariser terms), each of which rounds a partial sum whose magnitude is at most the sum of all
    magnitudes A = sum |t_i gw| + sum |s~_i|: total error <= A * (e_rtol + 1.01 u (3 + 16)), plus conversions of w, gw, s to fp32
    (inputs here are fp32 already)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    sc = clamp_s(np.asarray(s, np.float64)[list(slot)], clamp, np.float64)
    gwt = np.asarray([gw[g] for g in grp], np.float64)
    act = x != 0
    A = float(np.sum(np.where(act, np.abs(x * w * np.exp(-sc) * gwt) + np.abs(sc), 0.0)))
    u = 2.0 ** -24
    return A * (e_rtol + 1.01 * u * 19) + 1e-45
