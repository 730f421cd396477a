"""References of the HIP Adam (hn_adam_step, hn_adam_step_guarded, hn_adam_step_ema; adam_step_kernel in csrc/hn_loss.hip).

step()    the kernel's contract restated in numpy float32: one np.<op>(..., dtype=float32) per rounded operation, in the kernel's order,
          with the scalars formed as adam_launch forms them -- double arithmetic, rounded to fp32 once.  The kernel must give its bits.
step64()  textbook Adam in float64 with unrounded double scalars (L2 decay added to the gradient, bias-corrected moments, eps outside
          the root), with a first-order propagated rounding bound for m, v and p.  It is what keeps step() honest
          (tests/test_adam_ref_cpu.py): a fixed ulp count would not do, since g + wd p with |g| << wd |p| and m / denom with small v put
          the float32 sequence hundreds of ulps of the RESULT away from float64 by cancellation alone.
cases()   the inputs of tests/test_adam_exact_gpu.py, shared with the CPU test so that the bound is checked on exactly those."""
import functools
import math
import zlib

import numpy as np

from tests.ema_ref import ema_step

f32 = np.float32
U = 2.0 ** -24                                   # fp32 unit roundoff
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def scalars(lr, b1, b2, eps, wd, step):
    """adam_launch's kernel arguments: 1 - beta, 1 - beta ** step, lr / bias_correction1 and sqrt(bias_correction2) in double, rounded once"""
    bc1, bc2 = 1.0 - math.pow(b1, float(step)), 1.0 - math.pow(b2, float(step))
    return {"lr_over_bc1": f32(lr / bc1), "w1": f32(1.0 - b1), "b2": f32(b2), "w2": f32(1.0 - b2), "eps": f32(eps), "wd": f32(wd),
            "bc2_sqrt": f32(math.sqrt(bc2))}


def step(p, g, m, v, lr, b1, b2, eps, wd, step, coef=None):
    """one Adam step of float32 arrays -> (p', m', v'); coef (hn_adam_step_guarded's clipping coefficient, an fp32 value): the gradient is
    scaled by it first.  wd == 0 skips the decay term, as the kernel does."""
    s = scalars(lr, b1, b2, eps, wd, step)
    p, g, m, v = (np.asarray(a, dtype=f32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        if coef is not None:
            g = np.multiply(g, f32(coef), dtype=f32)
        if s["wd"] != 0:
            g = np.add(g, np.multiply(s["wd"], p, dtype=f32), dtype=f32)
        d = np.subtract(g, m, dtype=f32)
        m = np.add(m, np.multiply(s["w1"], d, dtype=f32), dtype=f32)
        g2 = np.multiply(g, g, dtype=f32)
        v = np.add(np.multiply(v, s["b2"], dtype=f32), np.multiply(s["w2"], g2, dtype=f32), dtype=f32)
        q = np.divide(np.sqrt(v, dtype=f32), s["bc2_sqrt"], dtype=f32)
        denom = np.add(q, s["eps"], dtype=f32)
        u = np.divide(m, denom, dtype=f32)
        p = np.subtract(p, np.multiply(s["lr_over_bc1"], u, dtype=f32), dtype=f32)
    return p, m, v


def step_ema(p, g, m, v, e, lr, b1, b2, eps, wd, step_, decay, coef=None):
    """hn_adam_step_ema: step(), then the moving average of the new parameter value (ema_ref.ema_step)"""
    p, m, v = step(p, g, m, v, lr, b1, b2, eps, wd, step_, coef)
    return p, m, v, ema_step(e, p, decay)


def step64(p, g, m, v, lr, b1, b2, eps, wd, step, coef=None, variant=None):
    """textbook Adam in float64 -> (p', m', v', bound_p, bound_m, bound_v).

    The bounds: every rounded operation of step()'s sequence (and every scalar rounded to fp32, counted like an operation) contributes
    u |its result| |d output / d that result|; the sum, to first order, bounds |step() - step64()|; times 2 for the neglected
    second-order terms.  variant (the CPU test's mutants, which must LEAVE the bound): "eps_inside" the root, "no_bc1" / "no_bc2" drop
    a bias correction, "decoupled" applies the decay to p instead of g."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    c = 1.0 if coef is None else float(f32(coef))                       # (the coefficient is an fp32 datum of the record, not a rounded scalar)
    w1, w2 = 1.0 - b1, 1.0 - b2
    bc1 = 1.0 if variant == "no_bc1" else 1.0 - b1 ** step
    bc2 = 1.0 if variant == "no_bc2" else 1.0 - b2 ** step
    l2 = 0.0 if variant == "decoupled" else wd
    with np.errstate(all="ignore"):
        a1 = c * g
        a2 = l2 * p
        gp = a1 + a2
        dg = (U * np.abs(a1) if coef is not None else 0.0) + (2 * U * np.abs(a2) + U * np.abs(gp) if wd != 0 else 0.0)
        d = gp - m
        dd = dg + U * np.abs(d)
        t1 = w1 * d
        m1 = m + t1
        dm = w1 * dd + 2 * U * np.abs(t1) + U * np.abs(m1)
        g2 = gp * gp
        dg2 = 2 * np.abs(gp) * dg + U * g2
        t2, t3 = w2 * g2, b2 * v
        v1 = t3 + t2
        dv = w2 * dg2 + 2 * U * t2 + 2 * U * t3 + U * v1
        r = np.sqrt(v1)
        dr = np.where(r > 0, dv / (2 * np.where(r > 0, r, 1.0)), 0.0) + U * r
        s2 = math.sqrt(bc2)
        if variant == "eps_inside":
            denom = np.sqrt(v1 / bc2 + eps)
            dden = dr / s2
        else:
            q = r / s2
            denom = q + eps
            dden = dr / s2 + 2 * U * q + U * eps + U * denom
        uu = m1 / denom
        duu = dm / denom + np.abs(uu) * dden / denom + U * np.abs(uu)
        lrb = lr / bc1
        t4 = lrb * uu
        p0 = p * (1.0 - lr * wd) if variant == "decoupled" else p
        p1 = p0 - t4
        dp = lrb * duu + 2 * U * np.abs(t4) + U * np.abs(p1)
    return p1, m1, v1, 2 * dp, 2 * dm, 2 * dv


# ---- the GPU test's inputs ---------------------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4099, 2, 257)      # one launch; tensor i's gradients are randn * 10 ** (i - 6): k = -6 .. 3
HYPER = ((0.0, 1e-2), (1e-2, 3e-4), (0.0, 3e-4), (1e-2, 1e-2))           # (weight decay, lr)
GMIN = 1e-15                                              # |g| >= GMIN unless planted as an exact zero: nothing goes denormal


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def grads(name, zero_at):
    """per tensor: randn * 10 ** k, |g| >= GMIN, exact zeros at the indices zero_at"""
    r = _rng(name)
    out = []
    for i, n in enumerate(SIZES):
        g = (r.standard_normal(n) * 10.0 ** (i - 6)).astype(f32)
        g = np.where(np.abs(g) < GMIN, np.copysign(f32(GMIN), g), g).astype(f32)
        for z in zero_at:
            if z < n:
                g[z] = 0.0
        out.append(g)
    return out


def params(name):
    r = _rng(name)
    return [(r.standard_normal(n) * 0.5).astype(f32) for n in SIZES]


def moments(name):
    """random state of a run in progress: m ~ gradient scale, v ~ its square; index 1 (where the zero gradient is planted) has ZERO moments
    behind it, index 2 non-zero ones"""
    r = _rng(name)
    ms, vs = [], []
    for i, n in enumerate(SIZES):
        sc = 10.0 ** (i - 6)
        m = (r.standard_normal(n) * sc * 0.3).astype(f32)
        v = ((r.standard_normal(n) * sc) ** 2 + (0.01 * sc) ** 2).astype(f32)
        if n > 1:
            m[1], v[1] = 0.0, 0.0
        ms.append(m)
        vs.append(v)
    return ms, vs


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, step number, p, g, m, v)]: a chain of steps 1, 2, 3 from zero moments (each entry starts from the reference's result of
    the one before; the tests chain the kernel's own results) as `chain`, and single steps 1000 and 100000 from random state"""
    p = params("p")
    zeros = [np.zeros(n, dtype=f32) for n in SIZES]
    chain = {"p": p, "m": zeros, "v": zeros,
             "g": [grads("g1", (1,)), grads("g2", (1, 2)), grads("g3", (1, 2))]}        # index 1: zero gradient on zero moments; 2: on live ones
    singles = []
    for st in (1000, 100000):
        m, v = moments(f"mv{st}")
        singles.append({"step": st, "p": params(f"p{st}"), "g": grads(f"g{st}", (1, 2)), "m": m, "v": v})
    return chain, singles


def run_chain(wd, lr, coef=None):
    """the reference's states after steps 1, 2, 3 of the chain: [(p, m, v) per tensor] per step"""
    chain, _ = cases()
    state = [(p, m, v) for p, m, v in zip(chain["p"], chain["m"], chain["v"])]
    out = []
    for it, gs in enumerate(chain["g"]):
        state = [step(p, g, m, v, lr, BETA1, BETA2, EPS, wd, it + 1, coef) for (p, m, v), g in zip(state, gs)]
        out.append(state)
    return out
