"""CPU: the float32 restatement of the HIP Adam's contract (tests/adam_ref.step, which tests/test_adam_exact_gpu.py demands bit for bit)
held to textbook Adam in float64 within a propagated rounding bound, on exactly the GPU test's inputs -- and the bound shown to be sharp
enough to mean something: the classic misreadings of Adam leave it."""
import numpy as np
import pytest

from tests import adam_ref as A

B1, B2, EPS = A.BETA1, A.BETA2, A.EPS


def single_steps(wd, lr):
    """(label, tensor index, step number, p, g, m, v) of every step the GPU test takes, one tensor each"""
    chain, singles = A.cases()
    states = [list(zip(chain["p"], chain["m"], chain["v"]))] + A.run_chain(wd, lr)[:-1]
    for it, gs in enumerate(chain["g"]):
        for i, ((p, m, v), g) in enumerate(zip(states[it], gs)):
            yield f"chain step {it + 1}, tensor {i}", i, it + 1, p, g, m, v
    for s in singles:
        for i in range(len(A.SIZES)):
            yield f"step {s['step']}, tensor {i}", i, s["step"], s["p"][i], s["g"][i], s["m"][i], s["v"][i]


def outside(got, want, bound):
    return ~(np.abs(got.astype(np.float64) - want) <= bound)


def test_inputs_are_what_the_gpu_test_promises():
    chain, singles = A.cases()
    assert A.SIZES[:8] == (1, 3, 4, 5, 1023, 1024, 1025, 4099) and len(A.SIZES) == 10          # gradient scales 10 ** -6 .. 10 ** 3
    for gs in chain["g"] + [s["g"] for s in singles]:
        for i, g in enumerate(gs):
            nz = g[g != 0]
            assert g.dtype == np.float32 and (nz.size == 0 or np.abs(nz).min() >= A.GMIN)
            if g.size > 1:
                assert g[1] == 0
            if g.size >= 1023:
                assert 0.5 * 10.0 ** (i - 6) < np.abs(g).mean() < 1.2 * 10.0 ** (i - 6)
    for s in singles:                                                     # a zero gradient on zero moments and one on live moments
        assert all(m[1] == 0 and v[1] == 0 for m, v in zip(s["m"], s["v"]) if m.size > 1)
        assert all(g[2] == 0 and m[2] != 0 and v[2] > 0 for g, m, v in zip(s["g"], s["m"], s["v"]) if m.size > 2)
    after1 = A.run_chain(0.0, 1e-2)[0]
    assert all(g[2] == 0 and st[1][2] != 0 for g, st in zip(chain["g"][1], after1) if g.size > 2)


@pytest.mark.parametrize("wd,lr", A.HYPER)
@pytest.mark.parametrize("coef", [None, 0.37])
def test_float32_sequence_stays_inside_the_float64_bound(wd, lr, coef):
    worst = 0.0
    for label, _, st, p, g, m, v in single_steps(wd, lr):
        got = A.step(p, g, m, v, lr, B1, B2, EPS, wd, st, coef)
        p64, m64, v64, bp, bm, bv = A.step64(p, g, m, v, lr, B1, B2, EPS, wd, st, coef)
        for nm, a, b, bound in (("p", got[0], p64, bp), ("m", got[1], m64, bm), ("v", got[2], v64, bv)):
            bad = outside(a, b, bound)
            assert not bad.any(), (f"{label} {nm}: {int(bad.sum())} elements outside the bound, first at {int(bad.argmax())}: "
                                   f"float32 {a[bad.argmax()]!r} float64 {b[bad.argmax()]!r} bound {bound[bad.argmax()]:.3e}")
            nzb = bound > 0
            if nzb.any():
                worst = max(worst, float((np.abs(a.astype(np.float64) - b)[nzb] / bound[nzb]).max()))
    assert worst > 0.02, f"the bound is slack everywhere (worst error / bound = {worst:.3f}): it would not notice a misreading"


@pytest.mark.parametrize("variant", ["eps_inside", "no_bc1", "no_bc2", "decoupled"])
def test_misread_adam_leaves_the_bound(variant):
    # eps inside the root only shows where sqrt(v) is not far above sqrt(eps) = 1e-4: without weight decay (wd p ~ 5e-3 would stand in for
    # the gradient), on the tensors whose gradients are 1e-2 and smaller (of the 1e-2 tensor, the few elements beyond two standard
    # deviations have sqrt(v) large enough to hide it: nine in ten must leave, not all)
    wd, lr = (0.0, 1e-2) if variant == "eps_inside" else (1e-2, 3e-4)
    left = total = 0
    for label, i, st, p, g, m, v in single_steps(wd, lr):
        if st > 3 or (variant == "eps_inside" and i > 4):
            continue                                                      # (1 - 0.9 ** 1000 == 1: a dropped correction is invisible there)
        got = A.step(p, g, m, v, lr, B1, B2, EPS, wd, st)
        _, _, _, bp, _, _ = A.step64(p, g, m, v, lr, B1, B2, EPS, wd, st)
        wrong = A.step64(p, g, m, v, lr, B1, B2, EPS, wd, st, variant=variant)[0]
        live = (g != 0) | (m != 0)
        left += int((outside(got[0], wrong, bp) & live).sum())
        total += int(live.sum())
    assert total > 1000 and left > 0.9 * total, f"{variant}: only {left} of {total} live elements leave the bound"
