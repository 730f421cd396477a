"""train.loss_balance without a GPU: the two forms of tests/loss_balance_ref.py against each other, the float64 form's
analytic gradients against finite differences, the clamp's edges, inactive terms, and the cfg parsing."""
import numpy as np
import pytest

from tests import loss_balance_ref as R

F = np.float32


def _case(n, seed, zeros=()):
    rng = np.random.default_rng(seed)
    x = (10.0 ** rng.uniform(-6, 4, n)).astype(F)
    for i in zeros:
        x[i] = 0
    w = rng.uniform(0.5, 50.0, n).astype(F)
    grp = sorted(rng.integers(0, 3, n).tolist())
    grp = [sorted(set(grp)).index(g) for g in grp]
    gw = rng.uniform(0.5, 2.0, max(grp) + 1).astype(F)
    s = rng.uniform(-5.0, 5.0, n).astype(F)
    return x, w, grp, gw, list(range(n)), s


@pytest.mark.parametrize("n", [1, 3, 5, 6, 8])
def test_exact_form_against_float64(n):
    x, w, grp, gw, slot, s = _case(n, 10 + n, zeros=(1,) if n > 2 else ())
    clamp = 6.0
    tot64, e64 = R.f64_forward(x, w, grp, gw, slot, s, clamp)
    e = e64.astype(F)                                   # a correctly rounded expf: within the 2e-6 the bound allows
    tot, act = R.exact_forward(x, w, grp, gw, slot, s, clamp, e)
    bound = R.forward_bound(x, w, grp, gw, slot, s, clamp)
    assert abs(float(tot) - tot64) <= bound, (float(tot), tot64, bound)
    assert act.tolist() == (x != 0).tolist()
    seeds, ds = R.exact_backward(x, w, grp, gw, slot, s, clamp, e, F(1.0), n)
    dx64, ds64 = R.f64_backward(x, w, grp, gw, slot, s, clamp, 1.0, n)
    # seeds: 3 rounded products and e's rounding; ds = 1 - t gw: absolute error <= |t gw| (4 roundings) + 1 rounding of the difference
    np.testing.assert_allclose(seeds, dx64, rtol=4 * 2.0 ** -24 * 1.01, atol=0)
    t = np.abs(x.astype(np.float64) * w * e64 * np.asarray([gw[g] for g in grp], np.float64))
    for i in range(n):
        assert abs(float(ds[i]) - ds64[i]) <= (t[i] * 4 + abs(ds64[i]) + 1) * 2.0 ** -24 * 1.01
        assert ds[n + i] == (1.0 if x[i] != 0 else 0.0)


def test_zero_log_variances_give_the_static_sum_bit_for_bit():
    for n in (1, 3, 6, 8):
        x, w, grp, gw, slot, _ = _case(n, 40 + n, zeros=(0,) if n > 1 else ())
        s = np.zeros(n, F)
        e = np.ones(n, F)
        tot, _ = R.exact_forward(x, w, grp, gw, slot, s, 6.0, e)
        assert tot == R.weighted_forward(x, w, grp, gw)
        seeds, _ = R.exact_backward(x, w, grp, gw, slot, s, 6.0, e, F(0.37), n)
        assert (seeds == R.weighted_backward(w, grp, gw, F(0.37))).all()


def test_float64_gradients_against_finite_differences():
    x, w, grp, gw, slot, s = _case(6, 77)
    x = np.clip(x.astype(np.float64), 1e-2, 1e2)
    s = s.astype(np.float64) * 0.5
    dx, ds = R.f64_backward(x, w, grp, gw, slot, s, 6.0, 1.0, 6)
    f = lambda x_, s_: R.f64_forward(x_, w, grp, gw, slot, s_, 6.0)[0]
    for i in range(6):
        h = 1e-6 * x[i]
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        assert abs((f(xp, s) - f(xm, s)) / (2 * h) - dx[i]) <= 1e-6 * abs(dx[i]) + 1e-9
        sp, sm = s.copy(), s.copy()
        sp[i] += 1e-6
        sm[i] -= 1e-6
        assert abs((f(x, sp) - f(x, sm)) / 2e-6 - ds[i]) <= 1e-6 * (abs(ds[i]) + abs(f(x, s))) + 1e-9


def test_clamp_edges():
    """at or outside the clamp the gradient is kept only when a descent step moves s back inside, and the value used is the clamped one"""
    S = 2.0
    w, grp, gw, slot = [1.0, 1.0], [0, 0], [1.0], [0, 1]
    for x0, sign in ((100.0, -1), (1e-3, +1)):             # t gw > 1: ds < 0 (s grows); t gw < 1: ds > 0 (s shrinks)
        for s0 in (S, 2 * S, -S, -2 * S):
            x, s = [x0, 1.0], [s0, 0.0]
            e = np.exp(-R.clamp_s(s, S, np.float64)).astype(F)
            assert e[0] == F(np.exp(-np.sign(s0) * S))
            _, ds = R.exact_backward(x, w, grp, gw, slot, s, S, e, F(1), 2)
            _, ds64 = R.f64_backward(x, w, grp, gw, slot, s, S, 1.0, 2)
            inward = (s0 > 0 and sign > 0) or (s0 < 0 and sign < 0)
            assert (ds[0] != 0) == inward and (ds64[0] != 0) == inward
            if inward:
                assert np.sign(ds[0]) == sign
            assert ds[2] == 1.0                              # active all the same
    # NaN in a slot that a term owns: the clamp gives -S (fmaxf / fminf), the gradient is dropped
    e = np.exp(-R.clamp_s([np.nan, 0.0], S, np.float64)).astype(F)
    assert e[0] == F(np.exp(S))
    _, ds = R.exact_backward([1.0, 1.0], w, grp, gw, slot, [np.nan, 0.0], S, e, F(1), 2)
    assert ds[0] == 0.0


def test_inactive_terms_add_nothing():
    x, w, grp, gw, slot, s = _case(6, 5, zeros=(1, 4))
    e = np.exp(-R.clamp_s(s, 6.0, np.float64)).astype(F)
    tot, act = R.exact_forward(x, w, grp, gw, slot, s, 6.0, e)
    keep = [i for i in range(6) if i not in (1, 4)]
    sub = lambda a: [a[i] for i in keep]
    tot_sub, _ = R.exact_forward(sub(x), sub(w), sub(grp), gw, sub(slot), s, 6.0, sub(e))
    assert tot == tot_sub and act.tolist() == [True, False, True, True, False, True]
    _, ds = R.exact_backward(x, w, grp, gw, slot, s, 6.0, e, F(1), 6)
    assert ds[1] == 0 and ds[4] == 0 and ds[6 + 1] == 0 and ds[6 + 4] == 0 and all(ds[6 + i] == 1 for i in keep)
    # all inactive: the total is exactly 0
    tot0, _ = R.exact_forward(np.zeros(6, F), w, grp, gw, slot, s, 6.0, e)
    assert tot0 == 0


def test_cfg_parsing():
    from multitask_hydranet_amd.train import loss_balance_options as opt
    base = dict(lr=1e-3)
    assert opt(dict(base), True) is None
    assert opt(dict(base, loss_balance="none"), True) is None
    assert opt(dict(base, loss_balance="none", loss_balance_lr=-1), True) is None        # (read only when the key is on)
    assert opt(dict(base, loss_balance="uncertainty"), True) == dict(lr=1e-3, init=0.0, clamp=6.0)
    assert opt(dict(base, loss_balance="uncertainty", loss_balance_lr=0.01, loss_balance_init=-1, loss_balance_clamp=3), True) == \
        dict(lr=0.01, init=-1.0, clamp=3.0)
    for bad in ("gradnorm", "Uncertainty", True, 1, ""):
        with pytest.raises(ValueError):
            opt(dict(base, loss_balance=bad), True)
    with pytest.raises(ValueError):
        opt(dict(base, loss_balance="uncertainty"), False)                                 # needs the HIP Adam
    for key, bad in (("loss_balance_lr", 0), ("loss_balance_lr", -1e-3), ("loss_balance_lr", "fast"), ("loss_balance_lr", float("nan")),
                     ("loss_balance_clamp", 0), ("loss_balance_clamp", 81), ("loss_balance_clamp", True), ("loss_balance_init", 7.0),
                     ("loss_balance_init", float("inf")), ("loss_balance_init", None)):
        with pytest.raises(ValueError):
            opt(dict(base, loss_balance="uncertainty", **{key: bad}), True)
