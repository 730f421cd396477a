"""tests/bn_ref.py, the float64 reference of the BatchNorm kernel tests, held to F.batch_norm (forward and running statistics) and to
autograd (backward) at 1e-12, for every activation code, with and without a residual, with the saved-output mask, and at a
constant channel (variance 0)."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as B

F64 = torch.float64
TOL = 1e-12


def close(got, want, name):
    err = float((got - want).abs().max())
    ref = max(float(want.abs().max()), 1.0)
    assert err <= TOL * ref, f"{name}: max err {err:.3e} (ref max {ref:.3e})"


def data(m, c, seed, const_channel=True):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(m, c, generator=g, dtype=F64) * 3.0 + torch.randn(c, generator=g, dtype=F64) * 5.0
    if const_channel:
        z[:, 0] = 2.5                                      # variance 0: rstd = eps^-1/2
        z[:, 1] = 0.0
    gamma = torch.rand(c, generator=g, dtype=F64) + 0.5
    beta = torch.randn(c, generator=g, dtype=F64)
    rm = torch.randn(c, generator=g, dtype=F64)
    rv = torch.rand(c, generator=g, dtype=F64) + 0.5
    return g, z, gamma, beta, rm, rv


def to_nchw(x):
    return x.t().reshape(1, x.shape[1], x.shape[0], 1)


def from_nchw(x):
    return x.reshape(x.shape[1], -1).t()


@pytest.mark.parametrize("m,c,eps,momentum", [(2, 16, 1e-5, 0.1), (3, 8, 1e-3, 1.0), (120, 24, 1e-5, 0.01), (1000, 40, 1e-3, 0.1)])
def test_forward_and_running_statistics(m, c, eps, momentum):
    _, z, gamma, beta, rm, rv = data(m, c, m * 7 + c)
    rm_t, rv_t = rm.clone(), rv.clone()
    want = from_nchw(F.batch_norm(to_nchw(z), rm_t, rv_t, gamma, beta, True, momentum, eps))
    st = B.stats(z, gamma, beta, eps)
    close(B.apply(z, st["scale"], st["shift"], B.ACT_NONE), want, "apply")
    rm_n, rv_n = B.running(rm, rv, st["mean"], st["var"], m, momentum)
    close(rm_n, rm_t, "running_mean")
    close(rv_n, rv_t, "running_var")
    assert float(st["rstd"][0]) == pytest.approx(eps ** -0.5, rel=1e-15)
    # the same through partial row blocks of every size: block_sums + finalize == stats
    for rb in (1, 7, m, m + 5):
        s1, s2 = B.block_sums(z, rb)
        assert s1.shape[0] == (m + rb - 1) // rb
        st2 = B.finalize(s1.sum(0), s2.sum(0), m, gamma, beta, eps)
        for k in ("mean", "var", "rstd", "scale", "shift"):
            close(st2[k], st[k], f"finalize {k} rb={rb}")
    # eval mode
    sc, sh = B.eval_coeff(gamma, beta, rm, rv, eps)
    close(B.apply(z, sc, sh, B.ACT_NONE), from_nchw(F.batch_norm(to_nchw(z), rm, rv, gamma, beta, False, momentum, eps)), "eval")


def test_group_sums_ragged():
    p = torch.arange(23 * 3, dtype=F64).view(23, 3)
    out = B.group_sums(p, 5)                               # S = 5: groups of 5, 5, 5, 5, 3
    assert out.shape == (5, 3)
    close(out.sum(0), p.sum(0), "group total")
    close(out[4], p[20:].sum(0), "last group")


TORCH_ACTS = {0: lambda x: x, 1: F.relu, 2: lambda x: x * torch.sigmoid(x), 3: F.elu, 4: torch.sigmoid}


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("res", [False, True])
def test_apply_and_backward_against_autograd(act, res):
    m, c, eps = 96, 16, 1e-5
    g, z, gamma, beta, _, _ = data(m, c, 31 + act * 2 + res)
    r = torch.randn(m, c, generator=g, dtype=F64) if res else None
    rs = torch.rand(c, generator=g, dtype=F64) + 0.5 if res else None
    rh = torch.randn(c, generator=g, dtype=F64) if res else None
    dout = torch.randn(m, c, generator=g, dtype=F64)
    zt, gt, bt = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = from_nchw(F.batch_norm(to_nchw(zt), None, None, gt, bt, True, 0.1, eps))
    if res:
        y = y + r * rs + rh
    y = TORCH_ACTS[act](y)
    y.backward(dout)
    st = B.stats(z, gamma, beta, eps)
    close(B.apply(z, st["scale"], st["shift"], act, r, rs, rh), y.detach(), "apply")
    # backward through the BatchNorm: g is the gradient at its output (the activation of the residual sum: the pre-activation with res)
    pre = B.pre_act(z, st["scale"], st["shift"], r, rs, rh)
    gin = dout * B.act_grad(pre, act)
    if not res:
        close(gin, B.grad_in(dout, z, st["scale"], st["shift"], act), "grad_in")
    bw = B.backward(gin, z, st["mean"], st["rstd"], st["scale"])
    close(bw["dz"], zt.grad, "dz")
    close(bw["dgamma"], gt.grad, "dgamma")
    close(bw["dbeta"], bt.grad, "dbeta")


def test_masked_backward_against_autograd():
    """y = relu(bn(z) + res) saved: g = dout * [y > 0]"""
    m, c, eps = 64, 8, 1e-3
    g, z, gamma, beta, _, _ = data(m, c, 5, const_channel=False)
    r = torch.randn(m, c, generator=g, dtype=F64)
    dout = torch.randn(m, c, generator=g, dtype=F64)
    zt = z.clone().requires_grad_(True)
    y = F.relu(from_nchw(F.batch_norm(to_nchw(zt), None, None, gamma, beta, True, 0.1, eps)) + r)
    y.backward(dout)
    st = B.stats(z, gamma, beta, eps)
    gin = B.grad_in(dout, z, st["scale"], st["shift"], B.ACT_NONE, y=y.detach())
    close(B.backward(gin, z, st["mean"], st["rstd"], st["scale"])["dz"], zt.grad, "dz")


def test_gamma_n():
    assert B.gamma_n(1) == pytest.approx(2.0 ** -24, rel=1e-6)
    assert B.gamma_n(128) > 128 * 2.0 ** -24
