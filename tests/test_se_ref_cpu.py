"""tests/se_ref.py, the float64 reference of the SE and elementwise kernel tests, held to autograd in float64 on
x * sigmoid(W2 relu(W1 avgpool(x) + b1) + b2) (values and all five gradients, for the MLP shapes of the GPU tests, with the squeeze and
the gate gradient going through partial rows), and the elementwise ops held to their torch equivalents."""
import pytest
import torch
import torch.nn.functional as F

from tests import se_ref as R

F64 = torch.float64
TOL = 1e-12


def close(got, want, name):
    """elementwise: |got - want| <= TOL * (|want| + the largest magnitude of the tensor's row of sums, which bounds the cancellation)"""
    err = (got - want).abs()
    bound = TOL * (want.abs() + want.abs().max() + 1e-300)
    bad = ~(err <= bound)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} values differ, first at {bad.nonzero()[0].tolist()}, max err {float(err.max()):.3e}"


SHAPES = sorted(set(R.MLP_FWD_SHAPES + R.MLP_BWD_SHAPES))


@pytest.mark.parametrize("c,cs", SHAPES, ids=[f"c{c}_cs{cs}" for c, cs in SHAPES])
@pytest.mark.parametrize("n,hw,rb", [(1, 1, 1), (3, 12, 4), (2, 15, 1)])
def test_se_block_against_autograd(c, cs, n, hw, rb):
    g = torch.Generator().manual_seed(c * 131 + cs * 7 + n + hw)
    x = (torch.randn(n, hw, c, generator=g, dtype=F64) * 2).to(torch.bfloat16).to(F64)     # bf16 values: gate_apply's rounding is the identity
    w1 = torch.randn(cs, c, generator=g, dtype=F64) / c ** 0.5
    b1 = torch.randn(cs, generator=g, dtype=F64) * 0.3
    w2 = torch.randn(c, cs, generator=g, dtype=F64) / cs ** 0.5
    b2 = torch.randn(c, generator=g, dtype=F64) * 0.3
    dout = torch.randn(n, hw, c, generator=g, dtype=F64)
    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    xa, w1a, b1a, w2a, b2a = leaves
    pa = xa.mean(1)
    gate_a = torch.sigmoid(F.linear(F.relu(F.linear(pa, w1a, b1a)), w2a, b2a))
    out_a = xa * gate_a[:, None, :]
    out_a.backward(dout)

    S = hw // rb
    xr, dr = x.view(n * hw, c), dout.view(n * hw, c)
    parts = xr.view(n * S, rb, c).sum(1)
    p = R.pooled(parts, S, 1.0 / hw)
    close(p, pa.detach(), "pooled")
    hid, pre2, gate = R.mlp_fwd(p, w1, b1, w2, b2)
    close(gate, gate_a.detach(), "gate")
    close(torch.sigmoid(pre2), gate, "gate = sigmoid(pre2)")
    out = R.gate_apply(xr, None, None, 0, gate, hw)
    close(out, out_a.detach().view(n * hw, c), "gate_apply")
    dparts = R.dgate_parts(dr, xr, rb, hw)
    assert dparts.shape == (n * S, c)
    bw = R.mlp_bwd(dparts, gate, hid, p, w1, w2, S=S)
    bw1 = R.mlp_bwd(dparts.view(n, S, c).sum(1), gate, hid, p, w1, w2)
    for k in bw:
        close(bw1[k], bw[k], f"mlp_bwd {k}: S partial rows against their sum")
    dx = R.data_bwd(dr, gate, bw["dpool"], hw)
    close(dx, xa.grad.view(n * hw, c), "data_bwd (dx)")
    close(bw["dw1"], w1a.grad, "dw1")
    close(bw["db1"], b1a.grad, "db1")
    close(bw["dw2"], w2a.grad, "dw2")
    close(bw["db2"], b2a.grad, "db2")
    assert bool((bw["dpre1"][hid <= 0] == 0).all()), "dpre1 not masked where hid <= 0"


def test_gate_apply_coefficients_and_rounding():
    g = torch.Generator().manual_seed(5)
    n, hw, c = 2, 7, 16
    z = torch.randn(n * hw, c, generator=g, dtype=F64)
    sc, sh = torch.rand(c, generator=g, dtype=F64) + 0.5, torch.randn(c, generator=g, dtype=F64)
    gate = torch.rand(n, c, generator=g, dtype=F64)
    for act, fn in ((0, lambda v: v), (1, F.relu)):
        y = fn(z * sc + sh).float().to(torch.bfloat16).double()
        want = (y.view(n, hw, c) * gate[:, None, :]).view(n * hw, c)
        assert torch.equal(R.gate_apply(z, sc, sh, act, gate, hw), want)


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_eltwise_against_torch(act):
    g = torch.Generator().manual_seed(11 + act)
    a = torch.randn(9, 16, generator=g, dtype=F64)
    b = torch.randn(9, 16, generator=g, dtype=F64)
    fwd = {0: lambda v: v, 1: F.relu, 2: F.silu, 3: F.elu, 4: torch.sigmoid}[act]
    close(R.eltwise(0, a, b), a + b, "op 0")
    close(R.eltwise(2, a, alpha=0.25), 0.25 * a, "op 2")
    close(R.eltwise(3, a, act=act), fwd(a), "op 3")
    pre = b.clone().requires_grad_(True)
    y = fwd(pre)
    y.backward(a)
    close(R.eltwise(4, a, b, act=act), pre.grad, "op 4 (pre-activation)")
    if act in (1, 3):
        close(R.eltwise(1, a, y.detach(), act=act), pre.grad, "op 1 (post-activation)")


def test_add_and_cast_against_torch():
    g = torch.Generator().manual_seed(3)
    o, b0, b1, b2 = (torch.randn(5, 8, generator=g, dtype=F64) for _ in range(4))
    assert torch.equal(R.add_n(o, b0), o + b0)
    assert torch.equal(R.add_n(o, b0, b1, b2), o + b0 + b1 + b2)
    n, ho, wo, c = 2, 3, 5, 8
    dx = torch.randn(n, 2 * ho, 2 * wo, c, generator=g, dtype=F64)
    full = torch.zeros(n, 2 * ho, 2 * wo, c, dtype=F64).requires_grad_(True)
    # the forward gathers the even rows and columns: its backward scatters dxs there
    dxs = torch.randn(n, ho, wo, c, generator=g, dtype=F64)
    full[:, ::2, ::2, :].backward(dxs)
    assert torch.equal(R.add_strided2(dx, dxs), dx + full.grad)
    src = torch.randn(4, 5, generator=g, dtype=F64)
    assert torch.equal(R.cast_pad(src, 8), F.pad(src, (0, 3)))
