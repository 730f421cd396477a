"""float64 restatement of one identity XBlock in training mode (oracle.hydranet_oracle.xblock at stride 1 with SE and no projection
shortcut; reference net/anynet.py:65-76), rounded to bf16 exactly where O.bf16_mirror() rounds -- i.e. where the HIP path stores bf16.

It returns every tensor the persistent stage launch (csrc/hn_xstage.hip: hn_xstage_fwd / hn_xstage_bwd) writes, in that launch's layouts
(NHWC activations, [3, 2, C] BatchNorm gradients, [N, C] / [N, Cs] SE vectors), so the launch can be held to a reference that shares no
code with it or with the launch chain (ops.XBlockFn).  Pinned to the oracle on the CPU by tests/test_xstage_gpu.py.

    r = forward(x, params)          # x [N, H, W, C]; params: the 19 tensors in ops.xstage.PER_BLOCK order
    g = backward(r, dout)           # dout [N, H, W, C]: the gradient of r["out"]
"""
import torch
import torch.nn.functional as F

# ops.xstage.PER_BLOCK order (XBlockFn.forward's arguments after x)
NAMES = ("w1", "g1", "b1", "rm1", "rv1", "w2", "g2", "b2", "rm2", "rv2", "sw1", "sb1", "sw2", "sb2", "w3", "g3", "b3", "rm3", "rv3")
RUNNING = ("rm1", "rv1", "rm2", "rv2", "rm3", "rv3")
# the trainable tensors and the names of their gradients in backward()'s result
GRADS = dict(w1="dw1", g1="dg1", b1="db1", w2="dw2", g2="dg2", b2="db2", sw1="dsw1", sb1="dsb1", sw2="dsw2", sb2="dsb2", w3="dw3",
             g3="dg3", b3="db3")
F64 = torch.float64


def bf16(t):
    """round to bf16 in the forward, identity in the backward (oracle.hydranet_oracle._r)"""
    return t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())


def _c(v):
    return v.view(1, -1, 1, 1)


def _bn(z, gamma, beta, rm, rv, eps, momentum):
    """training-mode BatchNorm2d: batch mean / biased variance normalise; the running variance takes the unbiased one"""
    count = z.shape[0] * z.shape[2] * z.shape[3]
    mean = z.mean((0, 2, 3))
    var = ((z - _c(mean)) ** 2).mean((0, 2, 3))
    y = (z - _c(mean)) / torch.sqrt(_c(var) + eps) * _c(gamma) + _c(beta)
    mean_d, var_d = mean.detach(), var.detach()
    rm_new = (1.0 - momentum) * rm + momentum * mean_d
    rv_new = (1.0 - momentum) * rv + momentum * var_d * (count / (count - 1.0))
    return y, mean_d, var_d, rm_new, rv_new


def forward(x, params, eps=1e-5, momentum=0.1):
    """x [N, H, W, C] (NHWC, any float dtype / device), params: 19 tensors in ops.xstage.PER_BLOCK order.  Computes in float64 on the CPU
    and leaves the inputs untouched.  -> dict of float64 CPU tensors:
      z1, a, z2, bg, z3, out            [N, H, W, C]  (bf16-valued, as stored)
      mean, var                         [3, C]        batch mean / biased variance of BatchNorm 1, 2, 3
      running                           dict rm1 .. rv3 after the update (momentum, unbiased variance)
      pooled, hid, gate                 [N, C], [N, Cs], [N, C]
    plus the autograd leaves and intermediates backward() needs."""
    p = {k: v.detach().to("cpu", F64) for k, v in zip(NAMES, params)}
    for k in GRADS:
        p[k].requires_grad_(True)
    c = p["w1"].shape[0]
    xin = x.detach().to("cpu", F64).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    z1 = bf16(F.conv2d(xin, bf16(p["w1"])))
    y1, m1, v1, rm1, rv1 = _bn(z1, p["g1"], p["b1"], p["rm1"], p["rv1"], eps, momentum)
    a = bf16(F.relu(y1))
    z2 = bf16(F.conv2d(a, bf16(p["w2"]), None, 1, 1, 1, c // p["w2"].shape[1]))
    y2, m2, v2, rm2, rv2 = _bn(z2, p["g2"], p["b2"], p["rm2"], p["rv2"], eps, momentum)
    b = bf16(F.relu(y2))
    pooled = b.mean((2, 3))
    pre1 = pooled @ p["sw1"].flatten(1).t() + p["sb1"]
    hid = F.relu(pre1)
    pre2 = hid @ p["sw2"].flatten(1).t() + p["sb2"]
    gate = torch.sigmoid(pre2)
    bg = bf16(b * gate[:, :, None, None])
    z3 = bf16(F.conv2d(bg, bf16(p["w3"])))
    y3, m3, v3, rm3, rv3 = _bn(z3, p["g3"], p["b3"], p["rm3"], p["rv3"], eps, momentum)
    out = bf16(F.relu(y3 + xin))
    for t in (z1, z2, z3, pre1, pre2):
        t.retain_grad()
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)
    return dict(z1=nhwc(z1), a=nhwc(a), z2=nhwc(z2), bg=nhwc(bg), z3=nhwc(z3), out=nhwc(out),
                mean=torch.stack([m1, m2, m3]), var=torch.stack([v1, v2, v3]),
                running=dict(rm1=rm1, rv1=rv1, rm2=rm2, rv2=rv2, rm3=rm3, rv3=rv3),
                pooled=pooled.detach(), hid=hid.detach(), gate=gate.detach(),
                _x=xin, _p=p, _t=dict(z1=z1, z2=z2, z3=z3, pre1=pre1, pre2=pre2, out=out))


def backward(r, dout):
    """autograd through forward()'s graph with the upstream gradient dout [N, H, W, C] (any dtype / device).  -> dict of float64 CPU tensors:
      dx, dz1, dz2, dz3                 [N, H, W, C]
      dgb                               [3, 2, C]  (dgamma, dbeta) of BatchNorm 1, 2, 3 -- hn_xstage_bwd's dgb layout
      dpre2, dpre1                      [N, C], [N, Cs]: gradients of the SE layers' pre-activations
      dw1, dw2, dw3, dsw1, dsb1, dsw2, dsb2, dg1 ... db3   in the parameters' shapes
    (one call per forward(): the graph is freed)"""
    t, p = r["_t"], r["_p"]
    t["out"].backward(dout.detach().to("cpu", F64).permute(0, 3, 1, 2))
    nhwc = lambda v: v.grad.detach().permute(0, 2, 3, 1)
    g = dict(dx=nhwc(r["_x"]), dz1=nhwc(t["z1"]), dz2=nhwc(t["z2"]), dz3=nhwc(t["z3"]), dpre2=t["pre2"].grad.detach(),
             dpre1=t["pre1"].grad.detach())
    g.update({GRADS[k]: p[k].grad.detach() for k in GRADS})
    g["dgb"] = torch.stack([torch.stack([g["dg1"], g["db1"]]), torch.stack([g["dg2"], g["db2"]]), torch.stack([g["dg3"], g["db3"]])])
    return g
