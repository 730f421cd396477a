"""Float64 reference of the squeeze-excite (SE) passes of csrc/hn_norm.hip and csrc/hn_fused.hip and of the small elementwise kernels,
pass by pass.  Plain torch on float64 CPU tensors; activations are [rows, C] (NHWC flattened, rows = N * HW), the MLP works on [N, C] /
[N, Cs] vectors, w1 is [Cs, C], w2 is [C, Cs].  The passes:
  pooled        the squeeze from S partial rows per image: alpha * their sum
  mlp_fwd       hid = relu(W1 p + b1), pre2 = W2 hid + b2, gate = sigmoid(pre2)
  gate_apply    bf16(act(scale * z + shift)) * gate[image]
  dgate_parts   per-row-block sums of dbg * b inside one image (the gate gradient as partial rows)
  mlp_bwd       dpre2 = dgate g (1 - g), dpre1 = [hid > 0] W2^T dpre2, dpool = W1^T dpre1 and the four parameter gradients
  data_bwd      dout * gate[image] + dpool[image] / HW
  eltwise       hn_eltwise's ops 0-4 as the comment above ew_kernel defines them; add_n, add_strided2, cast_pad
tests/test_se_ref_cpu.py holds all of it to autograd and to the torch equivalents."""
import torch

from tests.bn_ref import act_fwd, act_grad, gamma_n                       # noqa: F401  (gamma_n: re-exported for the bounds of the GPU tests)

F64 = torch.float64
BF16 = torch.bfloat16

# (C, Cs) of the MLP cases: the forward walks the contraction in rounds of 1024 and pairs outputs (1032 crosses the round; Cs 7 and 1
# leave an unpaired output); the backward cuts it into 64 / 16 partitions (C = 24: empty ones, > 1024: a second round) and 16-output tiles
# (C = 16: one tile, one workgroup in every launch)
MLP_FWD_SHAPES = [(24, 6), (152, 38), (936, 234), (1032, 7), (64, 1)]
MLP_BWD_SHAPES = [(16, 4), (24, 6), (40, 10), (152, 38), (936, 234), (1032, 17), (24, 300)]


def bf16_round(x):
    return x.to(torch.float32).to(BF16).to(F64)


def pooled(parts, S, alpha):
    """parts [N * S, C] (S partial rows per image) -> [N, C] = alpha * sum of the image's rows"""
    p = parts.to(F64)
    return alpha * p.view(-1, S, p.shape[1]).sum(1)


def mlp_fwd(pooled, w1, b1, w2, b2):
    """-> hid [N, Cs], pre2 [N, C], gate [N, C]"""
    hid = (pooled.to(F64) @ w1.to(F64).t() + b1.to(F64)).clamp(min=0.0)
    pre2 = hid @ w2.to(F64).t() + b2.to(F64)
    return hid, pre2, torch.sigmoid(pre2)


def gate_apply(z, scale, shift, act, gate, hw):
    """the bf16-rounded activation times the gate of the row's image: z [N * hw, C], gate [N, C]; scale / shift None = identity"""
    x = z.to(F64)
    if scale is not None:
        x = x * scale.to(F64) + shift.to(F64)
    return bf16_round(act_fwd(x, act)) * gate.to(F64).repeat_interleave(hw, 0)


def dgate_parts(dbg, b, rb, hw):
    """sums of dbg * b over row blocks of rb rows (rb divides hw: a block lies inside one image) -> [rows / rb, C]"""
    assert hw % rb == 0 and dbg.shape[0] % hw == 0
    p = dbg.to(F64) * b.to(F64)
    return p.view(-1, rb, p.shape[1]).sum(1)


def mlp_bwd(dgate, gate, hid, pooled, w1, w2, S=0):
    """dgate [N, C], or with S > 0 [N * S, C] partial rows summed first -> dict of dpre2 [N, C], dpre1 [N, Cs], dpool [N, C], dw1 [Cs, C],
    db1 [Cs], dw2 [C, Cs], db2 [C]"""
    dg = dgate.to(F64)
    if S > 0:
        dg = dg.view(-1, S, dg.shape[1]).sum(1)
    g, h, w1, w2 = gate.to(F64), hid.to(F64), w1.to(F64), w2.to(F64)
    dpre2 = dg * (g * (1.0 - g))
    dpre1 = torch.where(h > 0, dpre2 @ w2, torch.zeros_like(h))
    return {"dpre2": dpre2, "dpre1": dpre1, "dpool": dpre1 @ w1, "dw1": dpre1.t() @ pooled.to(F64), "db1": dpre1.sum(0),
            "dw2": dpre2.t() @ h, "db2": dpre2.sum(0)}


def data_bwd(dout, gate, dpool, hw):
    """gradient of the gated tensor's input: dout * gate[image] + dpool[image] / hw"""
    return dout.to(F64) * gate.to(F64).repeat_interleave(hw, 0) + (dpool.to(F64) / hw).repeat_interleave(hw, 0)


def eltwise(op, a, b=None, act=0, alpha=1.0):
    """hn_eltwise: 0: a + b; 1: a * act'(b), b the POST-activation (ELU: b > 0 ? 1 : b + 1, anything else: ReLU's b > 0); 2: alpha * a;
    3: act(a); 4: a * act'(b), b the PRE-activation"""
    a = a.to(F64)
    if b is not None:
        b = b.to(F64)
    if op == 0:
        return a + b
    if op == 1:
        if act == 3:
            return torch.where(b > 0, a, a * (b + 1.0))
        return torch.where(b > 0, a, torch.zeros_like(a))
    if op == 2:
        return alpha * a
    if op == 3:
        return act_fwd(a, act)
    if op == 4:
        return a * act_grad(b, act)
    raise ValueError(op)


def add_n(out, *bs):
    """out + b0 [+ b1] [+ b2]"""
    s = out.to(F64)
    for b in bs:
        s = s + b.to(F64)
    return s


def add_strided2(dx, dxs):
    """dx [N, 2 Ho, 2 Wo, C] with dxs [N, Ho, Wo, C] added at the even positions"""
    out = dx.to(F64).clone()
    out[:, ::2, ::2, :] += dxs.to(F64)
    return out


def cast_pad(src, ldo):
    """src [M, C] -> [M, ldo], zero padded (the kernel then rounds to bf16)"""
    m, c = src.shape
    out = torch.zeros(m, ldo, dtype=F64)
    out[:, :c] = src.to(F64)
    return out
