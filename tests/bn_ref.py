"""Float64 reference of training-mode BatchNorm as the kernels of csrc/hn_norm.hip and csrc/hn_fused.hip compute it, pass by pass.

Plain torch on float64 CPU tensors; tensors are [rows, C] (NHWC flattened).  The passes:
  block_sums   the partial statistic rows: sums of x and x^2 over consecutive row blocks
  finalize     partial sums -> mean, biased variance, rstd, scale = gamma * rstd, shift = beta - mean * scale
  running      the running-statistics update (unbiased variance, PyTorch's momentum convention)
  apply        act(scale * z + shift [+ rscale * res + rshift]) for every activation code of include/hydranet_hip.h
  backward     g = dout * act'(pre) (or dout * [y > 0]); dgamma = sum g * xhat, dbeta = sum g; dz = scale * (g - mean g - xhat mean(g xhat))
tests/test_bn_ref_cpu.py holds all of it to F.batch_norm and autograd."""
import torch

F64 = torch.float64
ACT_NONE, ACT_RELU, ACT_SWISH, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3, 4
ACTS = (ACT_NONE, ACT_RELU, ACT_SWISH, ACT_ELU, ACT_SIGMOID)


def block_sums(x, rb):
    """(sum x, sum x^2) over row blocks [b * rb, (b + 1) * rb) of x [M, C]; the last block may be short: [ceil(M / rb), C] each"""
    x = x.to(F64)
    m, c = x.shape
    nb = (m + rb - 1) // rb
    pad = torch.zeros(nb * rb - m, c, dtype=F64)
    xp = torch.cat([x, pad]).view(nb, rb, c)
    return xp.sum(1), (xp * xp).sum(1)


def group_sums(p, groups):
    """hn_rows_reduce2's ragged groups: row g = sum of rows [g * S, min((g + 1) * S, rows)), S = ceil(rows / groups)"""
    p = p.to(F64)
    rows, c = p.shape
    s = (rows + groups - 1) // groups
    out = torch.zeros(groups, c, dtype=F64)
    for g in range(groups):
        out[g] = p[g * s:min((g + 1) * s, rows)].sum(0)
    return out


def finalize(s1, s2, count, gamma, beta, eps):
    """channel sums (s1 = sum z, s2 = sum z^2 over `count` rows) -> dict of mean, var (biased), rstd, scale, shift"""
    s1, s2 = s1.to(F64), s2.to(F64)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.to(F64) * rstd
    shift = beta.to(F64) - mean * scale
    return {"mean": mean, "var": var, "rstd": rstd, "scale": scale, "shift": shift}


def stats(z, gamma, beta, eps):
    """finalize of the exact channel sums of z [M, C]"""
    z = z.to(F64)
    return finalize(z.sum(0), (z * z).sum(0), z.shape[0], gamma, beta, eps)


def running(rm, rv, mean, var, count, momentum):
    """nn.BatchNorm2d's update: new = (1 - momentum) * old + momentum * batch value, with the UNBIASED batch variance"""
    unb = var * (count / (count - 1.0)) if count > 1 else var
    return (1.0 - momentum) * rm.to(F64) + momentum * mean, (1.0 - momentum) * rv.to(F64) + momentum * unb


def eval_coeff(gamma, beta, rm, rv, eps):
    """eval-mode scale / shift from the running statistics"""
    scale = gamma.to(F64) / torch.sqrt(rv.to(F64) + eps)
    return scale, beta.to(F64) - rm.to(F64) * scale


def act_fwd(x, act):
    if act == ACT_RELU:
        return x.clamp(min=0.0)
    if act == ACT_SWISH:
        return x * torch.sigmoid(x)
    if act == ACT_ELU:
        return torch.where(x > 0, x, torch.expm1(x))
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    return x


def act_grad(x, act):
    """d act / d x at the pre-activation x"""
    if act == ACT_RELU:
        return (x > 0).to(F64)
    if act == ACT_SWISH:
        s = torch.sigmoid(x)
        return s * (1.0 + x * (1.0 - s))
    if act == ACT_ELU:
        return torch.where(x > 0, torch.ones_like(x), torch.exp(x))
    if act == ACT_SIGMOID:
        s = torch.sigmoid(x)
        return s * (1.0 - s)
    return torch.ones_like(x)


def act_slope(act):
    """max |act'| over the reals"""
    return {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_SWISH: 1.0999, ACT_ELU: 1.0, ACT_SIGMOID: 0.25}[act]


def pre_act(z, scale, shift, res=None, rscale=None, rshift=None):
    x = z.to(F64) * scale.to(F64) + shift.to(F64)
    if res is not None:
        r = res.to(F64)
        if rscale is not None:
            r = r * rscale.to(F64) + rshift.to(F64)
        x = x + r
    return x


def apply(z, scale, shift, act, res=None, rscale=None, rshift=None):
    return act_fwd(pre_act(z, scale, shift, res, rscale, rshift), act)


def grad_in(dout, z, scale, shift, act, y=None):
    """g, the gradient at the BatchNorm output: dout * [y > 0] with the saved block output y, else dout * act'(scale * z + shift)"""
    d = dout.to(F64)
    if y is not None:
        return torch.where(y.to(F64) > 0, d, torch.zeros_like(d))
    return d * act_grad(pre_act(z, scale, shift), act)


def backward(g, z, mean, rstd, scale, count=None):
    """from g [M, C]: dict of xhat, dbeta = sum g, dgamma = sum g * xhat, mg, mgx (their means over count rows), dz"""
    g, z = g.to(F64), z.to(F64)
    count = count or z.shape[0]
    xhat = (z - mean.to(F64)) * rstd.to(F64)
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    mg, mgx = dbeta / count, dgamma / count
    dz = scale.to(F64) * (g - mg - xhat * mgx)
    return {"xhat": xhat, "dbeta": dbeta, "dgamma": dgamma, "mg": mg, "mgx": mgx, "dz": dz}


def gamma_n(n, u=2.0 ** -24):
    """Higham's gamma_n = n u / (1 - n u): the relative bound of an n-term floating-point sum"""
    return n * u / (1.0 - n * u)

