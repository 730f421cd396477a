"""fp64 torch restatement of the Lovasz-softmax seg loss contract (segment.use_lovasz), written from the formulas: differentiable, with the
stable descending sort that defines the kernels' order inside ties.  Runs on CPU and GPU.

    p = softmax(logits) over C; pixels in (n, h, w) order, label == ignore_index dropped, other labels outside [0, C) background;
    per present class c: e = |fg - p_c| sorted descending (ties: pixel index ascending); F_j / B_j running fg / bg counts, G = fg count;
    J_j = 1 - (G - F_j) / (G + B_j); loss_c = sum_j e_(j) (J_j - J_{j-1}), J_{-1} = 0, the J differences held constant;
    loss = mean over present classes (0 with a zero gradient when none is present)."""
import torch


def lovasz_softmax_ref(logits_nchw, target, ignore_index=255):
    x = logits_nchw.to(torch.float64)
    c = x.shape[1]
    p = torch.softmax(x, 1).permute(0, 2, 3, 1).reshape(-1, c)
    lab = target.reshape(-1).to(torch.int64)
    keep = lab != ignore_index
    p, lab = p[keep], lab[keep]
    losses = []
    for k in range(c):
        fg = (lab == k).to(torch.float64)
        g = fg.sum()
        if g == 0:
            continue
        e = (fg - p[:, k]).abs()
        es, perm = torch.sort(e, descending=True, stable=True)
        fs = fg[perm]
        jac = 1.0 - (g - fs.cumsum(0)) / (g + (1.0 - fs).cumsum(0))
        wgt = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append((es * wgt.detach()).sum())
    if not losses:
        return (x * 0.0).sum()
    return torch.stack(losses).mean()
