"""GPU: the Lovasz-softmax seg loss (segment.use_lovasz, hn_lovasz.hip) against the fp64 restatement (tests/lovasz_ref.py): loss within
1e-5 relative and dlogits within 1e-4 of their max on small, odd and full-size maps with ignore regions, an absent class and out-of-range
labels, as float32 and int64 targets; exact ties in the stable order; the edge cases; bitwise determinism; the space-to-depth gradient
hand-over of the phase-form output conv; the module end to end and the captured training step against eager."""
import copy

import pytest
import torch

from tests.helpers import load_cfg, load_npz, tiny_state
from tests.lovasz_ref import lovasz_softmax_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops
    return ops


def _targets(n, h, w, c, gen):
    """class ids in [0, c) without class 3, a 255 block per image, scattered 255s and out-of-range ids (c + 2)"""
    t = torch.randint(0, c, (n, h, w), device=DEV, generator=gen)
    t[t == 3] = 0
    t[:, : h // 4, : w // 3] = 255
    r = torch.rand((n, h, w), device=DEV, generator=gen)
    t[r < 0.03] = 255
    t[(r >= 0.03) & (r < 0.05)] = c + 2
    return t


def _hip(K, logits_nhwc, target):
    x = logits_nhwc.clone().requires_grad_(True)
    loss = K.seg_lovasz_loss_hip(x.permute(0, 3, 1, 2), target)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), x.grad


def _ref(logits_nhwc, target):
    x = logits_nhwc.to(torch.float64).requires_grad_(True)
    loss = lovasz_softmax_ref(x.permute(0, 3, 1, 2), target)
    loss.backward()
    return float(loss.detach()), x.grad


def _check(K, logits, target):
    l1, g1 = _hip(K, logits, target)
    l0, g0 = _ref(logits, target)
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l1, l0)
    assert float((g1.double() - g0).abs().max()) <= 1e-4 * float(g0.abs().max()), float((g1.double() - g0).abs().max() / g0.abs().max())


@pytest.mark.parametrize("n,c,h,w", [(2, 5, 64, 96), (2, 5, 63, 95), (2, 5, 640, 640), (16, 5, 512, 1024)])
@pytest.mark.parametrize("tdtype", [torch.float32, torch.int64])
def test_kernel_equals_restatement(K, n, c, h, w, tdtype):
    gen = torch.Generator(device=DEV).manual_seed(h * 7 + w)
    logits = torch.randn((n, h, w, c), device=DEV, generator=gen) * 2.0
    _check(K, logits, _targets(n, h, w, c, gen).to(tdtype))


def test_generic_class_count(K):
    gen = torch.Generator(device=DEV).manual_seed(11)
    for c in (2, 7, 16):
        logits = torch.randn((2, 40, 56, c), device=DEV, generator=gen) * 2.0
        t = torch.randint(0, c, (2, 40, 56), device=DEV, generator=gen)
        t[:, :5] = 255
        _check(K, logits, t)


def test_edge_cases(K):
    gen = torch.Generator(device=DEV).manual_seed(5)
    logits = torch.randn((2, 32, 48, 5), device=DEV, generator=gen)
    loss, g = _hip(K, logits, torch.full((2, 32, 48), 255, device=DEV, dtype=torch.int64))
    assert loss == 0.0 and float(g.abs().max()) == 0.0
    loss, g = _hip(K, logits, torch.full((2, 32, 48), 9.0, device=DEV))         # valid pixels, but no class present
    assert loss == 0.0 and float(g.abs().max()) == 0.0
    t = torch.full((2, 32, 48), 255, device=DEV, dtype=torch.int64)
    t[:, 4:20, 10:30] = 2                                                       # exactly one present class
    t[1, 25:, :] = 0 + 7                                                        # plus out-of-range (background) pixels
    _check(K, logits, t)


def test_ties_follow_the_stable_order(K):
    gen = torch.Generator(device=DEV).manual_seed(9)
    n, h, w, c = 2, 96, 128, 5
    palette = torch.randn((6, c), device=DEV, generator=gen) * 2.0
    logits = palette[torch.randint(0, 6, (n, h, w), device=DEV, generator=gen)].contiguous()
    _check(K, logits, _targets(n, h, w, c, gen).to(torch.float32))


def test_deterministic(K):
    gen = torch.Generator(device=DEV).manual_seed(13)
    logits = torch.randn((4, 256, 320, 5), device=DEV, generator=gen)
    t = _targets(4, 256, 320, 5, gen).to(torch.float32)
    l0, g0 = _hip(K, logits, t)
    l1, g1 = _hip(K, logits, t)
    assert l0 == l1 and torch.equal(g0, g1)


def _tiny_net(lovasz=True):
    from multitask_hydranet_amd import HydraNet
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["segment"]["use_lovasz"] = lovasz
    net = HydraNet(cfgs)
    net.load_state_dict(tiny_state(z))
    net = net.to(DEV).train()
    net.lane_points_per_line = int(z["meta/lane_points_per_line"])
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    return z, cfgs, net, batch


def test_gradient_handover_is_bit_identical(K):
    """with use_lovasz the loss hands its gradient to the phase-form output conv in the space-to-depth bf16 operand form, as the CE loss
    does: every seg-head gradient must be bit-identical to the plain dlogits path (a second consumer of the logits on top: max-norm 2e-2)"""
    _, _, net, batch = _tiny_net()
    x, gt = batch["image"].to(DEV), batch["gt_seg"].to(DEV)
    names = [n for n, _ in net.named_parameters() if n.startswith("segheader.")]
    P = dict(net.named_parameters())

    def run(handover, extra):
        for p_ in net.parameters():
            p_.grad = None
        out = net(x)
        assert net._seg_grad_slot is not None
        if not handover:
            net._seg_grad_slot = None
        loss = net.loss_seg(out["seg"], gt)
        if extra:
            loss = loss + out["seg"].square().mean()
        loss.backward()
        return float(loss.detach()), {n: P[n].grad.clone() for n in names}

    for extra in (False, True):
        l0, g0 = run(False, extra)
        l1, g1 = run(True, extra)
        assert l0 == l1
        for n in names:
            if extra:
                assert float((g1[n] - g0[n]).abs().max()) <= 2e-2 * float(g0[n].abs().max()) + 1e-12, n
            else:
                assert torch.equal(g0[n], g1[n]), n


def test_end_to_end_against_restatement(K):
    """net(x) -> net.cal_loss (HIP Lovasz) against the same forward -> lovasz_ref on out["seg"]: the loss within 1e-5, the logits gradient
    within 1e-5 of its max, the output conv's gradients (the layer the loss gradient enters) at cosine >= 0.9999.  Deeper in the bf16
    network the gradients amplify round-off: many are zero in exact arithmetic (a bias in front of a BatchNorm) or cancel to bf16 noise,
    and the restatement against itself with its logits gradient times (1 + 1e-6 noise) falls below 0.9999 for about half of the
    parameters.  So the whole parameter gradient (one vector) is held to the bf16 bound 0.999."""
    _, _, net, batch = _tiny_net()
    gb = {k: v.to(DEV) for k, v in batch.items()}
    P = dict(net.named_parameters())
    gen = torch.Generator(device=DEV).manual_seed(17)

    def run(kind):
        out = net(gb["image"])
        net._seg_grad_slot = None               # fp32 dlogits on every run (the hand-over is bit-identical: test above)
        seg = out["seg"]
        seg.retain_grad()
        loss = net.cal_loss(out, gb)["loss_seg"] if kind == "hip" else lovasz_softmax_ref(seg, gb["gt_seg"])
        if kind == "control":
            seg.register_hook(lambda gr: gr * (1.0 + 1e-6 * torch.randn(gr.shape, device=DEV, generator=gen)))
        loss.backward()
        g = {n: p.grad.clone() for n, p in P.items() if p.grad is not None}
        for p in P.values():
            p.grad = None
        return float(loss.detach()), seg.grad.clone(), g

    l1, d1, g1 = run("hip")
    l0, d0, g0 = run("ref")
    _, _, gc = run("control")
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l1, l0)
    assert float((d1 - d0).abs().max()) <= 1e-5 * float(d0.abs().max())
    assert set(g1) == set(g0) == set(gc)
    cos = lambda u, v: float(u.double().flatten() @ v.double().flatten() / (u.double().norm() * v.double().norm()).clamp(min=1e-300))
    names = sorted(g0)
    whole = lambda g: torch.cat([g[n].double().flatten() for n in names])
    out_conv = [n for n in names if n.startswith(f"segheader.decoder.{net._seg_layers}.conv.")]
    assert len(out_conv) == 2
    for n in out_conv:
        assert cos(g1[n], g0[n]) >= 0.9999, (n, cos(g1[n], g0[n]))
    # the whole gradient carries the bf16 network's amplification of round-off (measured 0.99967; the control run lands there too)
    assert cos(whole(g1), whole(g0)) >= 0.999, (cos(whole(g1), whole(g0)), cos(whole(gc), whole(g0)))


def test_captured_step_equals_eager():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as gmod
    gmod.build()
    from multitask_hydranet_amd.train import HydraTrainer
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["segment"]["use_lovasz"] = True
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    g = torch.Generator().manual_seed(3)
    loader = []
    for _ in range(5):
        b = dict(batch)
        b["image"] = batch["image"] + 0.05 * torch.randn(batch["image"].shape, generator=g)
        loader.append(b)
    runs = []
    for capture in (False, True):
        tr = HydraTrainer(copy.deepcopy(cfgs), trainloader=loader, validloader=None, iters_per_epoch=len(loader), capture_step=capture)
        assert tr.hydranet.use_lovasz
        tr.hydranet.load_state_dict(tiny_state(z))
        tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
        losses = []
        for b in loader:
            ld = tr.train_step({k: v.clone() for k, v in b.items()})
            losses.append({k: float(v.detach()) for k, v in ld.items()})
        assert (tr._cap is not None) == capture
        runs.append((losses, {n: p.detach().clone() for n, p in tr.hydranet.named_parameters()}))
    (l0, p0), (l1, p1) = runs
    for step, (a, b) in enumerate(zip(l0, l1)):
        assert a == b, (step, a, b)
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n
