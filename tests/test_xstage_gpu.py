"""The persistent stage kernels (csrc/hn_xstage.hip: hn_xstage_fwd / hn_xstage_bwd; reference net/anynet.py:65-76,84-86) against the launch
chain they replace (ops.XBlockFn, itself checked block by block against the oracle in test_fullsize2_gpu.py / test_model_gpu.py).

Both paths do the same arithmetic with the same bf16 rounding points; reduction orders differ (MFMA K order, statistics trees), which
flips a bf16 result here and there.  So: the first block of a run (identical inputs) is compared tightly -- at most a small fraction of the
elements may differ, each by ~1 ulp of bf16 (rel-to-max 1e-2) -- and the backward is compared TEACHER FORCED (one-block launches fed the
chain's own output gradient).  Whole runs are compared through the last block's statistics (cosine), since 13 BatchNorms in sequence amplify
single-ulp differences on either path."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EPS, MOM = 1e-5, 0.1


def test_shape_envelope_and_abi():
    """host side: which runs the persistent launch takes (else the caller keeps the launch chain), and the entry points' presence"""
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    L = lib()
    for name in ("hn_xstage_fwd", "hn_xstage_bwd", "hn_xstage_supported", "hn_xstage_ws_bytes"):
        assert name in L.symbols()
    q = lambda *a: L.query("hn_xstage_supported", *a)
    assert q(16, 8, 16, 936, 234) == 1 and q(16, 10, 10, 936, 234) == 1            # stage 4 at 512 x 1024 and at 640 x 640
    assert q(16, 16, 32, 376, 94) == 2 and q(16, 20, 20, 376, 94) == 2            # stage 3
    assert q(8, 8, 16, 936, 234) == 1                                               # BASELINE config 2 (batch 8)
    assert q(16, 32, 64, 152, 38) == 0                                              # stage 2: maps beyond one workgroup per image
    assert q(4, 8, 16, 936, 234) == 0 and q(12, 8, 16, 936, 234) == 0               # batches that do not fill the 8 XCDs evenly
    assert q(32, 8, 16, 936, 234) == 0                                              # four images x 15 slices exceed an XCD's 32 CUs
    assert q(16, 8, 16, 940, 235) == 0                                              # channel count not a multiple of 8
    assert 1 << 20 <= L.query("hn_xstage_ws_bytes") <= 1 << 22


@pytest.mark.parametrize("n,h,w,c,cs", [(4, 3, 5, 24, 6), (8, 1, 1, 16, 4)])
def test_xblock_restatement_equals_oracle(n, h, w, c, cs):
    """CPU: tests/xblock_ref.py (the float64 reference of tests/test_xstage_oracle_gpu.py) against oracle.xblock under bf16_mirror, both in
    float64: the output and the six running statistics within 1e-6, and the input and parameter gradients equal to autograd through the
    oracle.  (8, 1, 1): a 1 x 1 map -- the grouped conv's centre tap only, BatchNorm over 8 values (unbiased factor 8 / 7)."""
    from oracle import hydranet_oracle as O
    from tests import xblock_ref as R
    ps = [t.double() for t in _params(1, c, "cpu", 5 + n)]
    assert ps[10].shape[0] == cs
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, h, w, c, generator=g, dtype=torch.float64).to(torch.bfloat16).double().relu()
    dout = torch.randn(n, h, w, c, generator=g, dtype=torch.float64)
    r = R.forward(x, ps, EPS, MOM)
    gr = R.backward(r, dout)
    q = "blk"
    keys = ("conv_block_1.0.weight", "conv_block_1.1.weight", "conv_block_1.1.bias", "conv_block_1.1.running_mean", "conv_block_1.1.running_var",
            "conv_block_2.0.weight", "conv_block_2.1.weight", "conv_block_2.1.bias", "conv_block_2.1.running_mean", "conv_block_2.1.running_var",
            "se.1.weight", "se.1.bias", "se.3.weight", "se.3.bias",
            "conv_block_3.0.weight", "conv_block_3.1.weight", "conv_block_3.1.bias", "conv_block_3.1.running_mean", "conv_block_3.1.running_var")
    sd = {f"{q}.{k}": t.clone().requires_grad_("running" not in k) for k, t in zip(keys, ps)}
    xin = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    with O.bf16_mirror():
        out = O.xblock(sd, q, xin, 1, c // 8, True)
    out.backward(dout.permute(0, 3, 1, 2))
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))
    assert rel(r["out"], out.detach().permute(0, 2, 3, 1)) <= 1e-6
    for i, k in enumerate(keys):
        nm = R.NAMES[i]
        if nm in R.RUNNING:
            assert rel(r["running"][nm], sd[f"{q}.{k}"]) <= 1e-6, (k, rel(r["running"][nm], sd[f"{q}.{k}"]))
            assert rel(r["running"][nm], ps[i]) > 1e-3, k                  # the update happened (momentum 0.1 of a different value)
        else:
            ref = sd[f"{q}.{k}"].grad
            assert ref is not None and rel(gr[R.GRADS[nm]], ref) <= 1e-6, (k, rel(gr[R.GRADS[nm]], ref))
    assert rel(gr["dx"], xin.grad.permute(0, 2, 3, 1)) <= 1e-6
    # the unbiased factor is live: the running variance is not the one the biased variance would give
    cnt = n * h * w
    biased = (1 - MOM) * ps[4] + MOM * r["var"][0]
    assert rel(r["running"]["rv1"], (1 - MOM) * ps[4] + MOM * r["var"][0] * cnt / (cnt - 1)) <= 1e-12
    assert rel(r["running"]["rv1"], biased) > 1e-6
    # the layouts hn_xstage_bwd writes: dgb [3, 2, C] = (dgamma, dbeta) per BatchNorm; the SE pre-activation gradients
    assert gr["dgb"].shape == (3, 2, c) and rel(gr["dgb"][2, 1], sd[f"{q}.conv_block_3.1.bias"].grad) <= 1e-6
    assert gr["dpre2"].shape == (n, c) and gr["dpre1"].shape == (n, cs)
    assert rel(gr["dpre2"].sum(0), sd[f"{q}.se.3.bias"].grad) <= 1e-12 and rel(gr["dpre1"].sum(0), sd[f"{q}.se.1.bias"].grad) <= 1e-12
    assert rel(gr["dpre2"].t() @ r["hid"], sd[f"{q}.se.3.weight"].grad.flatten(1)) <= 1e-12


def _params(nb, c, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    cs = c // 4
    ps = []
    for _ in range(nb):
        r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)
        bn = lambda: [1.0 + 0.1 * r(c), 0.1 * r(c), 0.05 * r(c), 1.0 + 0.1 * torch.rand(c, generator=g).to(dev)]
        ps += [r(c, c, 1, 1, scale=(2.0 / c) ** 0.5), *bn(), r(c, 8, 3, 3, scale=(2.0 / 72) ** 0.5), *bn(),
               r(c // 4, c, 1, 1, scale=(1.0 / c) ** 0.5), r(cs, scale=0.1), r(c, cs, 1, 1, scale=(1.0 / cs) ** 0.5), r(c, scale=0.1),
               r(c, c, 1, 1, scale=(2.0 / c) ** 0.5), *bn()]
    return ps


def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _cos(a, b):
    return float(F.cosine_similarity(a.float().flatten(), b.float().flatten(), dim=0))


def _frac(a, b):
    return float((a.float() != b.float()).float().mean())


CASES = [(16, 8, 16, 128, 2), (16, 8, 16, 936, 3), (16, 16, 32, 376, 2), (16, 10, 10, 936, 2), (16, 20, 20, 376, 2), (8, 8, 16, 936, 2),
         (16, 6, 10, 200, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w,c,nb", CASES)
@pytest.mark.parametrize("mode", [0, 1])
def test_persistent_forward_equals_launch_chain(n, h, w, c, nb, mode):
    """every tensor XBlockFn.forward saves, for every block of the run; mode 0 = XCD-local counters (the product form), 1 = agent-scope
    counters with release / acquire fences"""
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops as K
    import multitask_hydranet_amd.ops.xstage as XS
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(n, h, w, c, generator=gen).to(dev).to(torch.bfloat16).relu_()
    pa = _params(nb, c, dev, 11)
    pb = [t.clone() for t in pa]
    K.clear_pack_cache()
    t = x.clone().requires_grad_(True)
    saved = []
    for b in range(nb):
        t = K.XBlockFn.apply(t, *pa[b * 19:(b + 1) * 19], EPS, MOM, True, 1, None, None, None, None, None, None)
        saved.append(t.grad_fn.saved_tensors)
    with torch.no_grad():
        r = XS.xstage_forward_raw(x, pb, EPS, MOM, mode=mode)
    assert XS.xstage_status(dev) == 0
    names = ("z1", "a", "z2", "bg", "z3", "out")
    for b in range(nb):
        _, z1, a, z2, z3, out, c1, c2, c3, pooled, hid, gate, _, _, bg = saved[b][:15]
        ref = dict(z1=z1, a=a, z2=z2, bg=bg, z3=z3, out=out)
        for nm in names:
            got = r[nm][b]
            assert torch.isfinite(got.float()).all(), (b, nm)
            if b == 0:        # identical inputs: ~1 bf16 ulp on a small fraction of the elements
                assert _rel(got, ref[nm]) <= 1e-2 and _frac(got, ref[nm]) <= 0.06, (b, nm, _rel(got, ref[nm]), _frac(got, ref[nm]))
            assert _cos(got, ref[nm]) >= 0.995, (b, nm, _cos(got, ref[nm]))
        if b == 0:
            for k, cref in enumerate((c1, c2, c3)):
                assert _rel(r["coef"][b, k], cref) <= 2e-3, (b, k, _rel(r["coef"][b, k], cref))
            assert _rel(r["pooled"][b], pooled) <= 5e-3 and _rel(r["hid"][b], hid) <= 5e-3 and _rel(r["gate"][b], gate) <= 5e-3
    for i in range(19):        # running statistics of block 0 (indices 3, 4 / 8, 9 / 17, 18 of the block's 19 tensors)
        if i in (3, 4, 8, 9, 17, 18):
            assert _rel(pb[i], pa[i]) <= 1e-3, (i, _rel(pb[i], pa[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w,c,nb", CASES)
def test_persistent_backward_equals_launch_chain_teacher_forced(n, h, w, c, nb):
    """hn_xstage_bwd, one block per launch with XBlockFn.backward's own output gradient, on the persistent forward's tensors: dx, the six
    BatchNorm gradients, and the weight / SE gradients rebuilt from the dz / dpre tensors the launch leaves for the deferred launches"""
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops as K
    import multitask_hydranet_amd.ops.xstage as XS
    dev = torch.device("cuda:0")
    cs = c // 4
    gen = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(n, h, w, c, generator=gen).to(dev).to(torch.bfloat16).relu_()
    ps = _params(nb, c, dev, 11)
    K.clear_pack_cache()
    with torch.no_grad():
        r = XS.xstage_forward_raw(x, ps, EPS, MOM)
        d = (torch.randn(n, h, w, c, generator=gen) * 0.01).to(dev).to(torch.bfloat16)
        dout0 = d
        grid = (n, h, w)
        sws = [(ps[b * 19 + 10], ps[b * 19 + 12]) for b in range(nb)]
        for b in reversed(range(nb)):
            p = ps[b * 19:(b + 1) * 19]
            xb = x if b == 0 else r["out"][b - 1]
            fake = SimpleNamespace(saved_tensors=(xb, r["z1"][b], r["a"][b], r["z2"][b], r["z3"][b], r["out"][b], r["coef"][b, 0], r["coef"][b, 1],
                                                  r["coef"][b, 2], r["pooled"][b], r["hid"][b], r["gate"][b], p[10], p[12], r["bg"][b], None, None,
                                                  None, None),
                                   training=True, stride=1, packs=r["packs"][b], group=None,
                                   wrefs=(p[0], p[14], None, p[5], p[10], p[11], p[12], p[13]), needs_input_grad=(True,) * 30)
            ret = K.XBlockFn.backward(fake, d)
            sl = lambda t: t[b:b + 1]
            rb = XS.xstage_backward_raw(d.contiguous(), dict(z1=sl(r["z1"]), z2=sl(r["z2"]), z3=sl(r["z3"]), out=sl(r["out"]), coef=sl(r["coef"]),
                                                             hid=sl(r["hid"]), gate=sl(r["gate"])), [r["packs"][b]], [sws[b]])
            got = dict(dx=rb["dx"], dw1=K.k_gemm_tn(xb, None, 0, grid, rb["dz1"][0], c, K.kp32(c), 1, c),
                       dw3=K.k_gemm_tn(r["bg"][b], None, 0, grid, rb["dz3"][0], c, K.kp32(c), 1, c),
                       dw2=K.k_gemm_tn(r["a"][b], None, 5, grid, rb["dz2"][0], c, 64, 9, 8, kh=3),
                       dsw2=(rb["dpre2"][0].t() @ r["hid"][b]).view(c, cs, 1, 1), dsb2=rb["dpre2"][0].sum(0),
                       dsw1=(rb["dpre1"][0].t() @ r["pooled"][b]).view(cs, c, 1, 1), dsb1=rb["dpre1"][0].sum(0),
                       dg1=rb["dgb"][0, 0, 0], db1=rb["dgb"][0, 0, 1], dg2=rb["dgb"][0, 1, 0], db2=rb["dgb"][0, 1, 1], dg3=rb["dgb"][0, 2, 0],
                       db3=rb["dgb"][0, 2, 1])
            ref = dict(dx=ret[0], dw1=ret[1], dg1=ret[2], db1=ret[3], dw2=ret[6], dg2=ret[7], db2=ret[8], dsw1=ret[11], dsb1=ret[12],
                       dsw2=ret[13], dsb2=ret[14], dw3=ret[15], dg3=ret[16], db3=ret[17])
            for k in ref:
                assert torch.isfinite(got[k].float()).all(), (b, k)
                rr, cc = _rel(got[k].reshape(ref[k].shape), ref[k]), _cos(got[k].reshape(ref[k].shape), ref[k])
                assert rr <= 2e-2 and cc >= 0.9995, (b, k, rr, cc)
            d = ret[0]
        assert XS.xstage_status(dev) == 0
        # the whole run in one launch: same direction as the chain's result (single-ulp differences compound over the blocks)
        full = XS.xstage_backward_raw(dout0.contiguous(), r, r["packs"], sws)
        assert _cos(full["dx"], d) >= 0.995, _cos(full["dx"], d)
        assert XS.xstage_status(dev) == 0


@pytest.mark.gpu
def test_persistent_launches_replay_in_a_graph_and_keep_their_state():
    """counters, tickets and granule epochs continue across launches (no memset node): eager launches, a captured launch replayed many times
    and eager launches again give the same output; forward and backward launches interleave on the one workspace"""
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops as K
    import multitask_hydranet_amd.ops.xstage as XS
    dev = torch.device("cuda:0")
    n, h, w, c, nb = 16, 8, 16, 128, 3
    gen = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(n, h, w, c, generator=gen).to(dev).to(torch.bfloat16).relu_()
    ps = _params(nb, c, dev, 5)
    dout = (torch.randn(n, h, w, c, generator=gen) * 0.01).to(dev).to(torch.bfloat16)
    sws = [(ps[b * 19 + 10], ps[b * 19 + 12]) for b in range(nb)]
    K.clear_pack_cache()

    def step():
        pp = [t.clone() if i % 19 in (3, 4, 8, 9, 17, 18) else t for i, t in enumerate(ps)]        # fresh running statistics every call
        with torch.no_grad():
            r = XS.xstage_forward_raw(x, pp, EPS, MOM)
            bw = XS.xstage_backward_raw(dout, r, r["packs"], sws)
        return r["out"][nb - 1], bw["dx"], bw["dgb"]
    ref = [t.clone() for t in step()]
    step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(25):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, ref):
        assert torch.equal(a, b)
    again = step()
    for a, b in zip(again, ref):
        assert torch.equal(a, b)
    assert XS.xstage_status(dev) == 0


@pytest.mark.gpu
def test_model_with_and_without_the_persistent_stage_kernels():
    """The big backbone (batch 16, 512 x 1024) forward + backward three ways: persistent forward + backward launches, persistent forward
    with the per-block chain backward, the launch chain only.  State: random weights with the zero-init-residual conditioning of
    tests/helpers.conditioned_state (the plain random state amplifies any perturbation ~1.5x per block, which makes end-to-end bf16
    statements vacuous -- DESIGN.md section 4); upstream gradient: a fixed random projection of the five features."""
    import __graft_entry__ as g
    g.build()
    import yaml
    from multitask_hydranet_amd import HydraNet, ops as K
    dev = torch.device("cuda:0")
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_big.yml")))
    cfgs["dataloader"]["network_input_height"], cfgs["dataloader"]["network_input_width"] = 512, 1024
    res = {}
    try:
        for name, on, bwd in (("persistent", True, True), ("fwd_only", True, False), ("chain", False, False)):
            K.XSTAGE, K.XSTAGE_BWD = on, bwd
            K.clear_pack_cache()
            torch.manual_seed(0)
            net = HydraNet(cfgs).to(dev).train()
            with torch.no_grad():
                for k, p in net._idx.items():
                    if k.endswith("conv_block_3.1.weight"):
                        p.mul_(0.1)
            gen = torch.Generator(device="cpu").manual_seed(1)
            img = torch.randn(16, 3, 512, 1024, generator=gen).to(dev)
            feats = net._backbone(img)
            loss = sum((f.float() * torch.randn(f.shape, generator=gen).to(dev)).mean() for f in feats)
            loss.backward()
            grads = {k: p.grad.detach().float().clone() for k, p in net._idx.items() if p.grad is not None and k.startswith("backbone.")}
            res[name] = (float(loss.detach()), [f.detach().float() for f in feats], grads)
    finally:
        K.XSTAGE, K.XSTAGE_BWD = True, True
    (la, fa, ga), (lf, ff, gf), (lb, fb, gb) = res["persistent"], res["fwd_only"], res["chain"]
    assert la == lf                                                   # the same forward launches
    assert abs(la - lb) <= 2e-2 * abs(lb) + 1e-6, (la, lb)
    assert _cos(fa[3], fb[3]) >= 0.995 and _cos(fa[4], fb[4]) >= 0.995, (_cos(fa[3], fb[3]), _cos(fa[4], fb[4]))
    assert set(ga) == set(gb) == set(gf)
    big = [k for k in ga if ga[k].numel() >= 64 and gb[k].abs().max() > 0]
    cs = sorted(_cos(ga[k], gb[k]) for k in big)
    assert cs[len(cs) // 2] >= 0.98 and cs[len(cs) // 10] >= 0.97 and cs[0] >= 0.75, (cs[0], cs[len(cs) // 10], cs[len(cs) // 2])
    # the persistent backward against the chain backward on the SAME forward tensors
    cs2 = sorted(_cos(ga[k], gf[k]) for k in big)
    assert cs2[0] >= 0.99 and cs2[len(cs2) // 2] >= 0.9995, (cs2[0], cs2[len(cs2) // 2])
    assert all(torch.isfinite(v).all() for v in ga.values())
