"""Gradient-norm clipping and the non-finite step guard inside the HIP Adam (hn_grad_guard + hn_adam_step_guarded, optim.Adam(max_grad_norm=,
skip_nonfinite=), HydraTrainer's train.grad_clip_norm / train.skip_nonfinite): the norm against float64 and its run-to-run / layout
determinism, clipping against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam, skipped steps leaving parameters and moments bit-unchanged,
and the trainer surviving a poisoned batch, eagerly and under a replayed hipGraph."""
import ctypes

import pytest
import torch

from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu

NORM_SHAPES = [(1,), (3,), (7,), (1023,), (1024,), (1025,), (4099,), (64, 8, 3, 3), (936, 936, 1, 1), (1200000,)]
NORM_EXP = [2, -4, 1, -3, 0, -2, -1, 2, -4, -1]                                  # values randn * 10**k, k per tensor
ADAM_SHAPES = [(936, 936, 1, 1), (7,), (3, 5), (1,), (64, 8, 3, 3), (1023,), (1025,)]   # test_hip_adam_tracks_torch_adam's


@pytest.fixture(scope="module")
def built():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    return lib()


def dev():
    return torch.device("cuda:0")


def run_guard(l, grads, max_norm=1.0, flags=1, losses=(), words=(), record=None):
    """hn_grad_guard on tables built here from the header's description -> (record int32 [8], job_sq double [n])"""
    rows, owner, blk = [], [], 0
    for i, g in enumerate(grads):
        nb = (g.numel() + 1023) // 1024
        rows.append([g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), g.numel(), blk])
        owner += [i] * nb
        blk += nb
    jobs = torch.tensor(rows, dtype=torch.int64).to(dev())
    own = torch.tensor(owner, dtype=torch.int32).to(dev())
    nbytes = l.query("hn_grad_guard_ws_bytes", blk, len(grads))
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev())           # the launches must not depend on what the workspace held
    job_sq = torch.full((len(grads),), -1.0, dtype=torch.float64, device=dev())
    rec = torch.zeros((8,), dtype=torch.int32, device=dev()) if record is None else record
    la = (ctypes.c_void_p * max(len(losses), 1))(*[t.data_ptr() for t in losses])
    wa = (ctypes.c_void_p * max(len(words), 1))(*[t.data_ptr() for t in words])
    l.call("hn_grad_guard", jobs.data_ptr(), own.data_ptr(), blk, len(grads), float(max_norm), flags, ctypes.addressof(la), len(losses),
           ctypes.addressof(wa), len(words), ws.data_ptr(), nbytes, job_sq.data_ptr(), rec.data_ptr())
    torch.cuda.synchronize()
    return rec, job_sq


def rec_dict(rec):
    h = rec.cpu()
    norm, coef = h[:2].view(torch.float32).tolist()
    return dict(norm=norm, coef=coef, skip=int(h[2]), steps=int(h[3]), skipped=int(h[4]), skipped_consecutive=int(h[5]))


@pytest.fixture(scope="module")
def norm_grads(built):
    g = torch.Generator().manual_seed(7)
    return [(torch.randn(s, generator=g) * 10.0 ** k).to(dev()) for s, k in zip(NORM_SHAPES, NORM_EXP)]


def test_norm_against_float64_and_deterministic(built, norm_grads):
    rec, job_sq = run_guard(built, norm_grads, max_norm=1.0)
    want_sq = torch.stack([(g.double() ** 2).sum() for g in norm_grads])
    want = float(want_sq.sum().sqrt())
    r = rec_dict(rec)
    err = abs(r["norm"] - want) / want
    job_err = float(((job_sq.sqrt() - want_sq.sqrt()).abs() / want_sq.sqrt()).max())
    print("norm %.9g want %.9g rel %.3e; per-job rel max %.3e" % (r["norm"], want, err, job_err))
    assert err <= 2e-6 and job_err <= 2e-6
    assert r["skip"] == 0 and r["steps"] == 1 and r["skipped"] == 0
    # torch's formula in rounded fp32 operations
    n32 = torch.tensor(r["norm"], dtype=torch.float32)
    assert r["coef"] == float(torch.clamp(torch.tensor(1.0, dtype=torch.float32) / (n32 + torch.tensor(1e-6, dtype=torch.float32)), max=1.0))
    # twice: the same bits
    rec2, job_sq2 = run_guard(built, norm_grads, max_norm=1.0)
    assert torch.equal(rec, rec2) and torch.equal(job_sq.view(torch.int64), job_sq2.view(torch.int64))
    # the same values as views at element offset 1 of one flat buffer (no 16-byte alignment, the element-by-element loads): the same bits
    flat = torch.zeros((1 + sum(g.numel() for g in norm_grads),), device=dev())
    views, off = [], 1
    for g in norm_grads:
        v = flat[off:off + g.numel()]
        v.copy_(g.reshape(-1))
        views.append(v)
        off += g.numel()
    assert any(v.data_ptr() % 16 for v in views)
    rec3, job_sq3 = run_guard(built, views, max_norm=1.0)
    assert torch.equal(rec, rec3) and torch.equal(job_sq.view(torch.int64), job_sq3.view(torch.int64))
    # max_norm <= 0: no clipping, exactly 1
    assert rec_dict(run_guard(built, norm_grads, max_norm=0.0)[0])["coef"] == 1.0
    assert rec_dict(run_guard(built, norm_grads, max_norm=-1.0)[0])["coef"] == 1.0


def test_zero_gradients_and_fp32_overflow(built):
    zeros = [torch.zeros(s, device=dev()) for s in [(1,), (1025,), (3, 5)]]
    rec, job_sq = run_guard(built, zeros, max_norm=1.0)
    r = rec_dict(rec)
    assert r["norm"] == 0.0 and r["coef"] == 1.0 and r["skip"] == 0 and float(job_sq.abs().max()) == 0.0
    # finite values whose sum of squares leaves fp32's range count as not finite (flags & 1), and only then
    big = [torch.full((1,), 1.5e19, device=dev()), torch.full((1,), 1.5e19, device=dev())]      # 2.25e38 each, 4.5e38 together
    assert rec_dict(run_guard(built, big, flags=1)[0])["skip"] == 1
    r = rec_dict(run_guard(built, big, flags=0)[0])
    assert r["skip"] == 0 and abs(r["norm"] - 2.0 ** 0.5 * 1.5e19) <= 1e-6 * 2.2e19


def make_grads(shapes, it, gen):
    return [torch.randn(s, generator=gen) * (10.0 ** (it - 3)) for s in shapes]


def close(a, b, tol, name=""):
    err, ref = float((a.float() - b.float()).abs().max()), float(b.float().abs().max())
    assert err <= tol * ref + 1e-6, f"{name}: max err {err:.4e} vs ref max {ref:.4e} (tol {tol})"


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_clip_tracks_clip_grad_norm_then_torch_adam(built, wd):
    from multitask_hydranet_amd.optim import Adam
    gen = torch.Generator().manual_seed(1)
    init = [torch.randn(s, generator=gen).to(dev()) for s in ADAM_SHAPES]
    new = lambda: [torch.nn.Parameter(p.clone()) for p in init]
    pa, pb, pc, pd, pe = new(), new(), new(), new(), new()
    oa = Adam(pa, 1e-2, weight_decay=wd, max_grad_norm=1.0)                     # under test
    ob = torch.optim.Adam(pb, 1e-2, weight_decay=wd)                           # reference: clip_grad_norm_ first
    oc = Adam(pc, 1e-2, weight_decay=wd)                                       # unguarded, same gradients
    od = Adam(pd, 1e-2, weight_decay=wd, max_grad_norm=1e30, skip_nonfinite=True)   # guarded, coef == 1 throughout
    oe = Adam(pe, 1e-2, weight_decay=wd)                                       # od's unguarded twin
    coefs, all_unclipped = [], True
    for it in range(6):
        for o in (oa, ob, oc, od, oe):
            o.param_groups[0]["lr"] = 1e-2 / (1 + it)
        grads = [g.to(dev()) for g in make_grads(ADAM_SHAPES, it, gen)]
        for ps in (pa, pb, pc, pd, pe):
            for p, g in zip(ps, grads):
                p.grad = None if (it < 2 and p.numel() == 7) else g.clone()     # a late-starting parameter: its own step count
        torch.nn.utils.clip_grad_norm_(pb, 1.0)
        for o in (oa, ob, oc, od, oe):
            o.step()
        r = oa.grad_guard_record()
        coefs.append(r["coef"])
        assert r["skip"] == 0 and r["steps"] == it + 1
        for p, g in zip(pa, grads):                                            # step() reads the gradients, never writes them
            assert p.grad is None or torch.equal(p.grad, g)
        for a, b in zip(pa, pb):
            assert float((a - b).detach().abs().max()) <= 2e-6 * max(float(b.detach().abs().max()), 1e-3), (it, tuple(a.shape), r)
        all_unclipped = all_unclipped and r["coef"] == 1.0
        if all_unclipped:                                                      # nothing clipped so far: the unguarded optimizer's bits
            for a, c in zip(pa, pc):
                assert torch.equal(a, c), (it, tuple(a.shape))
        for d, e in zip(pd, pe):                                               # coef == 1.0f: hn_adam_step's bits, iteration after iteration
            assert torch.equal(d, e), (it, tuple(d.shape))
        assert od.grad_guard_record()["coef"] == 1.0
    assert coefs[0] == 1.0 and coefs[-1] < 1.0, coefs                         # both kinds occurred
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    for k in sb:
        assert float(sa[k]["step"]) == float(sb[k]["step"])
        close(sa[k]["exp_avg"], sb[k]["exp_avg"], 1e-5, "exp_avg")
        close(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"], 1e-5, "exp_avg_sq")
    sd, se = od.state_dict()["state"], oe.state_dict()["state"]
    for k in se:
        assert torch.equal(sd[k]["exp_avg"], se[k]["exp_avg"]) and torch.equal(sd[k]["exp_avg_sq"], se[k]["exp_avg_sq"])
    # the per-parameter sums of squares belong to guard_params, in order; the prefix view adds them up
    from multitask_hydranet_amd.optim import grad_norms_by_prefix
    named = [("head.%d" % i if i % 2 else "body.%d" % i, p) for i, p in enumerate(pa)]
    got = grad_norms_by_prefix(oa, named, ["head", "body", "nothing"])
    for pre in ("head", "body"):
        want = torch.stack([(p.grad.double() ** 2).sum() for n, p in named if n.startswith(pre)]).sum().sqrt()
        assert abs(float(got[pre]) - float(want)) <= 2e-6 * float(want)
    assert float(got["nothing"]) == 0.0 and len(oa.guard_params) == len(pa) == oa.grad_sq_by_param.numel()


SKIP_SHAPES = [(1,), (1025,), (3, 5), (64, 8, 3, 3)]


@pytest.mark.parametrize("case,bit", [("nan_grad", 1), ("inf_grad", 1), ("nan_loss", 2), ("word", 4)])
def test_skipped_step_leaves_state_untouched(built, case, bit):
    from multitask_hydranet_amd.optim import Adam
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=gen).to(dev()) for s in SKIP_SHAPES]
    pa = [torch.nn.Parameter(p.clone()) for p in init]
    pb = [torch.nn.Parameter(p.clone()) for p in init]
    oa = Adam(pa, 1e-2, weight_decay=1e-2, skip_nonfinite=True)
    ob = torch.optim.Adam(pb, 1e-2, weight_decay=1e-2)
    loss, word = torch.ones((), device=dev()), torch.zeros((1,), dtype=torch.int32, device=dev())

    def finite_step():
        for a, b in zip(pa, pb):
            g = torch.randn(a.shape, generator=gen).to(dev())
            a.grad, b.grad = g.clone(), g.clone()
        oa.step(losses=[loss], guard_words=[word])
        ob.step()
        for a, b in zip(pa, pb):
            assert float((a - b).detach().abs().max()) <= 2e-6 * max(float(b.detach().abs().max()), 1e-3), tuple(a.shape)

    finite_step()                                                              # moments are non-zero from here on
    r = oa.grad_guard_record()
    assert (r["skip"], r["steps"], r["skipped"], r["skipped_consecutive"]) == (0, 1, 0, 0), r
    for a in pa:
        a.grad = torch.randn(a.shape, generator=gen).to(dev())
    if case == "nan_grad":
        pa[1].grad.view(-1)[-1] = float("nan")                                 # the lone element of the 1025 tensor's second block
    elif case == "inf_grad":
        pa[0].grad.fill_(float("inf"))
    elif case == "nan_loss":
        loss.fill_(float("nan"))
    else:
        word.fill_(1)
    state = lambda: [t.detach().clone() for p in pa for t in (p, oa.state[p]["exp_avg"], oa.state[p]["exp_avg_sq"])]
    before = state()
    oa.step(losses=[loss], guard_words=[word])
    r = oa.grad_guard_record()
    for x, y in zip(before, state()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert r["skip"] == bit and r["steps"] == 2 and r["skipped"] == 1 and r["skipped_consecutive"] == 1, r
    # the host-side step count advanced all the same (documented deviation): the reference's is bumped by hand
    for b in pb:
        ob.state[b]["step"] += 1
    loss.fill_(1.0)
    word.fill_(0)
    finite_step()
    r = oa.grad_guard_record()
    assert r["skip"] == 0 and r["steps"] == 3 and r["skipped"] == 1 and r["skipped_consecutive"] == 0, r
    for a, x in zip(pa, before[::3]):
        assert not torch.equal(a, x)


def test_nan_gradient_flows_through_without_skip_nonfinite(built):
    """torch's behaviour: clip_grad_norm_ (error_if_nonfinite=False) and Adam carry the NaN on"""
    from multitask_hydranet_amd.optim import Adam
    p = torch.nn.Parameter(torch.ones(1025, device=dev()))
    o = Adam([p], 1e-2, max_grad_norm=1.0)
    p.grad = torch.ones(1025, device=dev())
    p.grad[-1] = float("nan")
    o.step()
    r = o.grad_guard_record()
    assert r["skip"] == 0 and r["skipped"] == 0 and r["norm"] != r["norm"] and r["coef"] != r["coef"]
    assert bool(torch.isnan(p).all())


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(built):
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    g = torch.Generator().manual_seed(3)
    loader = []
    for i in range(5):                                                         # different images per iteration, same targets
        b = dict(batch)
        b["image"] = batch["image"] + 0.05 * torch.randn(batch["image"].shape, generator=g)
        loader.append(b)
    return z, cfgs, loader


def make_trainer(tiny, capture=False, **keys):
    import copy
    from multitask_hydranet_amd.train import HydraTrainer
    z, cfgs, loader = tiny
    cfgs = copy.deepcopy(cfgs)
    cfgs["train"].update(keys)
    tr = HydraTrainer(cfgs, trainloader=loader, validloader=None, iters_per_epoch=len(loader), capture_step=capture)
    tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    return tr


def params_of(tr):
    return {n: p.detach().clone() for n, p in tr.hydranet.named_parameters()}


def step(tr, b):
    return tr.train_step({k: v.clone() for k, v in b.items()})


@pytest.fixture(scope="module")
def plain_and_guarded(tiny):
    """(a)'s two runs: 3 steps without the keys and with grad_clip_norm = 1e30 + skip_nonfinite -> parameters, buffers, first-step norm"""
    runs = []
    for keys in ({}, dict(grad_clip_norm=1e30, skip_nonfinite=True)):
        tr = make_trainer(tiny, **keys)
        recs = []
        for b in tiny[2][:3]:
            step(tr, b)
            if keys:
                recs.append(tr.optimizer.grad_guard_record())
        runs.append((params_of(tr), {n: b_.detach().clone() for n, b_ in tr.hydranet.named_buffers()}, recs, tr.hydranet.check_finite))
    return runs


def test_trainer_guard_with_coef_one_equals_plain_trainer(plain_and_guarded):
    (p0, b0, _, chk0), (p1, b1, recs, chk1) = plain_and_guarded
    assert chk0 is True and chk1 is False                                      # the device guard replaces the host guard
    assert [r["coef"] for r in recs] == [1.0] * 3 and recs[-1]["steps"] == 3 and recs[-1]["skipped"] == 0
    assert all(r["norm"] > 0 and r["norm"] == r["norm"] for r in recs)
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n
    for n in b0:
        assert torch.equal(b0[n], b1[n]), n


def test_trainer_clips_to_half_the_first_norm(tiny, plain_and_guarded):
    p1, n0 = plain_and_guarded[1][0], plain_and_guarded[1][2][0]["norm"]
    tr = make_trainer(tiny, grad_clip_norm=n0 / 2)
    assert tr.hydranet.check_finite is True                                    # clipping alone keeps the reference's host guard
    for i, b in enumerate(tiny[2][:3]):
        step(tr, b)
        if i == 0:
            r = tr.optimizer.grad_guard_record()
            assert abs(r["norm"] - n0) <= 1e-6 * n0 and abs(r["coef"] - 0.5) <= 1e-5, (r, n0)
    p = params_of(tr)
    assert any(not torch.equal(p[n], p1[n]) for n in p)


def poisoned(b):
    b = {k: v.clone() for k, v in b.items()}
    row = (b["gt_cls"][..., 1] > 0).nonzero()[0]
    b["gt_loc"][row[0], row[1], 0] = float("nan")
    return b


@pytest.mark.parametrize("capture,at", [(False, 1), (True, 3)])
def test_trainer_survives_a_poisoned_batch(tiny, capture, at):
    """(c) eager, poisoned second batch; (d) capture_step, poisoned at the fourth iteration -- a pure replay"""
    tr = make_trainer(tiny, capture=capture, skip_nonfinite=True)
    loader = tiny[2]
    for b in loader[:at]:
        step(tr, b)
    assert (tr._cap is not None) == capture
    before = params_of(tr)
    moments = [tr.optimizer.state[p][k].clone() for p in tr.optimizer.guard_params for k in ("exp_avg", "exp_avg_sq")]
    ld = step(tr, poisoned(loader[at]))                                        # returns: no SystemExit
    assert not bool(torch.isfinite(ld["total_loss"])), ld                      # precondition: the poison reaches the total loss
    r = tr.optimizer.grad_guard_record()
    assert r["skip"] != 0 and r["skipped"] == 1 and r["skipped_consecutive"] == 1 and r["steps"] == at + 1, r
    for n, p in tr.hydranet.named_parameters():
        assert torch.equal(p.detach().view(torch.int32), before[n].view(torch.int32)), n
    now = [tr.optimizer.state[p][k] for p in tr.optimizer.guard_params for k in ("exp_avg", "exp_avg_sq")]
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(moments, now))
    ld = step(tr, loader[at + 1])
    assert bool(torch.isfinite(ld["total_loss"]))
    r = tr.optimizer.grad_guard_record()
    assert r["skip"] == 0 and r["skipped"] == 1 and r["skipped_consecutive"] == 0, r
    after = params_of(tr)
    moved = [n for n in after if not torch.equal(after[n], before[n])]
    assert len(moved) >= 0.5 * len(after), (len(moved), len(after))           # the step was applied
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    assert (tr._cap is not None) == capture


def test_trainer_keys_need_the_hip_adam(tiny):
    import copy
    from multitask_hydranet_amd.train import HydraTrainer
    for keys in (dict(grad_clip_norm=1.0), dict(skip_nonfinite=True)):
        cfgs = copy.deepcopy(tiny[1])
        cfgs["train"].update(keys)
        with pytest.raises(ValueError):
            HydraTrainer(cfgs, trainloader=tiny[2], iters_per_epoch=5, hip_adam=False)
