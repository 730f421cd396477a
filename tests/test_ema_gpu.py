"""The weight average kept inside the HIP Adam launch (hn_adam_step_ema), the in-place exchange of live and averaged values (hn_swap_many),
optim.Adam(ema_decay=, ema_warmup=) and HydraTrainer's train.ema_decay: p, m and v against hn_adam_step / hn_adam_step_guarded bit for
bit, the average against tests/ema_ref.py bit for bit (every operation is individually rounded: no tolerance anywhere), aligned and
unaligned operands, skipped steps, the optimizer's state round trip, and a trainer that validates and saves the averaged weights while its
captured step keeps replaying."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import ema_ref
from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3, 5), (7,), (1023,), (1024,), (1025,), (64, 8, 3, 3)]
DECAYS = [0.1, 0.5, 0.9998]
HYPER = (1e-2, 0.9, 0.999, 1e-8)                                                 # lr, beta1, beta2, eps


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


def bits(t):
    """the tensor's 32-bit words, flat (a view of a flat buffer and a separate allocation compare by content)"""
    return t.detach().contiguous().view(torch.int32).cpu().numpy().reshape(-1).copy()


def place(values, flat):
    """`values` as separate allocations (flat False) or as views of ONE flat buffer starting at element offset 1 (no 16-byte alignment
    for most of them)"""
    if not flat:
        return [v.to(dev()).contiguous() for v in values]
    buf = torch.zeros((1 + sum(v.numel() for v in values),), device=dev())
    out, off = [], 1
    for v in values:
        w = buf[off:off + v.numel()]
        w.copy_(v.reshape(-1))
        out.append(w)
        off += v.numel()
    return out


def tables(*columns):
    """job rows {col0, col1, ..., numel, first_block} and the block -> job table, as the header describes them"""
    rows, owner, blk = [], [], 0
    for i, ts in enumerate(zip(*columns)):
        n = ts[0].numel()
        assert all(t.numel() == n and t.is_contiguous() for t in ts)
        nb = (n + 1023) // 1024
        rows.append([t.data_ptr() for t in ts] + [n, blk])
        owner += [i] * nb
        blk += nb
    return torch.tensor(rows, dtype=torch.int64).to(dev()), torch.tensor(owner, dtype=torch.int32).to(dev()), blk


def pointer_table(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64).to(dev())


def seeded(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * scale for s in SHAPES]


def run_guard(l, jobs, own, blk, n, max_norm, flags):
    nbytes = l.query("hn_grad_guard_ws_bytes", blk, n)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=dev())
    rec = torch.zeros((8,), dtype=torch.int32, device=dev())
    none = (ctypes.c_void_p * 1)()
    l.call("hn_grad_guard", jobs.data_ptr(), own.data_ptr(), blk, n, float(max_norm), flags, ctypes.addressof(none), 0, ctypes.addressof(none), 0,
           ws.data_ptr(), nbytes, None, rec.data_ptr())
    return rec, ws


def ema_run(l, wd, flat, flat_ema=None, max_norm=None):
    """three steps (decays DECAYS) of hn_adam_step_ema next to a twin stepped by hn_adam_step (or, with max_norm, both obeying one
    hn_grad_guard record: the gradients are the same) -> per step the bits of p, m, v, e; p, m, v are held to the twin and e to the numpy
    reference on the way"""
    flat_ema = flat if flat_ema is None else flat_ema
    p0 = seeded(11)
    p, m, v = place(p0, flat), place([torch.zeros(s) for s in SHAPES], flat), place([torch.zeros(s) for s in SHAPES], flat)
    e = place([x + 0.25 * y for x, y in zip(p0, seeded(12))], flat_ema)           # an average that differs from the parameter
    tp, tm, tv = place(p0, False), place([torch.zeros(s) for s in SHAPES], False), place([torch.zeros(s) for s in SHAPES], False)
    g = place([torch.zeros(s) for s in SHAPES], flat)
    jobs, own, blk = tables(p, g, m, v)
    tjobs, town, tblk = tables(tp, g, tm, tv)
    etab = pointer_table(e)
    ptrs = [t.data_ptr() for ts in (p, g, m, v, e) for t in ts]
    if flat or flat_ema:
        assert any(a % 16 for a in ptrs)
    else:
        assert not any(a % 16 for a in ptrs)
    out = []
    for it, decay in enumerate(DECAYS):
        for dst, src in zip(g, seeded(100 + it, scale=10.0 ** (it - 1))):
            dst.copy_(src.reshape(dst.shape))
        e_before = [x.detach().cpu().numpy().copy() for x in e]
        rec = None
        if max_norm is not None:
            rec, _ws = run_guard(l, jobs, own, blk, len(SHAPES), max_norm, 1)
        l.call("hn_adam_step_ema", jobs.data_ptr(), own.data_ptr(), blk, etab.data_ptr(), *HYPER, wd, it + 1, decay,
               None if rec is None else rec.data_ptr())
        if rec is None:
            l.call("hn_adam_step", tjobs.data_ptr(), town.data_ptr(), tblk, *HYPER, wd, it + 1)
        else:
            l.call("hn_adam_step_guarded", tjobs.data_ptr(), town.data_ptr(), tblk, *HYPER, wd, it + 1, rec.data_ptr())
        torch.cuda.synchronize()
        if rec is not None:
            coef = float(rec[:2].cpu().view(torch.float32)[1])
            assert int(rec[2]) == 0 and coef < 1.0, (it, coef)                     # the step was clipped, not skipped
        step_bits, moved = [], False
        for i, s in enumerate(SHAPES):
            for name, a, b in (("p", p[i], tp[i]), ("m", m[i], tm[i]), ("v", v[i], tv[i])):
                assert np.array_equal(bits(a), bits(b)), (name, s, it, wd, flat)
            want = ema_ref.ema_step(e_before[i].reshape(-1), p[i].detach().cpu().numpy().reshape(-1), decay)
            assert np.array_equal(bits(e[i]), want.view(np.int32).reshape(-1)), ("e", s, it, wd, flat)
            moved = moved or not np.array_equal(bits(e[i]), e_before[i].view(np.int32).reshape(-1))
            step_bits.append([bits(t).reshape(-1) for t in (p[i], m[i], v[i], e[i])])
        assert moved, ("the averages did not move", it)
        out.append(step_bits)
    return out


def same_bits(a, b):
    return all(np.array_equal(x, y) for sa, sb in zip(a, b) for ta, tb in zip(sa, sb) for x, y in zip(ta, tb))


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_kernel_against_the_reference_aligned_and_unaligned(built, wd):
    aligned = ema_run(built, wd, flat=False)
    assert same_bits(aligned, ema_run(built, wd, flat=True))                        # all five arrays at element offset 1 of flat buffers
    assert same_bits(aligned, ema_run(built, wd, flat=False, flat_ema=True))        # only the averages unaligned: the test includes them


def test_guarded_clip_and_skip(built):
    ema_run(built, 1e-2, flat=False, max_norm=1e-3)
    ema_run(built, 0.0, flat=True, max_norm=1e-3)
    # one infinite gradient element + skip_nonfinite: nothing is stored, the average included
    p, m, v = place(seeded(21), False), place(seeded(22, 0.1), False), place([x.abs() for x in seeded(23, 0.1)], False)
    e, g = place(seeded(24), False), place(seeded(25), False)
    g[5].view(-1)[-1] = float("inf")                                               # the lone element of the 1025 tensor's second block
    jobs, own, blk = tables(p, g, m, v)
    etab = pointer_table(e)
    before = [bits(t) for ts in (p, m, v, e) for t in ts]
    rec, _ws = run_guard(built, jobs, own, blk, len(SHAPES), 1.0, 1)
    built.call("hn_adam_step_ema", jobs.data_ptr(), own.data_ptr(), blk, etab.data_ptr(), *HYPER, 1e-2, 1, 0.5, rec.data_ptr())
    torch.cuda.synchronize()
    assert int(rec[2]) == 1
    for x, t in zip(before, [t for ts in (p, m, v, e) for t in ts]):
        assert np.array_equal(x, bits(t))
    # the same tables with a finite gradient: the step is taken (the record, not the kernel, held it back)
    g[5].view(-1)[-1] = 1.0
    rec, _ws = run_guard(built, jobs, own, blk, len(SHAPES), 1.0, 1)
    built.call("hn_adam_step_ema", jobs.data_ptr(), own.data_ptr(), blk, etab.data_ptr(), *HYPER, 1e-2, 1, 0.5, rec.data_ptr())
    torch.cuda.synchronize()
    assert int(rec[2]) == 0
    n = len(SHAPES)
    assert all(not np.array_equal(x, bits(t)) for x, t in zip(before[:n] + before[3 * n:], p + e))


def test_bad_arguments_launch_nothing(built):
    p, m, v, e, g = (place(seeded(30 + k), False) for k in range(5))
    jobs, own, blk = tables(p, g, m, v)
    etab = pointer_table(e)
    before = [bits(t) for ts in (p, m, v, e) for t in ts]
    f = built.raw("hn_adam_step_ema")
    st = torch.cuda.current_stream().cuda_stream
    for decay in (1.0, -0.1, float("nan")):
        assert f(jobs.data_ptr(), own.data_ptr(), blk, etab.data_ptr(), *HYPER, 0.0, 1, decay, None, st) == 1, decay
    assert f(jobs.data_ptr(), own.data_ptr(), blk, None, *HYPER, 0.0, 1, 0.5, None, st) == 1
    torch.cuda.synchronize()
    for x, t in zip(before, [t for ts in (p, m, v, e) for t in ts]):
        assert np.array_equal(x, bits(t))


SENTINEL = 0x5A5A5A5A


def swap_values(seed):
    """int32 bit patterns: random words (every kind of float among them) with NaNs of distinct payloads, +-0, +-inf and denormals planted
    at the start of every tensor that has room"""
    special = [0x7FC00001, 0x7FC12345, 0xFFC00002, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF]
    g = np.random.default_rng(seed)
    out = []
    for i, s in enumerate(SHAPES):
        n = int(np.prod(s))
        w = g.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        k = min(n, len(special))
        w[:k] = np.roll(np.array(special, dtype=np.uint32), i + seed)[:k]
        out.append(w.view(np.int32))
    return out


def swap_layout(values, one_sentinel):
    """the tensors as fp32 views of one flat buffer whose every other element is a sentinel: exactly one sentinel between neighbours
    (views at odd offsets), or sentinels padding every view to a multiple of 4 elements (16-byte aligned views)"""
    spans, off = [], 1 if one_sentinel else 4
    for w in values:
        spans.append((off, off + w.size))
        off += w.size + 1 if one_sentinel else (w.size + 1 + 3) // 4 * 4
    host = np.full((off,), SENTINEL, dtype=np.uint32).view(np.int32)
    for (a, b), w in zip(spans, values):
        host[a:b] = w
    buf = torch.from_numpy(host.copy()).to(dev()).view(torch.float32)
    return buf, [buf[a:b] for a, b in spans], host


@pytest.mark.parametrize("a_odd,b_odd", [(False, False), (True, True), (False, True)])
def test_swap_many(built, a_odd, b_odd):
    va, vb = swap_values(1), swap_values(2)
    assert len({int(x) for w in va + vb for x in w[:10] if (int(x) & 0x7F800000) == 0x7F800000 and int(x) & 0x7FFFFF}) >= 4   # distinct NaNs
    fa, a, ha = swap_layout(va, a_odd)
    fb, b, hb = swap_layout(vb, b_odd)
    ptrs = [t.data_ptr() for t in a + b]
    assert any(x % 16 for x in ptrs) == (a_odd or b_odd)
    jobs, own, blk = tables(a, b)
    built.call("hn_swap_many", jobs.data_ptr(), own.data_ptr(), blk)
    torch.cuda.synchronize()
    for i in range(len(SHAPES)):
        assert np.array_equal(bits(a[i]), vb[i]) and np.array_equal(bits(b[i]), va[i]), SHAPES[i]
    for flat, views in ((fa, a), (fb, b)):
        now = bits(flat)
        gaps = np.ones(now.shape, dtype=bool)
        for t in views:
            o = (t.data_ptr() - flat.data_ptr()) // 4
            gaps[o:o + t.numel()] = False
        assert gaps.sum() >= len(SHAPES) and np.all(now[gaps] == np.int32(SENTINEL))   # every sentinel intact
    built.call("hn_swap_many", jobs.data_ptr(), own.data_ptr(), blk)
    torch.cuda.synchronize()
    assert np.array_equal(bits(fa), ha) and np.array_equal(bits(fb), hb)           # twice: the original bits, sentinels included


# ------------------------------------------------------------------------------------------------------------------------------------
def fresh_params():
    return [torch.nn.Parameter(t.to(dev())) for t in seeded(41)]


def give_grads(param_sets, it, skip=()):
    grads = [t.to(dev()) for t in seeded(200 + it, scale=10.0 ** (it % 3 - 1))]
    for ps in param_sets:
        for i, (p, g) in enumerate(zip(ps, grads)):
            p.grad = None if i in skip else g.clone()


def test_optimizer_surface(built):
    from multitask_hydranet_amd.optim import Adam, ema_decay_at
    # off: the optimizer without the argument
    pa, pb = fresh_params(), fresh_params()
    oa, ob = Adam(pa, 1e-2, weight_decay=1e-2, ema_decay=None), Adam(pb, 1e-2, weight_decay=1e-2)
    for it in range(3):
        give_grads((pa, pb), it)
        oa.step()
        ob.step()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(pa, pb))
    assert all("ema" not in st and "ema_start" not in st for st in oa.state.values())
    # on: an average for every stepped parameter, none for one without a gradient
    pc, pd = fresh_params(), fresh_params()
    oc, od = Adam(pc, 1e-2, weight_decay=1e-2, ema_decay=0.99), Adam(pd, 1e-2, weight_decay=1e-2, ema_decay=0.99)
    start = [bits(p) for p in pc]
    want = [p.detach().cpu().numpy().copy() for p in pc]
    for it in range(3):
        give_grads((pc, pd), it, skip=(2,))
        oc.step()
        od.step()
        for i, p in enumerate(pc):
            if i != 2:
                want[i] = ema_ref.ema_step(want[i], p.detach().cpu().numpy(), ema_ref.ema_decay_at(it, 0.99, True))
    for i, (p, b) in enumerate(zip(pc, pb)):
        assert ("ema" in oc.state.get(p, {})) == (i != 2)
        if i != 2:
            assert np.array_equal(bits(p), bits(b))                                # the average changes nothing about the parameters
            assert np.array_equal(bits(oc.state[p]["ema"]), want[i].view(np.int32).reshape(-1)), SHAPES[i]
            assert oc.state[p]["ema"].shape == p.shape
        else:
            assert np.array_equal(bits(p), start[i])
    named = [("t%d" % i, p) for i, p in enumerate(pc)]
    got = oc.ema_named(named)
    assert sorted(got) == ["t%d" % i for i in range(len(pc)) if i != 2] and all(got[n] is oc.state[p]["ema"] for n, p in named if n in got)
    assert ema_decay_at(2, 0.99, True) == 0.25
    # the state round trip: a fresh optimizer continues with the uninterrupted twin's bits (the warm-up position travels with the state);
    # the late parameter joins with a gradient of its own and its own warm-up
    sd = oc.state_dict()
    assert all(("ema" in st) == (k != 2) for k, st in sd["state"].items()) and len(sd["state"]) == len(pc) - 1
    pe = [torch.nn.Parameter(p.detach().clone()) for p in pc]
    oe = Adam(pe, 1e-2, weight_decay=1e-2, ema_decay=0.99)
    oe.load_state_dict(copy.deepcopy(sd))
    for it in range(3, 5):
        give_grads((pd, pe), it)
        od.step()
        oe.step()
        for i, (d, e) in enumerate(zip(pd, pe)):
            assert np.array_equal(bits(d), bits(e)), (it, SHAPES[i])
            assert np.array_equal(bits(od.state[d]["ema"]), bits(oe.state[e]["ema"])), (it, SHAPES[i])
    late = od.state[pd[2]]
    assert late["ema_start"] == 0 and int(late["step"]) == 2 and od.state[pd[0]]["ema_start"] == 0 and int(od.state[pd[0]]["step"]) == 5
    # torch.optim.Adam loads the same state dict
    pt = [torch.nn.Parameter(p.detach().clone()) for p in pc]
    torch.optim.Adam(pt, 1e-2, weight_decay=1e-2).load_state_dict(copy.deepcopy(sd))
    # averaged(): the averages inside, the live bits again afterwards -- also when the body raises
    live = [bits(p) for p in pd]
    avg = [bits(od.state[p]["ema"]) for p in pd]
    with od.averaged():
        assert all(np.array_equal(bits(p), a) for p, a in zip(pd, avg))
        assert all(np.array_equal(bits(od.state[p]["ema"]), x) for p, x in zip(pd, live))
    with pytest.raises(KeyError):
        with od.averaged():
            raise KeyError("from the body")
    assert all(np.array_equal(bits(p), x) for p, x in zip(pd, live))
    assert all(np.array_equal(bits(od.state[p]["ema"]), a) for p, a in zip(pd, avg))


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(built):
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-3, weight_decay=0.0, ema_decay=0.9))
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    g = torch.Generator().manual_seed(3)
    loader = []
    for i in range(5):                                                             # different images per iteration, same targets
        b = dict(batch)
        b["image"] = batch["image"] + 0.05 * torch.randn(batch["image"].shape, generator=g)
        loader.append(b)
    assert batch["image"].shape[0] == 2
    return z, cfgs, loader


def make_trainer(tiny, capture=False, validloader=None, **keys):
    from multitask_hydranet_amd.train import HydraTrainer
    z, cfgs, loader = tiny
    cfgs = copy.deepcopy(cfgs)
    cfgs["train"].update(keys)
    tr = HydraTrainer(cfgs, trainloader=loader, validloader=validloader, iters_per_epoch=len(loader), capture_step=capture)
    tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    return tr


def host_params(tr):
    return {n: p.detach().cpu().numpy().copy() for n, p in tr.hydranet.named_parameters()}


def step(tr, b):
    return tr.train_step({k: v.clone() for k, v in b.items()})


@pytest.mark.parametrize("capture,steps", [(False, 3), (True, 4)])
def test_trainer_average_follows_the_host_recurrence(tiny, capture, steps):
    """eager: three steps; capture_step: two eager and two replayed ones"""
    tr = make_trainer(tiny, capture=capture)
    assert tr.optimizer.ema_decay == 0.9 and tr.optimizer.ema_warmup is True
    want = host_params(tr)
    for k in range(steps):
        step(tr, tiny[2][k])
        snap = host_params(tr)
        avg = tr.optimizer.ema_named(tr.hydranet.named_parameters())
        for n in avg:
            want[n] = ema_ref.ema_step(want[n], snap[n], ema_ref.ema_decay_at(k, 0.9, True))
    assert (tr._cap is not None) == capture
    avg = tr.optimizer.ema_named(tr.hydranet.named_parameters())
    without = [n for n, p in tr.hydranet.named_parameters() if n not in avg]
    assert len(avg) >= 0.9 * len(want) and all(p.grad is None for n, p in tr.hydranet.named_parameters() if n in without)
    assert all("p5_to_p6" in n for n in without), without                          # the tensors that never get a gradient
    moved = 0
    for n, e in avg.items():
        assert np.array_equal(bits(e).reshape(-1), want[n].view(np.int32).reshape(-1)), n
        moved += not np.array_equal(want[n], snap[n])
    assert moved >= 0.5 * len(avg)                                                 # the average lags the weights: it is not a copy of them


def eval_losses(tr, net, batch):
    """what valid() computes per batch, on `net`"""
    net.eval()
    with torch.no_grad():
        b = tr.to_gpu({k: v.clone() for k, v in batch.items()})
        ld = net.cal_loss(net(b["image"]), b)
        ld["total_loss"] = tr.cal_total_loss(ld)
    return {k: float(v) for k, v in ld.items()}


def test_validation_and_checkpoint_with_the_average(tiny, tmp_path):
    from multitask_hydranet_amd import HydraNet
    vb = tiny[2][4]
    tr = make_trainer(tiny, capture=True, validloader=[{k: v.clone() for k, v in vb.items()}])
    for k in range(3):
        step(tr, tiny[2][k])
    assert tr._cap is not None                                                     # the third step was captured
    live = {n: bits(p) for n, p in tr.hydranet.named_parameters()}
    buffers = {n: b.detach().clone() for n, b in tr.hydranet.named_buffers()}
    path = str(tmp_path / "ema.pth")
    tr.save(path, ema=True)
    tr.valid(use_ema=True)
    assert tr.last_valid["ema"] is True and len(tr.last_valid["losses"]) == 1
    with_avg = tr.last_valid["losses"][0]
    assert all(np.array_equal(bits(p), live[n]) for n, p in tr.hydranet.named_parameters())
    tr.valid(use_ema=False)
    assert tr.last_valid["ema"] is False
    with_live = tr.last_valid["losses"][0]
    assert all(np.array_equal(bits(p), live[n]) for n, p in tr.hydranet.named_parameters())
    tr.valid()                                                                     # None: on when the average is on
    assert tr.last_valid["ema"] is True and tr.last_valid["losses"][0] == with_avg
    # the checkpoint: strict load, averaged parameters, live buffers
    sd = torch.load(path, map_location="cpu")
    fresh = HydraNet(copy.deepcopy(tr.cfgs))
    fresh.load_state_dict(sd, strict=True)
    fresh = fresh.to(dev())
    fresh.lane_points_per_line = tr.hydranet.lane_points_per_line
    avg = tr.optimizer.ema_named(tr.hydranet.named_parameters())
    for n, p in fresh.named_parameters():
        assert np.array_equal(bits(p), bits(avg[n]) if n in avg else live[n]), n
    for n, b in fresh.named_buffers():
        assert torch.equal(b, buffers[n]), n
    got = eval_losses(tr, fresh, vb)
    print("valid(use_ema=True)", with_avg, "\nfresh net from save(ema=True)", got, "\nvalid(use_ema=False)", with_live)
    assert got == with_avg
    assert with_live != with_avg and with_live["total_loss"] != with_avg["total_loss"]       # the eval-mode caches were dropped
    # the captured step still replays: parameter addresses never changed
    cap = tr._cap
    ld = step(tr, tiny[2][3])
    assert tr._cap is cap and all(bool(torch.isfinite(v)) for v in ld.values())
    now = {n: bits(p) for n, p in tr.hydranet.named_parameters()}
    assert sum(not np.array_equal(now[n], live[n]) for n in now) >= 0.5 * len(now)


def test_trainer_key_needs_the_hip_adam(tiny):
    from multitask_hydranet_amd.train import HydraTrainer
    with pytest.raises(ValueError):
        HydraTrainer(copy.deepcopy(tiny[1]), trainloader=tiny[2], iters_per_epoch=5, hip_adam=False)
    for off in (None, -1.0):                                                    # absent or <= 0: off, with either optimizer
        cfgs = copy.deepcopy(tiny[1])
        if off is None:
            del cfgs["train"]["ema_decay"]
        else:
            cfgs["train"]["ema_decay"] = off
        tr = HydraTrainer(cfgs, trainloader=tiny[2], iters_per_epoch=5, hip_adam=False)
        assert tr.ema_decay is None
        with pytest.raises(ValueError):
            tr.save("unused.pth", ema=True)
