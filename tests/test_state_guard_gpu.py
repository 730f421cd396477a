"""BatchNorm running statistics under the step guard and the weight average: hn_state_guard's three modes against tests/state_guard_ref.py
bit for bit (word copies and individually rounded float operations: no tolerance anywhere) over mixed jobs inside sentinel bands, aligned
and with live / shadow / average off by 4 bytes; and HydraTrainer's train.protect_bn_stats / train.ema_buffers: a skipped step leaves the
statistics where they were (a twin without the key shows that they would have moved), the buffer averages follow the host recurrence, and
valid() / save(ema=True) use them while the captured step keeps replaying."""
import copy

import numpy as np
import pytest
import torch

from tests import ema_ref, state_guard_ref as ref
from tests.guards import BAND, SENT32
from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu

WORDS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 2049]
# (words, kind, has shadow, has average): every size as fp32 values and as raw words, with both, without an average, without a shadow
CASES = [(n, kind, s, a) for n in WORDS for kind in (0, 1) for s, a in ((True, True), (True, False), (False, True))] + [(5, 0, False, False)]
SPECIAL = [0x7FC00001, 0x7FC12345, 0xFFC00002, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF]
ROLES = ("live", "shadow", "avg")


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
    """the tensor's 32-bit words, flat (an int64 counter is two of them)"""
    return t.detach().reshape(-1).contiguous().view(torch.int32).cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel
def pattern_words(g, n, roll):
    """arbitrary bit patterns (every kind of float among them), with NaNs of distinct payloads, +-inf, +-0 and denormals planted at the
    start of every array that has room"""
    w = g.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    k = min(n, len(SPECIAL))
    w[:k] = np.roll(np.array(SPECIAL, dtype=np.uint32), roll)[:k]
    return w.view(np.int32)


def make_jobs(seed, floats):
    """floats: live and average of the kind 0 jobs are standard-normal values (the inputs of an averaging launch); else every array
    holds arbitrary bit patterns"""
    g = np.random.default_rng(seed)
    normal = lambda n: g.standard_normal(n).astype(np.float32).view(np.int32)
    jobs = []
    for i, (n, kind, has_shadow, has_avg) in enumerate(CASES):
        as_float = floats and kind == 0
        jobs.append(dict(live=normal(n) if as_float else pattern_words(g, n, i),
                         shadow=pattern_words(g, n, i + 3) if has_shadow else None,
                         avg=(normal(n) if as_float else pattern_words(g, n, i + 6)) if has_avg else None, kind=kind))
    return jobs


class Layout:
    """the arrays of one role (live / shadow / avg) in ONE flat device buffer of sentinel words: BAND sentinels before and after every
    tensor, every tensor starting on a 16-byte boundary plus `off` words"""

    def __init__(self, jobs, role, off):
        self.role, self.spans, pos = role, [], 0
        for j in jobs:
            if j[role] is None:
                self.spans.append(None)
                continue
            start = pos + BAND + off
            self.spans.append((start, start + j[role].size))
            pos = (start + j[role].size + 3) // 4 * 4
        self.total = pos + BAND
        self.buf = torch.empty((self.total,), dtype=torch.int32, device=dev())
        assert self.buf.data_ptr() % 16 == 0 and BAND % 4 == 0

    def host(self, jobs):
        h = np.full((self.total,), SENT32, dtype=np.int32)
        for j, sp in zip(jobs, self.spans):
            if sp is not None:
                h[sp[0]:sp[1]] = j[self.role]
        return h

    def ptr(self, i):
        return 0 if self.spans[i] is None else self.buf.data_ptr() + 4 * self.spans[i][0]


def run_all(l, offs):
    """every launch of the test with live / shadow / avg at offsets `offs` (words), each from fresh contents, each held to the yardstick
    over the WHOLE buffers (bands and the arrays a mode must not write included) -> the resulting buffers' tensors per launch"""
    pats, flts = make_jobs(1, False), make_jobs(2, True)
    lay = {r: Layout(pats, r, o) for r, o in zip(ROLES, offs)}
    rows, owner, blk = [], [], 0
    for i, j in enumerate(pats):
        nb = (j["live"].size + 1023) // 1024
        rows.append([lay["live"].ptr(i), lay["shadow"].ptr(i), lay["avg"].ptr(i), j["live"].size, blk, j["kind"]])
        owner += [i] * nb
        blk += nb
    for r, o in zip(ROLES, offs):
        assert all(p % 16 == 4 * o for p in (lay[r].ptr(i) for i in range(len(pats))) if p), (r, o)
    assert blk > len(pats) and any(r[1] == 0 for r in rows) and any(r[2] == 0 for r in rows)
    jobs_t, owner_t = torch.tensor(rows, dtype=torch.int64).to(dev()), torch.tensor(owner, dtype=torch.int32).to(dev())
    # (mode, skip word or None = no record, ema_decay); mode 0 ignores a raised record and a NaN decay
    launches = [(0, 1, float("nan"))] + [(1, s, 0.0) for s in (None, 0, 1, 2, 4)] + [(2, None, 0.9998), (2, 0, 0.9)] + [(2, s, 0.5) for s in (1, 2, 4)]
    results = []
    for mode, skip, decay in launches:
        start = flts if mode == 2 and not skip else pats
        want = ref.snapshot(start) if mode == 0 else ref.settle(start, skip, decay if mode == 2 else None)
        for r in ROLES:
            lay[r].buf.copy_(torch.from_numpy(lay[r].host(start)))
        rec = None
        if skip is not None:
            rec = torch.tensor([0x40490FDB, 0x3F800000, skip, 5, 1, 1, 0, 0], dtype=torch.int32).to(dev())     # norm, coef, skip, counters
        l.call("hn_state_guard", jobs_t.data_ptr(), owner_t.data_ptr(), blk, mode, None if rec is None else rec.data_ptr(), decay)
        torch.cuda.synchronize()
        got = {r: lay[r].buf.cpu().numpy() for r in ROLES}
        for r in ROLES:
            exp = lay[r].host(want)
            bad = np.nonzero(got[r] != exp)[0]
            assert bad.size == 0, (mode, skip, r, offs, "first differing words", bad[:4].tolist(), "of", bad.size)
        # the launch wrote what its mode writes, and only that role: the comparison above is not one of unchanged buffers
        changed = {r: not np.array_equal(got[r], lay[r].host(start)) for r in ROLES}
        writes = "shadow" if mode == 0 else "live" if skip else "avg" if mode == 2 else None
        assert changed == {r: r == writes for r in ROLES}, (mode, skip, changed)
        results.append([got[r][sp[0]:sp[1]].copy() for r in ROLES for sp in lay[r].spans if sp is not None])
    return results


def test_kernel_against_the_yardstick_aligned_and_offset(built):
    pats = make_jobs(1, False)
    nans = {int(x) & 0xFFFFFFFF for j in pats for x in j["live"][:10] if (int(x) & 0x7F800000) == 0x7F800000 and int(x) & 0x7FFFFF}
    assert len(nans) >= 4                                                          # NaNs of distinct payloads among the words
    aligned = run_all(built, (0, 0, 0))
    for offs in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):                      # each of live / shadow / avg off by 4 bytes
        other = run_all(built, offs)
        assert len(other) == len(aligned) == 11
        assert all(np.array_equal(x, y) for a, b in zip(aligned, other) for x, y in zip(a, b)), offs


def test_bad_arguments_launch_nothing(built):
    jobs = make_jobs(3, True)
    lay = {r: Layout(jobs, r, 0) for r in ROLES}
    rows, owner, blk = [], [], 0
    for i, j in enumerate(jobs):
        nb = (j["live"].size + 1023) // 1024
        rows.append([lay["live"].ptr(i), lay["shadow"].ptr(i), lay["avg"].ptr(i), j["live"].size, blk, j["kind"]])
        owner += [i] * nb
        blk += nb
    for r in ROLES:
        lay[r].buf.copy_(torch.from_numpy(lay[r].host(jobs)))
    jobs_t, owner_t = torch.tensor(rows, dtype=torch.int64).to(dev()), torch.tensor(owner, dtype=torch.int32).to(dev())
    rec = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32).to(dev())
    f, st = built.raw("hn_state_guard"), torch.cuda.current_stream().cuda_stream
    for decay in (1.0, -0.1, float("nan")):
        assert f(jobs_t.data_ptr(), owner_t.data_ptr(), blk, 2, None, decay, st) == 1, decay
    for mode in (-1, 3):
        assert f(jobs_t.data_ptr(), owner_t.data_ptr(), blk, mode, rec.data_ptr(), 0.5, st) == 1, mode
    assert f(jobs_t.data_ptr(), owner_t.data_ptr(), 0, 0, None, 0.5, st) == 1
    torch.cuda.synchronize()
    for r in ROLES:
        assert np.array_equal(lay[r].buf.cpu().numpy(), lay[r].host(jobs)), r


# ------------------------------------------------------------------------------------------------------------------------------------
# the trainer (the tiny cfg, batch 2: test_grad_guard_gpu.py's recipes, restated)
@pytest.fixture(scope="module")
def tiny(built):
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
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


def step(tr, b):
    return tr.train_step({k: v.clone() for k, v in b.items()})


def poisoned(b):
    """a NaN lane target: the loss is NaN while activations and statistics stay finite"""
    b = {k: v.clone() for k, v in b.items()}
    row = (b["gt_cls"][..., 1] > 0).nonzero()[0]
    b["gt_loc"][row[0], row[1], 0] = float("nan")
    return b


def buffers_of(tr):
    """{name: words} of every persistent buffer (the state dict's entries that are not parameters), counters included"""
    params = {n for n, _ in tr.hydranet.named_parameters()}
    out = {n: bits(t) for n, t in tr.hydranet.state_dict().items() if n not in params}
    assert any(n.endswith(".running_mean") for n in out) and any(n.endswith(".num_batches_tracked") for n in out)
    return out


def counter(words):
    return int(words.view(np.int64)[0])


def moved_report(before, now):
    """-> (fraction of running_mean tensors whose bits changed, {counter name: increment})"""
    means = [n for n in before if n.endswith(".running_mean")]
    frac = sum(not np.array_equal(before[n], now[n]) for n in means) / len(means)
    return frac, {n: counter(now[n]) - counter(before[n]) for n in before if n.endswith(".num_batches_tracked")}


def assert_statistics_moved(before, now, what):
    """what a training forward does to the statistics: at least half of the running means change and every counter goes up by one --
    except those of the BatchNorm the forward never runs (p5_to_p6: with five backbone stages P6 comes from the last stage)"""
    frac, incs = moved_report(before, now)
    assert frac >= 0.5, (what, frac)
    assert all(d == 1 or (d == 0 and "p5_to_p6" in n) for n, d in incs.items()), (what, {n: d for n, d in incs.items() if d != 1})
    assert sum(incs.values()) >= 0.9 * len(incs), what


def all_finite(tr):
    return all(bool(torch.isfinite(t).all()) for t in tr.hydranet.state_dict().values() if t.is_floating_point())


@pytest.mark.parametrize("capture,at", [(False, 1), (True, 3)])
def test_skipped_step_rolls_the_statistics_back(tiny, capture, at):
    """eager, poisoned second batch; capture_step, poisoned at the fourth iteration -- a pure replay"""
    loader = tiny[2]
    tr = make_trainer(tiny, capture=capture, skip_nonfinite=True, protect_bn_stats=True)
    twin = make_trainer(tiny, capture=capture, skip_nonfinite=True)
    assert twin.buffer_keeper is None and not twin.protect_bn_stats and tr.protect_bn_stats and not tr.ema_buffers
    for b in loader[:at]:
        step(tr, b)
        step(twin, b)
    assert twin.buffer_keeper is None and tr.buffer_keeper is not None and tr.buffer_keeper.avg is None
    assert (tr._cap is not None) == capture
    cap = tr._cap
    before, twin_before = buffers_of(tr), buffers_of(twin)
    assert all(np.array_equal(before[n], twin_before[n]) for n in before)           # without a skipped step the key changes nothing
    bad = poisoned(loader[at])
    for t in (tr, twin):
        ld = step(t, bad)
        assert not bool(torch.isfinite(ld["total_loss"])), ld                      # precondition: the poison reaches the total loss
        r = t.optimizer.grad_guard_record()
        assert r["skip"] != 0 and r["skipped"] == 1 and r["steps"] == at + 1, r
    now = buffers_of(tr)
    for n in before:
        assert np.array_equal(now[n], before[n]), n                                # every statistic and counter: the bits before the step
    assert_statistics_moved(twin_before, buffers_of(twin), "the twin without protect_bn_stats")   # ... which the forward had moved
    ld = step(tr, loader[at + 1])
    assert bool(torch.isfinite(ld["total_loss"]))
    assert tr.optimizer.grad_guard_record()["skip"] == 0
    after = buffers_of(tr)
    assert_statistics_moved(before, after, "the next clean step")
    assert all_finite(tr)
    assert tr._cap is cap
    if not capture:
        # [b0, poisoned b1, b2] against a trainer that never saw b1: the skip left parameters untouched, so b2's forward is the same
        clean = make_trainer(tiny, skip_nonfinite=True, protect_bn_stats=True)
        step(clean, loader[0])
        step(clean, loader[2])
        want = buffers_of(clean)
        for n in want:
            assert np.array_equal(after[n], want[n]), n


def host_buffers(tr):
    return {n: t.detach().cpu().numpy().copy() for n, t in tr.hydranet.named_buffers() if n.endswith((".running_mean", ".running_var", ".num_batches_tracked"))}


@pytest.mark.parametrize("capture,steps,poison", [(False, 3, False), (True, 4, False), (False, 3, True), (True, 4, True)])
def test_buffer_average_follows_the_host_recurrence(tiny, capture, steps, poison):
    """eager: three steps; capture_step: two eager and two replayed ones; poison: with skip_nonfinite, one more (skipped) step leaves
    every average as it was, and still counts as a step of the decay schedule"""
    loader = tiny[2]
    tr = make_trainer(tiny, capture=capture, ema_decay=0.9, ema_buffers=True, **(dict(skip_nonfinite=True) if poison else {}))
    assert tr.ema_buffers and not tr.protect_bn_stats and tr.buffer_keeper is None
    want = host_buffers(tr)                                                        # the averages start from the buffers before step 0
    floats = [n for n in want if not n.endswith(".num_batches_tracked")]

    def follow(k):
        live = host_buffers(tr)
        for n in floats:
            want[n] = ema_ref.ema_step(want[n], live[n], ema_ref.ema_decay_at(k, 0.9, True))
        return live

    def check(live, what):
        avg = tr.buffer_keeper.ema_named()
        assert sorted(avg) == sorted(want)
        for n, e in avg.items():
            exp = want[n] if n in floats else live[n]                              # the average of a counter is the counter
            assert e.shape == exp.shape and np.array_equal(bits(e), np.ascontiguousarray(exp).reshape(-1).view(np.int32)), (what, n)

    for k in range(steps):
        step(tr, loader[k])
        live = follow(k)
    assert (tr._cap is not None) == capture and tr.buffer_keeper.shadow is None
    check(live, "after %d steps" % steps)
    lag = sum(not np.array_equal(want[n], live[n]) for n in floats)
    assert lag >= 0.5 * len(floats)                                                # the average lags the statistics: it is not a copy
    if poison:
        cap = tr._cap
        avg_before = {n: bits(e) for n, e in tr.buffer_keeper.ema_named().items()}
        ld = step(tr, poisoned(loader[steps % len(loader)]))
        assert not bool(torch.isfinite(ld["total_loss"])) and tr.optimizer.grad_guard_record()["skip"] != 0
        for n, e in tr.buffer_keeper.ema_named().items():
            assert np.array_equal(bits(e), avg_before[n]), n
        assert tr.buffer_keeper.settles == steps + 1 and tr._cap is cap
        step(tr, loader[(steps + 1) % len(loader)])
        assert tr.optimizer.grad_guard_record()["skip"] == 0
        check(follow(steps + 1), "the clean step after the skipped one")           # (its decay is that of step number steps + 1)


def eval_losses(tr, net, batch):
    """what valid() computes per batch, on `net`"""
    net.eval()
    with torch.no_grad():
        b = tr.to_gpu({k: v.clone() for k, v in batch.items()})
        ld = net.cal_loss(net(b["image"]), b)
        ld["total_loss"] = tr.cal_total_loss(ld)
    return {k: float(v) for k, v in ld.items()}


def test_validation_and_checkpoint_with_the_averaged_buffers(tiny, tmp_path):
    from multitask_hydranet_amd import HydraNet
    loader = tiny[2]
    vb = loader[4]
    runs = {}
    for on in (True, False):
        tr = make_trainer(tiny, capture=True, validloader=[{k: v.clone() for k, v in vb.items()}], lr=1e-3, ema_decay=0.9, ema_buffers=on)
        for k in range(3):
            step(tr, loader[k])
        assert tr._cap is not None and (tr.buffer_keeper is not None) == on         # the third step was captured
        live = {n: bits(t) for n, t in tr.hydranet.state_dict().items()}
        path = str(tmp_path / ("ema_%d.pth" % on))
        tr.save(path, ema=True)
        tr.valid(use_ema=True)
        assert tr.last_valid["ema"] is True and len(tr.last_valid["losses"]) == 1
        # after valid(): every live parameter and every live buffer has its bits back
        assert all(np.array_equal(bits(t), live[n]) for n, t in tr.hydranet.state_dict().items())
        runs[on] = (tr, live, path, tr.last_valid["losses"][0])
    tr, live, path, with_avg = runs[True]
    # the same run without ema_buffers scores the same averaged weights under the live statistics: other losses
    assert all(np.array_equal(live[n], runs[False][1][n]) for n in live)             # (the key changes nothing about the training run)
    without = runs[False][3]
    print("valid(use_ema=True) with ema_buffers", with_avg, "\nwithout", without)
    assert without != with_avg and without["total_loss"] != with_avg["total_loss"]   # the buffers were exchanged, the folded caches dropped
    # the checkpoint: strict load, averaged parameters AND averaged buffers
    fresh = HydraNet(copy.deepcopy(tr.cfgs))
    fresh.load_state_dict(torch.load(path, map_location="cpu"), strict=True)
    fresh = fresh.to(dev())
    fresh.lane_points_per_line = tr.hydranet.lane_points_per_line
    avg_p = tr.optimizer.ema_named(tr.hydranet.named_parameters())
    avg_b = tr.buffer_keeper.ema_named()
    assert len(avg_b) == sum(n not in dict(tr.hydranet.named_parameters()) for n in live)      # every persistent buffer has an average
    for n, t in fresh.state_dict().items():
        assert np.array_equal(bits(t), bits(avg_b[n]) if n in avg_b else bits(avg_p[n]) if n in avg_p else live[n]), n
    assert sum(not np.array_equal(bits(avg_b[n]), live[n]) for n in avg_b if n.endswith(".running_mean")) >= 0.5 * len(avg_b) / 3
    got = eval_losses(tr, fresh, vb)
    print("fresh net from save(ema=True)", got)
    assert got == with_avg
    # without the key the checkpoint keeps the live buffers
    sd_off = torch.load(runs[False][2], map_location="cpu")
    assert all(np.array_equal(bits(sd_off[n]), live[n]) for n in avg_b)
    # the captured step still replays: no address changed
    cap = tr._cap
    ld = step(tr, loader[3])
    assert tr._cap is cap and all(bool(torch.isfinite(v)) for v in ld.values())
    assert_statistics_moved({n: live[n] for n in avg_b}, buffers_of(tr), "the replayed step after valid()")


def test_keys_off_and_prerequisites(tiny):
    from multitask_hydranet_amd.train import HydraTrainer
    tr = make_trainer(tiny)
    assert tr.buffer_keeper is None and tr._keeper() is None and (tr.protect_bn_stats, tr.ema_buffers) == (False, False)
    for keys, adam in ((dict(protect_bn_stats=True), True), (dict(ema_buffers=True), True), (dict(ema_buffers=True, skip_nonfinite=True), True),
                       (dict(protect_bn_stats=True, ema_decay=0.9), True)):
        cfgs = copy.deepcopy(tiny[1])
        cfgs["train"].update(keys)
        with pytest.raises(ValueError):
            HydraTrainer(cfgs, trainloader=tiny[2], iters_per_epoch=5, hip_adam=adam)
