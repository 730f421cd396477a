"""HydraTrainer.save_state / load_state / checkpoint_wait and run_training's train.state_file on the device: the tiny cfg and the eight
perturbed fixture batches of tests/test_grad_accum_train_gpu.py (this file's own copy of that set-up), with every option that adds
state on: grad_clip_norm, skip_nonfinite, ema_decay, protect_bn_stats, ema_buffers.  A run that is saved, loaded into a fresh trainer
with other weights and continued must end where the uninterrupted run ends: every comparison is bit for bit."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import ckpt_ref as ref
from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu

ALL_ON = dict(grad_clip_norm=5.0, skip_nonfinite=True, ema_decay=0.9, protect_bn_stats=True, ema_buffers=True)


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    g = torch.Generator().manual_seed(3)
    loader = []
    for i in range(8):                                                             # different images per batch, same targets
        b = dict(batch)
        b["image"] = batch["image"] + 0.05 * torch.randn(batch["image"].shape, generator=g)
        loader.append(b)
    return z, cfgs, loader


def fresh(b):
    return {k: v.clone() for k, v in b.items()}


def make_trainer(tiny, capture=False, distribute=False, loader=None, weights=True, validloader=None, **keys):
    """weights=False: the model keeps its random initial weights (drawn from a seed of its own: not the fixture's, not another
    trainer's) -- what a state file is loaded INTO"""
    from multitask_hydranet_amd.train import HydraTrainer
    z, cfgs, ld = tiny
    cfgs = copy.deepcopy(cfgs)
    cfgs["train"].update({k: v for k, v in {**ALL_ON, **keys}.items() if v is not None})      # (a key given as None: left out)
    loader = ld if loader is None else loader
    if not weights:
        torch.manual_seed(1000 + make_trainer.made)
    make_trainer.made += 1
    tr = HydraTrainer(cfgs, trainloader=loader, validloader=validloader, iters_per_epoch=len(loader), capture_step=capture, force_distribute=distribute)
    if weights:
        tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    return tr


make_trainer.made = 0


def bits(t):
    return t.detach().contiguous().view(torch.int32).clone() if t.dtype == torch.float32 else t.detach().contiguous().clone()


def device_state(tr):
    """every tensor of the training state, by name: parameters, buffers, moments and weight averages, keeper averages, the record"""
    out = {"p/" + n: bits(p) for n, p in tr.hydranet.named_parameters()}
    out.update({"b/" + n: bits(b) for n, b in tr.hydranet.named_buffers()})
    names = {p: n for n, p in tr.hydranet.named_parameters()}
    for p, st in tr.optimizer.state.items():
        out.update({"o/%s/%s" % (names[p], k): bits(st[k]) for k in ("exp_avg", "exp_avg_sq", "ema") if k in st})
    if tr.buffer_keeper is not None:
        out.update({"k/" + n: bits(a) for n, a in tr.buffer_keeper.ema_named().items()})
    if tr.optimizer.guarded:
        out["record"] = tr.optimizer.guard_record.clone()
    return out


def host_state(tr):
    names = {p: n for n, p in tr.hydranet.named_parameters()}
    return dict(last_epoch=tr.scheduler.last_epoch, lr=[g["lr"] for g in tr.optimizer.param_groups], last_lr=list(tr.scheduler.get_last_lr()),
                steps={names[p]: (int(st["step"]), st.get("ema_start")) for p, st in tr.optimizer.state.items()},
                settles=None if tr.buffer_keeper is None else tr.buffer_keeper.settles, phase=tr.phase,
                group=sorted(names[p] for p in tr.optimizer.param_groups[0]["params"]))


def differing(a, b):
    return [n for n in sorted(set(a) | set(b)) if n not in a or n not in b or not torch.equal(a[n], b[n])]


def assert_same_run(x, y):
    """two trainers hold the same training state: every device tensor bit for bit, the host-side state with =="""
    dx, dy = device_state(x), device_state(y)
    assert sorted(dx) == sorted(dy), sorted(set(dx) ^ set(dy))[:5]
    assert not differing(dx, dy), (len(differing(dx, dy)), differing(dx, dy)[:5])
    hx, hy = host_state(x), host_state(y)
    for k in hx:
        assert hx[k] == hy[k], (k, hx[k] if k not in ("steps", "group") else "...", hy[k] if k not in ("steps", "group") else "...")
    assert any(n.startswith("o/") and n.endswith("/ema") for n in dx) and any(n.startswith("k/") for n in dx) and "record" in dx


def step(tr, b):
    return tr.train_step(fresh(b))


def run(tr, batches):
    for b in batches:
        step(tr, b)
    return tr


@pytest.fixture(scope="module")
def straight(tiny):
    """A: batches 0-5, uninterrupted"""
    return run(make_trainer(tiny), tiny[2][:6])


@pytest.fixture(scope="module")
def saved3(tiny, tmp_path_factory):
    """B: batches 0-2, then save_state -> (B, the file's path)"""
    tr = run(make_trainer(tiny), tiny[2][:3])
    path = str(tmp_path_factory.mktemp("state") / "b3.hn")
    tr.save_state(path)
    return tr, path


def test_control_two_fresh_runs_are_bit_identical(tiny, straight):
    """every later assertion rests on this: the same six batches from the same start end in the same bits"""
    twin = run(make_trainer(tiny), tiny[2][:6])
    assert_same_run(straight, twin)
    r = twin.optimizer.grad_guard_record()
    print("control: the last step's record", r)
    assert r["steps"] == 6 and r["skipped"] == 0 and twin.buffer_keeper.settles == 6 and 0.0 < r["coef"] <= 1.0, r


def test_file_is_what_the_format_says(tiny, saved3):
    tr, path = saved3
    assert not os.path.exists(path + ".tmp")
    manifest, blob = ref.read(open(path, "rb").read())                              # the yardstick's reader, not checkpoint.py's
    assert ref.bad_tensors(manifest, blob) == []
    names = [e["name"] for e in manifest["tensors"]]
    sd = tr.hydranet.state_dict()
    assert names[:len(sd)] == ["model/" + k for k in sd]                            # every parameter and persistent buffer, in state_dict order
    assert "guard/record" in names and any(n.startswith("keeper/avg/") for n in names) and any(n.endswith("/ema") for n in names)
    assert not any("shadow" in n or "_seg_class_weight" in n for n in names)
    for n, p in tr.hydranet.named_parameters():
        assert np.array_equal(ref.tensor(manifest, blob, "model/" + n).view(np.int32), bits(p).cpu().numpy()), n
    host = manifest["host"]
    assert host["epoch"] == 0 and host["phase"] == "joint" and host["settles"] == 3 and host["scheduler"]["last_epoch"] == 3
    assert host["param_groups"][0]["lr"] == tr.optimizer.param_groups[0]["lr"]
    assert host["train"] == dict(grad_clip_norm=5.0, skip_nonfinite=True, ema_decay=0.9, ema_warmup=True, protect_bn_stats=True,
                                 ema_buffers=True, accum_steps=1)
    assert {v["step"] for v in host["params"].values()} == {3} and {v["ema_start"] for v in host["params"].values()} == {0}


def test_resume(tiny, straight, saved3):
    b, path = saved3
    c = make_trainer(tiny, weights=False)
    before = {n: bits(p) for n, p in c.hydranet.named_parameters()}
    live = {n: p for n, p in c.hydranet.named_parameters()}
    assert len(differing(before, {n: bits(p) for n, p in b.hydranet.named_parameters()})) > 0.5 * len(before)     # other weights
    host = c.load_state(path)
    assert host["epoch"] == 0 and c.next_epoch == 0
    assert all(live[n] is p for n, p in c.hydranet.named_parameters())              # written in place: no tensor object replaced
    assert_same_run(b, c)
    run(c, tiny[2][3:6])
    assert_same_run(straight, c)
    assert c.optimizer.param_groups[0]["lr"] == straight.optimizer.param_groups[0]["lr"] and c.scheduler.last_epoch == 6


def test_resume_under_capture(tiny, saved3):
    a = run(make_trainer(tiny, capture=True), tiny[2][:6])
    assert a._cap is not None                                                      # replaying from batch 2 on
    b = run(make_trainer(tiny, capture=True), tiny[2][:3])
    path = saved3[1] + ".cap"
    b.save_state(path)
    c = make_trainer(tiny, capture=True, weights=False)
    c.load_state(path)
    run(c, tiny[2][3:5])
    assert c._cap is None                                                          # two eager steps first
    step(c, tiny[2][5])
    assert c._cap is not None
    assert_same_run(a, c)


def phase_run(tiny, tr, stop=None, resume=None):
    """joint x2, lane x2, [save | load], lane x1, joint x1"""
    ld = tiny[2]
    if resume is None:
        run(tr, ld[:2])
        tr.set_phase("lane")
        run(tr, ld[2:4])
        if stop is not None:
            tr.save_state(stop)
            return tr
    else:
        tr.load_state(resume)
        assert tr.phase == "lane"
    step(tr, ld[4])
    tr.set_phase("joint")
    step(tr, ld[5])
    return tr


def test_resume_across_a_phase_change(tiny, tmp_path):
    path = str(tmp_path / "phase.hn")
    a = phase_run(tiny, make_trainer(tiny))
    phase_run(tiny, make_trainer(tiny), stop=path)
    steps = {v["step"] for v in ref.read(open(path, "rb").read())[0]["host"]["params"].values()}
    assert steps == {2, 4}                                                         # cohorts with different step counts in the file
    c = phase_run(tiny, make_trainer(tiny, weights=False), resume=path)
    assert_same_run(a, c)
    assert {s for s, _ in host_state(c)["steps"].values()} == {3, 6}


def test_resume_through_a_skipped_step(tiny, tmp_path):
    ld = [fresh(b) for b in tiny[2][:6]]
    ld[2]["image"][0, 0, 0, 0] = float("nan")
    a = run(make_trainer(tiny), ld)
    ra = a.optimizer.grad_guard_record()
    assert ra["steps"] == 6 and ra["skipped"] == 1 and ra["skipped_consecutive"] == 0, ra
    b = run(make_trainer(tiny), ld[:3])
    rb = b.optimizer.grad_guard_record()
    assert rb["skip"] != 0 and rb["skipped"] == 1 and rb["skipped_consecutive"] == 1, rb
    path = str(tmp_path / "skipped.hn")
    b.save_state(path)
    c = make_trainer(tiny, weights=False)
    c.load_state(path)
    assert_same_run(b, c)                                                          # (the record's eight words among the tensors)
    rc = c.optimizer.grad_guard_record()
    assert rc["skip"] == rb["skip"] and rc["steps"] == 3 and rc["skipped"] == 1 and rc["skipped_consecutive"] == 1, rc
    step(c, ld[3])
    rc = c.optimizer.grad_guard_record()
    assert rc["steps"] == 4 and rc["skipped"] == 1 and rc["skipped_consecutive"] == 0, rc
    run(c, ld[4:])
    assert_same_run(a, c)
    assert c.optimizer.grad_guard_record() == ra


def test_accumulation(tiny, tmp_path):
    ld = tiny[2]
    a = run(make_trainer(tiny, accum_steps=2), ld[:6])
    b = run(make_trainer(tiny, accum_steps=2), ld[:3])
    path = str(tmp_path / "accum.hn")
    assert b.accumulator.pending == 1
    with pytest.raises(RuntimeError):
        b.save_state(path)                                                         # mid-group
    assert not os.path.exists(path) and not os.path.exists(path + ".tmp")
    step(b, ld[3])
    assert b.accumulator.pending == 0
    b.save_state(path)                                                             # at a group's boundary
    c = make_trainer(tiny, weights=False, accum_steps=2)
    c.load_state(path)
    run(c, ld[4:6])
    assert_same_run(a, c)
    assert c.scheduler.last_epoch == 3
    d = make_trainer(tiny, weights=False)                                          # accum_steps differs: refused
    with pytest.raises(ValueError, match="accum_steps"):
        d.load_state(path)


def test_asynchronous_save(tiny, saved3, tmp_path):
    _, sync_path = saved3                                                          # the twin: wait=True after batches 0-2
    tr = run(make_trainer(tiny), tiny[2][:3])
    path = str(tmp_path / "async.hn")
    tr.save_state(path, wait=False)
    run(tr, tiny[2][3:5])                                                          # training goes on at once: it must not reach the file
    tr.checkpoint_wait()
    assert tr._ckpt_thread is None and not os.path.exists(path + ".tmp")
    assert open(path, "rb").read() == open(sync_path, "rb").read()
    tr.save_state(path, wait=False)                                                # a second save joins the first, and so does a load
    tr.load_state(path)
    assert tr._ckpt_thread is None
    assert ref.read(open(path, "rb").read())[0]["host"]["scheduler"]["last_epoch"] == 5


def flip_blob_byte(src, dst, name, word=0):
    data = bytearray(open(src, "rb").read())
    manifest, _ = ref.read(bytes(data))
    e = next(e for e in manifest["tensors"] if e["name"] == name)
    data[ref.sections(bytes(data))[3] + 4 * (e["offset"] + word) + 1] ^= 0x04
    with open(dst, "wb") as f:
        f.write(bytes(data))
    return dst


def optimizer_view(tr):
    sd = tr.optimizer.state_dict()
    return ({k: {kk: (vv.clone() if isinstance(vv, torch.Tensor) else vv) for kk, vv in v.items()} for k, v in sd["state"].items()},
            copy.deepcopy(sd["param_groups"]))


def same_optimizer_view(x, y):
    (sx, gx), (sy, gy) = x, y
    return gx == gy and sorted(sx) == sorted(sy) and all(
        sorted(sx[k]) == sorted(sy[k]) and all(torch.equal(a, sy[k][n]) if isinstance(a, torch.Tensor) else a == sy[k][n] for n, a in sx[k].items())
        for k in sx)


@pytest.mark.parametrize("stepped", [False, True])
def test_corrupt_file(tiny, saved3, tmp_path, stepped):
    from multitask_hydranet_amd.checkpoint import CheckpointCorrupt, CheckpointError
    _, path = saved3
    manifest, _ = ref.read(open(path, "rb").read())
    victim = [e["name"] for e in manifest["tensors"] if e["name"].endswith("/exp_avg_sq") and e["words"] > 8][5]
    bad = flip_blob_byte(path, str(tmp_path / "bad.hn"), victim, word=7)
    tr = make_trainer(tiny, weights=False)
    if stepped:
        run(tr, tiny[2][6:8])                                                      # moments, averages, a keeper and a record of its own
    before, opt_before, host_before = device_state(tr), optimizer_view(tr), host_state(tr)
    keeper = tr.buffer_keeper
    with pytest.raises(CheckpointCorrupt, match=victim.replace(".", r"\.")) as ei:
        tr.load_state(bad)
    assert ei.value.tensor == victim and isinstance(ei.value, CheckpointError)
    after = device_state(tr)
    assert sorted(before) == sorted(after) and not differing(before, after)        # every parameter, buffer and moment keeps its bits
    assert same_optimizer_view(opt_before, optimizer_view(tr)) and host_state(tr) == host_before and tr.buffer_keeper is keeper
    assert (len(opt_before[0]) > 0) == stepped
    step(tr, tiny[2][0])                                                           # the trainer still steps
    torch.cuda.synchronize()
    assert tr.optimizer.grad_guard_record()["steps"] == (3 if stepped else 1)
    tr.load_state(path)                                                            # and still loads the good file
    assert tr.scheduler.last_epoch == 3


def test_mismatch_is_refused_before_anything_is_touched(tiny, saved3):
    _, path = saved3
    tr = make_trainer(tiny, weights=False, ema_decay=None, ema_buffers=None)
    assert tr.ema_decay is None
    step(tr, tiny[2][0])
    before, opt_before, host_before = device_state(tr), optimizer_view(tr), host_state(tr)
    with pytest.raises(ValueError, match="ema_decay"):
        tr.load_state(path)
    assert not differing(before, device_state(tr)) and same_optimizer_view(opt_before, optimizer_view(tr)) and host_state(tr) == host_before


class StopsInSecondEpoch:
    """a loader whose second pass raises before its first batch: the run is interrupted after epoch 0"""

    def __init__(self, batches):
        self.batches, self.passes = batches, 0

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        self.passes += 1
        if self.passes > 1:
            raise KeyboardInterrupt("interrupted")
        return iter([fresh(b) for b in self.batches])


def test_run_training_with_a_state_file(tiny, tmp_path):
    from multitask_hydranet_amd.train import run_training
    batches = tiny[2][:3]
    quiet = lambda *a: None
    whole = make_trainer(tiny, loader=[fresh(b) for b in batches], epoch=2)
    run_training(whole, log=quiet)                                                 # a straight two-epoch run (no state_file: nothing changes)
    assert whole.scheduler.last_epoch == 6 and whole._packer is None
    path = str(tmp_path / "run.hn")
    first = make_trainer(tiny, loader=StopsInSecondEpoch(batches), epoch=2, state_file=path)
    with pytest.raises(KeyboardInterrupt):
        run_training(first, log=quiet)
    assert first.scheduler.last_epoch == 3 and os.path.isfile(path) and not os.path.exists(path + ".tmp")
    assert ref.read(open(path, "rb").read())[0]["host"]["epoch"] == 1
    second = make_trainer(tiny, loader=[fresh(b) for b in batches], weights=False, epoch=2, state_file=path)
    lines = []
    run_training(second, log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    assert any("RESUMED" in l for l in lines) and second.scheduler.last_epoch == 6
    assert_same_run(whole, second)
    assert not os.path.exists(path + ".tmp") and ref.read(open(path, "rb").read())[0]["host"]["epoch"] == 2


def test_world_one_exchange_path(tiny, tmp_path):
    """force_distribute=True: one save / load / step round trip on the data-parallel code path at world size 1"""
    f = run(make_trainer(tiny, distribute=True), tiny[2][:2])
    assert f.reducer is not None
    path = str(tmp_path / "ddp.hn")
    f.save_state(path)
    g = make_trainer(tiny, distribute=True, weights=False)
    g.load_state(path)
    assert_same_run(f, g)
    step(f, tiny[2][2])
    step(g, tiny[2][2])
    torch.cuda.synchronize()
    assert_same_run(f, g)


def test_validation_after_load(tiny, saved3):
    vb = tiny[2][4]
    b, path = saved3
    b.validloader = [fresh(vb)]
    want = b.valid()
    want_losses = b.last_valid["losses"]
    assert b.last_valid["ema"] is True
    c = make_trainer(tiny, weights=False, validloader=[fresh(vb)])
    c.hydranet.eval()
    with torch.no_grad():
        c.hydranet.prepare_inference()                                             # eval-mode operands folded from the OLD weights and statistics
        c.hydranet(c.to_gpu(fresh(vb))["image"])
    c.hydranet.train()
    c.load_state(path)
    c.hydranet.eval()
    with torch.no_grad():
        b.hydranet.eval()
        x = c.to_gpu(fresh(vb))["image"]
        got, ref_out = c.hydranet(x), b.hydranet(x)
        b.hydranet.train()
    c.hydranet.train()
    assert torch.equal(got["seg"], ref_out["seg"])                                 # the folded operands were rebuilt: the mutation cells were bumped
    scores = c.valid()
    assert torch.equal(scores, want) and c.last_valid["losses"] == want_losses and c.last_valid["ema"] is True
