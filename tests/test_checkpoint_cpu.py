"""CPU: the host side of full-state checkpoints (hn_ckpt.hip's entry points, multitask_hydranet_amd/checkpoint.py, tools/check_state.py):
the symbols are declared and exported, bad arguments are rejected before any HIP call, hn_state_checksum_host equals the yardstick
(tests/ckpt_ref.py), files round-trip, and damaged files are refused.  No kernel is launched here."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ckpt_ref as ref
from tests.helpers import ROOT

SYMBOLS = ("hn_state_pack", "hn_state_verify", "hn_state_unpack", "hn_state_checksum_host")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def C(built):
    from multitask_hydranet_amd import checkpoint
    return checkpoint


@pytest.fixture(scope="module")
def tool(built):
    spec = importlib.util.spec_from_file_location("check_state_tool", os.path.join(ROOT, "tools", "check_state.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_declares_and_library_exports_the_entry_points(built):
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    for name in SYMBOLS:
        assert name in sig and hasattr(dll, name) and name in built.lib().symbols(), name
    vp, lg = ctypes.c_void_p, ctypes.c_long
    tables = sig["hn_swap_many"][1][:3]                                            # jobs, block_job, total_blocks
    assert sig["hn_state_pack"] == (ctypes.c_int, tables + [lg, vp, vp, vp], True)
    assert sig["hn_state_verify"] == (ctypes.c_int, tables + [lg, vp, vp, vp, vp, vp], True)
    assert sig["hn_state_unpack"] == (ctypes.c_int, tables + [vp, vp], True)
    assert sig["hn_state_checksum_host"] == (ctypes.c_int, [vp, lg, vp], False)    # a host function: no stream
    assert "hn_ckpt.hip" in built.SOURCES


def test_bad_arguments_are_rejected_before_any_hip_call(built):
    pack, verify, unpack, host = (built.lib().raw(n) for n in SYMBOLS)
    buf = (ctypes.c_long * 64)()                           # host memory standing in for every pointer: a rejected call touches none of it
    p = ctypes.addressof(buf)
    assert pack(None, p, 1, 1, p, p, None) == 1 and pack(p, None, 1, 1, p, p, None) == 1
    assert pack(p, p, 1, 1, None, p, None) == 1 and pack(p, p, 1, 1, p, None, None) == 1
    assert verify(None, p, 1, 1, p, p, p, p, None) == 1 and verify(p, None, 1, 1, p, p, p, p, None) == 1
    for hole in range(4):                                  # expect, ws, sums, verdict
        args = [p, p, p, p]
        args[hole] = None
        assert verify(p, p, 1, 1, *args, None) == 1, hole
    assert unpack(None, p, 1, p, None) == 1 and unpack(p, None, 1, p, None) == 1
    assert unpack(None, p, 1, None, None) == 1
    for blocks in (0, -1, -2 ** 40, 2 ** 31, 2 ** 40):
        assert pack(p, p, blocks, 1, p, p, None) == 1, blocks
        assert verify(p, p, blocks, 1, p, p, p, p, None) == 1, blocks
        assert unpack(p, p, blocks, p, None) == 1 and unpack(p, p, blocks, None, None) == 1, blocks
    for n_jobs in (0, -1, 2 ** 31, -2 ** 40):
        assert pack(p, p, 1, n_jobs, p, p, None) == 1, n_jobs
        assert verify(p, p, 1, n_jobs, p, p, p, p, None) == 1, n_jobs
    out = (ctypes.c_ulonglong * 2)(7, 7)
    o = ctypes.addressof(out)
    assert host(p, -1, o) == 1 and host(None, 1, o) == 1 and host(p, 1, None) == 1
    assert all(v == 0 for v in buf) and list(out) == [7, 7]
    assert host(None, 0, o) == 0 and list(out) == [0, 0]                           # no words: both sums 0


def lib_sums(C, words):
    return C.checksum_host(words)


def test_yardstick_wraps_as_python_integers_do():
    g = np.random.default_rng(1)
    for n in (0, 1, 5, 1025):
        w = g.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        assert ref.sums(w) == ref.sums_exact(w), n
    ones = np.full(131072, 0xFFFFFFFF, dtype=np.uint32)
    assert ref.sums(ones) == ref.sums_exact(ones)
    assert ref.slots([1, 4, 5, 0, 1023]) == ([0, 4, 8, 16, 16], 16 + 1024)


def test_host_checksum_equals_the_yardstick(C):
    g = np.random.default_rng(2)
    for n in (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 4099):
        w = g.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        keep = w.copy()
        assert lib_sums(C, w) == ref.sums(w), n
        assert np.array_equal(w, keep)
    ones = np.full(131072, 0xFFFFFFFF, dtype=np.uint32)
    s1, s2 = lib_sums(C, ones)
    assert (s1, s2) == ref.sums(ones)
    exact = 0xFFFFFFFF * (131072 * 131073 // 2)
    assert exact >= 2 ** 64 and s2 == exact % 2 ** 64 and s1 == 131072 * 0xFFFFFFFF   # s2 wrapped; below ~92 700 such words it cannot
    a = g.integers(0, 2 ** 32, size=257, dtype=np.uint64).astype(np.uint32)
    b = a.copy()
    i, j = 3, 200
    assert a[i] != a[j]
    b[i], b[j] = a[j], a[i]
    (a1, a2), (b1, b2) = lib_sums(C, a), lib_sums(C, b)
    assert a1 == b1 and a2 != b2                                                   # a swap of two unequal words: s1 cannot see it, s2 does


def cosine_values():
    p = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.Adam([p], 1e-4)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 7, eta_min=1e-8)
    for _ in range(3):
        opt.step()
        sch.step()
    return opt.param_groups[0]["lr"], sch.state_dict()


def cpu_state():
    g = torch.Generator().manual_seed(5)
    named = [("model/w", torch.randn(3, 5, 7, generator=g)), ("model/b", torch.randn(1, generator=g)),
             ("model/bn.num_batches_tracked", torch.tensor(2 ** 40 + 3, dtype=torch.int64)),
             ("optim/w/exp_avg", torch.randn(1025, generator=g)), ("guard/record", torch.arange(8, dtype=torch.int32) - 3),
             ("model/big", torch.randn(4099, generator=g))]
    named[0][1].view(torch.int32)[0, 0, :4] = torch.tensor([0x7FC12345, -0x7FFFFFFF - 1, 1, -1], dtype=torch.int32)   # NaN payload, -0, denormal, all ones
    lr, sched = cosine_values()
    host = dict(epoch=3, phase="lane", lr=lr, scheduler=sched, floats=[1e-8, 5e-324, 2.2250738585072014e-308, 0.1, 1.0 / 3.0, lr], settles=4)
    return named, host


@pytest.fixture()
def good_file(C, tmp_path):
    named, host = cpu_state()
    entries, blob = C.pack_host(named)
    path = str(tmp_path / "state.hn")
    C.write_file(path, entries, blob, host)
    assert not os.path.exists(path + ".tmp")
    return path, named, host


def test_file_round_trips(C, good_file, tool):
    path, named, host = good_file
    manifest, blob = C.read_file(path)
    data = open(path, "rb").read()
    rm, rb = ref.read(data)                                                        # the independent reader agrees on every byte
    assert rm == manifest and np.array_equal(rb, blob)
    assert ref.bad_tensors(rm, rb) == [] and C.verify_host(manifest, blob) == []
    got = C.tensors_from(manifest, blob)
    assert list(got) == [n for n, _ in named]
    for n, t in named:
        assert got[n].dtype == t.dtype and got[n].shape == t.shape, n
        assert got[n].numpy().tobytes() == t.numpy().tobytes(), n                  # bit for bit: the NaN payload, -0 and the int64 included
    offs, total = ref.slots([e["words"] for e in manifest["tensors"]])
    assert offs == [e["offset"] for e in manifest["tensors"]] and total == manifest["blob_words"] and all(o % 4 == 0 for o in offs)
    for e in manifest["tensors"]:
        assert (e["s1"], e["s2"]) == ref.sums(blob[e["offset"]:e["offset"] + e["words"]]), e["name"]
    assert (len(data) - 4 * total) % 4096 == 0 and len(data) - 4 * total == ref.sections(data)[3]
    assert tool.main(path) == 0
    # a second write of the same state gives the same bytes
    entries, blob2 = C.pack_host(named)
    C.write_file(path + "2", entries, blob2, host)
    assert open(path + "2", "rb").read() == data


def test_manifest_floats_round_trip_exactly(C, good_file):
    path, _, host = good_file
    back = C.read_file(path)[0]["host"]
    assert back == host
    for a, b in zip(back["floats"], host["floats"]):
        assert a == b and a.hex() == b.hex()
    assert back["lr"] == host["lr"] and back["lr"].hex() == host["lr"].hex()
    assert back["scheduler"]["_last_lr"][0].hex() == host["scheduler"]["_last_lr"][0].hex() and back["scheduler"]["eta_min"] == 1e-8
    assert 5e-324 in back["floats"] and 1e-8 in back["floats"]


def damaged(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def test_truncated_and_flipped_files_are_refused(C, good_file, tool, tmp_path):
    path, _, _ = good_file
    data = open(path, "rb").read()
    cuts = ref.sections(data)
    assert cuts[0] == 8 and cuts[1] == 36 and cuts[2] < cuts[3] and cuts[3] % 4096 == 0 and cuts[4] == len(data)
    bad = str(tmp_path / "bad.hn")
    for cut in [0] + cuts[:-1] + [len(data) - 1, len(data) - 4]:                    # at every section boundary (and inside the last section)
        damaged(bad, data[:cut])
        with pytest.raises(C.CheckpointError):
            C.read_file(bad)
        assert tool.main(bad) != 0, cut
    damaged(bad, data + b"\0\0\0\0")                                                # too long is as wrong as too short
    with pytest.raises(C.CheckpointError):
        C.read_file(bad)
    for where, at in (("magic", 3), ("version", 8), ("length", 12), ("manifest", 36 + 40), ("manifest end", cuts[2] - 1),
                      ("padding", cuts[2]), ("padding end", cuts[3] - 1)):
        flipped = bytearray(data)
        flipped[at] ^= 0x10
        damaged(bad, bytes(flipped))
        with pytest.raises(C.CheckpointError):
            C.read_file(bad)
        assert tool.main(bad) != 0, where
        with pytest.raises(ValueError):
            ref.read(bytes(flipped))
    with pytest.raises(C.CheckpointError):
        C.read_file(str(tmp_path / "absent.hn"))


def test_a_flipped_blob_byte_is_found_by_the_tool(C, good_file, tool, tmp_path, capsys):
    path, named, _ = good_file
    data = open(path, "rb").read()
    manifest, _ = C.read_file(path)
    start = ref.sections(data)[3]
    bad = str(tmp_path / "bad.hn")
    for e in manifest["tensors"]:
        flipped = bytearray(data)
        flipped[start + 4 * (e["offset"] + e["words"] - 1) + 2] ^= 0x01            # one bit of the tensor's last word
        damaged(bad, bytes(flipped))
        m, blob = C.read_file(bad)                                                  # structurally sound: reading succeeds
        assert C.verify_host(m, blob) == [e["name"]] == ref.bad_tensors(*ref.read(bytes(flipped)))
        capsys.readouterr()
        assert tool.main(bad) == 1
        assert "CORRUPT " + e["name"] in capsys.readouterr().out
    pads = [e for e in manifest["tensors"] if e["words"] % 4]
    flipped = bytearray(data)
    flipped[start + 4 * (pads[0]["offset"] + pads[0]["words"])] ^= 0x80            # a pad word behind a slot
    damaged(bad, bytes(flipped))
    assert C.verify_host(*C.read_file(bad)) == [pads[0]["name"]] and tool.main(bad) == 1


def test_the_tool_as_a_program(good_file, tmp_path):
    path, _, _ = good_file
    data = bytearray(open(path, "rb").read())
    data[-1] ^= 0x40
    bad = damaged(str(tmp_path / "bad.hn"), bytes(data))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")                                  # needs no GPU
    runs = [subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_state.py"), f], capture_output=True, text=True, env=env)
            for f in (path, bad)]
    assert runs[0].returncode == 0 and "every checksum verified" in runs[0].stdout, runs[0].stdout + runs[0].stderr
    assert runs[1].returncode == 1 and "CORRUPT model/big" in runs[1].stdout, runs[1].stdout + runs[1].stderr


def test_layout_rejects_what_the_format_cannot_carry(C):
    with pytest.raises(ValueError):
        C.layout([("a", torch.zeros(3, dtype=torch.float16))])
    with pytest.raises(ValueError):
        C.layout([("a", torch.zeros(4, 4).t())])
    with pytest.raises(ValueError):
        C.layout([("a", torch.zeros(1)), ("a", torch.zeros(1))])
    assert json.dumps(C.layout([("a", torch.zeros(2, 3)), ("b", torch.zeros((), dtype=torch.int64))])[0]) == json.dumps(
        [dict(name="a", dtype="float32", shape=[2, 3], offset=0, words=6), dict(name="b", dtype="int64", shape=[], offset=8, words=2)])
