"""CPU: the Lovasz-softmax seg loss (segment.use_lovasz) without launching a kernel -- the fp64 restatement against the reference's own
recorded values, the module's switch, the C ABI's symbols, planning helper and argument checks, the dispatcher ops' schemas and fake kernels."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests.helpers import ROOT, load_cfg, load_npz
from tests.lovasz_ref import lovasz_softmax_ref

CASES = ["ignore_absent", "single_class", "out_of_range", "float_target", "plain_c3"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_fixture(case):
    z = load_npz("lovasz_kats.npz")
    x = torch.from_numpy(z[f"{case}/logits"]).to(torch.float64).requires_grad_(True)
    t = torch.from_numpy(z[f"{case}/target"])
    loss = lovasz_softmax_ref(x, t)
    loss.backward()
    want, gwant = float(z[f"{case}/loss"]), torch.from_numpy(z[f"{case}/grad"])
    assert abs(float(loss.detach()) - want) <= 1e-6 * abs(want), (float(loss.detach()), want)
    assert float((x.grad - gwant).abs().max()) <= 1e-4 * float(gwant.abs().max()), case


def test_restatement_edge_cases():
    x = torch.randn(1, 4, 3, 5, dtype=torch.float64, requires_grad=True)
    loss = lovasz_softmax_ref(x, torch.full((1, 3, 5), 255))            # every pixel ignored: 0 with a zero gradient
    loss.backward()
    assert float(loss) == 0.0 and float(x.grad.abs().max()) == 0.0
    x.grad = None
    loss = lovasz_softmax_ref(x, torch.full((1, 3, 5), 9))              # no class present: 0 with a zero gradient
    loss.backward()
    assert float(loss) == 0.0 and float(x.grad.abs().max()) == 0.0


def _cfg(lovasz):
    c = load_cfg("hydranet_tiny.yml")
    c["segment"]["use_lovasz"] = lovasz
    return c


def test_module_constructs_with_lovasz_and_dispatches_to_it(built, monkeypatch):
    from multitask_hydranet_amd import HydraNet
    from multitask_hydranet_amd import model as M
    on, off = HydraNet(_cfg(True)), HydraNet(_cfg(False))
    assert on.use_lovasz and not off.use_lovasz
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    calls = []
    monkeypatch.setattr(M.K, "seg_lovasz_loss_hip", lambda seg, tgt, ignore_index=255, slot=None: calls.append((seg, ignore_index, slot)) or 7.0)
    monkeypatch.setattr(M.K, "seg_loss_hip", lambda *a, **k: pytest.fail("the CE path ran with use_lovasz on"))
    monkeypatch.setattr(M.K, "seg_focal_loss_hip", lambda *a, **k: pytest.fail("the focal path ran with use_lovasz on"))
    seg = torch.zeros(1, 5, 4, 4)
    assert on.loss_seg(seg, torch.zeros(1, 4, 4)) == 7.0
    assert len(calls) == 1 and calls[0][0] is seg and calls[0][1] == 255 and calls[0][2] is None


def test_header_declares_and_library_exports_lovasz(built):
    names = ("hn_seg_lovasz_ws_bytes", "hn_seg_lovasz_fwd", "hn_seg_lovasz_bwd", "hn_seg_lovasz_bwd_s2d")
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    for n in names:
        assert n in sig and hasattr(dll, n), n
    assert re.search(r"long\s+hn_seg_lovasz_ws_bytes\s*\(\s*int N,\s*long HW,\s*int C\s*\)", open(built.HEADER).read())


def test_workspace_size_without_a_gpu(built):
    l = built.lib()
    for n, hw, c in ((2, 64 * 96, 5), (16, 512 * 1024, 5), (1, 7, 2), (3, 63 * 95, 16)):
        b = l.query("hn_seg_lovasz_ws_bytes", n, hw, c)
        assert b >= 16 * c * n * hw + 4 * c * 1024, (n, hw, c, b)        # four [C][P] u32 arrays + the digit totals at least
    assert l.query("hn_seg_lovasz_ws_bytes", 2, 64, 1) == 0 and l.query("hn_seg_lovasz_ws_bytes", 2, 64, 17) == 0


def test_bad_arguments_are_rejected_without_a_gpu(built):
    l = built.lib()
    fwd, bwd, s2d = l.raw("hn_seg_lovasz_fwd"), l.raw("hn_seg_lovasz_bwd"), l.raw("hn_seg_lovasz_bwd_s2d")
    p = 256                       # a non-null address that is never dereferenced: the checks return before any launch
    assert fwd(None, 5, 5, p, 0, 255, 2, 64, p, p, None) == 1
    assert fwd(p, 5, 5, p, 0, 255, 2, 64, None, p, None) == 1
    for c in (1, 17):
        assert fwd(p, c, c, p, 0, 255, 2, 64, p, p, None) == 1
        assert bwd(p, c, c, p, 0, 255, 2, 64, p, p, p, c, None) == 1
        assert s2d(p, c, c, p, 0, 255, 2, 8, 8, p, p, p, 72, None) == 1
    assert bwd(p, 5, 5, p, 0, 255, 2, 64, p, None, p, 5, None) == 1
    assert s2d(p, 5, 5, p, 0, 255, 2, 8, 8, p, p, None, 24, None) == 1
    assert s2d(p, 5, 5, p, 0, 255, 2, 7, 8, p, p, p, 24, None) == 1          # odd H
    assert s2d(p, 5, 5, p, 0, 255, 2, 8, 8, p, p, p, 16, None) == 1          # ldz < 4 C


def test_dispatcher_ops_are_registered_with_fake_kernels(built):
    import multitask_hydranet_amd.torch_ops  # noqa: F401
    ns = torch.ops.hydranet_hip
    assert hasattr(ns, "seg_lovasz_fwd") and hasattr(ns, "seg_lovasz_bwd")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 6, 8, 5, device="cuda")
        t = torch.empty(2, 6, 8, device="cuda")
        loss, ws = ns.seg_lovasz_fwd(x, t, 255)
        assert loss.shape == () and loss.dtype == torch.float32 and ws.dtype == torch.uint8
        dl = ns.seg_lovasz_bwd(torch.empty((), device="cuda"), x, t, ws, 255)
        assert dl.shape == x.shape and dl.dtype == torch.float32
