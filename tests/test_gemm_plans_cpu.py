"""CPU guard of the exact GEMM matrix (tests/test_gemm_exact_gpu.py): the test-side plan restatement (tests/gemm_plans.py) equals the
library's own plan queries on every case of the GPU matrix and on a grid of production shapes, and the GPU cases together reach every
kernel instantiation / reduce kind the product library launches.  A heuristic change, or a tile added without an exact case, fails here
before any GPU run."""
import ctypes
import itertools
import re

import pytest

from tests import gemm_plans as P
from tests import test_gemm_exact_gpu as X


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib.lib()


def lib_plan(l, mode, n, h, w, m, nout, kp, taps, phase_span=0):
    s, r, wsb = ctypes.c_int(), ctypes.c_long(), ctypes.c_long()
    if phase_span:
        rc = l.query("hn_wgrad_plan_phase", n, h, w, nout, kp, phase_span, ctypes.addressof(s), ctypes.addressof(r), ctypes.addressof(wsb))
    else:
        rc = l.query("hn_wgrad_plan", mode, n, h, w, m, nout, kp, taps, ctypes.addressof(s), ctypes.addressof(r), ctypes.addressof(wsb))
    assert rc == 0
    return s.value, r.value, wsb.value


# ---- the GPU matrix's weight-gradient cases, as (mode, n, h, w, nout, kp, taps, phase_span) -> the plan they claim -----------------------
def gpu_wgrad_cases():
    out = []
    for name, mode, (n, h, w), c0, c1, nout, kern, splits in X.TN_ROW_CASES:
        out.append((name, (mode, n, h, w, nout, P.kp32(c0), 1, 0), kern, splits, None))
    for name, mode, (n, h, w), c0, c1, up, nout, kern, splits, red in X.PATCH_CASES:
        out.append((name, (mode, n, h, w, nout, P.kp32(c0 + c1), 9, 0), kern, splits, red))
    for name, (n, h, w), c in X.GCONV_CASES:
        out.append((name, (5, n, h, w, c, 64, 9, 0), "patch<64,64>", None, 2))
    for name, (n, h, w), c0, c1, k, kern in X.PHASE_CASES:
        out.append((name, (4, n, h, w, 4 * k, P.kp32(c0), 9, k), kern, None, None))
        if c1:                                            # the skip operand's full-resolution conv
            out.append((name + "/dw1", (2, n, 2 * h, 2 * w, k, P.kp32(c1), 9, 0), None, None, None))
    for name, mode, (n, h, w), c0, c1, up, nout, taps in X.RAND_CASES:
        out.append((name, (mode, n, h, w, nout, 64 if mode == 5 else P.kp32(c0 + c1), taps, 0), None, None, None))
    return out


def production_grid():
    """weight-gradient shapes of the training step and of its neighbours: N = 3 and 16, 512 x 1024 and 640 x 640 inputs, the strides and
    channel widths the model uses (1x1 row gather, stride-2 1x1, 3x3 reflect / replicate, grouped 3x3)"""
    widths = [24, 32, 40, 56, 64, 112, 152, 232, 376, 936]
    out = []
    for n, (hh, ww) in itertools.product((3, 16), ((512, 1024), (640, 640))):
        for s in (2, 4, 8, 16, 32, 64, 128):
            h, w = hh // s, ww // s
            for nout, cin in itertools.product(widths, widths):
                out.append((0, n, h, w, nout, P.kp32(cin), 1, 0))
                out.append((1, n, max(h // 2, 1), max(w // 2, 1), nout, P.kp32(cin), 1, 0))
            for nout in (5, 20, 24, 40, 64, 112, 128, 256):
                for cin in (24, 40, 64, 128):
                    out.append((2, n, h, w, nout, P.kp32(cin), 9, 0))
                    out.append((4, n, h, w, 4 * nout if nout in (64, 128) else nout, P.kp32(cin), 9, nout if nout in (64, 128) and cin >= 64 else 0))
            for c in (24, 56, 152, 376, 936):
                out.append((5, n, h, w, c, 64, 9, 0))
    return out


def test_wgrad_plan_restatement_matches_library(lib):
    cases = [c[1] for c in gpu_wgrad_cases()] + production_grid()
    assert len(cases) > 2000
    for mode, n, h, w, nout, kp, taps, span in cases:
        q = P.wgrad_plan(mode, n, h, w, n * h * w, nout, kp, taps, phase_span=span)
        assert (q["splits"], q["rows_per_split"], q["ws_bytes"]) == lib_plan(lib, mode, n, h, w, n * h * w, nout, kp, taps, span), \
            (mode, n, h, w, nout, kp, taps, span, q)


def test_gpu_wgrad_cases_land_where_they_claim():
    for name, (mode, n, h, w, nout, kp, taps, span), kern, splits, red in gpu_wgrad_cases():
        q = P.wgrad_plan(mode, n, h, w, n * h * w, nout, kp, taps, phase_span=span)
        assert kern is None or q["kernel"] == kern, (name, q)
        assert splits is None or q["splits"] == splits, (name, q)
        assert red is None or q["reduce"] == red, (name, q)
    for name, mode, grid, c0, c1, up, nout, taps, out_f32, act, stats, kern in X.NT_CASES:
        n, h, w = grid
        assert P.nt_kernel(mode, n * h * w, nout, P.kp32(c0 + c1), taps) == kern, name
    for name, mode, grid, c0, c1, up, nout, out_f32, act, ldc, kern in X.DIRECT_CASES:
        assert P.direct_kernel(mode, nout, P.kp32(c0 + c1), out_f32, ldc)[0] == kern, name


def _group_tables():
    tabs = []
    for tile in X.GROUP_TILES:
        jobs = X._group_jobs(*X.GROUP_TILES[tile])
        tabs.append((tile, [(mode, n, h, w, cin, nout, n * h * w) for (mode, n, h, w, cin, nout) in jobs]))
    # production-like groups: a stage-4 group (no split), a stage-2 group (splits + reduce), more tiles than the chip target
    tabs.append((None, [(1, 16, 16, 32, 376, 936, 16 * 16 * 32)] + [(0, 16, 16, 32, 936, 936, 16 * 16 * 32)] * 8))
    tabs.append((None, [(1, 16, 64, 128, 64, 152, 16 * 64 * 128)] + [(0, 16, 64, 128, 152, 152, 16 * 64 * 128)] * 3))
    tabs.append((None, [(0, 3, 128, 256, 24, 32, 3 * 128 * 256), (0, 3, 64, 128, 32, 56, 3 * 64 * 128)]))
    return tabs


def test_group_plans_match_library(lib):
    for tile, jobs in _group_tables():
        gp = P.group_plan(jobs)
        assert tile is None or gp["kernel"] == tile, (tile, gp)
        tab = (ctypes.c_long * (12 * len(jobs)))()
        for i, (mode, n, h, w, cin, nout, m) in enumerate(jobs):
            tab[12 * i:12 * i + 12] = [1, 1, 1, mode, n, h, w, cin, P.cdiv(cin, 8) * 8, P.cdiv(nout, 8) * 8, nout, m]
        assert lib.query("hn_wgrad_group_ws_bytes", ctypes.addressof(tab), len(jobs)) == gp["ws_bytes"], (tile, jobs, gp)
    for jobs in ([(2, 13, 21, 64), (1, 16, 40, 152), (2, 8, 16, 376), (1, 9, 17, 40)], [(16, 8, 16, 936)] * 6, [(16, 64, 128, 56)]):
        gp = P.gconv_group_plan(jobs)
        tab = (ctypes.c_long * (9 * len(jobs)))()
        for i, (n, h, w, c) in enumerate(jobs):
            tab[9 * i:9 * i + 9] = [1, 1, 1, n, h, w, c, c, c]
        assert lib.query("hn_gconv_wgrad_group_ws_bytes", ctypes.addressof(tab), len(jobs)) == gp["ws_bytes"], (jobs, gp)


def test_nt_stat_tiles_match_library(lib):
    for name, mode, (n, h, w), c0, c1, up, nout, taps, out_f32, act, stats, kern in X.NT_CASES:
        m = n * h * w
        assert lib.query("hn_nt_stat_tile", m, nout) == P.stat_tile(m, nout), name
        assert lib.query("hn_nt_stat_rows", m, nout) == P.cdiv(m, P.stat_tile(m, nout)), name


# ---- coverage guard -------------------------------------------------------------------------------------------------------------------
# written in the source but not launchable by the product library, with the reason
UNREACHABLE = {
    # hn_conv_gemm_tn_phase requires KP >= 64, and patch_tiles picks 32-channel tiles only for KP <= 32
    "patch<128,32,1>": "KP >= 64",
}


def test_every_product_wgrad_instantiation_has_an_exact_case():
    launched = P.product_instantiations()
    assert {"tn<128,128>", "tng_regs<128,128>", "patch<64,64>", "reduce-1", "reduce0", "reduce1", "reduce2"} <= launched   # parser sanity
    assert len([k for k in launched if k.startswith("tn<")]) == 11 and len([k for k in launched if k.startswith("tng")]) == 11
    src = P.product_source()
    phase_entry = src[src.index('extern "C" int hn_conv_gemm_tn_phase('):]
    assert "KP >= 64" in phase_entry[:phase_entry.index("\n}\n")], "hn_conv_gemm_tn_phase no longer requires KP >= 64: patch<128,32,1> is reachable"
    assert all(P.patch_tiles(nout, kp)[1] == 64 for nout in range(8, 1024, 8) for kp in range(64, 1024, 32))
    covered = set()
    for name, (mode, n, h, w, nout, kp, taps, span), kern, splits, red in gpu_wgrad_cases():
        q = P.wgrad_plan(mode, n, h, w, n * h * w, nout, kp, taps, phase_span=span)
        covered.add(q["kernel"])
        covered.add("reduce%d" % q["reduce"])
    for tile in X.GROUP_TILES:
        covered.add(P.group_plan([(mode, n, h, w, cin, nout, n * h * w) for (mode, n, h, w, cin, nout) in X._group_jobs(*X.GROUP_TILES[tile])])["kernel"])
    missing = launched - covered - set(UNREACHABLE)
    assert not missing, f"product instantiations without an exact GPU case: {sorted(missing)}"
    assert not (set(UNREACHABLE) & covered)


# hand-kept mirror of run_gemm_nt / launch_direct: the forms the product library launches for plain NT calls
NT_FORMS = {"nt<16,128>", "nt<32,128>", "nt<64,128>", "nt<128,128>", "nt<64,64>", "nt<64,64,kg2>"}
DIRECT_FORMS = {"direct<16,f32,wpre>", "direct<16,bf16,wpre>", "direct<32,f32>", "direct<32,bf16>", "direct<64,f32>", "direct<64,bf16>",
                "direct<128,f32>", "direct<128,bf16>", "direct_narrow<64>"}


def test_nt_and_direct_forms_have_exact_cases():
    src = P.product_source()
    run = src[src.index("static int run_gemm_nt("):]
    run = run[:run.index("\n}\n")]
    tiles = set(re.findall(r"return launch_nt<(\d+), (\d+), \d+, \d+>\(p, out_f32, st\)", run))
    assert tiles == {("16", "128"), ("32", "128"), ("64", "128"), ("128", "128"), ("64", "64")}, "run_gemm_nt changed: update NT_FORMS"
    assert "launch_nt_r<64, 64, 2, 2, 2, 2>" in run
    direct = src[src.index("static int launch_direct("):]
    direct = direct[:direct.index("\n}\n")]
    assert re.findall(r"DIRECT_CASE\((\d+)\)", direct) == ["16", "32", "64", "128"], "launch_direct changed: update DIRECT_FORMS"
    assert "conv3x3_direct_kernel<64, false, true, 1>" in direct
    nt = {c[-1] for c in X.NT_CASES}
    assert NT_FORMS <= nt, sorted(NT_FORMS - nt)
    dr = {c[-1] for c in X.DIRECT_CASES}
    assert DIRECT_FORMS <= dr, sorted(DIRECT_FORMS - dr)
    assert {c[1] for c in X.DIRECT_CASES} >= {2, 3, 4}
    # pick_bc's least-padding choice is exercised both ways, and every statistics tile height
    assert P.pick_bc(152) == 64 and P.pick_bc(256) == 128
    assert {P.stat_tile(c[2][0] * c[2][1] * c[2][2], c[6]) for c in X.NT_CASES if c[10]} == {64, 128}
