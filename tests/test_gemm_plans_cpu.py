"""CPU guard of the exact GEMM matrix (tests/test_gemm_exact_gpu.py): the test-side plan restatement (tests/gemm_plans.py) equals the
library's own plan queries on every case of the GPU matrix and on a grid of production shapes, and the GPU cases together reach every
kernel instantiation / reduce kind the product library launches.  A heuristic change, or a tile added without an exact case, fails here
before any GPU run.  The same for the launch forms of tests/test_gemm_forms_exact_gpu.py and tests/test_gemm_epilogue_exact_gpu.py: every
case lands on the form it claims, and every persistent kernel, fold value, phase mode, statistics mode and GemmNT option keeps a GPU case."""
import ctypes
import itertools
import re

import pytest

from tests import gemm_plans as P
from tests import test_gemm_epilogue_exact_gpu as XE
from tests import test_gemm_exact_gpu as X
from tests import test_gemm_forms_exact_gpu as XF


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
    # ---- the launch forms beyond the plain calls (tests/test_gemm_forms_exact_gpu.py, tests/test_gemm_epilogue_exact_gpu.py) ----
    assert sorted(set(re.findall(r"hipLaunchKernelGGL\((seg_\w+(?:<\w+>)?),", direct))) == \
        ["seg_out_conv_kernel<false>", "seg_out_conv_kernel<true>", "seg_phase64_conv_kernel"], "launch_direct changed: update PERSISTENT_FORMS"
    assert direct.count("npatch >= 1024") == 2 and P.PERSIST_MIN_PATCHES == 1024, "the persistent threshold changed: update PERSISTENT_FORMS"
    assert "q.ppw = cdiv(npatch, 64);" in direct and "q.ppw = cdiv(npatch, 256);" in direct, "patch ranges changed: update persistent_ranges"
    covered = gpu_form_coverage()
    missing = (PERSISTENT_FORMS | FOLD_FORMS | PHASE_FORMS | EMODE_FORMS | OPTION_FORMS) - covered
    assert not missing, f"launch forms without an exact GPU case: {sorted(missing)}"
    # every GemmNT option the guard names still exists in the launch description
    desc = src[src.index("struct GemmNT {"):src.index("struct StatCoef")]
    for field in ("add_pre", "add_s2", "lcoef", "lo_n", "w_rpi", "rpi", "fold", "phase_mode", "emode", "d2s", "amax"):
        assert re.search(r"\b%s\b" % field, desc), f"GemmNT::{field} is gone: update OPTION_FORMS"


# hand-kept mirror of the launch forms beyond the plain calls
PERSISTENT_FORMS = {"seg_phase64", "seg_out<false>", "seg_out<true>"}
FOLD_FORMS = {"fold=1", "fold=2", "fold=3"}
PHASE_FORMS = {"phase_mode=1", "phase_mode=2"}
EMODE_FORMS = {"emode=1", "emode=2", "emode=3"}
OPTION_FORMS = {"add_pre", "add_s2", "lcoef", "lo_n", "w_rpi", "rpi"}


def gpu_form_coverage():
    """the forms / options the cases of the two form files reach, from their case tables"""
    cov = set()
    for case in XF.PHASE_FWD_CASES:
        for f in XF.phase_fwd_form(case):
            cov.add(f["kernel"])
            cov.add("phase_mode=1")
        if case[4]:
            cov.add("add_pre/phase")
    for name, k, (n, h, w), kern, kern_amax in XF.SEG_OUT_CASES:
        cov.add(P.seg_out_form(n, h, w, k)["kernel"])
        if kern_amax is not None:
            cov.add(P.seg_out_form(n, h, w, k, amax=True)["kernel"])
    for name, k, c0, (n, h, w), kern in XF.PHASE_DGRAD_CASES:
        cov.add("phase_mode=2")
    for case in XF.FOLD_CASES:
        cov.add("fold=%d" % case[1])
        if case[2]:
            cov.add("phase_mode=2/fold")
    if XE.IMGW_CASES:
        cov.update({"w_rpi", "add_pre"})
    if XE.LVL_CASES:
        cov.add("lcoef")
    if XE.LVLOUT_CASES:
        cov.add("lo_n")
    if XE.RPI_CASES:
        cov.add("rpi")
    for case in XE.ADD_CASES:
        cov.add({"pre": "add_pre", "s2": "add_s2", "post": "add_post"}[case[1]])
    if XE.STAT_CASES:
        cov.update({"emode=1", "emode=2"})
    if XE.STAT3_CASES:
        cov.add("emode=3")
    return cov


def test_gpu_form_cases_land_where_they_claim():
    for case in XF.PHASE_FWD_CASES:
        assert all(f["kernel"] == case[6] for f in XF.phase_fwd_form(case)), case[0]
    k, c0, (n, h, w) = XF.PHASE_FWD_BELOW
    assert P.npatch(n, h, w) == 1023 and P.phase_fwd_form(n, h, w, k, c0, P.ACT_ELU, ldc=72)["kernel"] == "direct<64,bf16,wpre,phase>"
    assert P.npatch(171, 17, 33) == 1026 and P.npatch(64, 64, 64) == 1024
    for name, k, (n, h, w), kern, kern_amax in XF.SEG_OUT_CASES:
        assert P.seg_out_form(n, h, w, k)["kernel"] == kern, name
        if kern_amax is not None:
            assert P.seg_out_form(n, h, w, k, amax=True)["kernel"] == kern_amax, name
        else:
            assert (2 * w * k) % 4 != 0, name                    # hn_conv3x3_out_argmax refuses the shape
    # both kernels, logits and arg-max, at every class count of the issue
    for k in (5, 3, 8):
        kerns = {(P.seg_out_form(n, h, w, kk)["persistent"], am is not None) for _, kk, (n, h, w), _, am in XF.SEG_OUT_CASES if kk == k}
        assert kerns >= {(False, True), (True, True)}, k
    for name, k, c0, (n, h, w), kern in XF.PHASE_DGRAD_CASES:
        assert P.phase_dgrad_form(n, h, w, k, c0, ldc=c0 + 8)["kernel"] == kern, name
    seen = set()
    for case in XF.FOLD_CASES:
        name, form, phase_k, clamp, with_y, grid, cz, nout = case
        status, f = XF.fold_case_form(case)
        assert status == 0 and f["bc"] in (64, 128), name
        assert f["kernel"] == "direct_narrow<64>" or ("fold%d" % form in f["kernel"] and ("dphase" in f["kernel"]) == bool(phase_k)), (name, f)
        seen.add((form, phase_k, clamp, with_y))
        seen.add(("shape", form == 1, grid))
        seen.add(("nout", nout))
        seen.add(("kernel", f["kernel"].split(",fold")[0]))
    assert len(set(c[0] for c in XF.FOLD_CASES)) == len(XF.FOLD_CASES)
    for form in (1, 2, 3):
        for phase_k, clamp in ((0, 0), (0, 1), (64, 1), (128, 1)):
            for with_y in (True, False):
                assert (form, phase_k, clamp, with_y) in seen
    assert all(("shape", True, s) in seen for s in XF.PLAIN_SHAPES) and all(("shape", False, s) in seen for s in XF.S2D_SHAPES)
    assert all(("nout", v) in seen for v in XF.NOUTS)
    assert {("kernel", "direct_narrow<64>"), ("kernel", "direct<64,bf16"), ("kernel", "direct<128,bf16"), ("kernel", "direct<64,bf16,dphase"),
            ("kernel", "direct<128,bf16,dphase")} <= seen
    for name, form, (n, h, w), nout, status in XF.FOLD_REFUSALS:
        assert P.fold_form(n, h, w, 64, nout, 0, plain=form != 2, s2d=form != 1)[0] == status, name
    assert {c[3] for c in XF.FOLD_REFUSALS} >= {32, 44} and {c[4] for c in XF.FOLD_REFUSALS} == {1, 3}
    # the gemm_nt_kernel options: both tilings per entry point (stat3: the 64 x 64 tiling only)
    for name, rpi, c, cout, kern in XE.IMGW_CASES:
        assert P.nt_entry_kernel("imgw", 3 * rpi, cout, P.kp32(c)) == kern, name
    for name, rows, nout, kern in XE.LVL_CASES:
        assert P.nt_entry_kernel("lvl", sum(rows), nout, 64) == kern, name
    for case in XE.LVLOUT_CASES:
        assert XE.lvlout_kernel(case, 36) == "nt<64,128>" and XE.lvlout_kernel(case, 81) == "nt<64,64>", case[0]
    for name, mode, (h, w), nout, out_f32, kern in XE.RPI_CASES:
        assert P.nt_kernel(mode, 3 * h * w, nout, 32, 9 if mode == 2 else 1) == kern, name
    for name, kind, (n, h, w), nout, kern in XE.ADD_CASES:
        assert P.nt_kernel(0, n * h * w, nout, 64, 1) == kern, name
    for name, mode, (n, h, w), c, nout, kind, kern in XE.STAT_CASES:
        got = P.direct_kernel(5, nout, 64, False, nout + 8)[0] if mode == 5 else P.nt_kernel(mode, n * h * w, nout, P.kp32(c), 1)
        assert got == kern, name
    for name, m, c, nout in XE.STAT3_CASES:
        assert P.nt_entry_kernel("stat3", m, nout, P.kp32(c)) == "nt<64,64>", name
    assert P.nt_entry_kernel("stat3", 256, 56, 64) is None
    for cases in (XE.IMGW_CASES, XE.LVL_CASES, XE.RPI_CASES, XE.ADD_CASES):
        assert {"nt<64,128>"} <= {c[-1] for c in cases} and any(c[-1].startswith("nt<64,64") for c in cases)
    assert {c[1] for c in XE.ADD_CASES} == {"post", "pre", "s2"} and {c[1] for c in XE.STAT_CASES} == {0, 1, 5}
    assert {c[5] for c in XE.STAT_CASES} == {None, "post", "s2"}


def test_each_form_needs_its_gpu_case(monkeypatch):
    """removing the GPU cases of a guarded form makes the coverage guard fail"""
    full = gpu_form_coverage()
    for table, mod, keep, lost in [
        ("PHASE_FWD_CASES", XF, lambda c: c[6] != "seg_phase64", {"seg_phase64"}),
        ("SEG_OUT_CASES", XF, lambda c: c[3] != "seg_out<false>", {"seg_out<false>", "seg_out<true>"}),
        ("PHASE_FWD_CASES", XF, lambda c: False, {"phase_mode=1", "seg_phase64"}),
        ("PHASE_DGRAD_CASES", XF, lambda c: False, {"phase_mode=2"}),
        ("FOLD_CASES", XF, lambda c: c[1] != 1, {"fold=1"}), ("FOLD_CASES", XF, lambda c: c[1] != 2, {"fold=2"}),
        ("FOLD_CASES", XF, lambda c: c[1] != 3, {"fold=3"}),
        ("STAT_CASES", XE, lambda c: False, {"emode=1", "emode=2"}), ("STAT3_CASES", XE, lambda c: False, {"emode=3"}),
        ("ADD_CASES", XE, lambda c: c[1] != "s2", {"add_s2"}), ("LVL_CASES", XE, lambda c: False, {"lcoef"}),
        ("LVLOUT_CASES", XE, lambda c: False, {"lo_n"}), ("IMGW_CASES", XE, lambda c: False, {"w_rpi"}), ("RPI_CASES", XE, lambda c: False, {"rpi"}),
    ]:
        monkeypatch.setattr(mod, table, [c for c in getattr(mod, table) if keep(c)])
        guarded = PERSISTENT_FORMS | FOLD_FORMS | PHASE_FORMS | EMODE_FORMS | OPTION_FORMS
        assert (full - gpu_form_coverage()) & guarded == lost, (table, full - gpu_form_coverage())
        with pytest.raises(AssertionError, match="launch forms without an exact GPU case"):
            test_nt_and_direct_forms_have_exact_cases()
        monkeypatch.undo()
    # add_pre is reached by the imgw entry point and by the pre-activation addend of hn_conv_gemm_nt_ex: both must go for it to be lost
    monkeypatch.setattr(XE, "IMGW_CASES", [])
    monkeypatch.setattr(XE, "ADD_CASES", [c for c in XE.ADD_CASES if c[1] != "pre"])
    assert "add_pre" not in gpu_form_coverage()
