"""hn_grad_tail kinds 0 and 1 (and the job table's edges, with kind 2 mixed in) through the C entry point on a HOST table built here from
the header ({kind, a, b, out, out2, n0, n1, n2 | float bits of f0} per job), never through ops.GradQueue.

Kind 0 (column sums of partial rows): integers in [-7, 7], so every sum is exact (2049 * 7 < 2^24) whatever the order, and the result is
compared with == against float64.  The launcher picks a column width cw in {32, 16, 8, 4} from the row count (more row lanes for tall
folds); cw_of() restates that ladder and the cases are asserted to reach every rung, with row counts at and one past each threshold.
Kind 1 (BiFPN fusion-weight Jacobian): against stencil_ref.fuse_dweights with the bound test_stencil_exact_gpu.py::test_fuse_dweights
derives -- fp32 running sums of the columns, then a handful of fp32 operations -- and exact 0 where the raw parameter is <= 0.
Kind 2 (SE outer products, exact in tests/test_se_exact_gpu.py) only fills the mixed table here, on integers, exactly."""
import struct

import pytest
import torch

from tests import stencil_ref as R
from tests.exact_checks import D, exact, gen, release, within
from tests.guards import Guarded

pytestmark = pytest.mark.gpu

F32, F64, I64 = torch.float32, torch.float64, torch.int64
U = 2.0 ** -24
EPS = 1e-4
TAIL_MAX = 64                                            # HN_TAIL_MAX


@pytest.fixture(scope="module")
def built():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    return lib()


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


def cw_of(rows):
    """the launcher's column width for a kind 0 job, restated: halve from 32 while the rows exceed 16 per row lane"""
    cw = 32
    while cw > 4 and rows > 16 * (256 // cw):
        cw //= 2
    return cw


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# ---- one job of each kind: (table row, check(), outputs) ---------------------------------------------------------------------------------------------
def fold_job(rows, cols, name):
    a = torch.randint(-7, 8, (rows, cols), generator=gen(name)).to(F32)
    ad, out = D(a), Guarded(1, cols)
    want = a.double().sum(0, keepdim=True)
    assert float(a.abs().double().sum(0).max()) < (1 << 24)

    def check():
        nm = f"hn_grad_tail kind 0 ({rows} rows x {cols} columns, cw {cw_of(rows)}; {name})"
        exact(out.view, want, nm, "row")
        out.check(nm)
    return [0, ad.data_ptr(), 0, out.ptr(), 0, rows, cols, 0], check, [out]


def fuse_job(blocks, praw, name):
    nw = len(praw)
    pw = torch.rand((blocks, 3), generator=gen(name), dtype=F32) * 2 - 1
    pd, rd, out = D(pw), D(torch.tensor(praw + [7.0] * (3 - nw), dtype=F32)), Guarded(1, nw)
    eps32 = float(torch.tensor(EPS, dtype=F32))
    want = R.fuse_dweights(pw.double().sum(0), torch.tensor(praw, dtype=F64), nw, eps32)
    mag = float(pw.double().abs().sum(0).max())
    s = float(sum(max(p, 0.0) for p in praw)) + EPS
    bound = (blocks // 256 + 2 + 8 + 8) * U * mag * 2 / s               # test_fuse_dweights' bound

    def check():
        nm = f"hn_grad_tail kind 1 ({blocks} blocks, raw {praw}; {name})"
        got = out.view.detach().double().cpu().reshape(nw)
        within(got, want, bound, nm, "weight")
        for i in range(nw):
            if praw[i] <= 0:
                assert float(got[i]) == 0.0, f"{nm}: d(raw[{i}]) = {float(got[i])!r} for a clamped parameter"
        out.check(nm)
    return [1, pd.data_ptr(), rd.data_ptr(), out.ptr(), 0, blocks, nw, f32_bits(EPS)], check, [out]


def outer_job(n, pi, qj, name):
    g = gen(name)
    a, b = torch.randint(-3, 4, (n, pi), generator=g).to(F32), torch.randint(-3, 4, (n, qj), generator=g).to(F32)
    ad, bd, out, out2 = D(a), D(b), Guarded(pi, qj), Guarded(1, pi)

    def check():
        nm = f"hn_grad_tail kind 2 (N {n}, {pi} x {qj}; {name})"
        exact(out.view, a.double().t() @ b.double(), nm + " out", "row")
        exact(out2.view, a.double().sum(0, keepdim=True), nm + " out2", "row")
        out.check(nm + " out")
        out2.check(nm + " out2")
    return [2, ad.data_ptr(), bd.data_ptr(), out.ptr(), out2.ptr(), pi, qj, n], check, [out, out2]


def launch(built, jobs):
    tab = torch.tensor([row for row, _, _ in jobs], dtype=I64)          # HOST table
    built.call("hn_grad_tail", tab.data_ptr(), len(jobs))
    torch.cuda.synchronize()
    for _, check, _ in jobs:
        check()


# ---- kind 0 ---------------------------------------------------------------------------------------------------------------------------------
ROWS = (1, 7, 8, 128, 129, 256, 257, 512, 513, 2049)
COLS = (1, 5, 33, 72)


def test_kind0_ladder_is_reached():
    assert [cw_of(r) for r in ROWS] == [32, 32, 32, 32, 16, 16, 8, 8, 4, 4]
    assert {cw_of(r) for r in ROWS} == {32, 16, 8, 4}


def test_kind0_column_sums(built):
    jobs = [fold_job(r, c, f"fold{r}x{c}") for r in ROWS for c in COLS]
    assert len(jobs) <= TAIL_MAX
    launch(built, jobs)


# ---- kind 1 ---------------------------------------------------------------------------------------------------------------------------------
RAW = ([1.5], [-1.0], [0.0], [0.5, 1.5], [2.0, -1.0], [0.0, 1.0], [2.0, 1.0, 1.0], [2.0, -1.0, 2.0], [0.5, 0.0, 1.5])
BLOCKS = (1, 255, 256, 257, 1024)


def test_kind1_fusion_weight_jacobian(built):
    jobs = [fuse_job(b, list(raw), f"fuse{b}-{i}") for b in BLOCKS for i, raw in enumerate(RAW)]
    assert len(jobs) <= TAIL_MAX and {len(r) for r in RAW} == {1, 2, 3}
    launch(built, jobs)


# ---- table edges ----------------------------------------------------------------------------------------------------------------------------
def mixed(n):
    jobs = []
    for j in range(n):
        if j % 3 == 0:
            jobs.append(fold_job(ROWS[(j // 3) % len(ROWS)], COLS[(j // 3) % len(COLS)], f"mixed-fold{j}"))
        elif j % 3 == 1:
            jobs.append(fuse_job(BLOCKS[(j // 3) % len(BLOCKS)], list(RAW[(j // 3) % len(RAW)]), f"mixed-fuse{j}"))
        else:
            jobs.append(outer_job((3, 16, 21)[(j // 3) % 3], (1, 17, 40)[(j // 3) % 3], (33, 16, 5)[(j // 6) % 3], f"mixed-outer{j}"))
    return jobs


def test_full_table_of_mixed_kinds(built):
    """64 jobs, the table's capacity: every first_block boundary between two kinds is crossed"""
    launch(built, mixed(TAIL_MAX))


def test_oversized_table_is_refused(built):
    jobs = mixed(TAIL_MAX + 1)
    tab = torch.tensor([row for row, _, _ in jobs], dtype=I64)
    f = built.raw("hn_grad_tail")
    st = torch.cuda.current_stream().cuda_stream
    assert f(tab.data_ptr(), TAIL_MAX + 1, st) == 1, "65 jobs accepted"
    assert f(tab.data_ptr(), 0, st) == 1, "0 jobs accepted"
    torch.cuda.synchronize()
    for j, (_, _, outs) in enumerate(jobs):                               # nothing was written: every output still holds the NaN sentinel
        for o in outs:
            assert bool(torch.isnan(o.view).all()), f"a refused hn_grad_tail call wrote job {j}'s output"
            o.check(f"hn_grad_tail (refused calls), job {j}")
