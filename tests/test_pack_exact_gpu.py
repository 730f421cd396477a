"""The weight packs held to the references of tests/pack_ref.py, bit for bit and padding included, through the C entry points on tables
and buffers built here from the header's description (never through ops.PackPlan): hn_pack_weight, hn_pack_weight_ex,
hn_pack_weights_batched, hn_pack_small_batched, hn_gconv_pack_diag, hn_pack_levels.

Two inputs per shape.  Position-coded integers ((31 co + 7 ci + 3 tap) mod 251) - 125 are bf16-exact and differ from their neighbours
along every axis, so a transposed or shifted index shows.  Random normals with pack_ref.rounding_set() planted need rounding on every
element and carry every tie / carry case of fp32 -> bf16, so a truncating or half-up conversion shows.  Phase packs use dyadic weights
k / 16, |k| <= 2047: a sum of up to four taps is below 2^13 in steps of 2^-4 (17 bits) -- exact in fp32 in any order -- while its bf16
rounding (8 bits) is not trivial.

Every output is a GuardedBytes payload that starts as the 0xA5 sentinel: an element the kernel did not write is a mismatch (no
reference value has the pattern 0xA5A5), and a write outside the payload fails check()."""
import ctypes

import pytest
import torch

from tests import pack_ref as P
from tests import stencil_ref as R
from tests.exact_checks import D, gen, release, same_bits
from tests.guards import GuardedBytes, dev

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
I16, I32, I64 = torch.int16, torch.int32, torch.int64
SENT16 = -0x5A5B                                       # 0xA5A5 as int16: GuardedBytes' sentinel seen through a bf16 view


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


def stream():
    return torch.cuda.current_stream().cuda_stream


def wbuf(w, off=0):
    """fp32 values on the GPU, `off` elements (4 bytes each) past a 16-byte boundary"""
    base = D(torch.zeros(w.numel() + 4, dtype=F32))
    v = base[off:off + w.numel()]
    v.copy_(w.reshape(-1))
    assert v.data_ptr() % 16 == 4 * off
    return v


def out16(n, fill=None):
    return GuardedBytes(2 * n, fill=fill)


def held(out, want, name, what):
    """a bf16 output (GuardedBytes) against the reference's unrounded operand"""
    same_bits(out.as_(I16, *want.shape), P.bits(want), name, what)
    out.check(name)


def inputs(cout, cin, taps, name):
    return [("coded", P.coded(cout, cin, taps)), ("random", P.randw((cout, cin, taps), gen(name)))]


def dyadic(shape, g):
    return torch.randint(-2047, 2048, tuple(shape), generator=g).to(F32) / 16


# =====================================================================================================================================
# hn_pack_weight
# =====================================================================================================================================
DENSE = [(1, 1, 1), (5, 3, 9), (33, 31, 1), (32, 32, 9), (65, 40, 1), (24, 30, 1), (7, 13, 9), (152, 64, 1)]


@pytest.mark.parametrize("cout,cin,taps", DENSE)
def test_pack_weight(built, cout, cin, taps):
    for kind, w in inputs(cout, cin, taps, f"pw{cout}x{cin}x{taps}"):
        wp_ref, wt_ref = P.dense(w)
        for with_wt in (True, False):                                      # wt = NULL: the inference fold's call
            name = f"hn_pack_weight ({cout}, {cin}, {taps}) {kind}{'' if with_wt else ', wt = NULL'}"
            wd, wp, wt = wbuf(w), out16(wp_ref.numel()), out16(wt_ref.numel())
            built.call("hn_pack_weight", wd.data_ptr(), wp.ptr(), wt.ptr() if with_wt else None, cout, cin, taps)
            held(wp, wp_ref, name + " wp", "(cout, tap, k)")
            if with_wt:
                held(wt, wt_ref, name + " wt", "(cin, tap, k)")
            else:
                assert wt.untouched(), name + ": wt written"
                wt.check(name + " wt")


# =====================================================================================================================================
# hn_pack_weight_ex: channel slices and the phase form
# =====================================================================================================================================
SLICES = [
    # cout, cin_total, ci0, cin, taps
    (5, 20, 3, 13, 9),                                 # ci0 > 0, Cin no multiple of 8, ends inside the tensor
    (33, 40, 8, 32, 1),                                # ci0 + Cin == Cin_total
    (7, 19, 14, 5, 9),                                 # both: an odd tail slice
    (64, 12, 0, 12, 1),                                # the whole tensor as a slice
]


@pytest.mark.parametrize("cout,ctot,ci0,cin,taps", SLICES)
def test_pack_weight_ex_slice(built, cout, ctot, ci0, cin, taps):
    for kind, w in inputs(cout, ctot, taps, f"slice{cout}x{ctot}x{taps}"):
        wp_ref, wt_ref = P.slice_(w, ci0, cin)
        for with_wt in (True, False):
            name = f"hn_pack_weight_ex slice ({cout}, {ctot}, ci0 {ci0}, cin {cin}, taps {taps}) {kind}{'' if with_wt else ', wt = NULL'}"
            wd, wp, wt = wbuf(w), out16(wp_ref.numel()), out16(wt_ref.numel())
            built.call("hn_pack_weight_ex", wd.data_ptr(), wp.ptr(), wt.ptr() if with_wt else None, cout, ctot, ci0, cin, taps, 0, None, None)
            held(wp, wp_ref, name + " wp", "(cout, tap, k)")
            if with_wt:
                held(wt, wt_ref, name + " wt", "(cin, tap, k)")
            else:
                assert wt.untouched(), name + ": wt written"
                wt.check(name + " wt")


def phase_case(k, ctot, name):
    g = gen(name)
    return dyadic((k, ctot, 3, 3), g), torch.randn(k, generator=g, dtype=F32)


def held_bias(b_eff, want, name):
    same_bits(b_eff.as_(I32, want.numel()), want.to(F32).view(I32), name + " b_eff", "(cout)")
    b_eff.check(name + " b_eff")


@pytest.mark.parametrize("k,ctot,c0", [(5, 12, 12), (5, 12, 8), (64, 16, 8), (72, 8, 5)])      # 4 * 5 = 20 sits under a KP of 32
def test_pack_weight_ex_phase(built, k, ctot, c0):
    w, bias = phase_case(k, ctot, f"phase{k}x{ctot}x{c0}")
    wp_ref, wt_ref, be_ref = P.phase(w, c0, bias)
    assert bool((P.bits(wp_ref).view(BF16).double() != wp_ref).any()), "the effective weights must need rounding"
    for with_wt in (True, False):
        for with_b in (True, False):
            name = f"hn_pack_weight_ex phase (k {k}, C {ctot}, c0 {c0}){'' if with_wt else ', wt = NULL'}{'' if with_b else ', b_eff = NULL'}"
            wd, bd = wbuf(w), wbuf(bias)
            wp, wt, be = out16(wp_ref.numel()), out16(wt_ref.numel()), GuardedBytes(16 * k)
            built.call("hn_pack_weight_ex", wd.data_ptr(), wp.ptr(), wt.ptr() if with_wt else None, k, ctot, 0, c0, 9, 1,
                       bd.data_ptr() if with_b else None, be.ptr() if with_b else None)
            held(wp, wp_ref, name + " wp", "(phase * k + cout, tap, k)")
            if with_wt:
                held(wt, wt_ref, name + " wt", "(cin, tap, phase * k + cout)")
            else:
                assert wt.untouched(), name + ": wt written"
                wt.check(name + " wt")
            if with_b:
                held_bias(be, be_ref, name)
            else:
                assert be.untouched(), name + ": b_eff written"
                be.check(name + " b_eff")


# =====================================================================================================================================
# hn_pack_weights_batched: one launch over a table, with block_job and with the in-kernel job search
# =====================================================================================================================================
BATCHED = [
    # cout, cin, taps, weight pointer's offset from 16-byte alignment (elements), loader
    (32, 32, 9, 0, "float4"),
    (33, 31, 1, 0, "element"),                         # Cin * taps % 4 != 0
    (1, 1, 1, 0, "element"),
    (31, 33, 9, 0, "element"),                         # 297 % 4 == 1
    (65, 70, 9, 0, "element"),                         # 3 x 3 tiles, ragged on both axes
    (65, 72, 9, 0, "float4"),                          # 3 x 3 tiles, the last cin tile 8 wide
    (32, 32, 1, 1, "element"),                         # Cin * taps % 4 == 0, but the pointer is 4 bytes off
    (33, 32, 1, 0, "float4"),
    (1, 33, 1, 0, "element"),
    (31, 1, 9, 0, "element"),
    (5, 4, 9, 1, "element"),                           # 36 % 4 == 0, pointer 4 bytes off
    (31, 32, 1, 0, "float4"),
]


def loader(cin, taps, ptr):
    """pack_tile's choice, restated"""
    return "float4" if (cin * taps) % 4 == 0 and ptr % 16 == 0 else "element"


@pytest.mark.parametrize("kind", ["coded", "random"])
def test_pack_weights_batched(built, kind):
    assert len(BATCHED) >= 9 and {t for _, _, t, _, _ in BATCHED} == {1, 9}
    assert {1, 31, 32, 33} <= {c for c, _, _, _, _ in BATCHED} and {1, 31, 32, 33} <= {c for _, c, _, _, _ in BATCHED}
    ws, refs = [], []
    for j, (cout, cin, taps, off, how) in enumerate(BATCHED):
        w = dict(inputs(cout, cin, taps, f"batched{j}"))[kind]
        ws.append(wbuf(w, off))
        refs.append(P.dense(w))
        assert loader(cin, taps, ws[-1].data_ptr()) == how, f"job {j} does not reach the {how} loader"
    for table in (True, False):                                                # block_job given / NULL: each block searches the table
        outs, rows, owner, blk = [], [], [], 0
        for j, (cout, cin, taps, off, how) in enumerate(BATCHED):
            wp, wt = out16(refs[j][0].numel()), out16(refs[j][1].numel())
            outs.append((wp, wt))
            nb = (P.kp(cout) // 32) * (P.kp(cin) // 32)                        # one block per 32 x 32 (cout, cin) tile
            rows.append([ws[j].data_ptr(), wp.ptr(), wt.ptr(), cout, cin, taps, blk, P.kp(cin) // 32])
            owner += [j] * nb
            blk += nb
        jobs, own = D(torch.tensor(rows, dtype=I64)), D(torch.tensor(owner, dtype=I32))
        built.call("hn_pack_weights_batched", jobs.data_ptr(), len(rows), blk, own.data_ptr() if table else None)
        for j, (cout, cin, taps, off, how) in enumerate(BATCHED):
            name = f"hn_pack_weights_batched job {j} ({cout}, {cin}, {taps}; {how} loader) {kind}, {'block_job' if table else 'job search'}"
            held(outs[j][0], refs[j][0], name + " wp", "(cout, tap, k)")
            held(outs[j][1], refs[j][1], name + " wt", "(cin, tap, k)")


# =====================================================================================================================================
# hn_gconv_pack_diag
# =====================================================================================================================================
def grouped(c, kind, name):
    w = dict(inputs(c, 8, 9, name))[kind]
    return w.reshape(c, 8, 3, 3)


@pytest.mark.parametrize("c", [8, 24, 64, 72, 152])
def test_gconv_pack_diag(built, c):
    for kind in ("coded", "random"):
        w = grouped(c, kind, f"diag{c}")
        wk_ref, wd_ref = P.diag(w)
        wd_, wk, wd = wbuf(w), out16(c * 576), out16(c * 576)
        built.call("hn_gconv_pack_diag", wd_.data_ptr(), wk.ptr(), wd.ptr(), c)
        held(wk, wk_ref, f"hn_gconv_pack_diag C {c} {kind} wk", "(cout, tap, column)")
        held(wd, wd_ref, f"hn_gconv_pack_diag C {c} {kind} wd", "(cin, tap, column)")


# =====================================================================================================================================
# hn_pack_small_batched: kinds 1-4 in one launch
# =====================================================================================================================================
def small_jobs(kind_of_input, sentinel_diag):
    """the mixed table: (row, blocks, checks) per job; the block counts (1, 6, 7, 5, 12, 21, 43, ...) put the job boundaries on no
    convenient multiple"""
    jobs = []

    def add(row, elements, checks):
        jobs.append((row, (elements + 255) // 256, checks))

    def pick(shape3, name):
        return dict(inputs(*shape3, name))[kind_of_input]

    # kind 1: depthwise, with and without the flipped pack
    for c, with_f in ((24, True), (8, False), (152, True)):
        w = pick((c, 1, 9), f"small-dw{c}")
        wk_ref, wf_ref = P.dw(w)
        wd, wk, wf = wbuf(w), out16(9 * c), out16(9 * c)
        name = f"kind 1 (depthwise, C {c}{'' if with_f else ', out1 = NULL'})"
        checks = [(wk, wk_ref, name + " wk", "(tap, c)")] + ([(wf, wf_ref, name + " wkf", "(tap, c)")] if with_f else [(wf, None, name + " wkf", None)])
        add([wd.data_ptr(), wk.ptr(), wf.ptr() if with_f else 0, 0, 0, 1, 0, c], 9 * c, checks)
    # kind 2: grouped stencil operands, both flips, with and without wd
    for c, flip, with_d in ((24, 1, True), (16, 0, True), (40, 1, False)):
        w = pick((c, 8, 9), f"small-g{c}").reshape(c, 8, 3, 3)
        wk_ref, wd_ref = P.gconv(w, flip)
        wd_, wk, wd = wbuf(w), out16(72 * c), out16(72 * c)
        name = f"kind 2 (grouped, C {c}, flip {flip}{'' if with_d else ', out1 = NULL'})"
        checks = [(wk, wk_ref, name + " wk", "(tap, i, g, o)")] + ([(wd, wd_ref, name + " wd", "(tap, o, g, i)")] if with_d else [(wd, None, name + " wd", None)])
        add([wd_.data_ptr(), wk.ptr(), wd.ptr() if with_d else 0, 0, 0, 2, 0, c // 8, flip], 72 * c, checks)
    # kind 3: the diagonal blocks only, on buffers the owner filled (zeros in production; here zeros or a sentinel)
    for c in (24, 72, 152):
        w = pick((c, 8, 9), f"small-diag{c}").reshape(c, 8, 3, 3)
        wd_ = wbuf(w)
        wk, wd = out16(c * 576, fill=None if sentinel_diag else 0), out16(c * 576, fill=None if sentinel_diag else 0)
        add([wd_.data_ptr(), wk.ptr(), wd.ptr(), 0, 0, 3, 0, c], 72 * c, [("diag", c, w, wk, wd)])
    # kind 4: slices and phase forms, with and without wt / b_eff
    for cout, ctot, ci0, cin, taps, with_wt in ((5, 20, 3, 13, 9, True), (33, 40, 8, 32, 1, False)):
        w = pick((cout, ctot, taps), f"small-slice{cout}")
        wp_ref, wt_ref = P.slice_(w, ci0, cin)
        wd_, wp, wt = wbuf(w), out16(wp_ref.numel()), out16(wt_ref.numel())
        name = f"kind 4 (slice {cout}, {ctot}, ci0 {ci0}, cin {cin}, taps {taps}{'' if with_wt else ', wt = NULL'})"
        checks = [(wp, wp_ref, name + " wp", "(cout, tap, k)"), (wt, wt_ref if with_wt else None, name + " wt", "(cin, tap, k)")]
        add([wd_.data_ptr(), wp.ptr(), wt.ptr() if with_wt else 0, 0, 0, 4, 0, cout, ctot, ci0, cin, taps, 0],
            wp_ref.numel() // 8 + (wt_ref.numel() // 8 if with_wt else 0), checks)
    for k, ctot, c0, with_wt, with_b in ((5, 12, 8, True, True), (64, 16, 8, False, True), (72, 8, 5, True, False)):
        w, bias = phase_case(k, ctot, f"small-phase{k}")
        wp_ref, wt_ref, be_ref = P.phase(w, c0, bias)
        wd_, bd, wp, wt, be = wbuf(w), wbuf(bias), out16(wp_ref.numel()), out16(wt_ref.numel()), GuardedBytes(16 * k)
        name = f"kind 4 (phase k {k}, C {ctot}, c0 {c0}{'' if with_wt else ', wt = NULL'}{'' if with_b else ', b_eff = NULL'})"
        checks = [(wp, wp_ref, name + " wp", "(phase * k + cout, tap, k)"), (wt, wt_ref if with_wt else None, name + " wt", "(cin, tap, column)"),
                  ("bias", be, be_ref if with_b else None, name)]
        add([wd_.data_ptr(), wp.ptr(), wt.ptr() if with_wt else 0, be.ptr() if with_b else 0, bd.data_ptr() if with_b else 0, 4, 0, k, ctot, 0, c0, 9, 1],
            wp_ref.numel() // 8 + (wt_ref.numel() // 8 if with_wt else 0) + (4 * k if with_b else 0), checks)
    # interleave the kinds so that neighbouring blocks belong to different branches
    order = [0, 3, 6, 9, 11, 1, 4, 7, 10, 12, 2, 5, 8, 13]
    assert sorted(order) == list(range(len(jobs)))
    return [jobs[i] for i in order]


def run_small(built, jobs):
    rows, owner, blk = [], [], 0
    for j, (row, nb, _) in enumerate(jobs):
        row = list(row)
        row[6] = blk
        rows.append(row + [0] * (16 - len(row)))
        owner += [j] * nb
        blk += nb
    assert any(r[6] % 2 for r in rows) and len({nb for _, nb, _ in jobs}) > 4
    tab, own = D(torch.tensor(rows, dtype=I64)), D(torch.tensor(owner, dtype=I32))
    built.call("hn_pack_small_batched", tab.data_ptr(), own.data_ptr(), blk)


@pytest.mark.parametrize("kind", ["coded", "random"])
@pytest.mark.parametrize("diag_fill", ["sentinel", "zeros"])
def test_pack_small_batched(built, kind, diag_fill):
    jobs = small_jobs(kind, diag_fill == "sentinel")
    run_small(built, jobs)
    for j, (_, _, checks) in enumerate(jobs):
        for chk in checks:
            if chk[0] == "diag":
                _, c, w, wk, wd = chk
                m = P.diag_mask(c)
                singles = (out16(c * 576), out16(c * 576))
                if diag_fill == "zeros":                                       # on zeros: hn_gconv_pack_diag's whole output
                    built.call("hn_gconv_pack_diag", wbuf(w).data_ptr(), singles[0].ptr(), singles[1].ptr(), c)
                for out, ref, single, nm in zip((wk, wd), P.diag(w), singles, ("wk", "wd")):
                    name = f"hn_pack_small_batched job {j} kind 3 (diagonal blocks, C {c}, {diag_fill}) {kind} {nm}"
                    got = out.as_(I16, c, 9, 64).cpu()
                    same_bits(got[m], P.bits(ref)[m], name + " diagonal blocks", "(element of the blocks)")
                    if diag_fill == "sentinel":                                # seven eighths of the operand are never written
                        same_bits(got[~m], torch.full_like(got[~m], SENT16), name + " off-diagonal elements", "(element outside the blocks)")
                    else:
                        same_bits(got, single.as_(I16, c, 9, 64).cpu(), name + " against hn_gconv_pack_diag", "(c, tap, column)")
                        same_bits(got, P.bits(ref), name, "(c, tap, column)")
                    out.check(name)
            elif chk[0] == "bias":
                _, be, ref, name = chk
                name = f"hn_pack_small_batched job {j} {name} {kind}"
                if ref is not None:
                    held_bias(be, ref, name)
                else:
                    assert be.untouched(), name + ": b_eff written"
                    be.check(name + " b_eff")
            else:
                out, ref, name, what = chk
                name = f"hn_pack_small_batched job {j} {name} {kind}"
                if ref is not None:
                    held(out, ref, name, what)
                else:
                    assert out.untouched(), name + ": written although its pointer was NULL"
                    out.check(name)


# =====================================================================================================================================
# hn_pack_levels
# =====================================================================================================================================
LEVELS_N, LEVELS_H, LEVELS_W = 2, (5, 3, 2, 1), (7, 4, 2, 1)


def level_sources(c, extra, name):
    """bf16 bit patterns per level, each a channel slice of a source `extra` columns wider"""
    g = gen(name)
    bits_, devs = [], []
    for l, (h, w) in enumerate(zip(LEVELS_H, LEVELS_W)):
        rows = LEVELS_N * h * w
        v = torch.randn(rows, c + extra, generator=g, dtype=F32).to(BF16)
        v[0, 0], v[-1, c - 1] = -0.0, 1000.0 + l                              # a signed zero and a per-level tag at the corners
        wide = D(v)
        bits_.append(v[:, :c].contiguous().view(I16))
        devs.append(wide)
    return bits_, devs


def levels_args(devs):
    nl = len(devs)
    srcs = (ctypes.c_void_p * nl)(*[d.data_ptr() for d in devs])
    lds = (ctypes.c_int * nl)(*[d.stride(0) for d in devs])
    hs, ws = (ctypes.c_int * nl)(*LEVELS_H), (ctypes.c_int * nl)(*LEVELS_W)
    return srcs, lds, hs, ws


@pytest.mark.parametrize("c", [8, 24])
@pytest.mark.parametrize("align", [1, 128])
@pytest.mark.parametrize("wide", [0, 8])
def test_pack_levels(built, c, align, wide):
    name = f"hn_pack_levels C {c}, row_align {align}, {'strides wider than C' if wide else 'dense rows'}"
    bits_, devs = level_sources(c, wide, f"levels{c}-{wide}")
    ldd = c + wide
    want = P.levels(bits_, LEVELS_N, LEVELS_H, LEVELS_W, align, SENT16, ldd)
    rows = R.row_offsets(LEVELS_N, LEVELS_H, LEVELS_W, align)[-1]
    assert want.shape == (rows, ldd) and (align == 1 or rows == 4 * 128)
    out = out16(rows * ldd)
    srcs, lds, hs, ws = levels_args(devs)
    built.call("hn_pack_levels", ctypes.addressof(srcs), ctypes.addressof(lds), out.ptr(), ldd, LEVELS_N, c, 4, ctypes.addressof(hs),
               ctypes.addressof(ws), align)
    # real rows carry the source bits; alignment rows and the columns beyond C keep the sentinel
    same_bits(out.as_(I16, rows, ldd), want, name, "(row, column)")
    out.check(name)


def test_pack_levels_refuses(built):
    f = built.raw("hn_pack_levels")
    _, devs = level_sources(8, 8, "levels-refused")
    srcs, lds, hs, ws = levels_args(devs)
    rows = R.row_offsets(LEVELS_N, LEVELS_H, LEVELS_W, 1)[-1]
    out = out16(rows * 16)
    a = lambda x: ctypes.addressof(x)
    assert f(a(srcs), a(lds), out.ptr(), 16, LEVELS_N, 12, 4, a(hs), a(ws), 1, stream()) == 1, "C % 8 != 0 accepted"
    assert f(a(srcs), a(lds), out.ptr(), 12, LEVELS_N, 8, 4, a(hs), a(ws), 1, stream()) == 1, "ldd % 8 != 0 accepted"
    bad = (ctypes.c_int * 4)(16, 16, 12, 16)
    assert f(a(srcs), a(bad), out.ptr(), 16, LEVELS_N, 8, 4, a(hs), a(ws), 1, stream()) == 1, "a source stride that is no multiple of 8 accepted"
    assert f(a(srcs), a(lds), out.ptr(), 16, LEVELS_N, 8, 6, a(hs), a(ws), 1, stream()) == 1, "more than 5 levels accepted"
    torch.cuda.synchronize()
    assert out.untouched(), "a refused hn_pack_levels call wrote"
    out.check("hn_pack_levels (refused calls)")
