"""The seg-head launch forms of the direct 3x3 kernels (csrc/hn_gemm.hip) held to EXACT integer references, form by form: the phase-form
forward (generic kernel and the persistent seg_phase64_conv_kernel), the depth-to-space output conv and its arg-max (generic kernel and
seg_out_conv_kernel<amax>), the phase-form data gradient on the padded grid, and the folded data gradient (folding epilogue +
seg_ring_fix_kernel) in plain and space-to-depth order.

The method of tests/test_gemm_exact_gpu.py: operands are small integers, which bf16 holds exactly; weights are integers and the phase
form's effective weights sums of at most 4 of them; so every fp32 accumulation is exact in any order below 2^24 (asserted with budget()),
an fp32 output equals the float64 reference (tests/seg_conv_ref.py, held to plain torch by tests/test_seg_conv_ref_cpu.py) bit for bit
and a bf16 output equals it rounded once.  ELU keeps bit equality because its pre-activations are integers and every expm1(-j) lies
>= 2^-12 from a bf16 rounding boundary (asserted on the reference) while the device's __expf(x) - 1 is accurate to ~1e-7.  The fold has
two documented bf16 roundings (the staged accumulator, the fix-up's sum); its cases keep every staged value bf16-exact (integers of
magnitude <= 256, quarter-integers of magnitude <= 64 under ELU'; asserted), so those roundings are identities.  Every case first
asserts the form it lands on (tests/gemm_plans.py), every output lies between guard bands, and a mismatch names its phase, cout tile,
16 x 16 patch, persistent workgroup range, or ring position / interior."""
import pytest
import torch

from tests import gemm_plans as P
from tests import seg_conv_ref as R
from tests.guards import BAND, Guarded, dev
from tests.test_gemm_exact_gpu import BF16, F32, RAND_TOL, budget, exact, gen, ints, randn, seed_of

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_ELU = 0, 3
HN_ERR_ARG, HN_ERR_UNSUPPORTED = 1, 3
SENT64 = 0x7FC000017FC00001


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops
    return ops


class GuardedI64:
    """an int64 output of `count` elements between two sentinel bands (the arg-max mask)"""

    def __init__(self, count):
        self.count = count
        self.buf = torch.full((2 * BAND + count,), SENT64, dtype=torch.int64, device=dev())
        self.view = self.buf[BAND:BAND + count]

    def ptr(self):
        return self.view.data_ptr()

    def check(self, name):
        bad = torch.cat([self.buf[:BAND], self.buf[BAND + self.count:]]) != SENT64
        if int(bad.sum()):
            pytest.fail(f"{name}: {int(bad.sum())} guard-band elements of the int64 mask overwritten")


def untouched(g):
    idt = torch.int32 if g.dtype == F32 else torch.int16
    sent = g.buf.view(idt)[0]
    return bool((g.buf.view(idt) == sent).all())


def rc_of(K, name, *args):
    """status of an entry point that is expected to refuse"""
    return K.lib().raw(name)(*args, torch.cuda.current_stream().cuda_stream)


def int_weights(k, c, g, lo=-2, hi=2, density=1.0):
    w = torch.randint(lo, hi + 1, (k, c, 3, 3), generator=g, device=dev()).float()
    if density < 1.0:
        w = w * (torch.rand(w.shape, generator=g, device=dev()) < density).float()
    return w.contiguous()


def packed_phase(K, w, c0, bias):
    """pack_phase_weight of integer weights, with pack_w_ex_kernel's phase mode held to the reference's effective weights: both operand
    layouts, their zero K padding and the repeated bias"""
    k = w.shape[0]
    wp, wt, be = K.pack_phase_weight(w, c0, bias)
    torch.cuda.synchronize()
    we, bref = R.phase_weights(w, bias, c0)
    assert float(we.abs().max()) <= 256                                   # sums of <= 4 small integers: exact in bf16
    kpi, kpo = P.kp32(c0), P.kp32(4 * k)
    wpv, wtv = wp.view(4 * k, 9, kpi).double(), wt.view(c0, 9, kpo).double()
    exact(wpv[:, :, :c0], we.reshape(4 * k, c0, 9).permute(0, 2, 1), "wp_eff", lambda ii: f"phase {ii[0][0] // k} cout {ii[0][0] % k} tap {ii[0][1]}")
    exact(wtv[:, :, :4 * k], we.reshape(4 * k, c0, 9).permute(1, 2, 0), "wt_eff", lambda ii: f"cin {ii[0][0]} tap {ii[0][1]} phase {ii[0][2] // k}")
    assert bool((wpv[:, :, c0:] == 0).all()) and bool((wtv[:, :, 4 * k:] == 0).all()), "K padding of the packed effective weights is not zero"
    exact(be, bref, "b_eff")
    return wp, wt, be, we


def where_phase(ii, grid, k, form):
    """name the place of full-resolution output element (row, channel) of a phase / depth-to-space form on the low-resolution grid"""
    n, h, w = grid
    row, col = ii[0][0], ii[0][1]
    img, r = divmod(row, 4 * h * w)
    yy, xx = divmod(r, 2 * w)
    ph = (yy & 1) * 2 + (xx & 1)
    patch = (img * P.cdiv(h, 16) + (yy // 2) // 16) * P.cdiv(w, 16) + (xx // 2) // 16
    s = f"{form['kernel']}: image {img} low-res pixel ({yy // 2}, {xx // 2}) phase {ph}, cout tile {(ph * k + col) // form['bc']}, 16x16 patch {patch}"
    if form["persistent"]:
        ppw, nwg = P.persistent_ranges(n, h, w, form["kernel"].split("<")[0])
        wg = patch // ppw
        s += f", workgroup {wg} of {nwg} walking patches [{wg * ppw}, {min((wg + 1) * ppw, P.npatch(n, h, w))})" + (" (the last, ragged range)" if wg == nwg - 1 and P.npatch(n, h, w) % ppw else "")
    return s


# ---- 1 / 2. phase-form forward -------------------------------------------------------------------------------------------------------
PHASE_FWD_CASES = [
    # name, k, C0, low-res grid, addend, acts, expected form
    ("ph64", 64, 64, (2, 17, 33), False, (ACT_ELU,), "direct<64,bf16,wpre,phase>"),
    ("ph128_addend", 128, 128, (1, 18, 20), True, (ACT_ELU,), "direct<128,bf16,phase>"),
    ("ph64_c40", 64, 40, (3, 5, 7), False, (ACT_NONE,), "direct<64,bf16,wpre,phase>"),
    ("ph64_addend", 64, 64, (2, 9, 17), True, (ACT_ELU, ACT_NONE), "direct<64,bf16,wpre,phase>"),
    # the persistent kernel: >= 1024 patches
    ("persistent_ragged", 64, 64, (171, 17, 33), False, (ACT_ELU, ACT_NONE), "seg_phase64"),
    ("persistent_whole", 64, 64, (64, 64, 64), False, (ACT_ELU, ACT_NONE), "seg_phase64"),
]
# one patch short of the threshold: stays on the generic kernel (restated only; the generic kernel has its cases above)
PHASE_FWD_BELOW = (64, 64, (341, 16, 33))


def phase_fwd_form(case):
    name, k, c0, (n, h, w), addend, acts, kern = case
    return [P.phase_fwd_form(n, h, w, k, c0, a, addend=addend, ldc=k + 8) for a in acts]


@pytest.mark.parametrize("case", PHASE_FWD_CASES, ids=[c[0] for c in PHASE_FWD_CASES])
def test_phase_forward_exact(K, case):
    name, k, c0, grid, with_add, acts, kern = case
    n, h, w = grid
    forms = phase_fwd_form(case)
    assert all(f["kernel"] == kern for f in forms), (name, forms)
    if name == "persistent_ragged":
        ppw, nwg = P.persistent_ranges(n, h, w, "seg_phase64")
        assert P.npatch(n, h, w) == 1026 and P.npatch(n, h, w) % ppw, "the last workgroup's patch range is no longer ragged"
    g = gen(seed_of(name))
    x0 = ints((n, h, w, c0), -2, 2, g, width=c0 + 8)
    wgt = int_weights(k, c0, g)
    bias = torch.randint(-4, 5, (k,), generator=g, device=dev()).float()
    add = ints((n, 2 * h, 2 * w, k), -6, 6, g, width=k + 16) if with_add else None   # ld_add wider than k
    wp, _, be, we = packed_phase(K, wgt, c0, bias)
    budget(float(R.conv3x3(x0.double().abs(), we.abs(), "clamp").max()) + 4 + 6, name)
    pre = R.phase_forward_pre(x0, wgt, bias, c0, add)
    assert bool((pre == pre.round()).all())
    for act, form in zip(acts, forms):
        if act == ACT_ELU:
            neg = pre[pre < 0]
            assert neg.numel() and R.elu_margin(neg.unique()) >= 2.0 ** -12, "an ELU value too close to a bf16 rounding boundary for bit equality"
            want = R.elu(pre).to(BF16)
        else:
            want = pre.to(BF16)
        out = Guarded(n * 4 * h * w, k, k + 8, BF16)
        K.lib().call("hn_conv3x3_phase", K.ptr(x0), 4, n, h, w, c0, x0.stride(2), K.ptr(wp), 4 * k, P.kp32(c0), K.ptr(be), act, out.ptr(), k + 8, k,
                     K.ptr(add), add.stride(2) if with_add else 0)
        torch.cuda.synchronize()
        exact(out.view, want.reshape(-1, k), f"{name} act {act} out", lambda ii: where_phase(ii, grid, k, form))
        out.check(f"{name} act {act} out")
        del out, want


# ---- 3 / 4. depth-to-space output conv and its arg-max ---------------------------------------------------------------------------------------
SEG_OUT_CASES = [
    # name, k, low-res grid, expected form of the logits launch, expected form of the arg-max launch (None: the entry point refuses the
    # shape, HN_ERR_ARG -- rows of 2 W k floats must be 16-byte multiples, which also keeps odd W k off the persistent kernel)
    ("k5_direct", 5, (2, 17, 33), "direct<32,f32,d2s>", None),
    ("k3_direct", 3, (2, 17, 33), "direct<16,f32,wpre,d2s>", None),
    ("k8_direct", 8, (2, 17, 33), "direct<32,f32,d2s>", "direct<32,f32,d2s,amax>"),
    ("k5_direct_evenW", 5, (2, 17, 34), "direct<32,f32,d2s>", "direct<32,f32,d2s,amax>"),
    ("k3_direct_evenW", 3, (2, 17, 34), "direct<16,f32,wpre,d2s>", "direct<16,f32,wpre,d2s,amax>"),
    ("k8_persistent", 8, (171, 17, 33), "seg_out<false>", "seg_out<true>"),
    ("k5_oddW_stays_direct", 5, (171, 17, 33), "direct<32,f32,d2s>", None),
    ("k5_persistent", 5, (171, 17, 34), "seg_out<false>", "seg_out<true>"),
    ("k3_persistent", 3, (171, 17, 34), "seg_out<false>", "seg_out<true>"),
]


def seg_out_inputs(K, name, k, grid, rand=False):
    n, h, w = grid
    g = gen(seed_of(name))
    x0 = randn((n, h, w, 64), g, width=72) if rand else ints((n, h, w, 64), -1, 1, g, 0.3, width=72)
    wgt = (torch.randn(k, 64, 3, 3, generator=g, device=dev()) * 0.1).contiguous() if rand else int_weights(k, 64, g, -1, 1)
    bias = torch.randn(k, generator=g, device=dev()) if rand else torch.randint(-2, 3, (k,), generator=g, device=dev()).float()
    return x0, wgt, bias


@pytest.mark.parametrize("case", SEG_OUT_CASES, ids=[c[0] for c in SEG_OUT_CASES])
def test_seg_out_conv_and_argmax_exact(K, case):
    name, k, grid, kern, kern_amax = case
    n, h, w = grid
    form, form_a = P.seg_out_form(n, h, w, k), P.seg_out_form(n, h, w, k, amax=True)
    assert form["kernel"] == kern and (kern_amax is None or form_a["kernel"] == kern_amax), (name, form, form_a)
    x0, wgt, bias = seg_out_inputs(K, name, k, grid)
    wp, _, be, we = packed_phase(K, wgt, 64, bias)
    budget(float(R.conv3x3(x0.double().abs(), we.abs(), "clamp").max()) + 2, name)
    logits = R.phase_forward_pre(x0, wgt, bias, 64)
    out = Guarded(n * 4 * h * w, k, k, F32)                               # (the depth-to-space store is dense: k floats per output pixel)
    K.lib().call("hn_conv_gemm_nt", K.ptr(x0), None, 4, n, h, w, 64, 0, x0.stride(2), 0, 0, n * h * w, K.ptr(wp), 4 * k, 64, 9, K.ptr(be), 0,
                 out.ptr(), 1, 4 * k, 0, -k, None, None)
    torch.cuda.synchronize()
    exact(out.view, logits.reshape(-1, k), f"{name} logits", lambda ii: where_phase(ii, grid, k, form))
    out.check(f"{name} logits")
    mask = GuardedI64(n * 4 * h * w)
    args = (K.ptr(x0), n, h, w, 64, x0.stride(2), K.ptr(wp), k, 64, K.ptr(be), mask.ptr())
    if kern_amax is None:
        assert (2 * w * k) % 4 != 0
        assert rc_of(K, "hn_conv3x3_out_argmax", *args) == HN_ERR_ARG
        torch.cuda.synchronize()
        assert bool((mask.buf == SENT64).all()), "a refused arg-max call wrote to the mask"
        return
    top = logits.max(-1, keepdim=True)[0]
    ties = int(((logits == top).sum(-1) > 1).sum())
    assert ties >= 1, "no output pixel with a tied maximum: 'first maximum wins' is not tested"
    want = torch.argmax(logits, -1).reshape(-1)
    assert bool((want == (logits == top).long().argmax(-1).reshape(-1)).all())     # the reference itself takes the FIRST maximum
    K.lib().call("hn_conv3x3_out_argmax", *args)
    torch.cuda.synchronize()
    exact(mask.view.reshape(-1, 1), want.reshape(-1, 1), f"{name} arg-max ({ties} tied pixels)", lambda ii: where_phase(ii, grid, 1, form_a))
    mask.check(f"{name} mask")


# ---- 5. phase-form data gradient on the padded grid -------------------------------------------------------------------------------------------
PHASE_DGRAD_CASES = [("dph64", 64, 64, (2, 6, 10), "direct<64,bf16,dphase>"), ("dph128_c256", 128, 256, (1, 8, 12), "direct<128,bf16,dphase>")]


def where_padded(ii, n, hp, wp_, bc, kern):
    row, col = ii[0][0], ii[0][1]
    img, r = divmod(row, hp * wp_)
    y, x = divmod(r, wp_)
    return f"{kern}: image {img} padded pixel ({y}, {x}), cout tile {col // bc}, 16x16 patch {(img * P.cdiv(hp, 16) + y // 16) * P.cdiv(wp_, 16) + x // 16}"


@pytest.mark.parametrize("case", PHASE_DGRAD_CASES, ids=[c[0] for c in PHASE_DGRAD_CASES])
def test_phase_dgrad_padded_exact(K, case):
    name, k, c0, (n, h, w), kern = case
    form = P.phase_dgrad_form(n, h, w, k, c0, ldc=c0 + 8)
    assert form["kernel"] == kern, form
    g = gen(seed_of(name))
    wgt = int_weights(k, c0, g)
    _, wt, _, we = packed_phase(K, wgt, c0, torch.zeros(k, device=dev()))
    dzs = ints((n, h, w, 4 * k), -2, 2, g, width=4 * k + 8)
    budget(float(R.dgrad_padded(dzs.double().abs(), we.abs()).max()), name)
    want = R.dgrad_padded(dzs, we)
    out = Guarded(n * (h + 2) * (w + 2), c0, c0 + 8, BF16)
    K.lib().call("hn_conv3x3_phase", K.ptr(dzs), 3, n, h + 2, w + 2, 4 * k, dzs.stride(2), K.ptr(wt), c0, P.kp32(4 * k), None, 0, out.ptr(), c0 + 8, k,
                 None, 0)
    torch.cuda.synchronize()
    exact(out.view, want.to(BF16).reshape(-1, c0), f"{name} padded-grid gradient", lambda ii: where_padded(ii, n, h + 2, w + 2, form["bc"], kern))
    out.check(f"{name} out")


# ---- 6. folded data gradient -----------------------------------------------------------------------------------------------------------------
YPREV_SET = (2.0, 0.5, 0.0, -0.25, -0.5, -0.75, -1.0)        # ELU outputs whose e + 1 is exact
PLAIN_SHAPES = [(1, 4, 4), (3, 5, 7), (2, 33, 18)]
S2D_SHAPES = [(2, 4, 6), (1, 16, 20)]
NOUTS = [40, 64, 112, 256]


def _fold_cases():
    out, i = [], 0
    for form in (1, 2, 3):                                    # GemmNT::fold: plain, space-to-depth only (out = NULL), both
        for phase_k, clamp in ((0, 0), (0, 1), (64, 1), (128, 1)):
            for with_y in (True, False):
                shapes = PLAIN_SHAPES + S2D_SHAPES if form == 1 else S2D_SHAPES
                grid = shapes[i % len(shapes)]
                nout = NOUTS[(i + i // 4) % 4]
                cz = 4 * phase_k if phase_k else (24, 64)[i % 2]
                out.append((f"fold{form}_k{phase_k}_clamp{clamp}_{'elu' if with_y else 'lin'}_{grid[1]}x{grid[2]}_n{nout}", form, phase_k, clamp,
                            with_y, grid, cz, nout))
                i += 1
    # every pixel of a 4 x 4 map but four is a border target, the frame's corners collect three ring positions: both paddings, with ELU'
    out.append(("fold1_k0_clamp1_elu_4x4_n64", 1, 0, 1, True, (1, 4, 4), 64, 64))
    out.append(("fold1_k64_clamp1_elu_4x4_n112", 1, 64, 1, True, (1, 4, 4), 256, 112))
    out.append(("fold1_k0_clamp0_lin_33x18_n256", 1, 0, 0, False, (2, 33, 18), 64, 256))
    return out


FOLD_CASES = _fold_cases()


def fold_case_form(case):
    name, form, phase_k, clamp, with_y, (n, h, w), cz, nout = case
    return P.fold_form(n, h, w, cz, nout, phase_k, plain=form != 2, s2d=form != 1)


def fold_call(K, form, dz, cz, grid, wt, nout, kp, phase_k, clamp, out, out2, yprev, ring):
    n, h, w = grid
    yargs = (K.ptr(yprev), yprev.stride(2) if yprev is not None else 0, ring.ptr())
    if form == 1:
        return ("hn_conv3x3_dgrad_fold", K.ptr(dz), dz.stride(2), cz, n, h, w, K.ptr(wt), nout, kp, phase_k, clamp, out.ptr(), out.ld, *yargs)
    return ("hn_conv3x3_dgrad_fold_s2d", K.ptr(dz), dz.stride(2), cz, n, h, w, K.ptr(wt), nout, kp, phase_k, clamp,
            out.ptr() if out is not None else None, out.ld if out is not None else 0, out2.ptr(), out2.ld, *yargs)


@pytest.mark.parametrize("case", FOLD_CASES, ids=[c[0] for c in FOLD_CASES])
def test_dgrad_fold_exact(K, case):
    name, form, phase_k, clamp, with_y, grid, cz, nout = case
    n, h, w = grid
    status, f = fold_case_form(case)
    assert status == 0 and ("fold%d" % form in f["kernel"] or f["kernel"] == "direct_narrow<64>"), (name, status, f)
    g = gen(seed_of(name))
    # sparse +-1 operands sized so that the accumulator's standard deviation is ~3: every staged value stays bf16-exact (asserted below)
    terms = 9 * cz if not phase_k else 4 * cz * 2.25
    dens = min(1.0, (10.0 / terms) ** 0.5)
    dz = ints((n, h, w, cz), -1, 1, g, dens, width=cz + 8)
    if phase_k:
        wgt = int_weights(phase_k, nout, g, -1, 1, dens)                   # forward weight [k][cin = nout]
        _, wt, _, wfull = packed_phase(K, wgt, nout, torch.zeros(phase_k, device=dev()))
        kp = P.kp32(4 * phase_k)
    else:
        wgt = int_weights(cz, nout, g, -1, 1, dens)                        # forward weight [cout = cz][cin = nout]
        wt = K.pack_conv_weight(wgt)[1]
        wfull, kp = wgt.double(), P.kp32(cz)
    yprev = None
    if with_y:
        pick = torch.randint(0, len(YPREV_SET), (n, h, w, nout + 8), generator=g, device=dev())
        yprev = torch.tensor(YPREV_SET, device=dev())[pick].to(BF16)[..., :nout]
    budget(float(R.dgrad_padded(dz.double().abs(), wfull.abs()).max()) * 4, name)
    dvp = R.dgrad_padded(dz, wfull)
    want, stages = R.fold_staged(dvp, clamp, yprev)
    lim = 64 if with_y else 256
    for sname, v in stages:
        q = v * 4 if with_y else v
        assert bool((q == q.round()).all()) and float(v.abs().max()) <= lim and R.bf16_exact(v), \
            f"{name}: {sname} leaves the {'quarter-' if with_y else ''}integers of magnitude <= {lim}: the staged roundings would not be identities"
    cnt = R.ring_count(h, w, clamp, dev())
    assert int((cnt > 0).sum()) == 2 * w + 2 * (h - 2) and int(cnt.max()) == 3
    if with_y:
        for e in YPREV_SET:
            hit = (yprev.double() == e).sum(-1).sum(0)                       # [h, w] occurrences
            assert int(hit[cnt > 0].sum()) > 0 and int(hit[cnt == 0].sum()) > 0, f"{name}: yprev value {e} missing on border or interior pixels"
    out = Guarded(n * h * w, nout, nout + 8, BF16) if form != 2 else None
    out2 = Guarded(n * (h // 2) * (w // 2), 4 * nout, 4 * nout + 8, BF16) if form != 1 else None
    ring = Guarded(n * (2 * (w + 2) + 2 * h), nout, nout, BF16)
    assert K.lib().query("hn_fold_ring_rows", h, w) == 2 * (w + 2) + 2 * h
    call = fold_call(K, form, dz, cz, grid, wt, nout, kp, phase_k, clamp, out, out2, yprev, ring)
    K.lib().call(*call)
    torch.cuda.synchronize()

    def where(ii, s2d):
        row, col = ii[0][0], ii[0][1]
        if s2d:
            img, r = divmod(row, (h // 2) * (w // 2))
            y, x = divmod(r, w // 2)
            ph, col = divmod(col, nout)
            y, x = 2 * y + ph // 2, 2 * x + ph % 2
        else:
            img, r = divmod(row, h * w)
            y, x = divmod(r, w)
        c = int(cnt[y, x])
        kind = f"ring position ({c} padded ring positions fold onto it: seg_ring_fix_kernel)" if c else "interior (the conv's folding epilogue)"
        return (f"{f['kernel']} fold {form}: image {img} pixel ({y}, {x}) channel {col}: {kind}; cout tile {col // f['bc']}, 16x16 patch of the "
                f"padded grid {(img * P.cdiv(h + 2, 16) + (y + 1) // 16) * P.cdiv(w + 2, 16) + (x + 1) // 16}")

    if out is not None:
        exact(out.view, want.to(BF16).reshape(-1, nout), f"{name} plain order", lambda ii: where(ii, False))
        out.check(f"{name} out")
    if out2 is not None:
        exact(out2.view, R.space_to_depth(want).to(BF16).reshape(-1, 4 * nout), f"{name} space-to-depth order", lambda ii: where(ii, True))
        out2.check(f"{name} out_s2d")
    exact(ring.view, R.ring_rows(dvp).to(BF16).reshape(-1, nout), f"{name} ring scratch",
          lambda ii: f"ring row {ii[0][0] % (2 * (w + 2) + 2 * h)} of image {ii[0][0] // (2 * (w + 2) + 2 * h)} (top row, bottom row, left column, right column)")
    ring.check(f"{name} ring scratch")


FOLD_REFUSALS = [
    # name, fold form, grid, Nout, expected status
    ("nout32", 1, (1, 8, 8), 32, HN_ERR_UNSUPPORTED),
    ("nout44", 1, (1, 8, 8), 44, HN_ERR_UNSUPPORTED),
    ("h3", 1, (1, 3, 8), 64, HN_ERR_UNSUPPORTED),
    ("h3_s2d_is_odd", 3, (1, 3, 8), 64, HN_ERR_ARG),
    ("odd_h_s2d", 2, (1, 5, 8), 64, HN_ERR_ARG),
    ("odd_h_both", 3, (1, 5, 8), 64, HN_ERR_ARG),
]


@pytest.mark.parametrize("case", FOLD_REFUSALS, ids=[c[0] for c in FOLD_REFUSALS])
def test_dgrad_fold_refusals_write_nothing(K, case):
    name, form, grid, nout, status = case
    n, h, w = grid
    assert P.fold_form(n, h, w, 64, nout, 0, plain=form != 2, s2d=form != 1)[0] == status
    g = gen(seed_of(name))
    dz = ints((n, h, w, 64), -1, 1, g)
    wt = K.pack_conv_weight(int_weights(64, nout, g, -1, 1))[1]
    ldo = P.cdiv(nout, 8) * 8 + 8
    out = Guarded(n * h * w, nout, ldo, BF16)                              # an aligned out in every refusal
    out2 = Guarded(n * (h // 2) * (w // 2), 4 * nout, 4 * ldo, BF16) if form != 1 else None
    ring = Guarded(n * (2 * (w + 2) + 2 * h), nout, nout, BF16)
    assert out.ptr() % 16 == 0
    call = fold_call(K, form, dz, 64, grid, wt, nout, 64, 0, 0, out, out2, None, ring)
    assert rc_of(K, *call) == status
    torch.cuda.synchronize()
    for gb, nm in ((out, "out"), (out2, "out_s2d"), (ring, "ring")):
        if gb is not None:
            gb.check(f"{name} {nm}")
            assert untouched(gb), f"{name}: the refused call wrote to {nm}"


# ---- random-operand companion ----------------------------------------------------------------------------------------------------------------
def test_seg_out_random_bound(K):
    """random companions of the depth-to-space output conv on both kernels (fp32 logits): |err| <= 2e-5 * (|x| . |w_eff|) elementwise, against
    the PACKED (bf16-rounded) effective weights"""
    ratios = []
    for name, k, grid, kern in (("rand_direct", 5, (2, 17, 33), "direct<32,f32,d2s>"), ("rand_persistent", 8, (171, 17, 33), "seg_out<false>")):
        n, h, w = grid
        assert P.seg_out_form(n, h, w, k)["kernel"] == kern
        x0, wgt, bias = seg_out_inputs(K, name, k, grid, rand=True)
        wp, _, be = K.pack_phase_weight(wgt, 64, bias)
        we = wp.view(4 * k, 9, 64).double().permute(0, 2, 1).reshape(4 * k, 64, 3, 3)
        out = Guarded(n * 4 * h * w, k, k, F32)
        K.lib().call("hn_conv_gemm_nt", K.ptr(x0), None, 4, n, h, w, 64, 0, x0.stride(2), 0, 0, n * h * w, K.ptr(wp), 4 * k, 64, 9, K.ptr(be), 0,
                     out.ptr(), 1, 4 * k, 0, -k, None, None)
        torch.cuda.synchronize()
        want = R.depth_to_space(R.conv3x3(x0, we, "clamp") + be.double()).reshape(-1, k)
        scale = R.depth_to_space(R.conv3x3(x0.double().abs(), we.abs(), "clamp") + be.double().abs()).reshape(-1, k)
        r = float(((out.view.double() - want).abs() / scale.clamp(min=1e-30)).max())
        print(f"{name} ({kern}): max |err| / (|x| . |w|) = {r:.3e}")
        assert r <= RAND_TOL, f"{name} ({kern}): max |err| / (|x| . |w|) = {r:.3e} > {RAND_TOL:.0e}"
        out.check(name)
        ratios.append(r)
    print("random ratios (direct, persistent):", ["%.3e" % v for v in ratios])
