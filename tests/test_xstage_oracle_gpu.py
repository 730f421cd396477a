"""The persistent stage launches (csrc/hn_xstage.hip: hn_xstage_fwd / hn_xstage_bwd) against the float64 reference tests/xblock_ref.py
(pinned to oracle.xblock on the CPU by tests/test_xstage_gpu.py), over every shape class hn_xstage_supported admits and its edges.

tests/test_xstage_gpu.py compares the launches with the launch chain (ops.XBlockFn): a misreading of the reference that both share passes
there.  Here every tensor the launches write is held to the reference, TEACHER FORCED: in the forward, block b's reference runs on the
launch's own stored input (out[b - 1]), so every block of an nb = 3 launch is held to the tight bounds; in the backward the gradient
entering an inner block is not stored, so an nb = 3 launch is held tightly on its last block (the one that receives dout) and its final dx
is compared with the reference's three-block composition; per-block backward tightness comes from the nb = 1 runs.

Every output buffer is poisoned with NaN (xstage_*_raw(fill=...)): an element the launch leaves unwritten, or a line read stale before its
write, shows up as a non-finite value or a mismatch instead of passing for the previous step's data.  Where the launch chain covers the
shape (xblock_fusable), it runs on the same inputs against the same reference; both sets of errors are recorded through
tests/test_fullsize2_gpu.py's dump() (fullsize2_xstage_oracle_*.json) and both are held to the same fixed bounds.  Each case runs once.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import xblock_ref as R
from tests.test_fullsize2_gpu import DIN_COS, DIN_L2, PARAM_MAX, dump
from tests.test_fullsize_gpu import ACT_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
STAT_TOL = 5e-3           # BatchNorm batch / running statistics, pooled / hidden / gate vectors (max-norm relative)
GRAD_COS = 0.995          # every gradient: cosine >= GRAD_COS, and
#                           dgb, dpre*, the SE parameter gradients: max-norm relative <= GRAD_TOL;
#                           dz1 / dz2 / dz3: relative L2 <= DIN_L2 -- the reason dx is held in L2 (tests/test_fullsize2_gpu.py cos_l2): an
#                           output within one bf16 ulp of zero flips a ReLU mask between two implementations and moves single elements by
#                           |upstream gradient| (measured max-norm 0.3-0.56 at cosine > 0.9999);
#                           conv weight gradients: max-norm <= PARAM_MAX, the bound the launch chain meets against the oracle in
#                           tests/test_fullsize2_gpu.py (the same flips, summed: the chain measures 0.164 on dw1 here, the persistent path too)
RUN_COS = 0.995           # the final dx of an nb = 3 launch against the reference's three-block composition

# (N, H, W, C, Cs) -> the variant hn_xstage_supported must return (a later envelope change is noticed here)
CASES = {
    (16, 8, 16, 936, 234): 1,      # stage 4 at 512 x 1024
    (16, 10, 10, 936, 234): 1,     # stage 4 at 640 x 640
    (8, 8, 16, 936, 234): 1,       # stage 4, BASELINE config 2
    (16, 16, 32, 376, 94): 2,      # stage 3 at 512 x 1024
    (16, 20, 20, 376, 94): 2,      # stage 3 at 640 x 640
    (8, 16, 32, 376, 94): 2,       # stage 3, config 2
    (8, 1, 1, 64, 16): 1,          # 1 x 1 map: the grouped conv's centre tap only; BatchNorm over 8 values (unbiased factor 8 / 7)
    (16, 1, 1, 64, 16): 1,         # ... over 16 values
    (8, 1, 37, 72, 18): 1,         # one-row map (halo above and below only); C = 72: the last slice holds 8 of 64 channels
    (16, 11, 11, 200, 50): 1,      # HW = 121 < 128, odd sides; 4 slices, the last one 8 channels; row stride 400 B
    (8, 3, 43, 40, 10): 2,         # HW = 129, the first size past variant 1; ragged variant-2 slice
    (8, 1, 128, 8, 2): 2,          # C = 8, Cs = 2 (the minimum); 1 x 128 falls to variant 2 through the halo-tile limit
    (16, 16, 32, 8, 2): 2,         # C = 8 at HW = 512, the variant-2 maximum
    (16, 8, 16, 512, 256): 1,      # Cs = 256, the maximum
    (16, 22, 23, 264, 66): 2,      # odd W, HW = 506 near the variant-2 limit, ragged slice
}
MODE1 = [(16, 8, 16, 936, 234), (16, 11, 11, 200, 50), (8, 3, 43, 40, 10)]
RUNS = [(s, nb, 0) for s in CASES for nb in (1, 3)] + [(s, nb, 1) for s in MODE1 for nb in (1, 3)]


def _params(nb, c, cs, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ps = []
    for _ in range(nb):
        r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)
        bn = lambda: [1.0 + 0.1 * r(c), 0.1 * r(c), 0.05 * r(c), 1.0 + 0.1 * torch.rand(c, generator=g).to(dev)]
        ps += [r(c, c, 1, 1, scale=(2.0 / c) ** 0.5), *bn(), r(c, 8, 3, 3, scale=(2.0 / 72) ** 0.5), *bn(),
               r(cs, c, 1, 1, scale=(1.0 / c) ** 0.5), r(cs, scale=0.1), r(c, cs, 1, 1, scale=(1.0 / cs) ** 0.5), r(c, scale=0.1),
               r(c, c, 1, 1, scale=(2.0 / c) ** 0.5), *bn()]
    return ps


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _cos(a, b):
    return float(F.cosine_similarity(a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten(), dim=0))


def _l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def _coef_ref(ref, ps, k):
    """[4, C] (scale, shift, mean, rstd) of BatchNorm k from the reference's batch statistics (the layout of the launches' coef)"""
    g, b = ps[(1, 6, 15)[k]].double().cpu(), ps[(2, 7, 16)[k]].double().cpu()
    rs = 1.0 / torch.sqrt(ref["var"][k] + EPS)
    return torch.stack([g * rs, b - ref["mean"][k] * g * rs, ref["mean"][k], rs])


class Errs:
    """named errors with their bounds: act / stat (max-norm <= bound), din (cosine + relative L2), grad (cosine + max-norm)"""

    def __init__(self):
        self.e, self.bad = {}, []

    def act(self, name, got, ref, tol=ACT_TOL):
        v = self.e[name] = _rel(got, ref)
        if not v <= tol:
            self.bad.append((name, v))

    def grad(self, name, got, ref, kind="max", tol=GRAD_TOL):
        """kind "max": cosine + max-norm <= tol; "l2": cosine + relative L2 <= tol.  An all-zero reference (an SE layer whose hidden units
        are all inactive) must be matched by an all-zero result."""
        if float(ref.abs().max()) == 0.0:
            m = float(got.detach().abs().max())
            self.e[name] = dict(zero_ref=True, max_abs=m)
            if not m == 0.0:
                self.bad.append((name, "nonzero", m))
            return
        c, m, l2 = _cos(got, ref), _rel(got, ref), _l2(got, ref)
        self.e[name] = dict(cos=c, max=m, rel_l2=l2)
        if not (c >= GRAD_COS and (m if kind == "max" else l2) <= tol):
            self.bad.append((name, c, m, l2))

    def din(self, name, got, ref):
        c, l2 = _cos(got, ref), _l2(got, ref)
        self.e[name] = dict(cos=c, rel_l2=l2, max=_rel(got, ref))
        if not (c >= DIN_COS and l2 <= DIN_L2):
            self.bad.append((name, c, l2))


def _weight_grads(K, inp, a, bg, hid, pooled, dz1, dz2, dz3, dpre2, dpre1, c, cs, grid):
    """the parameter gradients the deferred launches build from what hn_xstage_bwd leaves (ops.xstage.XStageFn.backward's group.add*)"""
    return dict(dw1=K.k_gemm_tn(inp, None, 0, grid, dz1, c, K.kp32(c), 1, c), dw3=K.k_gemm_tn(bg, None, 0, grid, dz3, c, K.kp32(c), 1, c),
                dw2=K.k_gemm_tn(a, None, 5, grid, dz2, c, 64, 9, 8, kh=3),
                dsw2=(dpre2.t() @ hid).view(c, cs, 1, 1), dsb2=dpre2.sum(0), dsw1=(dpre1.t() @ pooled).view(cs, c, 1, 1), dsb1=dpre1.sum(0))


def _finite(d, where):
    for k, v in d.items():
        if isinstance(v, torch.Tensor):
            assert bool(torch.isfinite(v.float()).all()), (where, k, int((~torch.isfinite(v.float())).sum()))


@pytest.mark.parametrize("shape,nb,mode", RUNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_persistent_launch_vs_float64_reference(shape, nb, mode):
    import __graft_entry__ as G
    G.build()
    from multitask_hydranet_amd import ops as K
    import multitask_hydranet_amd.ops.xstage as XS
    from multitask_hydranet_amd._lib import lib
    n, h, w, c, cs = shape
    assert lib().query("hn_xstage_supported", n, h, w, c, cs) == CASES[shape]
    dev = torch.device("cuda:0")
    seed = n * 7 + h * 131 + w * 17 + c + nb
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=gen).to(torch.bfloat16).relu_().to(dev)
    dout = (torch.randn(n, h, w, c, generator=gen) * 0.01).to(torch.bfloat16).to(dev)
    ps = _params(nb, c, cs, dev, seed + 1)
    p0 = [t.clone() for t in ps]                                   # the running statistics before the launch updates them in place
    K.clear_pack_cache()
    with torch.no_grad():
        r = XS.xstage_forward_raw(x, ps, EPS, MOM, mode=mode, fill=float("nan"))
        assert XS.xstage_status(dev) == 0
        sws = [(ps[b * 19 + 10], ps[b * 19 + 12]) for b in range(nb)]
        rb = XS.xstage_backward_raw(dout, r, r["packs"], sws, mode=mode, fill=float("nan"))
        assert XS.xstage_status(dev) == 0
    _finite(r, "forward")
    _finite(rb, "backward")
    grid = (n, h, w)
    inputs = [x] + [r["out"][b - 1] for b in range(1, nb)]
    blk = lambda b: p0[b * 19:(b + 1) * 19]
    refs = [R.forward(inputs[b], blk(b), EPS, MOM) for b in range(nb)]
    # backward reference, composed teacher-forced: block b's upstream is block b + 1's reference input gradient
    ups, grefs = [None] * nb, [None] * nb
    up = dout
    for b in reversed(range(nb)):
        ups[b] = up
        grefs[b] = R.backward(refs[b], up)
        up = grefs[b]["dx"]

    P = Errs()
    for b in range(nb):
        ref = refs[b]
        for k in ("z1", "a", "z2", "bg", "z3", "out"):
            P.act(f"b{b}.{k}", r[k][b], ref[k])
        for k in range(3):
            cr = _coef_ref(ref, blk(b), k)
            P.act(f"b{b}.bn{k + 1}.mean", r["coef"][b, k, 2], ref["mean"][k], STAT_TOL)
            P.act(f"b{b}.bn{k + 1}.var", 1.0 / r["coef"][b, k, 3].double() ** 2 - EPS, ref["var"][k], STAT_TOL)
            P.act(f"b{b}.bn{k + 1}.coef", r["coef"][b, k], cr, STAT_TOL)
        for i, nm in enumerate(R.NAMES):
            if nm in R.RUNNING:
                P.act(f"b{b}.{nm}", ps[b * 19 + i], ref["running"][nm], STAT_TOL)
        for k in ("pooled", "hid", "gate"):
            P.act(f"b{b}.{k}", r[k][b], ref[k], STAT_TOL)
    # backward: the last block tightly (it receives dout itself)
    b = nb - 1
    gr = grefs[b]
    for k in ("dz1", "dz2", "dz3"):
        P.grad(f"b{b}.{k}", rb[k][b], gr[k], "l2", DIN_L2)
    for k in ("dpre2", "dpre1"):
        P.grad(f"b{b}.{k}", rb[k][b], gr[k])
    P.grad(f"b{b}.dgb", rb["dgb"][b], gr["dgb"])
    wg = _weight_grads(K, inputs[b], r["a"][b], r["bg"][b], r["hid"][b], r["pooled"][b], rb["dz1"][b], rb["dz2"][b], rb["dz3"][b],
                       rb["dpre2"][b], rb["dpre1"][b], c, cs, grid)
    for k, v in wg.items():
        P.grad(f"b{b}.{k}", v.reshape(gr[k].shape), gr[k], tol=PARAM_MAX if k in ("dw1", "dw2", "dw3") else GRAD_TOL)
    if nb == 1:
        P.din("dx", rb["dx"], grefs[0]["dx"])
    else:
        v = P.e["dx_vs_composition_cos"] = _cos(rb["dx"], grefs[0]["dx"])
        if not v >= RUN_COS:
            P.bad.append(("dx_vs_composition_cos", v))

    # the launch chain on the same inputs, teacher-forced the same way (fresh copies of the initial parameters)
    C = None
    if K.xblock_fusable(x, p0[0], 1, True, False):
        C = Errs()
        for b in range(nb):
            pc = [t.clone().requires_grad_(R.NAMES[i] in R.GRADS) for i, t in enumerate(blk(b))]
            t = inputs[b].clone().requires_grad_(True)
            o = K.XBlockFn.apply(t, *pc, EPS, MOM, True, 1, None, None, None, None, None, None)
            _, z1, a, z2, z3, out, c1, c2, c3, pooled, hid, gate, _, _, bg = o.grad_fn.saved_tensors[:15]
            o.backward(ups[b].to(dev, torch.bfloat16))
            ref, gr = refs[b], grefs[b]
            for k, v in dict(z1=z1, a=a, z2=z2, bg=bg, z3=z3, out=out).items():
                C.act(f"b{b}.{k}", v, ref[k])
            for k, cf in enumerate((c1, c2, c3)):
                C.act(f"b{b}.bn{k + 1}.mean", cf[2], ref["mean"][k], STAT_TOL)
                C.act(f"b{b}.bn{k + 1}.var", 1.0 / cf[3].double() ** 2 - EPS, ref["var"][k], STAT_TOL)
                C.act(f"b{b}.bn{k + 1}.coef", cf, _coef_ref(ref, blk(b), k), STAT_TOL)
            for i, nm in enumerate(R.NAMES):
                if nm in R.RUNNING:
                    C.act(f"b{b}.{nm}", pc[i], ref["running"][nm], STAT_TOL)
            for k, v in dict(pooled=pooled, hid=hid, gate=gate).items():
                C.act(f"b{b}.{k}", v, ref[k], STAT_TOL)
            C.grad(f"b{b}.dgb", torch.stack([torch.stack([pc[i].grad, pc[i + 1].grad]) for i in (1, 6, 15)]), gr["dgb"])
            for i, nm in enumerate(R.NAMES):
                if nm in R.GRADS and nm[0] in "ws":
                    C.grad(f"b{b}.{R.GRADS[nm]}", pc[i].grad, gr[R.GRADS[nm]], tol=PARAM_MAX if nm[0] == "w" else GRAD_TOL)
            C.din(f"b{b}.dx", t.grad, gr["dx"])

    name = "x".join(map(str, shape)) + f"_nb{nb}_mode{mode}"
    res = dict(shape=list(shape), nb=nb, mode=mode, variant=CASES[shape], persistent=P.e, persistent_fails=P.bad,
               chain=C.e if C else None, chain_fails=C.bad if C else None)
    dump(f"xstage_oracle_{name}", res)
    assert XS.xstage_status(dev) == 0
    assert not P.bad, ("persistent", P.bad)
    assert C is None or not C.bad, ("chain", C.bad)
