"""Test-side restatement of the host planning of the conv GEMM families in csrc/hn_gemm.hip (wgrad_plan, tn_tiles, patch_tiles,
wgrad_reduce_kind, wgrad_group_plan, gconv_group_plan, pick_bc, small_tile, launch_direct's tile choice), with the shipped knob values.
tests/test_gemm_plans_cpu.py holds it to the library's own plan queries and to the instantiations the source launches;
tests/test_gemm_exact_gpu.py uses it to assert which branch every exact case lands on, and to name the split / patch / tile of a
mismatching element.  launch_direct's form choice beyond the plain call (phase, depth-to-space, arg-max and fold forms, the two
persistent seg-head predicates with their patch count and threshold) and the tiling of the plain-row entry points (imgw, lvl, lvlout,
stat3) serve tests/test_gemm_forms_exact_gpu.py and tests/test_gemm_epilogue_exact_gpu.py in the same way."""
import os
import re

KNOB_TN_TARGET = 2048        # g_hn_knob[0]: ~4 row-gather workgroups per CU
KNOB_TN_MIN_ROWS = 256       # g_hn_knob[1]: at least 256 rows per split
KNOB_SMALL_M = 8192          # g_hn_knob[4]
KNOB_SMALL_M_128 = 262144    # g_hn_knob[5]
KNOB_PATCH_TARGET = 256      # g_hn_knob[12]
KNOB_GCONV_TARGET = 384      # g_hn_knob[13]

GEMM_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multitask_hydranet_amd", "csrc", "hn_gemm.hip")


def cdiv(a, b):
    return -(-a // b)


def kp32(c):
    return cdiv(c, 32) * 32


def tn_tiles(nout, kp):
    bc = 16 if nout <= 16 else (32 if nout <= 32 else (64 if nout <= 64 else 128))
    bn = 32 if kp <= 32 else (64 if kp <= 64 else 128)
    if bc == 16 and bn < 64:
        bn = 64
    return bc, bn


def patch_tiles(nout, kp):
    """-> (bc, ci, ksplit)"""
    if kp <= 32 and nout > 64:
        return 128, 32, 2
    if nout <= 16:
        return 16, 64, 2
    if nout <= 32:
        return 32, 64, 2
    if nout <= 64:
        return 64, 64, 2
    return 128, 64, 1


def wgrad_plan(mode, n, h, w, m, nout, kp, taps, phase_span=0):
    """the plan of hn_conv_gemm_tn / _bias / _deferred / _phase (API mode; phase_span > 0: hn_conv_gemm_tn_phase).
    -> dict(patch, bc, bn, ksplit, splits, rows_per_split, patches, ws_bytes, kernel, reduce)"""
    diag = mode == 5
    gmode = 2 if mode in (4, 5) else mode
    if phase_span:
        gmode = 2
    q = dict(patch=gmode == 2 and kp >= 32)
    if q["patch"]:
        bc, bn, ks = patch_tiles(nout, kp)
        if diag or (phase_span and phase_span < bc):
            bc, bn, ks = 64, 64, 2
        tiles = cdiv(nout, bc) * cdiv(kp, bn)
        patches = n * cdiv(h, 8) * cdiv(w, 16)
        want = cdiv(KNOB_PATCH_TARGET, tiles)
        if bc <= 64 and 2 * want * ks * nout * taps * kp * 4 <= (64 << 20):
            want *= 2
        want = min(want, patches // 2)
        want = max(want, 1)
        pps = cdiv(patches, want)
        splits = cdiv(patches, pps) * ks
        q.update(bc=bc, bn=bn, ksplit=ks, splits=splits, rows_per_split=pps, patches=patches)
        if diag:
            kern = "patch<64,64>"
        elif phase_span:
            kern = "patch<128,32,1>" if (bc, bn) == (128, 32) else ("patch<128,64,1>" if bc == 128 else "patch<64,64,1>")
        else:
            kern = "patch<%d,%d>" % (bc, bn)
    else:
        bc, bn = tn_tiles(nout, kp)
        tiles = cdiv(nout, bc) * cdiv(kp, bn) * taps
        want = cdiv(KNOB_TN_TARGET, tiles)
        if tiles <= 2:
            want = 512 // tiles
        want = min(want, cdiv(m, KNOB_TN_MIN_ROWS))
        want = max(want, 1)
        rps = cdiv(cdiv(m, want), 64) * 64
        q.update(bc=bc, bn=bn, ksplit=1, splits=cdiv(m, rps), rows_per_split=rps, patches=0)
        kern = "tn<%d,%d>" % (bc, bn)
    q["ws_bytes"] = q["splits"] * nout * taps * kp * 4 + q["splits"] * nout * 4
    q["kernel"] = kern
    q["reduce"] = reduce_kind(q, diag, nout, kp, taps)
    return q


def reduce_kind(q, grouped, nout, kp, taps):
    """-1 wgrad_reduce9_kernel, 0 wgrad_reduce4_kernel, 1 wgrad_reduce_kernel, 2 gconv_diag_extract_kernel"""
    if grouped:
        return 2
    if q["patch"] and taps == 9 and q["splits"] <= 64:
        return -1
    return 0 if (q["splits"] <= 128 and nout * taps * kp >= 65536) else 1


REDUCE_NAMES = {-1: "wgrad_reduce9_kernel", 0: "wgrad_reduce4_kernel", 1: "wgrad_reduce_kernel", 2: "gconv_diag_extract_kernel"}


def split_of_row(q, row, n=None, h=None, w=None):
    """which pixel split (row-gather plans) or patch split (patch plans) an output row of the GEMM's pixel dimension falls in"""
    if not q["patch"]:
        return row // q["rows_per_split"]
    img, r = divmod(row, h * w)
    y, x = divmod(r, w)
    patch = (img * cdiv(h, 8) + y // 8) * cdiv(w, 16) + x // 16
    return patch // q["rows_per_split"]


def group_plan(jobs):
    """hn_wgrad_group: jobs = [(mode, n, h, w, cin, nout, m)] -> dict(bc, bn, kernel, splits[], rps[], reduce[] (None: unsplit), ws_bytes)"""
    max_nout = max(j[5] for j in jobs)
    max_kp = max(kp32(j[4]) for j in jobs)
    bc, bn = tn_tiles(max_nout, max_kp)
    tiles = sum(cdiv(j[5], bc) * cdiv(kp32(j[4]), bn) for j in jobs)
    want = 1 if 4 * tiles >= 3 * KNOB_TN_TARGET else cdiv(KNOB_TN_TARGET, tiles)
    splits, rps, red, ws = [], [], [], 0
    for (mode, n, h, w, cin, nout, m) in jobs:
        wj = max(min(want, cdiv(m, KNOB_TN_MIN_ROWS)), 1)
        r = cdiv(cdiv(m, wj), 64) * 64
        s = cdiv(m, r)
        splits.append(s)
        rps.append(r)
        cols = nout * kp32(cin)
        red.append(None if s == 1 else (0 if (s <= 128 and cols >= 65536) else 1))
        if s > 1:
            ws += s * cols
    kern = "tng_regs<128,128>" if (bc, bn) == (128, 128) else "tng<%d,%d>" % (bc, bn)
    return dict(bc=bc, bn=bn, kernel=kern, splits=splits, rps=rps, reduce=red, ws_bytes=ws * 4 + 64)


def gconv_group_plan(jobs):
    """hn_gconv_wgrad_group: jobs = [(n, h, w, c)] -> dict(splits[] (patch splits; slabs = 2x), pps[], ws_bytes)"""
    tiles = sum(cdiv(c, 64) for (_, _, _, c) in jobs)
    want = cdiv(KNOB_GCONV_TARGET, tiles)
    splits, pps, ws = [], [], 0
    for (n, h, w, c) in jobs:
        patches = n * cdiv(h, 8) * cdiv(w, 16)
        wj = max(min(want, patches // 2), 1)
        p = cdiv(patches, wj)
        s = cdiv(patches, p)
        splits.append(s)
        pps.append(p)
        ws += s * 2 * c * 576
    return dict(splits=splits, pps=pps, ws_bytes=ws * 4 + 64)


# ---- forward (NT) side ----------------------------------------------------------------------------------------------------------
def pick_bc(nout):
    if nout <= 16:
        return 16
    if nout <= 32:
        return 32
    if nout <= 64:
        return 64
    return 64 if cdiv(nout, 64) * 64 < cdiv(nout, 128) * 128 else 128


def small_tile(m, nout):
    return nout > 64 and (m <= KNOB_SMALL_M or (m <= KNOB_SMALL_M_128 and nout <= 128))


def nt_kernel(mode, m, nout, kp, taps, stats=False):
    """the GEMM instantiation run_gemm_nt launches for a plain call (no xform / addend / rpi / phase): modes 0 / 1, and 3x3 modes 2..4
    WITH statistics (without them they go to the direct kernel)"""
    if small_tile(m, nout):
        if mode <= 1 and taps == 1 and kp >= 512:
            return "nt<64,64,kg2>"
        return "nt<64,64>"
    return "nt<%d,128>" % pick_bc(nout)


def direct_kernel(mode, nout, kp, out_f32, ldc, aligned=True):
    """conv3x3_direct_kernel form launch_direct takes (no phase / d2s / persistent forms): -> (name, bc)"""
    diag = mode == 5
    bc = 64 if diag else (16 if nout <= 16 else (32 if nout <= 32 else (64 if nout <= 64 else 128)))
    staged_ok = ldc % 8 == 0 and nout % 8 == 0 and aligned
    if bc >= 64 and not out_f32 and not staged_ok:
        assert not diag
        bc = 32
    wpre = not diag and kp <= 64 and 9 * bc * 128 <= 32768
    narrow = bc == 64 and not out_f32 and not diag and not wpre and kp <= 32
    if narrow:
        return "direct_narrow<64>", bc
    return "direct<%d,%s%s>" % (bc, "f32" if out_f32 else "bf16", ",wpre" if wpre else ""), bc


def stat_tile(m, nout):
    return 64 if small_tile(m, nout) else 128


# ---- launch_direct's form choice beyond the plain call: phase / depth-to-space / arg-max / fold forms, the persistent seg-head kernels --------
PERSIST_MIN_PATCHES = 1024   # `npatch >= 1024` of both persistent predicates
ACT_NONE, ACT_ELU = 0, 3


def npatch(n, h, w):
    """16 x 16 output patches of the (low-resolution) grid: what launch_direct compares with the persistent threshold"""
    return n * cdiv(h, 16) * cdiv(w, 16)


def seg_phase64_persistent(n, h, w, nout, kp, c0, act, phase_mode, phase_span, d2s, out_f32=False, addend=False, stats=False, clamp=True,
                           ld0=None, ldc=64, aligned=True):
    """the predicate of seg_phase64_conv_kernel (the last decoder block's 64 -> 4 x 64 phase-form conv)"""
    ld0 = c0 if ld0 is None else ld0
    return (clamp and not out_f32 and d2s == 64 and phase_mode == 1 and phase_span == 64 and kp == 64 and c0 == 64 and nout == 256
            and not stats and not addend and act in (ACT_ELU, ACT_NONE) and ld0 % 8 == 0 and ldc % 8 == 0 and ldc >= 64 and aligned
            and npatch(n, h, w) >= PERSIST_MIN_PATCHES)


def seg_out_persistent(n, h, w, nout, kp, c0, act, phase_mode, d2s, out_f32=True, addend=False, stats=False, clamp=True, ld0=None,
                       aligned=True):
    """the predicate of seg_out_conv_kernel<amax> (the seg output conv, fp32 depth-to-space logits or their arg-max)"""
    ld0 = c0 if ld0 is None else ld0
    return bool(clamp and out_f32 and d2s and kp == 64 and c0 == 64 and nout == 4 * d2s and nout <= 32 and not stats and not addend
                and phase_mode == 0 and act == ACT_NONE and ld0 % 8 == 0 and (32 * d2s) % 4 == 0 and (2 * w * d2s) % 4 == 0 and aligned
                and npatch(n, h, w) >= PERSIST_MIN_PATCHES)


def persistent_ranges(n, h, w, kernel):
    """(patches per workgroup, workgroups [per phase for seg_phase64]): seg_phase64 walks 64 patch ranges x 4 phases, seg_out 256 ranges"""
    npt = npatch(n, h, w)
    ppw = cdiv(npt, 64 if kernel == "seg_phase64" else 256)
    return ppw, cdiv(npt, ppw)


def direct_form(mode, n, h, w, nout, kp, c0, out_f32, ldc, act=ACT_NONE, phase_mode=0, phase_span=0, d2s=0, amax=False, fold=0,
                addend=False, stats=False, aligned=True, ld0=None):
    """the kernel and form launch_direct takes for any direct 3x3 launch.  n, h, w: the grid the kernel runs on (mode 4 phase / d2s forms:
    the LOW-resolution grid; mode 3: the padded grid).  -> dict(kernel, bc, wpre, persistent) with kernel one of
    seg_phase64 | seg_out<true|false> | direct<bc,f32|bf16[,wpre][,phase|,dphase][,d2s][,amax][,foldN]> | direct_narrow<64>"""
    diag = mode == 5
    clamp = mode == 4
    if not diag and seg_phase64_persistent(n, h, w, nout, kp, c0, act, phase_mode, phase_span, d2s, out_f32, addend, stats, clamp, ld0, ldc, aligned):
        return dict(kernel="seg_phase64", bc=64, wpre=False, persistent=True)
    if not diag and seg_out_persistent(n, h, w, nout, kp, c0, act, phase_mode, d2s, out_f32, addend, stats, clamp, ld0, aligned):
        return dict(kernel="seg_out<%s>" % ("true" if amax else "false"), bc=32, wpre=False, persistent=True)
    bc = 64 if diag else (16 if nout <= 16 else (32 if nout <= 32 else (64 if nout <= 64 else 128)))
    if phase_mode == 1 and phase_span < bc:
        bc = 64                                               # a cout tile must lie inside one phase
    staged_ok = ldc % 8 == 0 and nout % 8 == 0 and aligned and (not d2s or (d2s % 8 == 0 and nout % bc == 0))
    if bc >= 64 and not out_f32 and not staged_ok:
        assert not diag
        bc = 32
    nsteps = 4 if phase_mode else 9
    wpre = not diag and kp <= 64 and nsteps * bc * 128 <= 32768
    narrow = bc == 64 and not out_f32 and not diag and not wpre and kp <= 32 and nsteps == 9
    if narrow:
        return dict(kernel="direct_narrow<64>", bc=bc, wpre=True, persistent=False)
    tags = ["f32" if out_f32 else "bf16"]
    if wpre:
        tags.append("wpre")
    if phase_mode:
        tags.append("phase" if phase_mode == 1 else "dphase")
    if d2s and not phase_mode:
        tags.append("d2s")
    if amax:
        tags.append("amax")
    if fold:
        tags.append("fold%d" % fold)
    return dict(kernel="direct<%d,%s>" % (bc, ",".join(tags)), bc=bc, wpre=wpre, persistent=False)


def phase_fwd_form(n, h, w, k, c0, act, addend=False, ldc=None):
    """hn_conv3x3_phase mode 4 on the low-resolution grid (n, h, w)"""
    return direct_form(4, n, h, w, 4 * k, kp32(c0), c0, False, ldc or k, act=act, phase_mode=1, phase_span=k, d2s=k, addend=addend)


def seg_out_form(n, h, w, k, c0=64, amax=False):
    """hn_conv_gemm_nt mode 4 with img_stride = -k (fp32 depth-to-space logits) / hn_conv3x3_out_argmax"""
    return direct_form(4, n, h, w, 4 * k, kp32(c0), c0, True, 4 * k, d2s=k, amax=amax)


def phase_dgrad_form(n, h, w, k, nout, fold=0, ldc=None):
    """hn_conv3x3_phase mode 3 / the phase form of hn_conv3x3_dgrad_fold on the padded grid (n, h + 2, w + 2) of the low-resolution map"""
    return direct_form(3, n, h + 2, w + 2, nout, kp32(4 * k), 4 * k, False, ldc or nout, phase_mode=2, phase_span=k, fold=fold)


def fold_form(n, h, w, cz, nout, phase_k, plain, s2d):
    """dgrad_fold_impl: -> (status, form) with status 0 ok / 1 HN_ERR_ARG / 3 HN_ERR_UNSUPPORTED (the refusals the header documents) and
    form = the GemmNT::fold value with the direct kernel's name"""
    if s2d and (h % 2 or w % 2):
        return 1, None
    if phase_k and (cz != 4 * phase_k or phase_k % 64):
        return 1, None
    if nout % 8 or nout <= 32 or h < 4 or w < 4:
        return 3, None
    fold = 1 if not s2d else (3 if plain else 2)
    if phase_k:
        return 0, phase_dgrad_form(n, h, w, phase_k, nout, fold=fold)
    return 0, direct_form(3, n, h + 2, w + 2, nout, kp32(cz), cz, False, nout, fold=fold)


def nt_entry_kernel(entry, m, nout, kp):
    """the gemm_nt_kernel tiling of the plain-row entry points hn_conv_gemm_nt_imgw / _lvl / _lvlout / _stat3 (all mode 0, one tap,
    through run_gemm_nt's tile choice); stat3 exists on the 64 x 64 tiling only (None: HN_ERR_ARG)"""
    assert entry in ("imgw", "lvl", "lvlout", "stat3")
    if entry == "stat3" and not small_tile(m, nout):
        return None
    return nt_kernel(0, m, nout, kp, 1)


# ---- what the product source launches ------------------------------------------------------------------------------------------
def product_source(path=GEMM_SRC):
    """hn_gemm.hip as the product library compiles it: every `#ifdef HN_TUNING` branch dropped (its `#else` branch kept); other
    conditionals are kept whole"""
    out, stack = [], []
    for line in open(path).read().splitlines():
        s = line.strip()
        if s.startswith("#if"):
            stack.append("tuning" if s.startswith("#ifdef HN_TUNING") else "other")
            continue
        if s.startswith("#else") and stack:
            stack[-1] = "product" if stack[-1] == "tuning" else stack[-1]
            continue
        if s.startswith("#endif") and stack:
            stack.pop()
            continue
        if "tuning" not in stack:
            out.append(line)
    return "\n".join(out)


def product_knobs(path=GEMM_SRC):
    src = product_source(path)
    m = re.search(r"extern const long g_hn_knob\[20\]\s*=\s*\{([^}]*)\}", src)
    return [int(v) for v in m.group(1).split(",")]


def product_instantiations(path=GEMM_SRC):
    """the kernel instantiations of the three wgrad families the product library can launch, in plan names:
    tn<bc,bn> (TN_CASE of run_gemm_tn), tng<bc,bn> / tng_regs<128,128> (hn_wgrad_group), patch<...> (wgrad3x3_patch_kernel launches)"""
    src = product_source(path)
    body = lambda name: src[src.index(name):src.index("\n}\n", src.index(name))]
    tn = body("static int run_gemm_tn(")
    grp = body('extern "C" int hn_wgrad_group(')
    out = set()
    for a, b in re.findall(r"\bTN_CASE\((\d+),\s*(\d+),", tn):
        out.add("tn<%s,%s>" % (a, b))
    for a, b in re.findall(r"\bTNG_CASE\((\d+),\s*(\d+),", grp):
        out.add("tng<%s,%s>" % (a, b))
    if re.search(r"g\.bc == 128 && g\.bn == 128 && variant != 1\)\s*hipLaunchKernelGGL\(\(gemm_tn_group_kernel<128, 128, 2, 2, 64, -2>\)", grp):
        out.add("tng_regs<128,128>")
        if product_knobs(path)[10] != 1:            # variant = knob 10, a constant 0: TNG_CASE(128, 128, ...) behind the else is never taken
            out.discard("tng<128,128>")
    for args in re.findall(r"hipLaunchKernelGGL\(\(wgrad3x3_patch_kernel<([\d,\s]+)>\)", tn):
        out.add("patch<%s>" % ",".join(a.strip() for a in args.split(",")))
    for name, kind in REDUCE_LAUNCHES.items():
        if re.search(r"hipLaunchKernelGGL\(%s\b" % name, tn):
            out.add("reduce%d" % kind)
    return out


REDUCE_LAUNCHES = {"wgrad_reduce9_kernel": -1, "wgrad_reduce4_kernel": 0, "wgrad_reduce_kernel": 1, "gconv_diag_extract_kernel": 2}
