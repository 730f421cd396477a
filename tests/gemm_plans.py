"""Test-side restatement of the host planning of the conv GEMM families in csrc/hn_gemm.hip (wgrad_plan, tn_tiles, patch_tiles,
wgrad_reduce_kind, wgrad_group_plan, gconv_group_plan, pick_bc, small_tile, launch_direct's tile choice), with the shipped knob values.
tests/test_gemm_plans_cpu.py holds it to the library's own plan queries and to the instantiations the source launches;
tests/test_gemm_exact_gpu.py uses it to assert which branch every exact case lands on, and to name the split / patch / tile of a
mismatching element."""
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
