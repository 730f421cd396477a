"""Inputs of tests/test_lovasz_exact_gpu.py, built on the host from seeded torch generators (the same arrays on every machine), with the
valid count V and the set of present classes each case is DESIGNED to have.  tests/test_lovasz_ref_cpu.py asserts those, the palettes'
gaps and the saturated inputs' exact keys without a GPU; the GPU file asserts them again on the device's own counts.

Logit kinds
  palette      every pixel's logits are one of `rows` rows of torch.randn * 2: the errors |fg - p_c| of a class are either equal bit for
               bit (long runs of exact ties, which the stable order -- pixel index ascending -- decides) or at least 1e-4 apart, far
               above what fp32 can reorder; so the float64 stable order IS the device's order and the payload is compared exactly
  saturated    N(0, 1) logits with one class ahead by 200: exp(-200) underflows, every key is exactly 0.0 or 1.0, every item of a radix
               pass falls into one digit bin; the order is compared exactly (float64 d rounded to float32)
  continuous   N(0, 2) logits: all 30 key bits vary; near-equal floats cannot be predicted, so the sort is held to its properties only

Labels are patterns of the flattened pixel index, so V is a number one can check by hand."""
import numpy as np
import torch

from tests import lovasz_ref as R

IGNORE = 255
TILE = R.TILE
EDGE_P = (1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 5)
MASKS3 = ((1, 1, 1), (1, 0, 1), (0, 0, 1), (0, 0, 0))
# palette seeds per (rows, C): the gap of every one is asserted >= 1e-4 by test_lovasz_ref_cpu.py (not every seed passes)
# (with 15 or 16 classes most probabilities are tiny and bunch up near 0: none of the seeds 0..2999 passes with 12 rows, so those take 6)
PALETTES = {(12, 5): 5, (6, 5): 0, (12, 2): 5, (6, 15): 20, (6, 16): 29}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def palette(rows, c):
    return torch.randn((rows, c), generator=_gen(PALETTES[(rows, c)])) * 2.0


def palette_gap(pal):
    """smallest distance between two distinct values of {p_c} u {1 - p_c} (float64 softmax of the palette rows), over the classes"""
    p = R.softmax64(pal.numpy())
    gap = np.inf
    for k in range(p.shape[1]):
        v = np.unique(np.concatenate([p[:, k], 1.0 - p[:, k]]))
        gap = min(gap, float(np.diff(v).min()))
    return gap


class Case:
    """logits fp32 [n, h, w, c], labels float32 | int64 [n, h, w], mask (tuple of n 0/1, or None), the designed V and present classes
    (under the mask), ld* row strides (None = dense)"""

    def __init__(self, name, logits, labels, kind, V, present, mask=None, ldl=None, ldd=None, ldz=None):
        self.name, self.kind, self.V, self.present, self.mask = name, kind, V, tuple(present), mask
        self.logits = np.ascontiguousarray(logits, np.float32)
        self.labels = np.ascontiguousarray(labels)
        assert self.labels.dtype in (np.float32, np.int64)
        self.n, self.h, self.w, self.c = self.logits.shape
        self.hw, self.P = self.h * self.w, self.n * self.h * self.w
        self.ldl, self.ldd, self.ldz = ldl or self.c, ldd or self.c, ldz or 4 * self.c
        self.s2d = self.h % 2 == 0 and self.w % 2 == 0

    def with_mask(self, mask, V, present):
        return Case(f"{self.name} mask {mask}", self.logits, self.labels, self.kind, V, present, mask, self.ldl, self.ldd, self.ldz)

    def effective(self):
        """-> (lab int64 [P] as the kernels read the labels -- a float label truncates toward zero, like .long() --, valid bool [P])"""
        lab = self.labels.reshape(-1).astype(np.int64)
        valid = lab != IGNORE
        if self.mask is not None:
            valid &= np.repeat(np.asarray(self.mask, bool), self.hw)
        return lab, valid

    def observed(self):
        """-> (V, present classes) of the arrays as built"""
        lab, valid = self.effective()
        return int(valid.sum()), tuple(k for k in range(self.c) if (valid & (lab == k)).any())

    def order(self, k, d=None):
        """the expected sorted payload of class k, u32 [P] (palette and saturated cases): valid pixels by error descending, ties by
        pixel index ascending, then the ignored pixels by index (d: key_d(...) of class k, if the caller has it)"""
        assert self.kind in ("palette", "saturated")
        lab, valid = self.effective()
        if d is None:
            d = R.key_d(self.logits.reshape(self.P, self.c), lab, k)
        if self.kind == "saturated":
            d = d.astype(np.float32).astype(np.float64)          # exactly 0.0 or 1.0 (asserted on the CPU)
        idx = np.flatnonzero(valid)
        e = 1.0 - d[idx]
        pix = np.concatenate([idx[np.argsort(-e, kind="stable")], np.flatnonzero(~valid)])
        return (pix | ((valid[pix] & (lab[pix] == k)).astype(np.int64) << 31)).astype(np.uint32)


def _logits(kind, n, h, w, c, seed, rows=12):
    g = _gen(seed)
    if kind == "palette":
        return palette(rows, c)[torch.randint(0, rows, (n, h, w), generator=g)].numpy()
    if kind == "continuous":
        return (torch.randn((n, h, w, c), generator=g) * 2.0).numpy()
    assert kind == "saturated"
    x = torch.randn((n, h, w, c), generator=g)
    win = torch.randint(0, c, (n, h, w, 1), generator=g)
    return x.scatter_add(3, win, torch.full((n, h, w, 1), 200.0)).numpy()


def _rand_labels(n, h, w, c, seed):
    return torch.randint(0, c, (n, h, w), generator=_gen(seed + 1000)).numpy().astype(np.int64)


def _typed(lab, tf):
    return lab.astype(np.float32) if tf else lab.astype(np.int64)


def edge_case(P, tf=None):
    """all P pixels valid, C = 5, palette logits; an even P is a 2 x P/2 map when P/2 is even (space-to-depth), else 1 x P"""
    h, w = (2, P // 2) if P % 4 == 0 else (1, P)
    lab = _rand_labels(1, h, w, 5, P)
    if P == 1:
        lab[:] = 2
    tf = P % 2 == 1 if tf is None else tf
    return Case(f"edge P={P}", _logits("palette", 1, h, w, 5, P), _typed(lab, tf), "palette", P, (2,) if P == 1 else range(5))


def tile_edge_valid(extra):
    """two tiles of pixels (2 x 64 x 128), every odd pixel ignored: V = 8192 is exactly one tile and the second sorted tile holds
    ignored pixels only; extra = 1 makes pixel 1 valid as well: V = 8193, one valid item in the second tile"""
    lab = _rand_labels(2, 64, 128, 5, 77).reshape(-1)
    lab[1::2] = IGNORE
    if extra:
        lab[1] = 4
    return Case(f"V={TILE + extra} of P={2 * TILE}", _logits("palette", 2, 64, 128, 5, 78), _typed(lab.reshape(2, 64, 128), extra), "palette",
                TILE + extra, range(5))


def saturated_case():
    """P = 3 * 8192 + 5, all valid.  Three of four pixels are labelled one class past the winner, so that for every class the run of
    keys 0.0 (a fg pixel of a losing class, a bg pixel of the winner) is longer than a tile, as the run of keys 1.0 is"""
    P = 3 * TILE + 5
    x = _logits("saturated", 1, 1, P, 5, 31)
    lab = _rand_labels(1, 1, P, 5, 31)
    lab = np.where(np.arange(P).reshape(1, 1, P) % 4 != 0, (x.argmax(-1) + 1) % 5, lab)
    return Case("saturated", x, _typed(lab, True), "saturated", P, range(5))


def continuous_case(P, c, tf):
    return Case(f"continuous P={P} C={c}", _logits("continuous", 1, 1, P, c, 400 + c), _typed(_rand_labels(1, 1, P, c, 400 + c), tf),
                "continuous", P, range(c))


def class_count_case(c, kind):
    """P = 8193 (one pixel in the second tile) at C = 2, 15, 16 (generic kernels; 16 takes the key kernel's LDS opt-in, 15 is the largest
    count that does not) and C = 5 (templated kernels), with padded rows on every operand"""
    P = TILE + 1
    lab = _rand_labels(1, 1, P, c, 500 + c)
    return Case(f"C={c} {kind}", _logits(kind, 1, 1, P, c, 500 + c, rows=6 if c > 5 else 12), _typed(lab, c % 2), kind, P, range(c),
                ldl=c + 3, ldd=c + 1)


def stride_case(ldz_extra):
    """N = 2, 66 x 64 (8448 pixels: the second tile holds 256), C = 5: ldl = C + 3, ldd = C + 1, ldz = 4C or 4C + 4; every 7th pixel ignored"""
    n, h, w, c = 2, 66, 64, 5
    lab = _rand_labels(n, h, w, c, 61).reshape(-1)
    lab[3::7] = IGNORE
    return Case(f"strides ldz=4C+{ldz_extra}", _logits("palette", n, h, w, c, 62), _typed(lab.reshape(n, h, w), True), "palette",
                n * h * w - len(range(3, n * h * w, 7)), range(c), ldl=c + 3, ldd=c + 1, ldz=4 * c + ldz_extra)


def label_forms_case(tf):
    """N = 2, 24 x 32 (1536 pixels), C = 5, by pixel index i: 255 (ignored) at i % 7 == 3, else -1 at i % 11 == 5, else C + 2 at
    i % 13 == 2, else 254 at i % 17 == 1 (background for every class, valid: only 255 is ignored), else a class id -- as float32 the
    class-2 pixels at i % 3 == 0 are written 2.7, which truncates to 2"""
    n, h, w, c = 2, 24, 32, 5
    P = n * h * w
    i = np.arange(P)
    lab = _rand_labels(n, h, w, c, 91).reshape(-1)
    cls2 = (lab == 2) & (i % 3 == 0)
    lab = np.where(i % 17 == 1, 254, lab)
    lab = np.where(i % 13 == 2, c + 2, lab)
    lab = np.where(i % 11 == 5, -1, lab)
    lab = np.where(i % 7 == 3, IGNORE, lab)
    typed = _typed(lab, tf)
    if tf:
        typed[cls2 & (lab == 2)] = 2.7
    return Case(f"label forms {'float32' if tf else 'int64'}", _logits("palette", n, h, w, c, 92), typed.reshape(n, h, w), "palette",
                P - len(range(3, P, 7)), range(c))


def present_case(which):
    """N = 2, 32 x 48, C = 5 (6 palette rows).  absent: class 3 relabelled 0; one: class 2 in a block, out-of-range 7 in another, the rest
    ignored; none: every pixel valid with label C + 2 (no class present); ignored: every pixel 255 (V = 0)"""
    n, h, w, c = 2, 32, 48, 5
    P = n * h * w
    lab = _rand_labels(n, h, w, c, 71)
    if which == "absent":
        lab[lab == 3] = 0
        V, present = P, (0, 1, 2, 4)
    elif which == "one":
        lab[:] = IGNORE
        lab[:, 4:20, 10:30] = 2
        lab[1, 25:, :] = 7
        V, present = 2 * 16 * 20 + 7 * 48, (2,)
    elif which == "none":
        lab[:] = c + 2
        V, present = P, ()
    else:
        assert which == "ignored"
        lab[:] = IGNORE
        V, present = 0, ()
    return Case(f"present: {which}", _logits("palette", n, h, w, c, 72, rows=6), _typed(lab, which in ("one", "none")), "palette", V, present)


MASKED_HW = (64, 66)


def masked_cases(tf):
    """N = 3, 64 x 66 (12672 pixels, 1.5 tiles; an image is 4224 pixels), C = 5: class 3 lives in images 0 and 2 only, class 4 in image 1
    only, a 255 block of 16 x 22 in every image.  -> the unmasked case and one case per mask of MASKS3 (V and the present set follow the
    labelled images)"""
    n, (h, w), c = 3, MASKED_HW, 5
    lab = _rand_labels(n, h, w, c, 81)
    lab[1][lab[1] == 3] = 0
    lab[0][lab[0] == 4] = 1
    lab[2][lab[2] == 4] = 1
    lab[:, : h // 4, : w // 3] = IGNORE
    per = h * w - (h // 4) * (w // 3)
    base = Case(f"masked base {'float32' if tf else 'int64'}", _logits("palette", n, h, w, c, 82), _typed(lab, tf), "palette", 3 * per, range(c))
    present = {(1, 1, 1): range(5), (1, 0, 1): (0, 1, 2, 3), (0, 0, 1): (0, 1, 2, 3), (0, 0, 0): ()}
    return base, [base.with_mask(m, sum(m) * per, present[m]) for m in MASKS3]


def big_case(w, kind, tf):
    """N = 1, 2050 x w, C = 2, every 13th pixel ignored.  w = 4098: 8 400 900 pixels = 1026 tiles, lv_scan_kernel's second trip (1024
    tiles per trip), 2 100 225 low-res pixels.  w = 4100: 8 405 000 pixels, above the plain backward's 2 097 152-pixel grid and the
    space-to-depth backward's 8 388 608-pixel grid: both grid-stride loops repeat"""
    h, c = 2050, 2
    P = h * w
    lab = _rand_labels(1, h, w, c, w).reshape(-1)
    lab[5::13] = IGNORE
    return Case(f"big 2050x{w}", _logits(kind, 1, h, w, c, w), _typed(lab.reshape(1, h, w), tf), kind, P - len(range(5, P, 13)), range(c),
                ldd=c + 1, ldz=4 * c + (4 if w == 4100 else 0))


# every P the GPU file uses: the workspace layout is held to hn_seg_lovasz_ws_bytes at each (test_lovasz_ref_cpu.py)
ALL_P = EDGE_P + (2 * TILE, 2 * 66 * 64, 2 * 24 * 32, 2 * 32 * 48, 3 * 64 * 66, 2050 * 4098, 2050 * 4100)
