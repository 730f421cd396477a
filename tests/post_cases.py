"""The cases of tests/test_post_exact_gpu.py, as numpy data, so that tests/test_post_ref_cpu.py can hold the references of
tests/post_ref.py to the oracle on exactly these inputs (and show that every mutant of a reference changes one of their expected
outputs) without a GPU.  Everything is built from fixed tables or a seeded RandomState.

Lane inputs: the logits are (0, l1) with l1 a multiple of 1/16 in [-2, 4] (equal l1 = an exact tie; different l1 give probabilities at
least 1e-3 apart, and at least 1e-3 from the threshold 0.5 unless l1 == 0, which is exactly 0.5); the location rows hold small integers,
so every x coordinate is an integer (times the interval) and exact."""
import numpy as np

F32 = np.float32
THR_NEXT = float(np.nextafter(F32(0.5), F32(1.0)))


# =====================================================================================================================================
# lane content cases: 256 x 128, stride 32, ppl 16 -> 8 x 4 = 32 anchors, interval 8, 4 positions per anchor row, N = 3
# =====================================================================================================================================
CONTENT_GEOMETRY = (256, 128, 32, 16)
OFF = -2.0                                 # l1 of an anchor that is no candidate


def _row(ppl, l1, rel_up=0.0, rel_down=0.0, up=(), down=()):
    """(logits, loc row): `up` / `down` are the walk's offsets in units of the interval, padded with their last value (0 when empty)"""
    loc = np.zeros(2 * ppl + 2, F32)
    for base, v in ((ppl + 2, up), (0, down)):
        v = list(v) or [0]
        loc[base:base + ppl] = (v + [v[-1]] * ppl)[:ppl]
    loc[ppl], loc[ppl + 1] = rel_down, rel_up
    return np.array([0.0, l1], F32), loc


def planted_image():
    """image 0: one anchor per content case of the kernel.  Anchor a = h * 8 + w, x centre 16 + 32 w, ypos = 4 (3 - h)."""
    ppl = 16
    cls = np.tile(np.array([0.0, OFF], F32), (32, 1))
    loc = np.zeros((32, 34), F32)
    loc[:, ppl:ppl + 2] = 3                                     # (rows of non-candidates: never read past the threshold)
    plant = {
        # ---- bottom row (h = 3, ypos 0: no down walk) ----
        24: dict(l1=3.0, rel_up=4),                             # A: x = 16 at positions 0..3
        25: dict(l1=2.0, rel_up=4, up=[-1]),                    # B: x = 40, 24 from A: suppressed at nms_thr 24 (equality)
        26: dict(l1=1.0, rel_up=4, up=[-2]),                    # C: x = 64, 24 from B, 48 from A: survives because B is dead
        27: dict(l1=2.5, rel_up=1),                             # one point: no lane, but prob / start / end / X are written
        28: dict(l1=0.0, rel_up=2),                             # two points, prob exactly 0.5
        29: dict(l1=0.0, rel_up=0.5),                           # fractional rel_up: one point
        30: dict(l1=1.5, rel_up=4, up=[0, 1, 2, 6]),            # x = 208, 216, 224, then 256 == W: the up walk stops there
        # ---- h = 2, ypos 4 ----
        16: dict(l1=2.25, rel_up=2.5, rel_down=0.5),            # 3 up points (i < 2.5), 1 down point: positions 3..6
        17: dict(l1=0.375, rel_up=0, rel_down=3),               # no up point: end == ypos; positions 1..3
        18: dict(l1=1.75, rel_up=-1, rel_down=20, down=[3]),    # rel_down above ppl: the walk ends at position 0; x = 104
        19: dict(l1=0.75, rel_up=17, rel_down=-1),              # rel_up above ppl: the walk ends at position 15
        20: dict(l1=3.5, rel_up=4),                             # x = 144 at 4..7
        21: dict(l1=0.5, rel_up=4, up=[-4, -4, -4, 2]),         # x = 144, 144, 144, 192: mean distance to anchor 20 is 12, its maximum 48
        22: dict(l1=0.25, rel_up=5, rel_down=2, up=[0, -26, -27]),      # x = 208, 0 (kept: not < 0), -8 (stops)
        23: dict(l1=2.75, rel_up=2, rel_down=4, down=[1, 2, 14, 15]),   # x = 248, 256, 352, 360: the down walk stops at W + margin
        # ---- h = 1, ypos 8: tie groups interleaved in raster order (l1 = 1 at 8, 10, 12 and 26; l1 = 2 at 9, 11, 14 and 25; 0 at 13, 15, 28)
        8: dict(l1=1.0), 9: dict(l1=2.0), 10: dict(l1=1.0), 11: dict(l1=2.0), 12: dict(l1=1.0), 13: dict(l1=0.0), 14: dict(l1=2.0),
        15: dict(l1=0.0),
        # ---- top row (h = 0, ypos 12: at most 4 up points) ----
        0: dict(l1=1.25, rel_up=20, rel_down=20),               # every position 0..15
        4: dict(l1=0.0625, rel_up=4),                           # positions 12..15: no overlap with anchor 28 (0..1) at the same x
    }
    for a, d in plant.items():
        d = dict(d)
        if 8 <= a < 16:
            d.update(rel_up=3, rel_down=2)
        cls[a], loc[a] = _row(ppl, **d)
    return cls, loc


def full_image(rs):
    """every one of the 32 anchors a lane of >= 2 points, probabilities in interleaved tie groups, small random integer offsets"""
    ppl = 16
    cls, loc = np.zeros((32, 2), F32), np.zeros((32, 34), F32)
    l1s = [1.0, 2.0, 0.5, 1.0, 3.0, 2.0, 0.5, 1.0]
    for a in range(32):
        cls[a], loc[a] = _row(ppl, l1s[(a * 3 + a // 8) % 8], rel_up=[2, 2.5, 3, 17][rs.randint(4)], rel_down=[0, -1, 0.5, 1, 3, 20][rs.randint(6)],
                              up=list(rs.randint(-1, 2, size=4)), down=list(rs.randint(-1, 2, size=4)))
    return cls, loc


def empty_image():
    cls = np.tile(np.array([0.0, OFF], F32), (32, 1))
    loc = np.full((32, 34), 2, F32)
    return cls, loc


def _content_batch():
    imgs = [planted_image(), empty_image(), full_image(np.random.RandomState(11))]
    return np.stack([c for c, _ in imgs]), np.stack([l for _, l in imgs])


def lane_content_cases():
    """name -> dict(cls, loc, geometry, thr, nms_thr, use_mean, margin); image 1 of every batch has no candidate, image 2 has 32"""
    cls, loc = _content_batch()
    base = dict(cls=cls, loc=loc, geometry=CONTENT_GEOMETRY, thr=0.5, nms_thr=24.0, use_mean=0, margin=100.0)
    return {
        "margin100": dict(base),
        "margin0": dict(base, margin=0.0),
        "thr_next": dict(base, thr=THR_NEXT),
        "use_mean": dict(base, use_mean=1),
        "nms_off": dict(base, nms_thr=-1.0),                   # the decode_lane path: every candidate kept
        "nms_wide": dict(base, nms_thr=1000.0),                # whatever overlaps is suppressed: only the `hi <= lo` pairs survive each other
    }


# =====================================================================================================================================
# lane geometry cases: stride 32
# =====================================================================================================================================
GEOMETRIES = [
    # name, fw, fh, ppl
    ("35x32", 35, 32, 16),                 # 1120 anchors: more than one per thread, not a multiple of 64
    ("60x51", 60, 51, 16),                 # 3060 anchors: 64 292 bytes of LDS, just below the opt-in
    ("60x52", 60, 52, 16),                 # 3120 anchors: 65 552 bytes, just above
    ("112x64", 112, 64, 16),               # 7168 anchors: the cap
    ("8x4_ppl18", 8, 4, 18),               # ppl / fh = 4.5; interval 128 / 18 is no float32 integer: products and sums round
]
REFUSED_GEOMETRY = ("113x64", 113, 64, 16)  # 7232 anchors


def lane_geometry_case(name, fw, fh, ppl, N=2):
    """candidates at anchors 0, 1023, 1024, 2047, 2048 and hw - 1 (those that exist) of both images, image 1 with 40 more at random
    anchors; l1 distinct per planted anchor, from the tie table for the random ones"""
    rs = np.random.RandomState(fw * 1000 + fh)
    hw, L = fw * fh, 2 * ppl + 2
    cls = np.tile(np.array([0.0, OFF], F32), (N, hw, 1))
    loc = np.zeros((N, hw, L), F32)
    planted = [a for a in (0, 1023, 1024, 2047, 2048, hw - 1) if a < hw]
    planted = sorted(set(planted))
    for n in range(N):
        anchors = list(planted)
        if n == 1:
            anchors += [int(a) for a in rs.choice(hw, size=min(40, hw // 2), replace=False) if int(a) not in planted]
        for j, a in enumerate(anchors):
            l1 = 1.0 + j / 16 if a in planted else [0.25, 0.5, 0.75][rs.randint(3)]
            sign = 1 if a % fw < fw // 2 else -1               # offsets lean into the frame: every candidate is a lane of >= 2 points
            cls[n, a], loc[n, a] = _row(ppl, l1, rel_up=3, rel_down=2, up=list(sign * rs.randint(0, 3, size=3)),
                                        down=list(sign * rs.randint(0, 3, size=2)))
    return dict(cls=cls, loc=loc, geometry=(fw * 32, fh * 32, 32, ppl), thr=0.5, nms_thr=40.0, use_mean=0, margin=100.0, planted=planted)


# =====================================================================================================================================
# seg confusion
# =====================================================================================================================================
CONF_C = (1, 5, 19, 63)
CONF_M = (1, 255, 256, 257, 4097)


def confusion_case(C, M, is_float, negatives=True):
    """pred int64 [M], target int64 or float32 [M]: classes 0..C-1 with the special ids planted in front (cycled when M is short):
    255, C, C + 1, 2^40 and, with `negatives`, -1 and -2^40 (int) / -1.0 and -3.5 (float); float targets add 4.99, 0.99, 255.0 and -0.5 (which truncates to class 0)"""
    rs = np.random.RandomState(C * 10007 + M * 3 + int(is_float))
    pred = rs.randint(0, C, size=M).astype(np.int64)
    special_p = [255, C, C + 1, 1 << 40] + ([-1, -(1 << 40)] if negatives else [])
    k = rs.randint(0, M, size=2 * len(special_p)) if M > 8 else np.arange(M)
    pred[k] = np.resize(np.array(special_p, np.int64), len(k))
    if is_float:
        target = rs.randint(0, C, size=M).astype(F32)
        special_t = [255.0, float(C), C + 1.0, float(1 << 40), 4.99, 0.99, -0.5] + ([-1.0, -3.5] if negatives else [])
        target[(k * 7 + 1) % M if M > 8 else k] = np.resize(np.array(special_t, F32), len(k))
    else:
        target = rs.randint(0, C, size=M).astype(np.int64)
        special_t = [255, C, C + 1, 1 << 40] + ([-1, -(1 << 40)] if negatives else [])
        target[(k * 7 + 1) % M if M > 8 else k] = np.resize(np.array(special_t[::-1], np.int64), len(k))
    if M == 1:                                                  # the one pixel: a negative prediction against a real class
        pred[0] = -1 if negatives else C + 1
        target[0] = 0
    return pred, target


# =====================================================================================================================================
# seg overlay and pre-processing
# =====================================================================================================================================
LUT = np.array([[0, 0, 0], [1, 3, 5], [255, 255, 255], [128, 7, 250], [2, 4, 6]], np.uint8)     # ncls = 5
OVERLAY_SHAPES = [
    # name, N, mask H x W, frame Ho x Wo
    ("1x1_up", 1, (1, 1), (9, 13)),
    ("1x7_up", 2, (1, 7), (9, 13)),
    ("5x1_up", 1, (5, 1), (9, 13)),
    ("identity", 2, (6, 10), (6, 10)),
    ("12x20_down", 3, (12, 20), (5, 9)),
]


def overlay_case(name, n, mhw, fhw):
    """masks over the ids 0..4 and the out-of-range ids -1, 5 (= ncls) and 2^33; frames random with 0 and 255 planted.  The identity
    case has a black frame strip over class 1 (colour 1, 3, 5: the blends 0.5, 1.5, 2.5) and white pixels over class 2 (255 + 255)."""
    rs = np.random.RandomState(len(name) * 101 + mhw[0] * 7 + fhw[1])
    ids = np.array([0, 1, 2, 3, 4, -1, 5, 1 << 33], np.int64)
    mask = ids[rs.randint(0, len(ids), size=(n,) + mhw)]
    frames = rs.randint(0, 256, size=(n,) + fhw + (3,)).astype(np.uint8)
    frames.reshape(-1)[rs.randint(0, frames.size, size=8)] = 255
    frames.reshape(-1)[rs.randint(0, frames.size, size=8)] = 0
    if mhw == (1, 1):
        mask[0, 0, 0] = 3
    if name == "identity":
        mask[0, 0, :] = 1
        frames[0, 0, :, :] = 0
        mask[0, 1, :] = 2
        frames[0, 1, :, :] = 255
        mask[1, 2, :3] = [-1, 5, 1 << 33]
        frames[1, 2, :3] = 200
    return mask, frames


PREPROCESS_SHAPES = [
    # name, N, source Hs x Ws, output Hd x Wd
    ("1x1_to_4x6", 1, (1, 1), (4, 6)),
    ("1x9_to_5x5", 1, (1, 9), (5, 5)),
    ("7x1_to_3x3", 1, (7, 1), (3, 3)),
    ("5x7_identity", 1, (5, 7), (5, 7)),
    ("37x53_to_48x64", 1, (37, 53), (48, 64)),
    ("40x64_to_13x21_n3", 3, (40, 64), (13, 21)),              # 3 * 273 = 819 output pixels: 3 blocks and a tail, images straddle blocks
]


def preprocess_case(name, n, shw, dhw):
    rs = np.random.RandomState(shw[0] * 131 + shw[1])
    frames = rs.randint(0, 256, size=(n,) + shw + (3,)).astype(np.uint8)
    flat = frames.reshape(-1)
    flat[0] = 0
    flat[-1] = 255
    if flat.size > 6:
        flat[rs.randint(0, flat.size, size=4)] = 255
        flat[rs.randint(0, flat.size, size=4)] = 0
    return frames


# =====================================================================================================================================
# lane rasteriser and pair counts: a 24 x 40 frame
# =====================================================================================================================================
RASTER_HW = (24, 40)
LANE_WIDTHS = (1, 2, 3, 30, 31)


def raster_lanes():
    """polylines as lists of integer (x, y) points, one per lane: interior, zero-length, crossing and beyond every border"""
    return [
        [(5, 20), (12, 9), (20, 4)],                  # interior polyline, oblique segments
        [(17, 11), (17, 11)],                         # zero-length segment: a disc
        [(-6, 12), (8, 12)],                          # crosses the left border
        [(30, 5), (47, 9)],                           # crosses the right border
        [(10, -5), (14, 6)],                          # crosses the top border
        [(25, 18), (28, 30)],                         # crosses the bottom border
        [(-9, 3), (-4, 20)],                          # left of the frame (within reach of the wide widths only)
        [(44, 2), (60, 10)],                          # right of the frame
        [(3, -40), (30, -33)],                        # above: out of every width's reach (an empty bounding box)
        [(2, 60), (9, 70), (30, 64)],                 # below: the same
        [(0, 0), (39, 23)],                           # corner to corner
        [(39, 0), (39, 23), (0, 23)],                 # along the right and bottom borders
    ]


def pack_segments(lanes, lane_ids=None):
    """(pts int32 [npts, 2], seg_lane, seg_first int32 [nseg]) in hn_lane_raster's layout: lanes back to back, one segment per point pair"""
    pts, seg_lane, seg_first = [], [], []
    for j, lane in enumerate(lanes):
        base = len(pts)
        pts += lane
        for i in range(len(lane) - 1):
            seg_lane.append(j if lane_ids is None else lane_ids[j])
            seg_first.append(base + i)
    return np.array(pts, np.int32).reshape(-1, 2), np.array(seg_lane, np.int32), np.array(seg_first, np.int32)


PAIR_SHAPES = [(1, 1), (32, 32), (32, 1)]


def pair_lanes(G, P):
    """G ground truths then P predictions on the 24 x 40 frame: short two-point lanes stepping across it, every one non-empty at width 3
    (ground truth 31 and prediction 31 among them), neighbours overlapping"""
    gts = [[(1 + (j * 7) % 37, 2 + j % 5), (3 + (j * 7) % 35, 20 - j % 7)] for j in range(G)]
    prs = [[(2 + (j * 5) % 36, 1 + j % 6), (1 + (j * 5) % 38, 21 - j % 4)] for j in range(P)]
    return gts, prs
