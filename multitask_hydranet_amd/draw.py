"""Drawing on the device (hn_draw.hip): thick polylines, rectangles and text painted into packed BGR frames in place, one
launch for a ragged batch, and on top of it the two visualisation helpers of the reference's heads -- LaneHeader.visual
(head_lane/lanedetect.py:126-178) and DetectionHeader.display (head_detect/display.py:49-84).

A drawing is an ORDERED list of primitives per image; a pixel takes the colour of the last primitive of the list that covers it.
    segment(x0, y0, x1, y1, thickness, colour)       cv2.line: the pixel centres within thickness / 2 of the segment (the distance test
                                                     of hn_lane_raster, the project's one restatement of OpenCV's thick line; cv2 is
                                                     absent, parity at boundary pixels is unpinned)
    rect_outline(x0, y0, x1, y1, thickness, colour)  cv2.rectangle, thickness > 0: its four thick segments
    rect_filled(x0, y0, x1, y1, colour)              cv2.rectangle, thickness < 0: both corners inclusive
    text(x, y, scale, string, colour)                cv2.putText: (x, y) is the bottom-left corner of the text

Text is OURS, not OpenCV's: the Hershey font data is not available, so the module carries a 5 x 7 bitmap font in a 6 x 8 cell (FONT:
digits, Latin letters, ". : % _ -" and space; any other character draws an empty cell), every bit a scale x scale square with
scale = max(1, round(3 * fontScale)) (Hershey simplex capitals are 21 pixels tall at fontScale 1, ours 7 at scale 1).  The text extent is
therefore text_size() = (6 * scale * len(string), 7 * scale) instead of cv2.getTextSize's, and with it the size of display()'s label
box; the stroke thickness argument of cv2.putText has no counterpart.  Coordinates are clamped to +-16383 (the kernel's integer range).
"""
from __future__ import annotations

import warnings
from typing import List, Sequence

import numpy as np

from ._lib import lib

# hn_draw.hip struct DrawPrim / DrawImage
PRIM_DTYPE = np.dtype({"names": ["kind", "x0", "y0", "x1", "y1", "param", "color", "pad"], "formats": ["<i4"] * 6 + ["<u4", "<i4"],
                       "offsets": [0, 4, 8, 12, 16, 20, 24, 28], "itemsize": 32})
IMAGE_DTYPE = np.dtype({"names": ["off", "W", "H", "p0", "p1"], "formats": ["<i8", "<i4", "<i4", "<i4", "<i4"], "offsets": [0, 8, 12, 16, 20],
                        "itemsize": 24})
SEGMENT, RECT, GLYPH = 0, 1, 2
COORD_MAX = 16383

# 5 x 7 glyphs: seven rows, top to bottom, five bits each, the left column in the high bit
FONT = {
    " ": (0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00), ".": (0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C), ":": (0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x0C, 0x00),
    "%": (0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03), "_": (0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x1F), "-": (0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00),
    "0": (0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E), "1": (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E), "2": (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F),
    "3": (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E), "4": (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02), "5": (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
    "6": (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E), "7": (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08), "8": (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E),
    "9": (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C),
    "A": (0x0E, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11), "B": (0x1E, 0x11, 0x11, 0x1E, 0x11, 0x11, 0x1E), "C": (0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E),
    "D": (0x1E, 0x11, 0x11, 0x11, 0x11, 0x11, 0x1E), "E": (0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x1F), "F": (0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x10),
    "G": (0x0E, 0x11, 0x10, 0x17, 0x11, 0x11, 0x0F), "H": (0x11, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11), "I": (0x0E, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E),
    "J": (0x07, 0x02, 0x02, 0x02, 0x02, 0x12, 0x0C), "K": (0x11, 0x12, 0x14, 0x18, 0x14, 0x12, 0x11), "L": (0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1F),
    "M": (0x11, 0x1B, 0x15, 0x15, 0x11, 0x11, 0x11), "N": (0x11, 0x19, 0x15, 0x13, 0x11, 0x11, 0x11), "O": (0x0E, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E),
    "P": (0x1E, 0x11, 0x11, 0x1E, 0x10, 0x10, 0x10), "Q": (0x0E, 0x11, 0x11, 0x11, 0x15, 0x12, 0x0D), "R": (0x1E, 0x11, 0x11, 0x1E, 0x14, 0x12, 0x11),
    "S": (0x0F, 0x10, 0x10, 0x0E, 0x01, 0x01, 0x1E), "T": (0x1F, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04), "U": (0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E),
    "V": (0x11, 0x11, 0x11, 0x11, 0x11, 0x0A, 0x04), "W": (0x11, 0x11, 0x11, 0x15, 0x15, 0x15, 0x0A), "X": (0x11, 0x11, 0x0A, 0x04, 0x0A, 0x11, 0x11),
    "Y": (0x11, 0x11, 0x0A, 0x04, 0x04, 0x04, 0x04), "Z": (0x1F, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1F),
    "a": (0x00, 0x00, 0x0E, 0x01, 0x0F, 0x11, 0x0F), "b": (0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x1E), "c": (0x00, 0x00, 0x0E, 0x10, 0x10, 0x11, 0x0E),
    "d": (0x01, 0x01, 0x0D, 0x13, 0x11, 0x11, 0x0F), "e": (0x00, 0x00, 0x0E, 0x11, 0x1F, 0x10, 0x0E), "f": (0x06, 0x09, 0x08, 0x1C, 0x08, 0x08, 0x08),
    "g": (0x00, 0x0F, 0x11, 0x11, 0x0F, 0x01, 0x0E), "h": (0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x11), "i": (0x04, 0x00, 0x0C, 0x04, 0x04, 0x04, 0x0E),
    "j": (0x02, 0x00, 0x06, 0x02, 0x02, 0x12, 0x0C), "k": (0x10, 0x10, 0x12, 0x14, 0x18, 0x14, 0x12), "l": (0x0C, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E),
    "m": (0x00, 0x00, 0x1A, 0x15, 0x15, 0x11, 0x11), "n": (0x00, 0x00, 0x16, 0x19, 0x11, 0x11, 0x11), "o": (0x00, 0x00, 0x0E, 0x11, 0x11, 0x11, 0x0E),
    "p": (0x00, 0x00, 0x1E, 0x11, 0x1E, 0x10, 0x10), "q": (0x00, 0x00, 0x0D, 0x13, 0x0F, 0x01, 0x01), "r": (0x00, 0x00, 0x16, 0x19, 0x10, 0x10, 0x10),
    "s": (0x00, 0x00, 0x0E, 0x10, 0x0E, 0x01, 0x1E), "t": (0x08, 0x08, 0x1C, 0x08, 0x08, 0x09, 0x06), "u": (0x00, 0x00, 0x11, 0x11, 0x11, 0x13, 0x0D),
    "v": (0x00, 0x00, 0x11, 0x11, 0x11, 0x0A, 0x04), "w": (0x00, 0x00, 0x11, 0x11, 0x15, 0x15, 0x0A), "x": (0x00, 0x00, 0x11, 0x0A, 0x04, 0x0A, 0x11),
    "y": (0x00, 0x00, 0x11, 0x11, 0x0F, 0x01, 0x0E), "z": (0x00, 0x00, 0x1F, 0x02, 0x04, 0x08, 0x1F),
}

# the CSS colours display.py gives its classes, in class order (public CSS Color Module values, written as BGR): LawnGreen, Chartreuse,
# Aqua, Beige, Azure, BlanchedAlmond, Bisque, Aquamarine, BlueViolet, BurlyWood, CadetBlue, AntiqueWhite.  A class beyond the table wraps.
CLASS_COLORS_BGR = [(0, 252, 124), (0, 255, 127), (255, 255, 0), (220, 245, 245), (255, 255, 240), (205, 235, 255), (196, 228, 255), (212, 255, 127),
                    (226, 43, 138), (135, 184, 222), (160, 158, 95), (215, 235, 250)]

LANE_COLOR, LANE_THICKNESS, LANE_FONT_SCALE = (255, 255, 0), 15, 2.0     # lanedetect.py:157-176


# ---- primitives (plain tuples: kind, x0, y0, x1, y1, param, colour word) ----------------------------------------------------------------
def _c(v) -> int:
    return int(min(COORD_MAX, max(-COORD_MAX, int(v))))


def _word(colour) -> int:
    b, g, r = (int(c) & 255 for c in colour)
    return b | (g << 8) | (r << 16)


def segment(x0, y0, x1, y1, thickness, colour) -> list:
    return [(SEGMENT, _c(x0), _c(y0), _c(x1), _c(y1), max(1, int(thickness)), _word(colour))]


def rect_outline(x0, y0, x1, y1, thickness, colour) -> list:
    return (segment(x0, y0, x1, y0, thickness, colour) + segment(x1, y0, x1, y1, thickness, colour) + segment(x1, y1, x0, y1, thickness, colour)
            + segment(x0, y1, x0, y0, thickness, colour))


def rect_filled(x0, y0, x1, y1, colour) -> list:
    return [(RECT, _c(x0), _c(y0), _c(x1), _c(y1), 1, _word(colour))]


def font_scale(cv_font_scale: float) -> int:
    return max(1, int(round(3.0 * float(cv_font_scale))))


def text_size(string: str, scale: int):
    return 6 * scale * len(string), 7 * scale


def text(x, y, scale, string, colour) -> list:
    """(x, y): bottom-left corner of the text, as cv2.putText's org; glyph rows end at y - 1"""
    out = []
    for i, ch in enumerate(string):
        rows = FONT.get(ch)
        if rows is None or not any(rows):
            continue                                                     # an unknown character (and the space) draws an empty cell
        lo = rows[0] | (rows[1] << 5) | (rows[2] << 10) | (rows[3] << 15)
        hi = rows[4] | (rows[5] << 5) | (rows[6] << 10)
        out.append((GLYPH, _c(int(x) + 6 * scale * i), _c(int(y) - 7 * scale), lo, hi, int(scale), _word(colour)))
    return out


def to_records(prims: Sequence[tuple]) -> np.ndarray:
    rec = np.zeros(len(prims), dtype=PRIM_DTYPE)
    for e, p in zip(rec, prims):
        e["kind"], e["x0"], e["y0"], e["x1"], e["y1"], e["param"], e["color"] = p
    return rec


# ---- the launch ------------------------------------------------------------------------------------------------------------------------
def draw_packed(frames: dict, prim_lists: Sequence[Sequence[tuple]]) -> dict:
    """frames: the packed device layout of augment.pack() / jpeg.decode_batch ({"data", "offsets", "shapes"}, BGR uint8); prim_lists: one
    ordered primitive list per image.  Paints in place (one launch), returns `frames`."""
    import torch
    data = frames["data"]
    shapes = np.asarray(frames["shapes"], dtype=np.int64).reshape(-1, 2)
    offsets = np.asarray(frames["offsets"], dtype=np.int64)
    n = len(shapes)
    assert data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous() and len(prim_lists) == n
    flat = [p for lst in prim_lists for p in lst]
    if n == 0 or not flat:
        return frames
    imgs = np.zeros(n, dtype=IMAGE_DTYPE)
    p = 0
    for i, e in enumerate(imgs):
        h, w = int(shapes[i, 0]), int(shapes[i, 1])
        assert 0 < h <= 16384 and 0 < w <= 16384 and 0 <= offsets[i] and offsets[i] + h * w * 3 <= data.numel(), (i, h, w)
        e["off"], e["W"], e["H"], e["p0"], e["p1"] = int(offsets[i]), w, h, p, p + len(prim_lists[i])
        p += len(prim_lists[i])
    rec = to_records(flat)
    with torch.cuda.device(data.device):
        blob = torch.from_numpy(np.concatenate([imgs.view(np.uint8), rec.view(np.uint8)])).to(data.device)      # 24 n bytes, then the primitives
        assert (24 * n) % 8 == 0
        lib().call("hn_draw", data.data_ptr(), int(data.numel()), blob.data_ptr(), n, int(shapes[:, 0].max()), int(shapes[:, 1].max()),
                   blob.data_ptr() + 24 * n, len(flat))
    return frames


def draw(frames, prim_lists):
    """packed device frames -> painted in place, returned; a list of host uint8 H x W x 3 arrays -> uploaded, painted, the painted list"""
    if isinstance(frames, dict):
        return draw_packed(frames, prim_lists)
    import torch
    from .augment import pack
    arrs = [np.ascontiguousarray(f) for f in frames]
    for a in arrs:
        assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3, (a.dtype, a.shape)
    if not any(len(l) for l in prim_lists):
        return arrs
    pk = pack(arrs)
    dev = torch.device("cuda", torch.cuda.current_device())
    out = draw_packed({"data": pk["data"].to(dev), "offsets": pk["offsets"], "shapes": pk["shapes"]}, prim_lists)["data"].cpu().numpy()
    return [out[int(o):int(o) + a.size].reshape(a.shape) for o, a in zip(pk["offsets"], arrs)]


def _shapes_of(imgs):
    if isinstance(imgs, dict):
        return [(int(h), int(w)) for h, w in np.asarray(imgs["shapes"]).reshape(-1, 2)]
    return [tuple(im.shape[:2]) for im in imgs]


# ---- LaneHeader.visual ------------------------------------------------------------------------------------------------------------------
def lane_primitives(predict_json, org_width=1920, min_length=2, filter_vertical=True, filter_thres=65) -> list:
    """one image's lanes ([{"score", "points": [{"x", "y"}, ...]}, ...]) -> its primitive list, by lanedetect.py:133-176"""
    out = []
    for line in predict_json:
        score, pts = line["score"], line["points"]
        length = len(pts)
        if length < min_length:
            continue
        ipts = [(int(pt["x"]), int(pt["y"])) for pt in pts]
        if filter_vertical:                                              # the reference's slope filter, on the host as there
            arr = np.array(ipts)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                coeff = np.polyfit(arr[:, 0], arr[:, 1], 1)
            theta = abs(np.arctan(coeff[0])) / 3.1415 * 180
            if theta > filter_thres:
                continue
        for a, b in zip(ipts[:-1], ipts[1:]):
            out += segment(a[0], a[1], b[0], b[1], LANE_THICKNESS, LANE_COLOR)
        tx, ty = ipts[min_length - 1]
        if tx < 0:
            tx = 30
        if tx > org_width:
            tx, ty = org_width - 300, ty - 60
        out += text(tx, ty - 10, font_scale(LANE_FONT_SCALE), "%s: %.2f" % ("Lane", float(score)), LANE_COLOR)
    return out


def visual(imgs, predict_jsons, org_width=1920, min_length=2, filter_vertical=True, filter_thres=65):
    """LaneHeader.visual: imgs = a list of host uint8 BGR frames (painted like cv2 does, in place when writable; the list is returned) or
    the packed device layout (painted in place, returned)"""
    lists = [lane_primitives(pj, org_width, min_length, filter_vertical, filter_thres) for pj in predict_jsons]
    n = len(_shapes_of(imgs))
    assert len(lists) >= n, (len(lists), n)
    if isinstance(imgs, dict):
        return draw_packed(imgs, lists[:n])
    painted = draw(imgs, lists[:n])
    out = []
    for im, p in zip(imgs, painted):
        if isinstance(im, np.ndarray) and im.flags.writeable and im.flags.c_contiguous:
            np.copyto(im, p)
            out.append(im)
        else:
            out.append(p)
    return out


# ---- DetectionHeader.display -------------------------------------------------------------------------------------------------------------
def box_primitives(pred, img_hw, obj_list, org_size, target_size) -> list:
    """one image's detections ({"rois", "class_ids", "scores"}) -> its primitive list, by display.py:49-82"""
    out = []
    rois = np.asarray(pred["rois"])
    tl = int(round(0.003 * max(img_hw)))
    thick, scale = max(1, tl), font_scale(float(tl) / 3)
    for j in range(len(rois)):
        x1, y1, x2, y2 = (int(v) for v in rois[j])                      # .astype(int): truncation before the scaling
        x1, x2 = x1 / float(target_size[0]) * org_size[0], x2 / float(target_size[0]) * org_size[0]
        y1, y2 = y1 / float(target_size[1]) * org_size[1], y2 / float(target_size[1]) * org_size[1]
        obj = obj_list[int(pred["class_ids"][j])]
        score = float(pred["scores"][j])
        colour = CLASS_COLORS_BGR[obj_list.index(obj) % len(CLASS_COLORS_BGR)]
        c1, c2 = (int(x1), int(y1)), (int(x2), int(y2))
        out += rect_outline(c1[0], c1[1], c2[0], c2[1], thick, colour)
        pct = "{:.0%}".format(score)
        tw, th = text_size(obj, scale)
        sw, _ = text_size(pct, scale)
        out += rect_filled(c1[0], c1[1], c1[0] + tw + sw + 15, c1[1] - th - 3, colour)
        out += text(c1[0], c1[1] - 2, scale, obj + pct, (0, 0, 0))
    return out


def display(preds, imgs, obj_list, org_size, target_size):
    """DetectionHeader.display: every image that has boxes is painted (the reference returns after the first such image; its only caller
    passes one).  imgs = a list of host uint8 BGR frames (painted copies replace the entries, as display.py:69 does; the list is
    returned) or the packed device layout (painted in place, returned)."""
    shapes = _shapes_of(imgs)
    lists = [box_primitives(preds[i], shapes[i], list(obj_list), org_size, target_size) if len(preds[i]["rois"]) else [] for i in range(len(shapes))]
    if isinstance(imgs, dict):
        return draw_packed(imgs, lists)
    painted = draw(imgs, lists)
    for i, p in enumerate(painted):
        if lists[i]:
            imgs[i] = p
    return imgs


__all__ = ["segment", "rect_outline", "rect_filled", "text", "text_size", "font_scale", "draw", "draw_packed", "lane_primitives", "box_primitives",
           "visual", "display", "FONT", "CLASS_COLORS_BGR"]
