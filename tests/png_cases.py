"""PNG label cases for the device decode (hn_png.hip): a deterministic generator with its own minimal PNG writer (zlib, struct, numpy), so
that the filter of every row, the deflate block types and the IDAT split are chosen, not hoped for.  PIL is the decoder of record: a case's
expected result is dataset.imread_label on the same bytes.

A case is (colour, filters, deflate, idat, (W, H), content, seed):
  colour   "grey" (type 0), "rgb" (type 2), "pal" (type 3 with PLTE), "pal+trns" (type 3 with PLTE and tRNS)
  filters  "f0" .. "f4": that type on every row; "cycle": rows 0, 1, 2, 3, 4, 0, ...; "random": a seeded choice per row
  deflate  "stored" (level 0), "fixed" (Z_FIXED), "l6", "l9", "flush" (level 6, Z_FULL_FLUSH every 997 raw bytes: many blocks, empty stored ones)
  idat     0: one chunk; else chunks of that many bytes
  content  "poly" (polygon label map, values 0..4), "stripe2" / "stripe3" (period-2 / -3 bytes), "noise", "far" (a byte pattern that
           repeats every 32 500 bytes of the raw scanlines: near-maximal match distances)
MATRIX is the committed list (the product of the axes, thinned); BIG_FILES are two 1080x1920 polygon labels written by PIL's own encoder.
"""
import io
import struct
import zlib

import numpy as np

COLOURS = ("grey", "rgb", "pal", "pal+trns")
FILTERS = ("f0", "f1", "f2", "f3", "f4", "cycle", "random")
DEFLATES = ("stored", "fixed", "l6", "l9", "flush")
SIZES = ((1, 1), (1, 70), (70, 1), (63, 5), (64, 5), (65, 5), (5, 63), (5, 64), (5, 65), (5, 129), (97, 61), (640, 360))
FLUSH_EVERY = 997
FAR_PERIOD = 32500

MATRIX = [
    ("grey", "f0", "stored", 0, (1, 1), "poly", 0),
    ("rgb", "f1", "fixed", 1, (1, 1), "stripe2", 1),
    ("pal", "f2", "l6", 7, (1, 1), "stripe3", 2),
    ("pal+trns", "f3", "l9", 8192, (1, 1), "noise", 3),
    ("grey", "f4", "flush", 0, (1, 1), "poly", 4),
    ("rgb", "cycle", "stored", 1, (1, 1), "poly", 5),
    ("pal", "random", "fixed", 7, (1, 1), "stripe2", 6),
    ("pal+trns", "f0", "l6", 8192, (1, 70), "stripe3", 7),
    ("grey", "f1", "l9", 0, (1, 70), "noise", 8),
    ("rgb", "f2", "flush", 1, (1, 70), "poly", 9),
    ("pal", "f3", "stored", 7, (1, 70), "poly", 10),
    ("pal+trns", "f4", "fixed", 8192, (1, 70), "stripe2", 11),
    ("grey", "cycle", "l6", 0, (1, 70), "stripe3", 12),
    ("rgb", "random", "l9", 1, (1, 70), "noise", 13),
    ("pal", "f0", "l9", 7, (70, 1), "poly", 14),
    ("pal+trns", "f1", "flush", 8192, (70, 1), "poly", 15),
    ("grey", "f2", "stored", 0, (70, 1), "stripe2", 16),
    ("rgb", "f3", "fixed", 1, (70, 1), "stripe3", 17),
    ("pal", "f4", "l6", 7, (70, 1), "noise", 18),
    ("pal+trns", "cycle", "l9", 8192, (70, 1), "poly", 19),
    ("grey", "random", "flush", 0, (70, 1), "poly", 20),
    ("rgb", "f0", "flush", 1, (63, 5), "stripe2", 21),
    ("pal", "f1", "stored", 7, (63, 5), "stripe3", 22),
    ("pal+trns", "f2", "fixed", 8192, (63, 5), "noise", 23),
    ("grey", "f3", "l6", 0, (63, 5), "poly", 24),
    ("rgb", "f4", "l9", 1, (63, 5), "poly", 25),
    ("pal", "cycle", "flush", 7, (63, 5), "stripe2", 26),
    ("pal+trns", "random", "stored", 8192, (63, 5), "stripe3", 27),
    ("grey", "f0", "fixed", 0, (64, 5), "noise", 28),
    ("rgb", "f1", "l6", 1, (64, 5), "poly", 29),
    ("pal", "f2", "l9", 7, (64, 5), "poly", 30),
    ("pal+trns", "f3", "flush", 8192, (64, 5), "stripe2", 31),
    ("grey", "f4", "stored", 0, (64, 5), "stripe3", 32),
    ("rgb", "cycle", "fixed", 1, (64, 5), "noise", 33),
    ("pal", "random", "l6", 7, (64, 5), "poly", 34),
    ("pal+trns", "f0", "l6", 8192, (65, 5), "poly", 35),
    ("grey", "f1", "l9", 0, (65, 5), "stripe2", 36),
    ("rgb", "f2", "flush", 1, (65, 5), "stripe3", 37),
    ("pal", "f3", "stored", 7, (65, 5), "noise", 38),
    ("pal+trns", "f4", "fixed", 8192, (65, 5), "poly", 39),
    ("grey", "cycle", "l6", 0, (65, 5), "poly", 40),
    ("rgb", "random", "l9", 1, (65, 5), "stripe2", 41),
    ("pal", "f0", "l9", 7, (5, 63), "stripe3", 42),
    ("pal+trns", "f1", "flush", 8192, (5, 63), "noise", 43),
    ("grey", "f2", "stored", 0, (5, 63), "poly", 44),
    ("rgb", "f3", "fixed", 1, (5, 63), "poly", 45),
    ("pal", "f4", "l6", 7, (5, 63), "stripe2", 46),
    ("pal+trns", "cycle", "l9", 8192, (5, 63), "stripe3", 47),
    ("grey", "random", "flush", 0, (5, 63), "noise", 48),
    ("rgb", "f0", "flush", 1, (5, 64), "poly", 49),
    ("pal", "f1", "stored", 7, (5, 64), "poly", 50),
    ("pal+trns", "f2", "fixed", 8192, (5, 64), "stripe2", 51),
    ("grey", "f3", "l6", 0, (5, 64), "stripe3", 52),
    ("rgb", "f4", "l9", 1, (5, 64), "noise", 53),
    ("pal", "cycle", "flush", 7, (5, 64), "poly", 54),
    ("pal+trns", "random", "stored", 8192, (5, 64), "poly", 55),
    ("grey", "f0", "fixed", 0, (5, 65), "stripe2", 56),
    ("rgb", "f1", "l6", 1, (5, 65), "stripe3", 57),
    ("pal", "f2", "l9", 7, (5, 65), "noise", 58),
    ("pal+trns", "f3", "flush", 8192, (5, 65), "poly", 59),
    ("grey", "f4", "stored", 0, (5, 65), "poly", 60),
    ("rgb", "cycle", "fixed", 1, (5, 65), "stripe2", 61),
    ("pal", "random", "l6", 7, (5, 65), "stripe3", 62),
    ("pal+trns", "f0", "l6", 8192, (5, 129), "noise", 63),
    ("grey", "f1", "l9", 0, (5, 129), "poly", 64),
    ("rgb", "f2", "flush", 1, (5, 129), "poly", 65),
    ("pal", "f3", "stored", 7, (5, 129), "stripe2", 66),
    ("pal+trns", "f4", "fixed", 8192, (5, 129), "stripe3", 67),
    ("grey", "cycle", "l6", 0, (5, 129), "noise", 68),
    ("rgb", "random", "l9", 1, (5, 129), "poly", 69),
    ("pal", "f0", "l9", 7, (97, 61), "poly", 70),
    ("pal+trns", "f1", "flush", 8192, (97, 61), "stripe2", 71),
    ("grey", "f2", "stored", 0, (97, 61), "stripe3", 72),
    ("rgb", "f3", "fixed", 1, (97, 61), "noise", 73),
    ("pal", "f4", "l6", 7, (97, 61), "poly", 74),
    ("pal+trns", "cycle", "l9", 8192, (97, 61), "poly", 75),
    ("grey", "random", "flush", 0, (97, 61), "stripe2", 76),
    ("grey", "f0", "l9", 0, (640, 360), "far", 77),
    ("rgb", "f1", "l6", 8192, (640, 360), "poly", 78),
    ("pal", "f2", "flush", 8192, (640, 360), "poly", 79),
    ("grey", "f3", "l6", 0, (640, 360), "poly", 80),
    ("pal+trns", "f4", "l9", 8192, (640, 360), "poly", 81),
    ("grey", "cycle", "fixed", 0, (640, 360), "stripe3", 82),
    ("rgb", "random", "stored", 8192, (640, 360), "noise", 83),
    ("grey", "f1", "stored", 7, (97, 61), "poly", 84),
    ("rgb", "f2", "stored", 8192, (65, 5), "poly", 85),
    ("pal", "f3", "stored", 0, (5, 129), "poly", 86),
    ("pal+trns", "f4", "stored", 1, (63, 5), "poly", 87),
    ("grey", "cycle", "stored", 7, (5, 65), "stripe2", 88),
    ("rgb", "random", "stored", 8192, (97, 61), "stripe2", 89),
    ("pal", "f0", "stored", 0, (65, 5), "stripe2", 90),
    ("pal+trns", "f1", "stored", 1, (5, 129), "stripe2", 91),
    ("grey", "f2", "stored", 7, (63, 5), "stripe3", 92),
    ("rgb", "f3", "stored", 8192, (5, 65), "stripe3", 93),
    ("pal", "f4", "stored", 0, (97, 61), "stripe3", 94),
    ("pal+trns", "cycle", "stored", 1, (65, 5), "stripe3", 95),
    ("grey", "random", "stored", 7, (5, 129), "noise", 96),
    ("rgb", "f0", "stored", 8192, (63, 5), "noise", 97),
    ("pal", "f1", "stored", 0, (5, 65), "noise", 98),
    ("pal+trns", "f2", "stored", 1, (97, 61), "noise", 99),
    ("grey", "f3", "fixed", 7, (65, 5), "poly", 100),
    ("rgb", "f4", "fixed", 8192, (5, 129), "poly", 101),
    ("pal", "cycle", "fixed", 0, (63, 5), "poly", 102),
    ("pal+trns", "random", "fixed", 1, (5, 65), "poly", 103),
    ("grey", "f0", "fixed", 7, (97, 61), "stripe2", 104),
    ("rgb", "f1", "fixed", 8192, (65, 5), "stripe2", 105),
    ("pal", "f2", "fixed", 0, (5, 129), "stripe2", 106),
    ("pal+trns", "f3", "fixed", 1, (63, 5), "stripe2", 107),
    ("grey", "f4", "fixed", 7, (5, 65), "stripe3", 108),
    ("rgb", "cycle", "fixed", 8192, (97, 61), "stripe3", 109),
    ("pal", "random", "fixed", 0, (65, 5), "stripe3", 110),
    ("pal+trns", "f0", "fixed", 1, (5, 129), "stripe3", 111),
    ("grey", "f1", "fixed", 7, (63, 5), "noise", 112),
    ("rgb", "f2", "fixed", 8192, (5, 65), "noise", 113),
    ("pal", "f3", "fixed", 0, (97, 61), "noise", 114),
    ("pal+trns", "f4", "fixed", 1, (65, 5), "noise", 115),
    ("grey", "cycle", "l6", 7, (5, 129), "poly", 116),
    ("rgb", "random", "l6", 8192, (63, 5), "poly", 117),
    ("pal", "f0", "l6", 0, (5, 65), "poly", 118),
    ("pal+trns", "f1", "l6", 1, (97, 61), "poly", 119),
    ("grey", "f2", "l6", 7, (65, 5), "stripe2", 120),
    ("rgb", "f3", "l6", 8192, (5, 129), "stripe2", 121),
    ("pal", "f4", "l6", 0, (63, 5), "stripe2", 122),
    ("pal+trns", "cycle", "l6", 1, (5, 65), "stripe2", 123),
    ("grey", "random", "l6", 7, (97, 61), "stripe3", 124),
    ("rgb", "f0", "l6", 8192, (65, 5), "stripe3", 125),
    ("pal", "f1", "l6", 0, (5, 129), "stripe3", 126),
    ("pal+trns", "f2", "l6", 1, (63, 5), "stripe3", 127),
    ("grey", "f3", "l6", 7, (5, 65), "noise", 128),
    ("rgb", "f4", "l6", 8192, (97, 61), "noise", 129),
    ("pal", "cycle", "l6", 0, (65, 5), "noise", 130),
    ("pal+trns", "random", "l6", 1, (5, 129), "noise", 131),
    ("grey", "f0", "l9", 7, (63, 5), "poly", 132),
    ("rgb", "f1", "l9", 8192, (5, 65), "poly", 133),
    ("pal", "f2", "l9", 0, (97, 61), "poly", 134),
    ("pal+trns", "f3", "l9", 1, (65, 5), "poly", 135),
    ("grey", "f4", "l9", 7, (5, 129), "stripe2", 136),
    ("rgb", "cycle", "l9", 8192, (63, 5), "stripe2", 137),
    ("pal", "random", "l9", 0, (5, 65), "stripe2", 138),
    ("pal+trns", "f0", "l9", 1, (97, 61), "stripe2", 139),
    ("grey", "f1", "l9", 7, (65, 5), "stripe3", 140),
    ("rgb", "f2", "l9", 8192, (5, 129), "stripe3", 141),
    ("pal", "f3", "l9", 0, (63, 5), "stripe3", 142),
    ("pal+trns", "f4", "l9", 1, (5, 65), "stripe3", 143),
    ("grey", "cycle", "l9", 7, (97, 61), "noise", 144),
    ("rgb", "random", "l9", 8192, (65, 5), "noise", 145),
    ("pal", "f0", "l9", 0, (5, 129), "noise", 146),
    ("pal+trns", "f1", "l9", 1, (63, 5), "noise", 147),
    ("grey", "f2", "flush", 7, (5, 65), "poly", 148),
    ("rgb", "f3", "flush", 8192, (97, 61), "poly", 149),
    ("pal", "f4", "flush", 0, (65, 5), "poly", 150),
    ("pal+trns", "cycle", "flush", 1, (5, 129), "poly", 151),
    ("grey", "random", "flush", 7, (63, 5), "stripe2", 152),
    ("rgb", "f0", "flush", 8192, (5, 65), "stripe2", 153),
    ("pal", "f1", "flush", 0, (97, 61), "stripe2", 154),
    ("pal+trns", "f2", "flush", 1, (65, 5), "stripe2", 155),
    ("grey", "f3", "flush", 7, (5, 129), "stripe3", 156),
    ("rgb", "f4", "flush", 8192, (63, 5), "stripe3", 157),
    ("pal", "cycle", "flush", 0, (5, 65), "stripe3", 158),
    ("pal+trns", "random", "flush", 1, (97, 61), "stripe3", 159),
    ("grey", "f0", "flush", 7, (65, 5), "noise", 160),
    ("rgb", "f1", "flush", 8192, (5, 129), "noise", 161),
    ("pal", "f2", "flush", 0, (63, 5), "noise", 162),
    ("pal+trns", "f3", "flush", 1, (5, 65), "noise", 163),
    ("grey", "f0", "stored", 8192, (640, 360), "far", 164),
    ("pal", "f1", "fixed", 0, (640, 360), "far", 165),
    ("rgb", "f0", "l6", 8192, (640, 360), "far", 166),
    ("pal+trns", "f2", "flush", 0, (640, 360), "far", 167),
]


def case_id(case):
    c, f, d, i, (w, h), content, seed = case
    return "%s-%s-%s-idat%d-%dx%d-%s-%d" % (c, f, d, i, w, h, content, seed)


def channels(colour):
    return 3 if colour == "rgb" else 1


def polygon_map(w, h, seed):
    """a label map with values 0..4: four seeded triangles over background 0"""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((h, w), dtype=np.uint8)
    for k in range(1, 5):
        p = rng.uniform(-0.2, 1.2, size=(3, 2)) * np.array([w, h])
        s = [(p[(j + 1) % 3, 0] - p[j, 0]) * (yy - p[j, 1]) - (p[(j + 1) % 3, 1] - p[j, 1]) * (xx - p[j, 0]) for j in range(3)]
        inside = ((s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)) | ((s[0] <= 0) & (s[1] <= 0) & (s[2] <= 0))
        out[inside] = k
    return out


def pixels(case):
    """the case's image: uint8 [H, W, channels]"""
    colour, _, _, _, (w, h), content, seed = case
    ch = channels(colour)
    rng = np.random.default_rng(seed)
    if content == "poly":
        m = polygon_map(w, h, seed)
        img = np.stack([m, m * 40, 255 - m], axis=-1)[..., :ch]
    elif content in ("stripe2", "stripe3"):
        p = 2 if content == "stripe2" else 3
        vals = rng.integers(0, 256, size=p, dtype=np.uint8)
        img = np.broadcast_to(vals[np.arange(w * ch) % p].reshape(1, w, ch), (h, w, ch))
    elif content == "noise":
        img = rng.integers(0, 256, size=(h, w, ch), dtype=np.uint8)
    elif content == "far":
        base = rng.integers(0, 256, size=FAR_PERIOD, dtype=np.uint8)
        at = np.arange(h)[:, None] * (1 + w * ch) + 1 + np.arange(w * ch)[None, :]        # the byte's place in the raw scanlines
        img = base[at % FAR_PERIOD].reshape(h, w, ch)
    else:
        raise ValueError(content)
    return np.ascontiguousarray(img, dtype=np.uint8)


def row_filters(case):
    """the filter type of every row"""
    _, filt, _, _, (w, h), _, seed = case
    if filt == "cycle":
        return [y % 5 for y in range(h)]
    if filt == "random":
        return [int(v) for v in np.random.default_rng(500 + seed).integers(0, 5, size=h)]
    return [int(filt[1])] * h


def filter_rows(img, types):
    """PNG's forward filters on uint8 [H, W, channels] -> the raw scanlines (filter byte + filtered row, row after row).  The row above the
    first one and the pixel left of the first one are zero."""
    h, w, ch = img.shape
    rows = img.reshape(h, w * ch).astype(np.int32)
    out = np.zeros((h, 1 + w * ch), dtype=np.uint8)
    for y, t in enumerate(types):
        cur = rows[y]
        up = rows[y - 1] if y else np.zeros_like(cur)
        left = np.concatenate([np.zeros(ch, np.int32), cur[:-ch]])
        upleft = np.concatenate([np.zeros(ch, np.int32), up[:-ch]])
        if t == 0:
            pred = 0
        elif t == 1:
            pred = left
        elif t == 2:
            pred = up
        elif t == 3:
            pred = (left + up) >> 1
        else:
            pa, pb, pc = np.abs(up - upleft), np.abs(left - upleft), np.abs(left + up - 2 * upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        out[y, 0] = t
        out[y, 1:] = (cur - pred) & 255
    return out.tobytes()


def deflate(raw, mode):
    if mode == "stored":
        return zlib.compress(raw, 0)
    if mode == "fixed":
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        return c.compress(raw) + c.flush()
    if mode in ("l6", "l9"):
        return zlib.compress(raw, int(mode[1]))
    if mode == "flush":
        c = zlib.compressobj(6)
        parts = []
        for o in range(0, len(raw), FLUSH_EVERY):
            parts.append(c.compress(raw[o:o + FLUSH_EVERY]))
            parts.append(c.flush(zlib.Z_FULL_FLUSH))
        parts.append(c.flush())
        return b"".join(parts)
    raise ValueError(mode)


def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def write_png(w, h, ctype, stream, idat=0, plte=None, trns=None, depth=8, interlace=0):
    """a PNG file around a finished zlib stream; idat: 0 = one IDAT chunk, else IDAT chunks of that many bytes"""
    out = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))]
    if plte is not None:
        out.append(chunk(b"PLTE", plte))
    if trns is not None:
        out.append(chunk(b"tRNS", trns))
    step = idat if idat else max(1, len(stream))
    for o in range(0, len(stream), step):
        out.append(chunk(b"IDAT", stream[o:o + step]))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def raw_scanlines(case):
    return filter_rows(pixels(case), row_filters(case))


_CACHE = {}


def encode(case):
    """the case's PNG file (cached)"""
    if case not in _CACHE:
        colour, _, mode, idat, (w, h), _, seed = case
        stream = deflate(raw_scanlines(case), mode)
        plte = trns = None
        if colour.startswith("pal"):
            plte = np.random.default_rng(77 + seed).integers(0, 256, size=768, dtype=np.uint8).tobytes()
            if colour == "pal+trns":
                trns = bytes((i * 7) & 255 for i in range(40))
        _CACHE[case] = write_png(w, h, {"grey": 0, "rgb": 2}.get(colour, 3), stream, idat, plte, trns)
    return _CACHE[case]


def expected(data):
    """PIL's word on the bytes: dataset.imread_label"""
    from multitask_hydranet_amd.dataset import imread_label
    return imread_label(io.BytesIO(data))


def first_block_type(stream):
    """BTYPE of a zlib stream's first deflate block (bits 1..2 of the byte behind the two header bytes)"""
    return (stream[2] >> 1) & 3


def big_label(seed=0, w=1920, h=1080):
    """a 1080x1920 polygon label map, values 0..4"""
    return polygon_map(w, h, 9000 + seed)


def big_files():
    """the two 1080x1920 polygon labels as PIL's own encoder writes them: default settings, and optimize=True"""
    if "big" not in _CACHE:
        from PIL import Image
        out = []
        for k, kw in enumerate(({}, {"optimize": True})):
            bio = io.BytesIO()
            Image.fromarray(big_label(k)).save(bio, "PNG", **kw)
            out.append(bio.getvalue())
        _CACHE["big"] = out
    return _CACHE["big"]
