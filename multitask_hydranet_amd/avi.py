"""Motion-JPEG in an AVI container, host side: the reference's demo reads a video with cv2.VideoCapture and writes one with
cv2.VideoWriter; cv2 is absent here, and a Motion-JPEG AVI is a RIFF chunk list around a sequence of baseline JPEGs, which the project
decodes and encodes itself (jpeg.py, jpeg_encode.py).  Pure Python, `struct` only.

    index = avi.read_index(path_or_bytes)        # width, height, rate / scale, fourcc, frames [(offset, size)], truncated
    data = avi.frame_bytes(index, data, i)       # the JPEG of frame i (None: "repeat the previous frame"), Huffman tables spliced in
    with avi.AviWriter(path, width, height, fps=(10, 1)) as out:
        out.write(jpeg_bytes)

The subset read: AVI 1.0 (one RIFF 'AVI ' segment; OpenDML 'AVIX' extension segments are refused), the first video stream, compression
MJPG; the frames are found by walking 'movi' (through LIST 'rec ' groups, past other streams' chunks and JUNK, honouring the pad byte
after an odd-sized chunk), never through 'idx1', which an interrupted recording lacks.  The subset written: 'hdrl' (avih, one strl of
strh vids / MJPG and strf BITMAPINFOHEADER), 'movi' of 00dc chunks, 'idx1'; below 2 GiB."""
from __future__ import annotations

import struct
from typing import Optional

# ITU-T T.81 Annex K.3: BITS and HUFFVAL of the four typical Huffman tables -- csrc/hn_jpeg_tables.h restated (tests/test_avi_cpu.py holds
# the two to each other).  A Motion-JPEG frame commonly leaves its DHT segments out and means these.
STD_DC_BITS = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0))
STD_DC_VALS = tuple(range(12))
STD_AC_BITS = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77))
STD_AC_VALS = (
    (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa),
    (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa))

MAX_FILE_BYTES = (1 << 31) - 1           # AVI 1.0: what lies past 2 GiB needs OpenDML segments, which are neither read nor written here


def std_dht_segment() -> bytes:
    """one DHT segment holding the four standard tables: DC 0, AC 0, DC 1, AC 1"""
    body = b""
    for t in (0, 1):
        body += bytes([0x00 | t]) + bytes(STD_DC_BITS[t]) + bytes(STD_DC_VALS)
        body += bytes([0x10 | t]) + bytes(STD_AC_BITS[t]) + bytes(STD_AC_VALS[t])
    return b"\xff\xc4" + struct.pack(">H", 2 + len(body)) + body


def _u32(data, pos: int) -> int:
    return struct.unpack_from("<I", data, pos)[0]


def _chunks(data, pos: int, end: int):
    """the chunks of [pos, end): (fourcc, payload offset, declared size); stops at the first header that does not fit"""
    while pos + 8 <= end:
        size = _u32(data, pos + 4)
        yield bytes(data[pos:pos + 4]), pos + 8, size
        pos += 8 + size + (size & 1)                                    # the pad byte after an odd-sized chunk


def read_index(path_or_bytes) -> dict:
    """-> {"width", "height", "rate", "scale" (frames per second = rate / scale), "fourcc" (the compression, as in the file), "stream" (the
    video stream's number), "frames": [(offset, size)] of its chunks in file order (size 0 = repeat the previous frame), "truncated": a
    chunk ran past the end of the file and the list ends at the last complete frame}.  ValueError for what is no AVI, has no video
    stream, is not Motion-JPEG, or continues in OpenDML 'AVIX' segments."""
    if isinstance(path_or_bytes, str) or hasattr(path_or_bytes, "__fspath__"):
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    else:
        data = path_or_bytes                                            # bytes, or anything that slices like them (an mmap)
    n = len(data)
    if n < 12 or bytes(data[0:4]) != b"RIFF" or bytes(data[8:12]) != b"AVI ":
        raise ValueError("not a RIFF AVI file")
    riff_end = 8 + _u32(data, 4)
    if riff_end + 12 <= n and bytes(data[riff_end:riff_end + 4]) == b"RIFF" and bytes(data[riff_end + 8:riff_end + 12]) == b"AVIX":
        raise ValueError("OpenDML AVI (RIFF AVIX extension segments) is not supported")
    end = n if riff_end > n or riff_end <= 12 else riff_end              # an unpatched or overlong size field: walk what is there
    info = {"width": 0, "height": 0, "rate": 0, "scale": 0, "fourcc": "", "stream": -1, "frames": [], "truncated": False}
    movi = None
    for cid, off, size in _chunks(data, 12, end):
        if cid != b"LIST" or off + 4 > n:
            continue
        kind = bytes(data[off:off + 4])
        if kind == b"hdrl":
            _read_hdrl(data, off + 4, min(off + size, n), info)
        elif kind == b"movi" and movi is None:
            movi = (off + 4, off + size if 4 <= size and off + size <= n else n, off + size > n)
    if info["stream"] < 0:
        raise ValueError("no video stream in the AVI header")
    if info["fourcc"].upper() != "MJPG":
        raise ValueError("compression %r is not Motion-JPEG (MJPG)" % info["fourcc"])
    if movi is None:
        raise ValueError("no movi list")
    tags = (b"%02ddc" % info["stream"], b"%02ddb" % info["stream"])
    complete = _walk_movi(data, movi[0], movi[1], n, tags, info["frames"])
    info["truncated"] = movi[2] or not complete                       # the movi list itself, or a chunk in it, runs past the end
    return info


def _read_hdrl(data, pos: int, end: int, info: dict) -> None:
    stream = 0
    for cid, off, size in _chunks(data, pos, end):
        if cid == b"avih" and size >= 40 and off + 40 <= end:
            info["width"], info["height"] = _u32(data, off + 32), _u32(data, off + 36)
        elif cid == b"LIST" and bytes(data[off:off + 4]) == b"strl":
            strh = strf = None
            for c2, o2, s2 in _chunks(data, off + 4, min(off + size, end)):
                if c2 == b"strh" and s2 >= 48:
                    strh = o2
                elif c2 == b"strf" and s2 >= 40:
                    strf = o2
            if info["stream"] < 0 and strh is not None and bytes(data[strh:strh + 4]) == b"vids":
                info["stream"] = stream
                info["scale"], info["rate"] = _u32(data, strh + 20), _u32(data, strh + 24)
                fourcc = bytes(data[strh + 4:strh + 8])
                if strf is not None:
                    w, h = struct.unpack_from("<ii", data, strf + 4)
                    info["width"], info["height"] = w, abs(h)
                    fourcc = bytes(data[strf + 16:strf + 20])
                info["fourcc"] = fourcc.decode("latin-1")
            stream += 1


def _walk_movi(data, pos: int, end: int, n: int, tags, frames: list) -> bool:
    """appends the stream's chunks; False when a chunk runs past the end of the file (the walk stops there)"""
    for cid, off, size in _chunks(data, pos, end):
        if cid == b"LIST":
            if off + 4 <= n and bytes(data[off:off + 4]) == b"rec ":
                if not _walk_movi(data, off + 4, min(off + size, n), n, tags, frames):
                    return False
            if off + size > n:
                return False
            continue
        if off + size > n:
            return False
        if cid in tags:
            frames.append((off, size))
    return True


def has_dht(jpeg: bytes) -> Optional[int]:
    """None when a DHT segment precedes the first scan (or the stream cannot be walked); else the offset of the SOS marker"""
    pos, n = 2, len(jpeg)
    if n < 4 or jpeg[0:2] != b"\xff\xd8":
        return None
    while pos + 4 <= n:
        if jpeg[pos] != 0xFF:
            return None
        m = jpeg[pos + 1]
        if m == 0xFF:                                                   # a fill byte
            pos += 1
            continue
        if m == 0xC4:
            return None
        if m == 0xDA:
            return pos
        if m == 0x01 or 0xD0 <= m <= 0xD7:                               # markers without a length
            pos += 2
            continue
        pos += 2 + struct.unpack_from(">H", jpeg, pos + 2)[0]
    return None


def frame_bytes(index: dict, data, i: int) -> Optional[bytes]:
    """the JPEG of frame i of `index` (read_index's) out of the file's bytes `data`; None for a zero-length chunk, AVI's "repeat the
    previous frame".  A frame without a DHT segment gets the standard tables spliced in before its SOS, so every decoder of the project
    (and PIL) takes it as it is; a frame that has its own is returned byte for byte."""
    off, size = index["frames"][i]
    if size == 0:
        return None
    jpeg = bytes(data[off:off + size])
    sos = has_dht(jpeg)
    if sos is None:
        return jpeg
    return jpeg[:sos] + std_dht_segment() + jpeg[sos:]


class AviWriter:
    """cv2.VideoWriter(path, MJPG, fps, (width, height)) for frames that are JPEG streams already: every write() appends one 00dc chunk;
    close() writes idx1 and patches the sizes and frame counts.  fps = (rate, scale); 10 / 1 is the reference's."""

    _MOVI_LIST = 12 + 8 + 4 + (8 + 56) + 8 + 4 + (8 + 56) + (8 + 40)         # offset of the movi LIST header

    def __init__(self, path, width: int, height: int, fps=(10, 1)):
        self.width, self.height = int(width), int(height)
        self.rate, self.scale = int(fps[0]), int(fps[1])
        assert self.width > 0 and self.height > 0 and self.rate > 0 and self.scale > 0, (width, height, fps)
        self._index = []                                                # (offset relative to the 'movi' fourcc, size)
        self._max = 0
        self._f = open(path, "wb")
        self._f.write(self._header(0, 0))
        self._pos = self._MOVI_LIST + 12

    def _header(self, movi_bytes: int, idx_bytes: int) -> bytes:
        n = len(self._index)
        usec = (1000000 * self.scale + self.rate // 2) // self.rate
        avih = struct.pack("<14I", usec, 0, 0, 0x10 if idx_bytes else 0, n, 0, 1, self._max, self.width, self.height, 0, 0, 0, 0)       # AVIF_HASINDEX
        strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._max, 0xFFFFFFFF, 0, 0, 0,
                           self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh \
            + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        head = b"RIFF" + struct.pack("<I", 4 + len(hdrl) + 12 + movi_bytes + idx_bytes) + b"AVI " + hdrl
        assert len(head) == self._MOVI_LIST, len(head)
        return head + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"

    def write(self, jpeg: bytes) -> None:
        if self._f is None:
            raise ValueError("write() on a closed AviWriter")
        size = len(jpeg)
        grown = self._pos + 8 + size + (size & 1) + 8 + 16 * (len(self._index) + 1)
        if grown > MAX_FILE_BYTES:
            raise ValueError("the AVI file would pass 2 GiB (%d bytes with this frame and its index)" % grown)
        self._f.write(b"00dc" + struct.pack("<I", size) + jpeg + (b"\0" if size & 1 else b""))
        self._index.append((self._pos - (self._MOVI_LIST + 8), size))
        self._pos += 8 + size + (size & 1)
        self._max = max(self._max, size)

    def close(self) -> None:
        if self._f is None:
            return
        idx = b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, size) for off, size in self._index)                      # AVIIF_KEYFRAME
        self._f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        self._f.seek(0)
        self._f.write(self._header(self._pos - (self._MOVI_LIST + 12), 8 + len(idx)))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


__all__ = ["read_index", "frame_bytes", "AviWriter", "std_dht_segment", "has_dht", "MAX_FILE_BYTES"]
