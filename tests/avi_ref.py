"""Test-side AVI container reference, independent of multitask_hydranet_amd/avi.py (`struct` only): a minimal muxer for the files the reader
is held to, a generic RIFF walker for the files the writer produces, and the five-frame Motion-JPEG clip the video tests share.  The
reader is never checked against our own writer only, nor the writer against our own reader only."""
import functools
import io
import struct

import numpy as np

from tests import jpeg_cases as C

CLIP_FRAME = "frame_1570x660.jpg"
CLIP_STRIPPED = (1, 3)                   # the frames of the clip that carry no DHT segment


def chunk(cid, payload):
    return cid + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def riff_list(kind, body):
    return b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body


def _strh(kind, handler, scale, rate, length, sample_size, width, height):
    # fccType fccHandler dwFlags wPriority wLanguage dwInitialFrames dwScale dwRate dwStart dwLength dwSuggestedBufferSize dwQuality dwSampleSize rcFrame
    return struct.pack("<4s4sIHHIIIIIIII4h", kind, handler, 0, 0, 0, 0, scale, rate, 0, length, 0, 0xFFFFFFFF, sample_size, 0, 0, width, height)


def mux(items, width, height, rate, scale, fourcc=b"MJPG", idx1=True, audio=False, junk=True):
    """items: the movi list in file order -- (chunk id, payload) or (b"rec ", [(chunk id, payload), ...]); -> (the file's bytes, [(payload offset, size)]
    of the video stream's 00dc / 00db chunks in file order).
    audio: a second stream (auds) in the header, whose 01wb chunks the items may hold; junk: a JUNK chunk in hdrl and one before movi."""
    n = sum(1 for cid, p in _flat(items) if cid in (b"00dc", b"00db"))
    avih = struct.pack("<14I", 1000000 * scale // rate, 0, 0, 0x10 if idx1 else 0, n, 0, 2 if audio else 1, 0, width, height, 0, 0, 0, 0)
    strh = _strh(b"vids", fourcc, scale, rate, n, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, fourcc, width * height * 3, 0, 0, 0, 0)
    hdrl = chunk(b"avih", avih) + riff_list(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf))
    if audio:
        astrh = _strh(b"auds", b"\0\0\0\0", 1, 8000, 0, 1, 0, 0)
        astrf = struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8)
        hdrl += riff_list(b"strl", chunk(b"strh", astrh) + chunk(b"strf", astrf))
    if junk:
        hdrl += chunk(b"JUNK", b"\0" * 13)
    body = riff_list(b"hdrl", hdrl)
    if junk:
        body += chunk(b"JUNK", b"\0" * 20)
    movi, index = b"", []
    for it in items:
        if it[0] == b"rec ":
            inner = b""
            for cid, p in it[1]:
                index.append((cid, 4 + len(movi) + 12 + len(inner), len(p)))
                inner += chunk(cid, p)
            movi += riff_list(b"rec ", inner)
        else:
            index.append((it[0], 4 + len(movi), len(it[1])))
            movi += chunk(*it)
    movi_pos = 12 + len(body) + 8                                        # of the 'movi' fourcc
    body += riff_list(b"movi", movi)
    spans = [(movi_pos + off + 8, size) for cid, off, size in index if cid in (b"00dc", b"00db")]
    if idx1:
        body += chunk(b"idx1", b"".join(struct.pack("<4sIII", cid, 0x10, off, size) for cid, off, size in index))
    data = b"RIFF" + struct.pack("<I", 4 + len(body)) + b"AVI " + body
    for off, size in spans:
        assert data[off - 8:off - 6] == b"00" and struct.unpack_from("<I", data, off - 4)[0] == size
    return data, spans


def _flat(items):
    for it in items:
        if it[0] == b"rec ":
            yield from it[1]
        else:
            yield it


def walk(data):
    """a file AviWriter wrote -> everything a player reads from it: {"riff_size", "width", "height", "rate", "scale", "handler",
    "compression", "bit_count", "avih_frames", "strh_length", "movi_size", "movi_pos" (of the 'movi' fourcc), "frames": [bytes],
    "chunk_pos": [offset of every frame's chunk header], "idx1": [(id, flags, offset, size)], "end": where the walk ended}"""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI ", data[:12]
    out = {"riff_size": struct.unpack_from("<I", data, 4)[0], "frames": [], "chunk_pos": [], "idx1": []}

    def visit(pos, end, path):
        while pos + 8 <= end:
            cid, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
            body = pos + 8
            assert body + size <= end, (path, cid, pos, size, end)
            if cid == b"LIST":
                kind = data[body:body + 4]
                if kind == b"movi":
                    out["movi_size"], out["movi_pos"] = size, body
                visit(body + 4, body + size, path + (kind,))
            elif cid == b"avih":
                f = struct.unpack_from("<14I", data, body)
                out["usec"], out["avih_frames"], out["streams"], out["avih_wh"] = f[0], f[4], f[6], (f[8], f[9])
            elif cid == b"strh":
                assert data[body:body + 4] == b"vids"
                out["handler"] = data[body + 4:body + 8]
                out["scale"], out["rate"], _, out["strh_length"] = struct.unpack_from("<4I", data, body + 20)
            elif cid == b"strf":
                _, out["width"], out["height"], _, out["bit_count"], out["compression"] = struct.unpack_from("<IiiHH4s", data, body)
            elif cid == b"00dc" and path[-1:] == (b"movi",):
                out["frames"].append(data[body:body + size])
                out["chunk_pos"].append(pos)
            elif cid == b"idx1":
                out["idx1"] = [struct.unpack_from("<4sIII", data, body + 16 * k) for k in range(size // 16)]
            pos = body + size + (size & 1)
        return pos

    out["end"] = visit(12, 8 + out["riff_size"], ())
    return out


# ---- the clip --------------------------------------------------------------------------------------------------------------------------
def strip_dht(jpeg):
    """the stream without its DHT segments (a table-less Motion-JPEG frame when the tables were the standard ones)"""
    out, pos = jpeg[:2], 2
    while True:
        assert jpeg[pos] == 0xFF, pos
        m = jpeg[pos + 1]
        ln = struct.unpack_from(">H", jpeg, pos + 2)[0]
        if m == 0xDA:
            return out + jpeg[pos:]
        if m != 0xC4:
            out += jpeg[pos:pos + 2 + ln]
        pos += 2 + ln


@functools.lru_cache(maxsize=None)
def clip():
    """five frames of one size: frame t = the golden 1570 x 660 picture rolled by 16 t pixels along x, re-encoded by PIL at quality 90,
    4:2:2, standard Huffman tables; frames CLIP_STRIPPED then lose their DHT segments.  -> (frames as stored in the AVI, the same frames
    with their tables kept)"""
    from PIL import Image
    with Image.open(io.BytesIO(C.golden_bytes(CLIP_FRAME))) as im:
        rgb = np.asarray(im.convert("RGB"))
    full = []
    for t in range(5):
        bio = io.BytesIO()
        Image.fromarray(np.roll(rgb, 16 * t, axis=1)).save(bio, "JPEG", quality=90, subsampling="4:2:2", optimize=False)
        full.append(bio.getvalue())
    stored = [strip_dht(f) if t in CLIP_STRIPPED else f for t, f in enumerate(full)]
    for t in CLIP_STRIPPED:
        assert b"\xff\xc4" not in stored[t][:stored[t].index(b"\xff\xda")] and len(stored[t]) < len(full[t])
    return tuple(stored), tuple(full)


CLIP_W, CLIP_H = 1570, 660
