"""PNG label encode on the device (hn_png_enc.hip), the mirror image of png.py: class maps -- the int64 [N, Hs, Ws] mask of
ops.argmax_channels / the deploy forward, or packed uint8 maps in augment.pack's layout -- are resized to a per-image (Ho, Wo) with cv2's
INTER_NEAREST index rule, filtered row by row (the five PNG filters, smallest sum of |int8|) and deflated on the device -- with one
fixed-Huffman block per chunk or, huffman="dynamic", with blocks of 16 chunks whose code is built from their own tokens; the host only
frames the few KB that come back (signature, IHDR, an optional PLTE, one IDAT, IEND, with zlib.crc32).

    files = png_encode.encode_batch(mask, out_sizes=[(1080, 1920)] * n)                 # list of bytes: 8-bit grey PNG files
    files = png_encode.encode_batch(mask, palette={0: (0, 0, 0), 1: (128, 0, 128)})     # colour type 3, the same index bytes
    png_encode.imwrite("seg.png", class_map)

An image the device reports a non-zero status for (its stream outgrew the capacity it was given) is encoded on the host, that image only:
the same resize and filters in numpy, then zlib.compress.  A class id outside 0..255 has no 8-bit PNG: ValueError."""
from __future__ import annotations

import struct
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import lib
from .png import SIGNATURE

# hn_png_enc.hip struct PngEncDesc / PngEncResult
DESC_DTYPE = np.dtype({
    "names": ["src_off", "raw_off", "out_off", "out_cap", "Hs", "Ws", "Ho", "Wo"],
    "formats": ["<i8", "<i8", "<i8", "<i8", "<i4", "<i4", "<i4", "<i4"],
    "offsets": [0, 8, 16, 24, 32, 36, 40, 44],
    "itemsize": 64})
RESULT_DTYPE = np.dtype({"names": ["stream_bytes", "status"], "formats": ["<i8", "<i4"], "offsets": [0, 8], "itemsize": 16})

STATUS = {0: "encoded", 1: "a class id outside 0..255", 2: "the stream is longer than its capacity", 3: "record does not fit the buffers"}
ST_RANGE, ST_FULL, ST_RECORD = 1, 2, 3


# ------------------------------------------------------------------------------------------------ host: framing and the fallback

def _chunk(kind: bytes, payload: bytes) -> bytes:
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def palette_bytes(palette: Dict[int, Sequence[int]]) -> bytes:
    """{id: (r, g, b)} -> the PLTE payload: entries 0..max id, black where the dict has none"""
    n = max(int(k) for k in palette) + 1
    assert 1 <= n <= 256 and min(int(k) for k in palette) >= 0, sorted(palette)
    lut = np.zeros((n, 3), np.uint8)
    for k, c in palette.items():
        lut[int(k)] = np.asarray(c, dtype=np.int64).astype(np.uint8)[:3]
    return lut.tobytes()


def assemble(width: int, height: int, stream: bytes, palette: Optional[Dict[int, Sequence[int]]] = None) -> bytes:
    """the zlib stream of the filtered scanlines -> a PNG file: bit depth 8, non-interlaced, colour type 0 (grey), or 3 with a PLTE when
    a palette is given (the stream holds the same index bytes either way).  Host only."""
    assert 1 <= width <= 65535 and 1 <= height <= 65535, (width, height)
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 3 if palette is not None else 0, 0, 0, 0)
    out = [SIGNATURE, _chunk(b"IHDR", ihdr)]
    if palette is not None:
        out.append(_chunk(b"PLTE", palette_bytes(palette)))
    out += [_chunk(b"IDAT", bytes(stream)), _chunk(b"IEND", b"")]
    return b"".join(out)


def resize_nearest(m: np.ndarray, out_hw) -> np.ndarray:
    """cv2.resize(m, (Wo, Ho), interpolation=cv2.INTER_NEAREST): source index min(floor(x * (1 / (Wo / Ws))), Ws - 1) in float64"""
    hs, ws = m.shape
    ho, wo = int(out_hw[0]), int(out_hw[1])
    sx = np.minimum(np.floor(np.arange(wo, dtype=np.float64) * (1.0 / (float(wo) / float(ws)))).astype(np.int64), ws - 1)
    sy = np.minimum(np.floor(np.arange(ho, dtype=np.float64) * (1.0 / (float(ho) / float(hs)))).astype(np.int64), hs - 1)
    return m[sy][:, sx]


def filter_rows(img: np.ndarray) -> np.ndarray:
    """uint8 H x W -> the H x (1 + W) filtered scanlines: per row the PNG filter (bpp = 1, zeros above row 0) with the smallest sum of
    |(int8) byte|, ties to the lowest filter number"""
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    cur = img.astype(np.int32)
    a = np.zeros_like(cur); a[:, 1:] = cur[:, :-1]
    b = np.zeros_like(cur); b[1:] = cur[:-1]
    c = np.zeros_like(cur); c[1:, 1:] = cur[:-1, :-1]
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([cur, cur - a, cur - b, cur - ((a + b) >> 1), cur - paeth], 0) & 255          # [5, H, W]
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)                                      # [5, H]
    ft = np.argmin(cost, axis=0)                                                                    # the first minimum
    out = np.empty((h, 1 + w), np.uint8)
    out[:, 0] = ft
    out[:, 1:] = cand[ft, np.arange(h)]
    return out


def _check_range(m: np.ndarray) -> np.ndarray:
    m = np.asarray(m)
    assert m.ndim == 2 and m.dtype.kind in "iu", (m.dtype, m.shape)
    if m.size and (int(m.min()) < 0 or int(m.max()) > 255):
        raise ValueError("a class id outside 0..255 has no 8-bit PNG (found %d..%d)" % (int(m.min()), int(m.max())))
    return m.astype(np.uint8)


def host_stream(m: np.ndarray, out_hw=None, level: int = 6) -> bytes:
    """the per-image fallback: one class map (any integer dtype, values 0..255) -> the zlib stream of its filtered scanlines, on the host"""
    m = _check_range(m)
    if out_hw is not None:
        m = resize_nearest(m, out_hw)
    return zlib.compress(filter_rows(np.ascontiguousarray(m)).tobytes(), level)


def encode_host(m: np.ndarray, out_hw=None, palette=None) -> bytes:
    """one class map -> a PNG file without the device"""
    hw = tuple(int(v) for v in (out_hw if out_hw is not None else np.asarray(m).shape))
    return assemble(hw[1], hw[0], host_stream(m, out_hw), palette)


# ------------------------------------------------------------------------------------------------ device

def chunk_bytes() -> int:
    return int(lib().query("hn_png_enc_chunk_bytes"))


def capacity(raw_bytes: int) -> int:
    """a capacity no stream of `raw_bytes` filtered bytes exceeds (hn_png_enc_cap_bytes)"""
    c = int(lib().query("hn_png_enc_cap_bytes", int(raw_bytes)))
    assert c > 0, raw_bytes
    return c


def describe(src_shapes, src_offs, out_sizes, caps) -> Tuple[np.ndarray, np.ndarray, int, int]:
    """-> (descriptors, byte offsets of every image's stream slot [n + 1], the largest Ho, the largest raw size); the slots are the
    capacities rounded up to 16, back to back"""
    n = len(src_shapes)
    desc = np.zeros(n, dtype=DESC_DTYPE)
    raws = [int(ho) * (1 + int(wo)) for ho, wo in out_sizes]
    max_raw = max(raws)
    slot = (max_raw + 15) // 16 * 16
    ooff = np.zeros(n + 1, dtype=np.int64)
    ooff[1:] = np.cumsum([(int(c) + 15) // 16 * 16 for c in caps])
    for i in range(n):
        e = desc[i]
        e["src_off"], e["raw_off"], e["out_off"], e["out_cap"] = int(src_offs[i]), i * slot, int(ooff[i]), int(caps[i])
        e["Hs"], e["Ws"], e["Ho"], e["Wo"] = int(src_shapes[i][0]), int(src_shapes[i][1]), int(out_sizes[i][0]), int(out_sizes[i][1])
    return desc, ooff, max(int(ho) for ho, _ in out_sizes), max_raw


def _as_source(maps, device):
    """-> (flat device tensor, is_int64, per-image (Hs, Ws), per-image element offsets)"""
    import torch
    dev = torch.device(device) if device is not None else None
    if isinstance(maps, dict):
        data = maps["data"]
        assert data.dtype == torch.uint8, data.dtype
        dev = dev or (data.device if data.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        shapes = [tuple(int(v) for v in s) for s in np.asarray(maps["shapes"]).reshape(-1, 2)]
        return data.to(dev).contiguous().view(-1), False, shapes, [int(o) for o in np.asarray(maps["offsets"]).reshape(-1)]
    if torch.is_tensor(maps):
        if maps.dim() == 2:
            maps = maps[None]
        assert maps.dim() == 3 and maps.dtype in (torch.int64, torch.uint8), (maps.dtype, tuple(maps.shape))
        dev = dev or (maps.device if maps.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        n, hs, ws = (int(v) for v in maps.shape)
        return maps.to(dev).contiguous().view(-1), maps.dtype == torch.int64, [(hs, ws)] * n, [i * hs * ws for i in range(n)]
    arrs = [np.asarray(maps)] if isinstance(maps, np.ndarray) and maps.ndim == 2 else [np.asarray(a) for a in maps]
    dev = dev or torch.device("cuda", torch.cuda.current_device())
    if all(a.dtype == np.uint8 for a in arrs):
        from .augment import pack
        return _as_source(pack(arrs), dev)
    offs = np.concatenate([[0], np.cumsum([a.size for a in arrs])])
    flat = np.concatenate([a.astype(np.int64).reshape(-1) for a in arrs])
    return torch.from_numpy(flat).to(dev), True, [tuple(a.shape) for a in arrs], [int(o) for o in offs[:-1]]


HUFFMAN = {"fixed": ("hn_png_encode", "hn_png_enc_ws_bytes"), "dynamic": ("hn_png_encode_dyn", "hn_png_enc_dyn_ws_bytes")}


def _entry(huffman: str) -> Tuple[str, str]:
    if huffman not in HUFFMAN:
        raise ValueError("huffman must be 'fixed' or 'dynamic', not %r" % (huffman,))
    return HUFFMAN[huffman]


def block_chunks() -> int:
    """chunks per deflate block of huffman="dynamic" streams"""
    return int(lib().query("hn_png_enc_block_chunks"))


def encode_streams(maps, out_sizes=None, cap=None, device=None, lean: bool = False, huffman: str = "fixed") -> dict:
    """the device part, nothing read back: maps -- an int64 (or uint8) tensor [N, Hs, Ws], a packed uint8 dict of augment.pack's layout, or
    a list of H x W integer arrays; out_sizes: one (Ho, Wo) or one per image, the source sizes without; cap: bytes per stream slot (one
    value or one per image, rounded down to a multiple of 4; default: what no stream exceeds, hn_png_enc_cap_bytes -- with lean, at most
    64 KB plus a quarter of the raw size).  -> {"buf": device
    uint8 tensor, the N result records (RESULT_DTYPE) then the stream slots; "rbytes": where the slots start; "offsets" [n + 1]: every
    slot's byte offset behind rbytes; "caps"; "sizes": the (Ho, Wo); "src": (flat tensor, is_int64, shapes, offsets)}.  One launch
    sequence on the current stream.  huffman: "fixed" -- one fixed-Huffman block per chunk -- or "dynamic" -- one block per 16 chunks with
    a code built from its own tokens where that is smaller (hn_png_encode_dyn): never longer, on label maps less than half the bytes."""
    import torch
    entry, ws_query = _entry(huffman)
    src, is_i64, shapes, soffs = _as_source(maps, device)
    n = len(shapes)
    assert n > 0
    if out_sizes is None:
        sizes = list(shapes)
    elif np.ndim(out_sizes) == 1:
        sizes = [(int(out_sizes[0]), int(out_sizes[1]))] * n
    else:
        sizes = [(int(h), int(w)) for h, w in out_sizes]
    assert len(sizes) == n and all(1 <= h <= 65535 and 1 <= w <= 65535 for h, w in sizes), sizes
    if cap is None:
        caps = _default_caps(sizes) if lean else [capacity(h * (1 + w)) for h, w in sizes]
    else:
        caps = [int(cap) // 4 * 4] * n if np.isscalar(cap) else [int(c) // 4 * 4 for c in cap]
    assert len(caps) == n and min(caps) >= 0, caps
    desc, ooff, max_h, max_raw = describe(shapes, soffs, sizes, caps)
    rbytes = (n * RESULT_DTYPE.itemsize + 15) // 16 * 16
    with torch.cuda.device(src.device):
        ws_bytes = int(lib().query(ws_query, n, max_raw))
        assert ws_bytes > 0, (n, max_raw)
        ws = torch.empty((ws_bytes,), device=src.device, dtype=torch.uint8)
        desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(src.device)
        buf = torch.empty((rbytes + max(int(ooff[-1]), 16),), device=src.device, dtype=torch.uint8)
        lib().call(entry, src.data_ptr(), int(src.numel()), int(is_i64), desc_d.data_ptr(), n, max_h, max_raw, ws.data_ptr(), ws_bytes,
                   buf.data_ptr() + rbytes, max(int(ooff[-1]), 16), buf.data_ptr())
    return {"buf": buf, "rbytes": rbytes, "offsets": ooff, "caps": caps, "sizes": sizes, "src": (src, is_i64, shapes, soffs), "ws": ws}


def _default_caps(sizes) -> List[int]:
    # a label map deflates to a small fraction of its raw size; what does not fit a quarter of it (noise) goes to the host's zlib, so the
    # one copy back stays small
    return [min(capacity(h * (1 + w)), ((1 << 16) + h * (1 + w) // 4) // 4 * 4) for h, w in sizes]


def encode_batch(maps, out_sizes=None, palette=None, cap=None, device=None, huffman: str = "fixed") -> List[bytes]:
    """class maps -> whole PNG files (bit depth 8, colour type 0, or 3 with palette = {id: (r, g, b)}; non-interlaced, one IDAT).  One
    launch sequence (encode_streams) and ONE copy of the result records and the streams through a pinned staging buffer; an image whose
    stream outgrew its capacity (status "full") is encoded on the host (host_stream), that image only.  A class id outside 0..255 raises
    ValueError; a record the device refuses is a bug in the caller's buffers and raises RuntimeError.  huffman: see encode_streams."""
    import torch
    from .jpeg_encode import _staging
    st = encode_streams(maps, out_sizes, cap, device, lean=True, huffman=huffman)
    buf, rbytes, ooff, sizes = st["buf"], st["rbytes"], st["offsets"], st["sizes"]
    n = len(sizes)
    with torch.cuda.device(buf.device):
        stage = _staging(buf.device, int(buf.numel()))
        stage.copy_(buf, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    host = stage.numpy()
    res = host[:n * RESULT_DTYPE.itemsize].view(RESULT_DTYPE)
    files = []
    for i, (ho, wo) in enumerate(sizes):
        if int(res["status"][i]) == 0:
            o = rbytes + int(ooff[i])
            stream = host[o:o + int(res["stream_bytes"][i])].tobytes()
        elif int(res["status"][i]) == ST_FULL:
            stream = host_stream(source_map(st["src"], i), (ho, wo))
        elif int(res["status"][i]) == ST_RANGE:
            raise ValueError("image %d: a class id outside 0..255 has no 8-bit PNG" % i)
        else:
            raise RuntimeError("%s: image %d: %s" % (_entry(huffman)[0], i, STATUS.get(int(res["status"][i]), int(res["status"][i]))))
        files.append(assemble(wo, ho, stream, palette))
    return files


def source_map(src, i: int) -> np.ndarray:
    """image i of encode_streams' "src" on the host"""
    flat, _, shapes, offs = src
    hs, ws = shapes[i]
    return flat[offs[i]:offs[i] + hs * ws].view(hs, ws).cpu().numpy()


def imwrite(path, class_map, out_size=None, palette=None, device=None, huffman: str = "fixed") -> None:
    """one class map (H x W integer array, or a [H, W] / [1, H, W] tensor) -> one PNG file"""
    blobs = encode_batch(class_map, out_size, palette, device=device, huffman=huffman)
    assert len(blobs) == 1
    with open(path, "wb") as f:
        f.write(blobs[0])


__all__ = ["encode_batch", "encode_streams", "assemble", "imwrite", "host_stream", "encode_host", "resize_nearest", "filter_rows", "describe",
           "capacity", "chunk_bytes", "block_chunks", "source_map", "STATUS", "DESC_DTYPE", "RESULT_DTYPE"]
