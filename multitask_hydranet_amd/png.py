"""PNG label decode on the device (hn_png.hip): the host only walks the chunk list -- in a DataLoader worker, without a GPU --
and the zlib stream crosses to the device as it lies in the file; inflate (stored, fixed and dynamic blocks, Adler-32 checked) and the five
row filters run there, and channel 0 of every pixel is written straight into the packed label layout of augment.pack(), so that
augment.augment_batch takes the result as its `segs`.  All integer: the maps equal dataset.imread_label's element for element.

    head = png.parse(data)                       # None: outside the supported set, decode that image with PIL
    head, idat = png.stream_stage(data)          # host only: the concatenated IDAT payloads
    segs = png.decode_batch(png.pack_streams([(head, idat), ...]))      # {"data" (device uint8), "offsets", "shapes", "status"}

An image whose stream the device rejects (a non-zero status word, read back once per batch) is decoded with PIL, that image only.

Supported: bit depth 8, colour type 0 (grey), 2 (RGB: channel 0 is kept) or 3 (palette: the indices, as np.asarray of PIL's P image),
non-interlaced, any number of IDAT chunks, ancillary chunks skipped.
"""
from __future__ import annotations

import io
import struct
import zlib
from typing import Optional, Sequence

import numpy as np

from ._lib import lib

SIGNATURE = b"\x89PNG\r\n\x1a\n"

# hn_png.hip struct PngDesc
DESC_DTYPE = np.dtype({
    "names": ["idat_off", "idat_len", "raw_off", "out_off", "W", "H", "bpp", "pad"],
    "formats": ["<i8", "<i8", "<i8", "<i8", "<i4", "<i4", "<i4", "<i4"],
    "offsets": [0, 8, 16, 24, 32, 36, 40, 44],
    "itemsize": 48})

STATUS = {0: "decoded", 1: "reserved block type", 2: "stored block LEN / NLEN mismatch", 3: "bad code lengths",
          4: "invalid litlen / distance symbol", 5: "distance before the start of the output", 6: "input exhausted",
          7: "raw size differs from H (1 + W bpp)", 8: "filter byte > 4", 9: "Adler-32 mismatch", 10: "bad zlib header",
          11: "record does not fit the buffers"}


class PngError(ValueError):
    """the bytes are not a well-formed PNG file: bad signature, a chunk that overruns the file or fails its CRC, no IHDR / IDAT / IEND"""


def _as_bytes(data) -> bytes:
    return data if isinstance(data, bytes) else bytes(data)


def parse(data) -> Optional[dict]:
    """PNG bytes -> the head as a dict (width, height, color_type, bpp, raw_bytes = H (1 + W bpp), "idat": the (offset, length) spans of
    the IDAT payloads in file order, "file": the bytes); None for a PNG outside the supported set; PngError for bytes that are no PNG.
    Every chunk's CRC is verified.  Host only."""
    data = _as_bytes(data)
    if data[:8] != SIGNATURE:
        raise PngError("not a PNG signature")
    pos, ihdr, idat, end = 8, None, [], False
    while pos < len(data):
        if pos + 12 > len(data):
            raise PngError("truncated chunk header")
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind = data[pos + 4:pos + 8]
        if pos + 12 + n > len(data):
            raise PngError("chunk %r overruns the file" % kind)
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(data[pos + 4:pos + 8 + n]) & 0xFFFFFFFF != crc:
            raise PngError("chunk %r fails its CRC" % kind)
        if ihdr is None:
            if kind != b"IHDR" or n != 13:
                raise PngError("the first chunk is not IHDR")
            ihdr = struct.unpack(">IIBBBBB", data[pos + 8:pos + 21])
        elif kind == b"IDAT":
            idat.append((pos + 8, n))
        elif kind == b"IEND":
            end = True
            break
        pos += 12 + n
    if ihdr is None or not idat or not end:
        raise PngError("IHDR, IDAT or IEND is missing")
    w, h, depth, ctype, comp, filt, lace = ihdr
    if w == 0 or h == 0:
        raise PngError("zero width or height")
    if depth != 8 or ctype not in (0, 2, 3) or comp != 0 or filt != 0 or lace != 0 or w > 65535 or h > 65535:
        return None
    bpp = 3 if ctype == 2 else 1
    return {"width": w, "height": h, "color_type": ctype, "bpp": bpp, "raw_bytes": h * (1 + w * bpp), "idat": idat, "file": data}


def idat_bytes(head: dict) -> bytes:
    """the zlib stream of a parsed file: its IDAT payloads concatenated"""
    data = head["file"]
    if len(head["idat"]) == 1:
        o, n = head["idat"][0]
        return data[o:o + n]
    return b"".join(data[o:o + n] for o, n in head["idat"])


def read_bytes(src) -> bytes:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def pil_label(data: bytes) -> np.ndarray:
    """dataset.imread_label on the bytes (PIL's decode, channel 0)"""
    from .dataset import imread_label
    return imread_label(io.BytesIO(data))


def stream_stage(data):
    """one image's host share: (head, the concatenated IDAT payloads), or (None, imread_label's array) when the file is outside the
    supported set (PIL then speaks for that file)"""
    data = _as_bytes(data)
    try:
        head = parse(data)
    except PngError:
        head = None
    if head is None:
        return None, pil_label(data)
    return head, idat_bytes(head)


def pack_streams(items: Sequence, pin: bool = False) -> dict:
    """[(head, zlib stream (bytes or a uint8 array)) | (None, uint8 H x W label map decoded elsewhere)] -> the batch's host buffers: "heads",
    one uint8 tensor "data" with every stream at "offsets" (bytes, multiples of 16; -1 for a map), "lengths" (of the streams) and "maps"
    (the maps, None elsewhere)"""
    import torch
    offs, total = [], 0
    for it in items:
        if it[0] is None:
            offs.append(-1)
            continue
        offs.append(total)
        total += (len(it[1]) + 15) // 16 * 16
    buf = torch.zeros((max(16, total),), dtype=torch.uint8, pin_memory=pin)
    view = buf.numpy()
    for it, o in zip(items, offs):
        if it[0] is not None:
            view[o:o + len(it[1])] = np.frombuffer(it[1], dtype=np.uint8) if isinstance(it[1], (bytes, bytearray, memoryview)) else it[1]
    return {"heads": [it[0] for it in items], "data": buf, "offsets": np.array(offs, dtype=np.int64),
            "lengths": np.array([len(it[1]) if it[0] is not None else 0 for it in items], dtype=np.int64),
            "maps": [None if it[0] is not None else np.ascontiguousarray(it[1]) for it in items]}


def describe_batch(pk: dict):
    """pack_streams' dict -> (descriptors of the images that carry a stream, their indices, byte offsets [n + 1] and (H, W) of every image's
    map in the packed label buffer, the largest stream, the largest raw size)"""
    heads, maps = pk["heads"], pk["maps"]
    n = len(heads)
    shapes = np.array([(h["height"], h["width"]) if h is not None else m.shape[:2] for h, m in zip(heads, maps)], dtype=np.int64).reshape(-1, 2)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(shapes[:, 0] * shapes[:, 1])
    idx = [i for i in range(n) if heads[i] is not None]
    desc = np.zeros(len(idx), dtype=DESC_DTYPE)
    max_idat = max([int(pk["lengths"][i]) for i in idx] + [1])
    max_raw = max([int(heads[i]["raw_bytes"]) for i in idx] + [1])
    slot = (max_raw + 15) // 16 * 16
    for k, (e, i) in enumerate(zip(desc, idx)):
        h = heads[i]
        e["idat_off"], e["idat_len"], e["raw_off"], e["out_off"] = int(pk["offsets"][i]), int(pk["lengths"][i]), k * slot, int(offs[i])
        e["W"], e["H"], e["bpp"] = h["width"], h["height"], h["bpp"]
    return desc, idx, offs, shapes, max_idat, max_raw


def decode_batch(items, device=None) -> dict:
    """items: a list of (head, zlib stream) -- (None, label map) for an image decoded elsewhere, which is uploaded as it is -- or
    pack_streams' dict of them (pin its "data" for an asynchronous upload).  -> the packed uint8 label maps on `device` in augment.pack's
    layout: {"data", "offsets", "shapes"}, and "status": int32 device tensor, one word per STREAM (in batch order, maps left out), as the
    device reported it.  One read-back of the status words; an image with a non-zero one is decoded by dataset.imread_label and uploaded
    into its slot (PIL's error propagates if it rejects the file too)."""
    import torch
    pk = items if isinstance(items, dict) else pack_streams(items)
    heads, maps = pk["heads"], pk["maps"]
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    desc, idx, offs, shapes, max_idat, max_raw = describe_batch(pk)
    n = len(idx)
    with torch.cuda.device(dev):
        dst = torch.empty((max(1, int(offs[-1])),), device=dev, dtype=torch.uint8)
        status = torch.zeros((max(1, n),), device=dev, dtype=torch.int32)
        for i, m in enumerate(maps):
            if heads[i] is None:
                assert m.dtype == np.uint8 and m.ndim == 2, (m.dtype, m.shape)
                dst[int(offs[i]):int(offs[i + 1])].copy_(torch.from_numpy(m).reshape(-1))
        if n:
            assert pk["data"].dtype == torch.uint8
            streams = pk["data"].to(dev, non_blocking=pk["data"].is_pinned())
            desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
            ws_bytes = int(lib().query("hn_png_ws_bytes", n, max_idat, max_raw))
            assert ws_bytes > 0, (n, max_idat, max_raw)
            ws = torch.empty((ws_bytes,), device=dev, dtype=torch.uint8)
            lib().call("hn_png_decode", streams.data_ptr(), int(streams.numel()), desc_d.data_ptr(), n, max_idat, max_raw, ws.data_ptr(),
                       ws_bytes, dst.data_ptr(), int(dst.numel()), status.data_ptr())
            # the one read-back: an image the device rejected is PIL's to decode, into its slot of the packed maps
            for k in np.nonzero(status[:n].cpu().numpy())[0]:
                i = idx[int(k)]
                m = pil_label(heads[i]["file"])
                assert m.shape == (int(shapes[i, 0]), int(shapes[i, 1])), (m.shape, shapes[i])
                dst[int(offs[i]):int(offs[i + 1])].copy_(torch.from_numpy(m).reshape(-1))
    return {"data": dst, "offsets": offs[:-1].copy(), "shapes": shapes, "status": status}


def imread_label_device(paths_or_bytes, device=None) -> dict:
    """label files (paths) or encoded bytes, one or a list -> their H x W uint8 maps on the device, packed ({"data", "offsets", "shapes",
    "status"}): dataset.imread_label's values"""
    if isinstance(paths_or_bytes, (str, bytes, bytearray, memoryview)) or hasattr(paths_or_bytes, "__fspath__"):
        paths_or_bytes = [paths_or_bytes]
    return decode_batch(pack_streams([stream_stage(read_bytes(s)) for s in paths_or_bytes]), device=device)


__all__ = ["parse", "stream_stage", "pack_streams", "decode_batch", "imread_label_device", "PngError", "idat_bytes", "pil_label", "STATUS"]
