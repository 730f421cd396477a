"""Baseline JPEG encode split between device and host (hn_jpeg_enc.hip), the mirror image of jpeg.py: colour conversion,
chroma down-sampling, the 8x8 forward DCT and quantisation on the device, straight from the packed frame layout of augment.pack() /
jpeg.decode_batch; the Huffman stage on the host by default (entropy="host": only int16 coefficients leave the device, in the layout
jpeg.entropy_decode produces, so both directions share one format) or on the device as well (entropy="device", hn_jpeg_huff.hip: only the
compressed scans leave it; the host writes the few hundred header bytes).  Both give the same bytes.  The arithmetic is libjpeg's default compressor (quality-scaled Annex K tables, 16-bit
fixed-point colour tables, h2v1 / h2v2 down-sampling, accurate integer DCT), all integer: PIL decodes our stream to exactly the pixels it
decodes from its own encode of the same frame at the same settings.

    blobs = jpeg_encode.encode_batch(frames, quality=95, subsampling="4:2:0")     # frames: packed device dict or a list of host BGR arrays
    blobs = jpeg_encode.encode_batch(frames, entropy="device")                     # the same bytes, Huffman stage on the device
    jpeg_encode.imwrite("out.jpg", frame)

Out of scope: optimised Huffman tables, restart markers, progressive output.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from ._lib import lib
from .jpeg import HEAD_DTYPE

# hn_jpeg_enc.hip struct JpegEncDesc
DESC_DTYPE = np.dtype({
    "names": ["src_off", "coef_off", "W", "H", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "qt"],
    "formats": ["<i8", "<i8", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", ("<u2", (3, 64))],
    "offsets": [0, 8, 16, 20, 24, 28, 32, 36, 40, 48],
    "itemsize": 432})

# hn_jpeg_huff.hip struct JpegHuffDesc / JpegHuffResult
HUFF_DESC_DTYPE = np.dtype({
    "names": ["coef_off", "out_off", "out_cap", "W", "H", "ncomp", "hs", "vs", "mcus_x", "mcus_y"],
    "formats": ["<i8", "<i8", "<i8", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4"],
    "offsets": [0, 8, 16, 24, 28, 32, 36, 40, 44, 48],
    "itemsize": 56})
HUFF_RESULT_DTYPE = np.dtype({"names": ["scan_bytes", "status"], "formats": ["<i8", "<i4"], "offsets": [0, 8], "itemsize": 16})

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), "grey": (1, 1)}
CAPACITY_TOO_SMALL = -4               # hn_jpeg_entropy_encode's status

# ITU-T T.81 Annex K.1 / K.2, natural (row-major) order
_BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
                       62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98,
                       112, 100, 103, 99], dtype=np.int64)
_BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
                         99] + [99] * 32, dtype=np.int64)


def quant_tables(quality: int) -> np.ndarray:
    """libjpeg's jpeg_set_quality: uint16 [3, 64] (luma, chroma, chroma), natural order"""
    q = min(100, max(1, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    t = [np.clip((b * scale + 50) // 100, 1, 255) for b in (_BASE_LUMA, _BASE_CHROMA)]
    return np.stack([t[0], t[1], t[1]]).astype(np.uint16)


def make_head(width: int, height: int, quality: int = 95, subsampling: str = "4:2:0") -> dict:
    """the header (jpeg.parse's dict, with "rec") of the stream written for a width x height frame"""
    hs, vs = SAMPLING[subsampling]
    ncomp = 1 if subsampling == "grey" else 3
    assert 1 <= width <= 65535 and 1 <= height <= 65535, (width, height)
    rec = np.zeros(1, dtype=HEAD_DTYPE)
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    vals = dict(width=width, height=height, ncomp=ncomp, hs=hs, vs=vs, mcus_x=mx, mcus_y=my, restart_interval=0,
                coef_bytes=mx * my * (hs * vs + (2 if ncomp == 3 else 0)) * 128, scan_offset=0)
    for k, v in vals.items():
        rec[k] = v
    rec["qt"] = quant_tables(quality)
    head = dict(vals)
    head["qt"] = rec["qt"][0].copy()
    head["rec"] = rec
    return head


def entropy_status(coefs: np.ndarray, head: dict, out: np.ndarray) -> int:
    """the library's answer for `out` (uint8, its size is the capacity): the stream's length, CAPACITY_TOO_SMALL, or -1.  Host only."""
    coefs = np.ascontiguousarray(coefs)
    assert coefs.dtype == np.int16 and out.dtype == np.uint8 and out.flags.c_contiguous
    return int(lib().raw("hn_jpeg_entropy_encode")(coefs.ctypes.data, coefs.nbytes, head["rec"].ctypes.data, out.ctypes.data, out.nbytes))


def first_capacity(head: dict) -> int:
    """the first guess of a stream's size; a stage that finds it too small doubles it"""
    return 1024 + int(head["coef_bytes"]) // 8


def entropy_encode(coefs: np.ndarray, head: dict) -> bytes:
    """the Huffman stage: quantised int16 coefficients (jpeg.entropy_decode's layout) -> a complete JFIF stream.  Host only."""
    cap = 1024 + int(head["coef_bytes"]) // 8
    while True:
        out = np.empty(cap, dtype=np.uint8)
        n = entropy_status(coefs, head, out)
        if n == CAPACITY_TOO_SMALL:
            cap *= 2
            continue
        if n <= 0:
            raise ValueError("hn_jpeg_entropy_encode: bad header or a coefficient outside the baseline range (status %d)" % n)
        return out[:n].tobytes()


def write_header(head: dict) -> bytes:
    """the stream's bytes before the first scan bit (SOI ... SOS), as entropy_encode writes them.  Host only."""
    out = np.empty(1024, dtype=np.uint8)
    n = int(lib().raw("hn_jpeg_write_header")(head["rec"].ctypes.data, out.ctypes.data, out.nbytes))
    if n <= 0:
        raise ValueError("hn_jpeg_write_header: bad header (status %d)" % n)
    return out[:n].tobytes()


def huff_describe(heads, coff, caps):
    """-> (JpegHuffDesc records, byte offsets of every image's scan in the output buffer [n + 1]); the scans lie back to back"""
    desc = np.zeros(len(heads), dtype=HUFF_DESC_DTYPE)
    ooff = np.zeros(len(heads) + 1, dtype=np.int64)
    for i, (e, h) in enumerate(zip(desc, heads)):
        e["coef_off"], e["out_off"], e["out_cap"] = int(coff[i]), int(ooff[i]), int(caps[i])
        e["W"], e["H"], e["ncomp"], e["hs"], e["vs"], e["mcus_x"], e["mcus_y"] = (h[k] for k in ("width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y"))
        ooff[i + 1] = ooff[i] + int(caps[i])
    return desc, ooff


def huff_workspace_bytes(n: int, max_blocks: int, max_cap: int) -> int:
    need = int(lib().query("hn_jpeg_huff_ws_bytes", n, max_blocks, max_cap))
    if need <= 0:
        raise ValueError("hn_jpeg_huff_ws_bytes: arguments out of range (%d images, %d blocks, capacity %d)" % (n, max_blocks, max_cap))
    return need


_STAGING = {}                          # device -> pinned uint8 host tensor, grown when a batch needs more and reused across calls


def _staging(device, nbytes: int):
    import torch
    buf = _STAGING.get(device)
    if buf is None or buf.numel() < nbytes:
        buf = _STAGING[device] = torch.empty((max(nbytes, 1 << 20),), dtype=torch.uint8, pin_memory=True)
    return buf[:nbytes]


def entropy_encode_device(heads, coefs, coff, capacity=None) -> List[bytes]:
    """the Huffman stage on the device: encode_coefs_device's (heads, int16 device tensor, byte offsets) -> one complete JFIF stream per
    image (header + scan + EOI), byte for byte entropy_encode's.  capacity: bytes of scan per image for the first attempt (one value or one
    per image; default 1024 + coef_bytes // 8, the host path's first guess); an image whose scan does not fit has it doubled and the batch
    runs again.  The result records and every scan come back in ONE copy through a pinned staging buffer."""
    import torch
    n = len(heads)
    assert coefs.is_cuda and coefs.dtype == torch.int16 and coefs.dim() == 1 and coefs.is_contiguous() and len(coff) == n + 1
    if capacity is None:
        caps = [first_capacity(h) for h in heads]
    else:
        caps = [int(capacity)] * n if np.isscalar(capacity) else [int(c) for c in capacity]
    assert len(caps) == n and min(caps) >= 0
    headers = [write_header(h) for h in heads]
    max_blocks = max(int(h["coef_bytes"]) // 128 for h in heads)
    rbytes = (n * HUFF_RESULT_DTYPE.itemsize + 15) // 16 * 16
    with torch.cuda.device(coefs.device):
        while True:
            desc, ooff = huff_describe(heads, coff, caps)
            ws = torch.empty((huff_workspace_bytes(n, max_blocks, max(caps)),), device=coefs.device, dtype=torch.uint8)
            desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(coefs.device)
            buf = torch.empty((rbytes + max(int(ooff[-1]), 1),), device=coefs.device, dtype=torch.uint8)       # result records, then the scans
            lib().call("hn_jpeg_huff_encode", coefs.data_ptr(), int(coefs.numel()) * 2, desc_d.data_ptr(), n, max_blocks, max(caps), ws.data_ptr(),
                       int(ws.numel()), buf.data_ptr() + rbytes, int(ooff[-1]), buf.data_ptr())
            stage = _staging(coefs.device, int(buf.numel()))
            stage.copy_(buf, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            host = stage.numpy()
            res = host[:n * HUFF_RESULT_DTYPE.itemsize].view(HUFF_RESULT_DTYPE)
            bad = [i for i in range(n) if int(res["status"][i]) not in (0, CAPACITY_TOO_SMALL)]
            if bad:
                raise ValueError("hn_jpeg_huff_encode: image %d: bad descriptor or a coefficient outside the baseline range (status %d)"
                                 % (bad[0], int(res["status"][bad[0]])))
            small = [i for i in range(n) if int(res["status"][i]) == CAPACITY_TOO_SMALL]
            if not small:
                return [headers[i] + host[rbytes + int(ooff[i]):rbytes + int(ooff[i]) + int(res["scan_bytes"][i])].tobytes() + b"\xff\xd9"
                        for i in range(n)]
            for i in small:
                caps[i] = max(2 * caps[i], 64)


def _as_packed(frames, device=None) -> dict:
    import torch
    if isinstance(frames, dict):
        return frames
    if isinstance(frames, np.ndarray) and frames.ndim == 3:
        frames = [frames]
    from .augment import pack
    arrs = [np.ascontiguousarray(f) for f in frames]
    for a in arrs:
        assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3, (a.dtype, a.shape)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    pk = pack(arrs)
    return {"data": pk["data"].to(dev), "offsets": pk["offsets"], "shapes": pk["shapes"]}


def describe_batch(shapes, offsets, quality, subsampling):
    """-> (heads, descriptors, byte offsets of every image's coefficients [n + 1])"""
    n = len(shapes)
    subs = [subsampling] * n if isinstance(subsampling, str) else list(subsampling)
    quals = [quality] * n if np.isscalar(quality) else list(quality)
    heads = [make_head(int(w), int(h), q, s) for (h, w), q, s in zip(shapes, quals, subs)]
    desc = np.zeros(n, dtype=DESC_DTYPE)
    coff = np.zeros(n + 1, dtype=np.int64)
    for i, (e, h) in enumerate(zip(desc, heads)):
        e["src_off"], e["coef_off"] = int(offsets[i]), int(coff[i])
        e["W"], e["H"], e["ncomp"], e["hs"], e["vs"], e["mcus_x"], e["mcus_y"] = (h[k] for k in ("width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y"))
        e["qt"] = h["qt"]
        coff[i + 1] = coff[i] + (int(h["coef_bytes"]) + 15) // 16 * 16
    return heads, desc, coff


def encode_coefs_device(frames, quality=95, subsampling="4:2:0", out=None):
    """the device half: packed frames -> (heads, int16 device tensor of every image's coefficients, their byte offsets [n + 1]).
    `out`: a flat int16 device tensor to write into instead of a new one.  `quality` / `subsampling`: one value or one per image."""
    import torch
    pk = _as_packed(frames)
    data = pk["data"]
    assert data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous() and data.data_ptr() % 16 == 0
    shapes = np.asarray(pk["shapes"], dtype=np.int64).reshape(-1, 2)
    offsets = np.asarray(pk["offsets"], dtype=np.int64)
    heads, desc, coff = describe_batch(shapes, offsets, quality, subsampling)
    for i, (h, w) in enumerate(shapes):
        assert 0 <= offsets[i] and offsets[i] + h * w * 3 <= data.numel(), (i, int(offsets[i]), int(h), int(w), int(data.numel()))
    with torch.cuda.device(data.device):
        if out is None:
            coefs = torch.empty((int(coff[-1]) // 2,), device=data.device, dtype=torch.int16)
        else:
            assert out.dtype == torch.int16 and out.device == data.device and out.dim() == 1 and out.is_contiguous() and out.numel() * 2 >= int(coff[-1])
            coefs = out
        desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(data.device)
        lib().call("hn_jpeg_encode", data.data_ptr(), int(data.numel()), desc_d.data_ptr(), len(heads), max(h["mcus_y"] for h in heads),
                   max(h["mcus_x"] * 8 * h["hs"] for h in heads), coefs.data_ptr(), int(coefs.numel()) * 2)
    return heads, coefs, coff


def encode_batch(frames, quality=95, subsampling="4:2:0", entropy="host") -> List[bytes]:
    """frames: the packed device layout of augment.pack() / jpeg.decode_batch ({"data", "offsets", "shapes"}, BGR uint8, ragged) or a list
    of host BGR uint8 arrays (uploaded) -> one JFIF stream per frame.  subsampling: "4:4:4" | "4:2:2" | "4:2:0" | "grey" (channel 0).
    entropy: "host" (the coefficients are copied to the host and coded there) | "device" (entropy_encode_device); the same bytes."""
    if entropy not in ("host", "device"):
        raise ValueError("entropy must be \"host\" or \"device\", not %r" % (entropy,))
    heads, coefs, coff = encode_coefs_device(frames, quality, subsampling)
    if entropy == "device":
        return entropy_encode_device(heads, coefs, coff)
    host = coefs.cpu().numpy()
    return [entropy_encode(host[int(coff[i]) // 2:int(coff[i]) // 2 + int(h["coef_bytes"]) // 2], h) for i, h in enumerate(heads)]


def imwrite(path, frame, quality=95, subsampling="4:2:0", entropy="host") -> None:
    """cv2.imwrite for one BGR frame (a host array, or a packed device dict holding one frame)"""
    blobs = encode_batch(frame if isinstance(frame, dict) else [frame], quality, subsampling, entropy)
    assert len(blobs) == 1
    with open(path, "wb") as f:
        f.write(blobs[0])


__all__ = ["encode_batch", "imwrite", "entropy_encode", "entropy_encode_device", "write_header", "encode_coefs_device", "make_head", "quant_tables"]
