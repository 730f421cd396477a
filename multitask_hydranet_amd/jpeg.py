"""Baseline JPEG decode split between host and device (hn_jpeg.hip): the serial Huffman stage on the host -- in a DataLoader
worker, without a GPU -- and dequantisation, the 8x8 inverse DCT, chroma up-sampling and YCbCr -> BGR on the device, written straight into
the packed frame layout of augment.pack(), so that augment.augment_batch takes the result as its `frames`.  The arithmetic is
libjpeg-turbo's default decode (accurate integer IDCT, fancy up-sampling, 16-bit fixed-point colour tables), all integer: the frames equal
PIL's bit for bit.

    head = jpeg.parse(data)                      # None: outside the supported set, decode that image with PIL
    coefs = jpeg.entropy_decode(data, head)      # host only: int16 [blocks, 64]
    frames = jpeg.decode_batch([(head, coefs), ...])        # {"data" (device uint8), "offsets", "shapes"}: pack()'s layout

The Huffman stage runs on the device as well (hn_jpeg_scan.hip), opt-in: the file's bytes are uploaded as they are and the host only parses
the header and prepares the scan's tables.  An image whose scan the device reports corrupt is decoded with PIL, that image only.

    scan = jpeg.scan_prepare(data, head)         # host only: where the scan lies + its Huffman tables
    frames = jpeg.decode_batch(jpeg.pack_streams([(head, scan, data), ...]))

Supported: 8-bit Huffman SOF0 / SOF1, one interleaved scan, greyscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0 (luma 1x1 / 2x1 / 2x2, chroma 1x1),
DHT / DQT anywhere before the scan, 8- and 16-bit DQT entries, restart intervals, APPn / COM skipped.  Coefficient layout: one de-zigzagged
64-entry block per 8x8 block, component plane after component plane (Y, Cb, Cr), blocks in raster order of the plane padded to whole MCUs.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ._lib import lib

# hn_jpeg.hip struct JpegHead
HEAD_DTYPE = np.dtype({
    "names": ["width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "restart_interval", "coef_bytes", "scan_offset", "qt"],
    "formats": ["<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i8", "<i8", ("<u2", (3, 64))],
    "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48],
    "itemsize": 432})

# hn_jpeg.hip struct JpegDesc
DESC_DTYPE = np.dtype({
    "names": ["coef_off", "plane_off", "dst_off", "W", "H", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "qt"],
    "formats": ["<i8", "<i8", "<i8", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", ("<u2", (3, 64))],
    "offsets": [0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 56],
    "itemsize": 440})

# hn_jpeg_scan.h struct JpegScanHuff / JpegScanRec
SCAN_HUFF_DTYPE = np.dtype({
    "names": ["look_n", "look_v", "maxcode", "valoff", "vals"],
    "formats": [("u1", 512), ("u1", 512), ("<i4", 17), ("<i4", 17), ("u1", 256)],
    "offsets": [0, 512, 1024, 1092, 1160],
    "itemsize": 1416})
SCAN_DTYPE = np.dtype({
    "names": ["scan_offset", "scan_bytes", "stream_off", "coef_off", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "restart_interval", "td", "ta",
              "dc", "ac"],
    "formats": ["<i8", "<i8", "<i8", "<i8", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", ("<i4", 3), ("<i4", 3), (SCAN_HUFF_DTYPE, 3),
                (SCAN_HUFF_DTYPE, 3)],
    "offsets": [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56, 68, 80, 80 + 3 * 1416],
    "itemsize": 8576})

UNSUPPORTED = 3


class JpegError(ValueError):
    """the stream is not a well-formed JPEG, or its scan is corrupt or truncated"""


def _as_bytes(data) -> bytes:
    return data if isinstance(data, bytes) else bytes(data)


def parse(data) -> Optional[dict]:
    """JPEG bytes -> the header as a dict (width, height, ncomp, hs, vs, mcus_x, mcus_y, restart_interval, coef_bytes, qt uint16 [3, 64] in
    natural order, and "rec": the library's record); None for a JPEG outside the supported set; JpegError for bytes that are no JPEG.
    Host only."""
    data = _as_bytes(data)
    rec = np.zeros(1, dtype=HEAD_DTYPE)
    rc = lib().raw("hn_jpeg_parse")(data, len(data), rec.ctypes.data)
    if rc == UNSUPPORTED:
        return None
    if rc != 0:
        raise JpegError("not a well-formed JPEG stream")
    head = {k: int(rec[k][0]) for k in HEAD_DTYPE.names if k != "qt"}
    head["qt"] = rec["qt"][0].copy()
    head["rec"] = rec
    return head


def n_blocks(head: dict) -> int:
    return int(head["coef_bytes"]) // 128


def entropy_status(data, head: dict, out: np.ndarray) -> int:
    """the library's status of the entropy decode into `out` (int16, at least coef_bytes): 0, or 1 for a corrupt / truncated scan"""
    data = _as_bytes(data)
    assert out.dtype == np.int16 and out.flags.c_contiguous and out.nbytes >= head["coef_bytes"], (out.dtype, out.nbytes)
    return int(lib().raw("hn_jpeg_entropy_decode")(data, len(data), head["rec"].ctypes.data, out.ctypes.data, int(head["coef_bytes"])))


def entropy_decode(data, head: dict, out: Optional[np.ndarray] = None) -> np.ndarray:
    """the Huffman stage: quantised int16 coefficients [blocks, 64] (into `out`, e.g. a pinned tensor's numpy view, when given).  Host only."""
    if out is None:
        out = np.empty((n_blocks(head), 64), dtype=np.int16)
    if entropy_status(data, head, out) != 0:
        raise JpegError("corrupt or truncated entropy-coded segment")
    return out


def scan_prepare(data, head: dict) -> np.ndarray:
    """the scan of a parsed stream for the device's entropy stage: one SCAN_DTYPE record (scan_offset, scan_bytes, geometry, the Huffman
    tables its components select; stream_off / coef_off are pack_streams' to fill).  Host only."""
    data = _as_bytes(data)
    rec = np.zeros(1, dtype=SCAN_DTYPE)
    rc = lib().raw("hn_jpeg_scan_prepare")(data, len(data), head["rec"].ctypes.data, rec.ctypes.data)
    if rc != 0:
        raise JpegError("the header does not belong to this stream" if rc == 1 else "outside the supported set")
    return rec


def pack_streams(items: Sequence, pin: bool = False) -> dict:
    """[(head, scan record, the file's bytes (bytes or a uint8 array)) | (None, BGR uint8 H x W x 3 frame decoded elsewhere)] -> the batch's
    host buffers, as pack_coefs: "heads", one uint8 tensor "data" with every stream at "offsets" (bytes, multiples of 16; -1 for a frame),
    "lengths" (of the streams), "scans" (the records of the streams, stream_off / coef_off filled in), "coef_bytes" (of the coefficient buffer
    they index) and "frames"."""
    import torch
    offs, total, ctotal, scans = [], 0, 0, []
    for it in items:
        if it[0] is None:
            offs.append(-1)
            continue
        head, scan, data = it
        n = len(data)
        assert int(scan["scan_offset"][0]) + int(scan["scan_bytes"][0]) <= n and int(scan["scan_offset"][0]) == head["scan_offset"]
        rec = scan.copy()
        rec["stream_off"], rec["coef_off"] = total, ctotal
        scans.append(rec)
        offs.append(total)
        total += (n + 15) // 16 * 16
        ctotal += (int(head["coef_bytes"]) + 15) // 16 * 16
    buf = torch.zeros((max(16, total),), dtype=torch.uint8, pin_memory=pin)
    view = buf.numpy()
    for it, o in zip(items, offs):
        if it[0] is not None:
            view[o:o + len(it[2])] = np.frombuffer(it[2], dtype=np.uint8) if isinstance(it[2], (bytes, bytearray, memoryview)) else it[2]
    return {"heads": [it[0] for it in items], "data": buf, "offsets": np.array(offs, dtype=np.int64),
            "lengths": np.array([len(it[2]) if it[0] is not None else 0 for it in items], dtype=np.int64), "scans": np.concatenate(scans) if scans else np.zeros(0, dtype=SCAN_DTYPE), "coef_bytes": ctotal,
            "frames": [None if it[0] is not None else np.ascontiguousarray(it[1]) for it in items]}


def entropy_decode_device(pk: dict, device=None) -> dict:
    """pack_streams' dict -> the Huffman stage on the device (hn_jpeg_scan_decode): {"data": int16 device tensor, every image's coefficients in
    entropy_decode's layout at "offsets" (bytes; -1 for a frame), "heads", "status": int32 device tensor, one word per STREAM (in batch order,
    frames left out): 0, or 1 for a scan that does not decode, whose coefficients mean nothing}.  No synchronisation."""
    import torch
    assert pk["data"].dtype == torch.uint8 and "scans" in pk
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    scans, heads = pk["scans"], pk["heads"]
    n = len(scans)
    coef_offs = np.full(len(heads), -1, dtype=np.int64)
    coef_offs[[i for i, h in enumerate(heads) if h is not None]] = scans["coef_off"]
    with torch.cuda.device(dev):
        coefs = torch.empty((max(8, int(pk["coef_bytes"]) // 2),), device=dev, dtype=torch.int16)
        status = torch.zeros((max(1, n),), device=dev, dtype=torch.int32)
        if n:
            streams = pk["data"].to(dev, non_blocking=pk["data"].is_pinned())
            desc_d = torch.from_numpy(scans.view(np.uint8).copy()).to(dev)
            max_scan, max_blocks = int(scans["scan_bytes"].max()), max(n_blocks(h) for h in heads if h is not None)
            ws_bytes = int(lib().query("hn_jpeg_scan_ws_bytes", n, max_scan, max_blocks))
            assert ws_bytes > 0, (n, max_scan, max_blocks)
            ws = torch.empty((ws_bytes,), device=dev, dtype=torch.uint8)
            lib().call("hn_jpeg_scan_decode", streams.data_ptr(), int(streams.numel()), desc_d.data_ptr(), n, max_scan, max_blocks, ws.data_ptr(),
                       ws_bytes, coefs.data_ptr(), int(coefs.numel()) * 2, status.data_ptr())
    return {"data": coefs, "offsets": coef_offs, "heads": heads, "status": status}


def pack_coefs(items: Sequence, pin: bool = False) -> dict:
    """[(head, coefficients) | (None, BGR uint8 H x W x 3 frame decoded elsewhere)] -> the batch's host buffers: "heads", one int16 tensor
    "data" with every image's coefficients at "offsets" (bytes, multiples of 16; -1 for a frame) and "frames" (the frames, None elsewhere)"""
    import torch
    offs, total = [], 0
    for head, arr in items:
        if head is None:
            offs.append(-1)
            continue
        assert arr.dtype == np.int16 and arr.nbytes == head["coef_bytes"], (arr.dtype, arr.nbytes, head["coef_bytes"])
        offs.append(total)
        total += (int(head["coef_bytes"]) + 15) // 16 * 16
    data = torch.empty((max(8, total // 2),), dtype=torch.int16, pin_memory=pin)
    buf = data.numpy()
    for (head, arr), o in zip(items, offs):
        if head is not None:
            buf[o // 2:o // 2 + arr.size] = np.ascontiguousarray(arr).reshape(-1)
    return {"heads": [h for h, _ in items], "data": data, "offsets": np.array(offs, dtype=np.int64),
            "frames": [None if h is not None else np.ascontiguousarray(a) for h, a in items]}


def describe_batch(pk: dict):
    """pack_coefs' dict -> (descriptors of the images that carry coefficients, their indices, byte offsets [n + 1] and (H, W) of every
    image's frame in the packed frame buffer, bytes of sample-plane scratch)"""
    heads, frames = pk["heads"], pk["frames"]
    n = len(heads)
    shapes = np.array([(h["height"], h["width"]) if h is not None else f.shape[:2] for h, f in zip(heads, frames)], dtype=np.int64).reshape(-1, 2)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(shapes[:, 0] * shapes[:, 1] * 3)
    idx = [i for i in range(n) if heads[i] is not None]
    desc = np.zeros(len(idx), dtype=DESC_DTYPE)
    coef_bytes = int(pk["data"].numel()) * 2
    plane_total = 0
    for e, i in zip(desc, idx):
        h = heads[i]
        e["coef_off"], e["plane_off"], e["dst_off"] = int(pk["offsets"][i]), plane_total, int(offs[i])
        e["W"], e["H"], e["ncomp"], e["hs"], e["vs"], e["mcus_x"], e["mcus_y"] = (h[k] for k in ("width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y"))
        e["qt"] = h["qt"]
        assert e["coef_off"] >= 0 and e["coef_off"] % 16 == 0 and e["coef_off"] + h["coef_bytes"] <= coef_bytes
        plane_total += (n_blocks(h) * 64 + 15) // 16 * 16
    return desc, idx, offs, shapes, plane_total


def decode_batch(items, device=None, out=None) -> dict:
    """items: a list of (head, coefficients) -- (None, BGR frame) for an image decoded elsewhere, which is uploaded as it is -- or
    pack_coefs' dict of them (pin its "data" for an asynchronous upload).  -> the packed BGR uint8 frames on `device` in augment.pack's
    layout: {"data", "offsets", "shapes"}; `out`: a flat uint8 tensor on the device to write them into (at least sum H * W * 3 bytes)
    instead of a new one.  The sample planes and the frames stay on the device."""
    import torch
    pk = items if isinstance(items, dict) else pack_coefs(items)
    heads, frames = pk["heads"], pk["frames"]
    status = None
    if "scans" in pk:                                    # pack_streams' dict: the Huffman stage on the device first
        ent = entropy_decode_device(pk, device=device)
        status = ent["status"]
        pk = {"heads": heads, "frames": frames, "data": ent["data"], "offsets": ent["offsets"], "streams": pk}
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    desc, idx, offs, shapes, plane_total = describe_batch(pk)
    if out is None:
        dst = torch.empty((max(1, int(offs[-1])),), device=dev, dtype=torch.uint8)
    else:
        assert out.dtype == torch.uint8 and out.device == dev and out.dim() == 1 and out.is_contiguous() and out.numel() >= int(offs[-1])
        dst = out
    for i, f in enumerate(frames):
        if heads[i] is None:
            assert f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3, (f.dtype, f.shape)
            dst[int(offs[i]):int(offs[i + 1])].copy_(torch.from_numpy(f).reshape(-1))
    if idx:
        assert pk["data"].dtype == torch.int16
        coefs = pk["data"] if pk["data"].is_cuda else pk["data"].to(dev, non_blocking=pk["data"].is_pinned())
        desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        with torch.cuda.device(dev):
            planes = torch.empty((plane_total,), device=dev, dtype=torch.uint8)
            lib().call("hn_jpeg_decode", coefs.data_ptr(), int(coefs.numel()) * 2, desc_d.data_ptr(), len(idx), max(n_blocks(heads[i]) for i in idx),
                       int(shapes[idx, 0].max()), int(shapes[idx, 1].max()), planes.data_ptr(), plane_total, dst.data_ptr(), int(dst.numel()))
        if status is not None:
            # the one read-back: an image whose scan the device could not decode is PIL's to decode, into its slot of the packed frames
            src = pk["streams"]
            for k in np.nonzero(status[:len(idx)].cpu().numpy())[0]:
                i = idx[int(k)]
                o, ln = int(src["offsets"][i]), int(src["lengths"][i])
                f = pil_bgr(src["data"].numpy()[o:o + ln].tobytes())
                assert f.shape == (int(shapes[i, 0]), int(shapes[i, 1]), 3), (f.shape, shapes[i])
                dst[int(offs[i]):int(offs[i + 1])].copy_(torch.from_numpy(f).reshape(-1))
    return {"data": dst, "offsets": offs[:-1].copy(), "shapes": shapes}


def read_bytes(src) -> bytes:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def pil_bgr(data: bytes) -> np.ndarray:
    """PIL's decode of the bytes, swapped to BGR (what dataset.imread_bgr returns for the file)"""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[..., ::-1])


def host_stage(data: bytes):
    """one image's host half: (head, coefficients), or (None, PIL's BGR frame) when the stream is outside the supported set or its scan
    does not decode (PIL then speaks for that file)"""
    try:
        head = parse(data)
    except JpegError:
        head = None
    if head is not None:
        out = np.empty((n_blocks(head), 64), dtype=np.int16)
        if entropy_status(data, head, out) == 0:
            return head, out
    return None, pil_bgr(data)


def stream_stage(data: bytes):
    """one image's host share when the device runs the entropy stage: (head, scan record, bytes), or (None, PIL's BGR frame) when the
    stream is outside the supported set"""
    try:
        head = parse(data)
    except JpegError:
        head = None
    if head is None:
        return None, pil_bgr(data)
    return head, scan_prepare(data, head), data


def imread_bgr_device(paths_or_bytes, device=None, entropy: str = "host") -> dict:
    """files (paths) or encoded bytes, one or a list -> their BGR frames on the device, packed ({"data", "offsets", "shapes"}).  entropy:
    where the Huffman stage runs, "host" or "device"; the frames are the same."""
    if entropy not in ("host", "device"):
        raise ValueError("entropy should be one of ('host', 'device')")
    if isinstance(paths_or_bytes, (str, bytes, bytearray, memoryview)) or hasattr(paths_or_bytes, "__fspath__"):
        paths_or_bytes = [paths_or_bytes]
    if entropy == "device":
        return decode_batch(pack_streams([stream_stage(read_bytes(s)) for s in paths_or_bytes]), device=device)
    return decode_batch([host_stage(read_bytes(s)) for s in paths_or_bytes], device=device)


__all__ = ["parse", "entropy_decode", "decode_batch", "imread_bgr_device", "pack_coefs", "host_stage", "JpegError", "scan_prepare", "pack_streams",
           "entropy_decode_device", "stream_stage"]
