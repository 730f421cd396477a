"""The yardstick of the full-state checkpoint tests: the checksum, the slot layout rule and a reader of the file format, restated in
numpy and the standard library, independently of multitask_hydranet_amd/checkpoint.py and of the library.

Checksum of words w[0 .. W-1] (uint32, zero-extended to 64 bits):  s1 = sum w[i] mod 2^64,  s2 = sum (i + 1) * w[i] mod 2^64.
Layout: slots in the given order, every slot on a 16-byte boundary (4 words), pad words zero.
File:   magic 8 | version u32 | manifest length u64 | manifest s1 u64 | manifest s2 u64 | manifest JSON (space-padded to 4) | zeros to
        a multiple of 4096 | blob (all little-endian)."""
import json
import struct

import numpy as np

MAGIC = b"HNSTATE\n"
VERSION = 1
HEADER = 36
ALIGN = 4096
ITEM_WORDS = {"float32": 1, "int32": 1, "int64": 2}


def sums(words):
    """(s1, s2) as Python ints.  numpy's uint64 arithmetic wraps modulo 2^64, which is the definition."""
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint32).astype(np.uint64)
    idx = np.arange(1, w.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s1 = np.add.reduce(w, dtype=np.uint64) if w.size else np.uint64(0)
        s2 = np.add.reduce(w * idx, dtype=np.uint64) if w.size else np.uint64(0)
    return int(s1), int(s2)


def sums_exact(words):
    """the same with Python's unbounded integers (slow; cross-checks the wrap of `sums` on small inputs)"""
    w = [int(v) for v in np.ascontiguousarray(words).reshape(-1).view(np.uint32)]
    return sum(w) % 2 ** 64, sum((i + 1) * v for i, v in enumerate(w)) % 2 ** 64


def slots(word_counts):
    """-> ([offset of every slot, in words], total words)"""
    offs, off = [], 0
    for w in word_counts:
        offs.append(off)
        off += (int(w) + 3) // 4 * 4
    return offs, off


def blob_start(manifest_len):
    return (HEADER + manifest_len + ALIGN - 1) // ALIGN * ALIGN


def sections(data: bytes):
    """byte offsets of the section boundaries of a well-formed file: after the magic, the header, the manifest, the padding, the blob"""
    length = struct.unpack("<Q", data[12:20])[0]
    return [8, HEADER, HEADER + length, blob_start(length), len(data)]


def read(data: bytes):
    """-> (manifest, blob uint32).  Raises ValueError on anything that is not a well-formed file."""
    if len(data) < HEADER or data[:8] != MAGIC:
        raise ValueError("magic / header")
    version, length, s1, s2 = struct.unpack("<IQQQ", data[8:HEADER])
    if version != VERSION or length % 4 or HEADER + length > len(data):
        raise ValueError("version / length")
    text = data[HEADER:HEADER + length]
    if sums(np.frombuffer(text, dtype="<u4")) != (s1, s2):
        raise ValueError("manifest checksum")
    manifest = json.loads(text.decode("utf-8"))
    start = blob_start(length)
    if any(data[HEADER + length:start]):
        raise ValueError("padding")
    if start + 4 * manifest["blob_words"] != len(data):
        raise ValueError("blob length")
    offs, total = slots([e["words"] for e in manifest["tensors"]])
    if total != manifest["blob_words"] or offs != [e["offset"] for e in manifest["tensors"]]:
        raise ValueError("slots")
    for e in manifest["tensors"]:
        if e["words"] != int(np.prod(e["shape"], dtype=np.int64)) * ITEM_WORDS[e["dtype"]]:
            raise ValueError("words of " + e["name"])
    return manifest, np.frombuffer(data, dtype="<u4", count=manifest["blob_words"], offset=start)


def bad_tensors(manifest, blob):
    out = []
    for e in manifest["tensors"]:
        o, w = e["offset"], e["words"]
        if sums(blob[o:o + w]) != (e["s1"], e["s2"]) or blob[o + w:o + (w + 3) // 4 * 4].any():
            out.append(e["name"])
    return out


def tensor(manifest, blob, name):
    e = next(e for e in manifest["tensors"] if e["name"] == name)
    return blob[e["offset"]:e["offset"] + e["words"]].view({"float32": np.float32, "int32": np.int32, "int64": np.int64}[e["dtype"]]).reshape(e["shape"])
