"""Full-state training checkpoints: the file format, and the packer that gathers the state on the device (hn_ckpt.hip).

A state file holds every tensor a restart needs -- in one blob, each with a checksum -- and the host-side state next to them:

    offset 0    magic  b"HNSTATE\\n"                                                  8 bytes
           8    format version                                                       uint32, little-endian
          12    length L of the manifest in bytes (a multiple of 4)                  uint64, little-endian
          20    s1, s2 of the manifest's bytes read as little-endian 32-bit words    2 x uint64, little-endian
          36    the manifest: JSON (UTF-8), padded with spaces to a multiple of 4
      36 + L    zero bytes up to the next multiple of 4096
        B       the blob: manifest["blob_words"] 32-bit words; the file ends with it

    manifest = {"tensors": [{"name", "dtype", "shape", "offset", "words", "s1", "s2"}, ...], "blob_words": int, "host": {...}}

`offset` and `words` count 32-bit words of the blob; every tensor's slot starts on a 16-byte boundary (offset % 4 == 0), slots follow
one another in the manifest's order, and the up to three pad words behind a slot are zero.  Checksum of words w[0 .. W-1] (uint32,
zero-extended): s1 = sum w[i], s2 = sum (i + 1) * w[i], both mod 2^64 (hn_state_checksum_host on the host, hn_state_pack /
hn_state_verify on the device).  Floats in the manifest are JSON's shortest round-trip `repr`: every bit comes back.

Reading validates all of that against the file's size before anything touches a device; a file that fails raises CheckpointError.
A tensor whose words do not give its recorded sums is CheckpointCorrupt (a CheckpointError): found on the host by verify_host()
(tools/check_state.py, no GPU needed) and on the device by StatePacker.restore().
"""
from __future__ import annotations

import ctypes
import json
import os
import struct

import numpy as np
import torch

from ._lib import lib

MAGIC = b"HNSTATE\n"
VERSION = 1
HEADER_BYTES = 36
BLOB_ALIGN = 4096
_DTYPES = {"float32": torch.float32, "int64": torch.int64, "int32": torch.int32}
_NAMES = {v: k for k, v in _DTYPES.items()}


class CheckpointError(RuntimeError):
    """the file is not a readable state file: short, malformed, or inconsistent with its own manifest"""


class CheckpointCorrupt(CheckpointError):
    """the file reads, but a tensor's words do not give the sums its manifest records; `.tensor` names the first such tensor"""

    def __init__(self, msg, tensor=None):
        super().__init__(msg)
        self.tensor = tensor


def checksum_host(words) -> tuple:
    """(s1, s2) of a C-contiguous array of 32-bit words (hn_state_checksum_host: a host function of the library, no GPU call)"""
    a = np.ascontiguousarray(words)
    if a.dtype.itemsize != 4:
        a = a.view(np.uint32)
    out = (ctypes.c_ulonglong * 2)()
    rc = lib().raw("hn_state_checksum_host")(a.ctypes.data if a.size else None, a.size, ctypes.addressof(out))
    if rc != 0:
        raise RuntimeError("hn_state_checksum_host: bad argument")
    return int(out[0]), int(out[1])


def words_of(t: torch.Tensor) -> int:
    """32-bit words of a tensor the format can carry: contiguous float32 / int64 / int32"""
    if t.dtype not in _NAMES or not t.is_contiguous():
        raise ValueError("checkpoint: contiguous float32 / int64 / int32 tensors only, not %s%s" % (t.dtype, "" if t.is_contiguous() else " (strided)"))
    return t.numel() * (t.element_size() // 4)


def layout(named) -> tuple:
    """[(name, tensor)] -> ([{"name", "dtype", "shape", "offset", "words"}], blob_words): slots in order, each on a 16-byte boundary"""
    entries, off, seen = [], 0, set()
    for name, t in named:
        if name in seen:
            raise ValueError("checkpoint: duplicate tensor name %r" % name)
        seen.add(name)
        w = words_of(t)
        entries.append(dict(name=name, dtype=_NAMES[t.dtype], shape=[int(v) for v in t.shape], offset=off, words=w))
        off += (w + 3) // 4 * 4
    return entries, off


def pack_host(named) -> tuple:
    """CPU tensors -> (entries with their sums, the blob as uint32): what StatePacker.pack() gives for device tensors, on the host"""
    entries, total = layout(named)
    blob = np.zeros(total, dtype=np.uint32)
    for e, (_, t) in zip(entries, named):
        w = np.ascontiguousarray(t.detach().cpu().numpy()).reshape(-1).view(np.uint32)
        blob[e["offset"]:e["offset"] + e["words"]] = w
        e["s1"], e["s2"] = checksum_host(w)
    return entries, blob


def write_file(path: str, entries, blob, host: dict) -> None:
    """entries: layout() rows with "s1" / "s2"; blob: uint32 [blob_words] (a numpy array, or anything with the buffer protocol).  Written
    to path + ".tmp" and renamed: a killed writer never leaves a half file under the final name."""
    blob = np.asarray(blob)
    manifest = dict(tensors=entries, blob_words=int(blob.size), host=host)
    text = json.dumps(manifest, sort_keys=True, separators=(",", ":")).encode("utf-8")
    text += b" " * (-len(text) % 4)
    s1, s2 = checksum_host(np.frombuffer(text, dtype="<u4"))
    head = MAGIC + struct.pack("<IQQQ", VERSION, len(text), s1, s2)
    assert len(head) == HEADER_BYTES
    pad = -(len(head) + len(text)) % BLOB_ALIGN
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(head)
        f.write(text)
        f.write(b"\0" * pad)
        f.write(memoryview(blob).cast("B"))
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def read_file(path: str, blob_out=None) -> tuple:
    """-> (manifest, blob as uint32).  Validates magic, version, lengths, the manifest's own checksum, the zero padding and every
    tensor's slot against the file size; raises CheckpointError.  Tensor checksums are NOT verified here (verify_host, or the device).
    blob_out: a writable uint32 numpy array of at least blob_words to read the blob into (a pinned buffer); else a new array."""
    try:
        size = os.path.getsize(path)
        f = open(path, "rb")
    except OSError as e:
        raise CheckpointError("%s: %s" % (path, e))
    with f:
        head = f.read(HEADER_BYTES)
        if len(head) < HEADER_BYTES:
            raise CheckpointError("%s: %i bytes: shorter than a state file's header" % (path, size))
        if head[:8] != MAGIC:
            raise CheckpointError("%s: not a state file (magic %r)" % (path, head[:8]))
        version, length, s1, s2 = struct.unpack("<IQQQ", head[8:])
        if version != VERSION:
            raise CheckpointError("%s: format version %i, this reader knows %i" % (path, version, VERSION))
        if length % 4 or length < 2 or HEADER_BYTES + length > size:
            raise CheckpointError("%s: manifest length %i does not fit the file (%i bytes)" % (path, length, size))
        text = f.read(length)
        if len(text) != length or checksum_host(np.frombuffer(text, dtype="<u4")) != (s1, s2):
            raise CheckpointError("%s: the manifest does not give its recorded checksum" % path)
        try:
            manifest = json.loads(text.decode("utf-8"))
            entries, blob_words, host = manifest["tensors"], manifest["blob_words"], manifest["host"]
            if not (isinstance(entries, list) and isinstance(blob_words, int) and not isinstance(blob_words, bool) and isinstance(host, dict)):
                raise TypeError("types")
            off = 0
            for e in entries:
                dt = _DTYPES[e["dtype"]]
                numel = 1
                for v in e["shape"]:
                    if not isinstance(v, int) or isinstance(v, bool) or v < 0:
                        raise ValueError("shape")
                    numel *= v
                ints = [e["offset"], e["words"], e["s1"], e["s2"]]
                if not (isinstance(e["name"], str) and all(isinstance(v, int) and not isinstance(v, bool) for v in ints)):
                    raise TypeError("types")
                if e["words"] != numel * (torch.empty((), dtype=dt).element_size() // 4) or e["offset"] != off or not (
                        0 <= e["s1"] < 2 ** 64 and 0 <= e["s2"] < 2 ** 64):
                    raise ValueError("slot of %s" % e["name"])
                off += (e["words"] + 3) // 4 * 4
            if off != blob_words or len({e["name"] for e in entries}) != len(entries):
                raise ValueError("blob_words")
        except (KeyError, TypeError, ValueError, UnicodeDecodeError) as e:
            raise CheckpointError("%s: malformed manifest (%s)" % (path, e))
        start = (HEADER_BYTES + length + BLOB_ALIGN - 1) // BLOB_ALIGN * BLOB_ALIGN
        if start + blob_words * 4 != size:
            raise CheckpointError("%s: %i bytes, but header, manifest and a blob of %i words make %i" % (path, size, blob_words, start + blob_words * 4))
        if f.read(start - HEADER_BYTES - length).strip(b"\0"):
            raise CheckpointError("%s: the padding before the blob is not zero" % path)
        if blob_out is None:
            blob_out = np.empty(blob_words, dtype=np.uint32)
        blob = blob_out[:blob_words]
        if f.readinto(memoryview(blob).cast("B")) != blob_words * 4:
            raise CheckpointError("%s: short read of the blob" % path)
    return manifest, blob


def verify_host(manifest, blob) -> list:
    """names of the tensors whose words (or the pad words behind them) are not what the manifest records, in order; [] = a good file"""
    bad = []
    for e in manifest["tensors"]:
        o, w = e["offset"], e["words"]
        if checksum_host(blob[o:o + w]) != (e["s1"], e["s2"]) or blob[o + w:o + (w + 3) // 4 * 4].any():
            bad.append(e["name"])
    return bad


def tensors_from(manifest, blob) -> dict:
    """{name: CPU tensor} (copies) of a file read by read_file"""
    out = {}
    for e in manifest["tensors"]:
        w = np.array(blob[e["offset"]:e["offset"] + e["words"]], dtype=np.uint32)
        out[e["name"]] = torch.from_numpy(w).view(_DTYPES[e["dtype"]]).reshape(e["shape"])
    return out


def summary(manifest) -> str:
    host = manifest["host"]
    by = {}
    for e in manifest["tensors"]:
        k = e["name"].split("/")[0]
        n, w = by.get(k, (0, 0))
        by[k] = (n + 1, w + e["words"])
    lines = ["%i tensors, %i words (%.1f MB)" % (len(manifest["tensors"]), manifest["blob_words"], manifest["blob_words"] * 4 / 1e6)]
    lines += ["  %-8s %5i tensors %12i words" % (k, n, w) for k, (n, w) in by.items()]
    lines += ["  %s: %s" % (k, json.dumps(host[k])) for k in ("epoch", "phase", "settles", "train") if k in host]
    return "\n".join(lines)


class StatePacker:
    """An ordered list of (name, device tensor) <-> one device staging buffer and one pinned host buffer of the same size.

    pack(): ONE hn_state_pack launch gathers every tensor into its slot of the staging buffer and leaves every tensor's {s1, s2} behind
    the slots (so that one device-to-host copy brings words and sums).  restore(): one host-to-device copy of a blob and its expected
    sums, hn_state_verify, and hn_state_unpack under its verdict: the tensors are written in place, or not at all.  The staging buffer
    is zeroed once, here; pad words are never written, so the blob's bytes are a function of the tensors alone.  Job tables are cached
    and rebuilt when a tensor's pointer changes (optim.Adam._plan's rule).  Nothing here synchronises except wait_host()."""

    def __init__(self, named):
        self.named = list(named)
        if not self.named:
            raise ValueError("StatePacker: no tensors")
        for n, t in self.named:
            if not t.is_cuda:
                raise ValueError("StatePacker: %s is not on a GPU" % n)
        self.entries, self.blob_words = layout(self.named)
        self.device = self.named[0][1].device
        n = len(self.named)
        self.sum_words = n * 4                                      # uint64 [n][2]
        total = self.blob_words + self.sum_words                    # (blob_words % 4 == 0: the sums are 16-byte aligned)
        self.staging = torch.zeros(total, dtype=torch.int32, device=self.device)
        self.pinned = torch.zeros(total, dtype=torch.int32).pin_memory()
        self.blocks = sum((e["words"] + 1023) // 1024 for e in self.entries)
        self._ws = torch.empty(max(self.blocks, 1) * 2, dtype=torch.int64, device=self.device)
        self._sums = torch.empty(n * 2, dtype=torch.int64, device=self.device)      # hn_state_verify's own sums
        self.verdict = torch.zeros(4, dtype=torch.int32, device=self.device)
        self._tables = None                                         # (pointer signature, pack jobs, unpack jobs, block_job)
        self._side = torch.cuda.Stream(device=self.device)
        self._copied = None                                         # event: the last device-to-host copy

    def signature(self):
        return tuple((n, t.data_ptr(), e["words"]) for (n, t), e in zip(self.named, self.entries))

    def _plan(self):
        sig = tuple(t.data_ptr() for _, t in self.named)
        tb = self._tables
        if tb is not None and tb[0] == sig:
            return tb
        base = self.staging.data_ptr()
        rows, back, owner, blk = [], [], [], 0
        for i, ((_, t), e) in enumerate(zip(self.named, self.entries)):
            nb = (e["words"] + 1023) // 1024
            slot = base + 4 * e["offset"]
            rows.append([t.data_ptr(), slot, e["words"], blk])
            back.append([slot, t.data_ptr(), e["words"], blk])
            owner += [i] * nb
            blk += nb
        if blk < 1:
            raise ValueError("StatePacker: every tensor is empty")
        dev = self.device
        tb = self._tables = (sig, torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(back, dtype=torch.int64).to(dev),
                             torch.tensor(owner, dtype=torch.int32).to(dev))
        return tb

    def pack(self):
        """on the current stream: one hn_state_pack (slots and sums into the staging buffer), then -- on a side stream that waits for it --
        ONE device-to-host copy into the pinned buffer.  Returns at once; wait_host() waits for the copy."""
        _, jobs, _, owner = self._plan()
        if self._copied is not None:
            torch.cuda.current_stream().wait_event(self._copied)    # the staging buffer is not rewritten under an earlier copy
        sums = self.staging.data_ptr() + 4 * self.blob_words
        lib().call("hn_state_pack", jobs.data_ptr(), owner.data_ptr(), self.blocks, len(self.named), self._ws.data_ptr(), sums)
        packed = torch.cuda.Event()
        packed.record()
        with torch.cuda.stream(self._side):
            self._side.wait_event(packed)
            self.pinned.copy_(self.staging, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record()
        # (the HOST side of the hand-off is the caller's: wait_host() before the pinned buffer is read, and before the next pack())

    def wait_host(self):
        """wait for pack()'s copy (an event wait: nothing is launched) -> (entries with sums, the blob: a uint32 view of the pinned buffer)"""
        if self._copied is None:
            raise RuntimeError("StatePacker.wait_host: no pack() in flight")
        self._copied.synchronize()
        host = self.pinned.numpy().view(np.uint32)
        sums = host[self.blob_words:].view(np.uint64).reshape(-1, 2)
        entries = [dict(e, s1=int(sums[i, 0]), s2=int(sums[i, 1])) for i, e in enumerate(self.entries)]
        return entries, host[:self.blob_words]

    def host_blob(self):
        """the pinned buffer's blob part as a writable uint32 array: read_file(path, blob_out=...) reads a file straight into it"""
        return self.pinned.numpy().view(np.uint32)[:self.blob_words]

    def restore(self, manifest) -> int:
        """the blob in host_blob() (read from `manifest`'s file) -> the tensors, in place, on the current stream: one host-to-device copy
        of blob and expected sums, hn_state_verify on the staging buffer, hn_state_unpack under its verdict, one host read of the
        verdict.  -> -1: every tensor holds the file's words; else the index of the first tensor whose words do not give the manifest's
        sums -- and then NO tensor was written."""
        ents = manifest["tensors"]
        if [(e["name"], e["dtype"], e["shape"], e["offset"]) for e in ents] != [(e["name"], e["dtype"], e["shape"], e["offset"]) for e in self.entries]:
            raise ValueError("StatePacker.restore: the manifest's tensors are not this packer's")
        if self._copied is not None:
            self._copied.synchronize()                              # (a pack's copy still reading the staging buffer / writing the pinned one)
        host = self.pinned.numpy().view(np.uint32)
        for i, e in enumerate(ents):                                # pad words are zero in every file written here, and stay zero in the staging buffer
            if e["words"] % 4 and host[e["offset"] + e["words"]:e["offset"] + (e["words"] + 3) // 4 * 4].any():
                return i
        host[self.blob_words:].view(np.uint64).reshape(-1, 2)[:] = np.array([[e["s1"], e["s2"]] for e in ents], dtype=np.uint64)
        _, _, back, owner = self._plan()
        torch.cuda.current_stream().wait_stream(self._side)
        self.staging.copy_(self.pinned, non_blocking=True)
        expect = self.staging.data_ptr() + 4 * self.blob_words
        lib().call("hn_state_verify", back.data_ptr(), owner.data_ptr(), self.blocks, len(ents), expect, self._ws.data_ptr(),
                   self._sums.data_ptr(), self.verdict.data_ptr())
        lib().call("hn_state_unpack", back.data_ptr(), owner.data_ptr(), self.blocks, self.verdict.data_ptr())
        bad, first = self.verdict.cpu().tolist()[:2]                # the one synchronising read
        return first if bad else -1
