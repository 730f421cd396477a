"""CPU: the Motion-JPEG AVI container (multitask_hydranet_amd/avi.py) against tests/avi_ref.py's independent muxer and walker -- the reader
on files the reference muxer built, the writer's files through the reference walker -- and the Huffman-table splice of table-less frames."""
import os
import re
import struct

import numpy as np
import pytest

from tests import avi_ref as R
from tests import jpeg_cases as C


def frames_of(index, data):
    return [bytes(data[o:o + s]) for o, s in index["frames"]]


def test_read_index_plain_file():
    from multitask_hydranet_amd import avi
    stored, _ = R.clip()
    data, spans = R.mux([(b"00dc", f) for f in stored], R.CLIP_W, R.CLIP_H, 30000, 1001)
    idx = avi.read_index(data)
    assert idx["frames"] == spans and len(spans) == 5
    assert (idx["width"], idx["height"], idx["rate"], idx["scale"], idx["fourcc"], idx["truncated"]) == (R.CLIP_W, R.CLIP_H, 30000, 1001, "MJPG", False)
    assert frames_of(idx, data) == list(stored)


def test_read_index_from_a_path(tmp_path):
    from multitask_hydranet_amd import avi
    stored, _ = R.clip()
    data, spans = R.mux([(b"00dc", f) for f in stored[:2]], R.CLIP_W, R.CLIP_H, 10, 1)
    (tmp_path / "a.avi").write_bytes(data)
    assert avi.read_index(str(tmp_path / "a.avi"))["frames"] == spans
    assert avi.read_index(tmp_path / "a.avi")["frames"] == spans


def test_read_index_odd_chunks_audio_junk_rec_and_no_idx1():
    """odd-sized chunks (pad byte), an interleaved 01wb chunk and a JUNK chunk inside movi, frames inside LIST rec, a 00db chunk, no idx1"""
    from multitask_hydranet_amd import avi
    payloads = [b"\xff\xd8" + bytes([i]) * n + b"\xff\xd9" for i, n in enumerate((7, 10, 1, 33, 2))]         # sizes 11, 14, 5, 37, 6
    items = [(b"00dc", payloads[0]), (b"01wb", b"\x80" * 5), (b"00dc", payloads[1]), (b"JUNK", b"\0" * 3),
             (b"rec ", [(b"00dc", payloads[2]), (b"01wb", b"\x80" * 7), (b"00db", payloads[3])]), (b"00dc", b""), (b"00dc", payloads[4])]
    data, spans = R.mux(items, 64, 48, 25, 1, idx1=False, audio=True)
    assert b"idx1" not in data
    idx = avi.read_index(data)
    assert idx["frames"] == spans and [s for _, s in spans] == [11, 14, 5, 37, 0, 6]
    assert frames_of(idx, data) == payloads[:4] + [b"", payloads[4]]
    assert (idx["width"], idx["height"], idx["rate"], idx["scale"], idx["stream"], idx["truncated"]) == (64, 48, 25, 1, 0, False)
    assert avi.frame_bytes(idx, data, 4) is None                         # the zero-length chunk: repeat the previous frame
    # lower-case fourcc is Motion-JPEG as well
    data2, spans2 = R.mux(items, 64, 48, 25, 1, fourcc=b"mjpg")
    assert avi.read_index(data2)["frames"] == spans2


def test_read_index_of_a_file_cut_inside_the_last_frame():
    from multitask_hydranet_amd import avi
    stored, _ = R.clip()
    data, spans = R.mux([(b"00dc", f) for f in stored], R.CLIP_W, R.CLIP_H, 10, 1, idx1=False)
    cut = data[:spans[4][0] + spans[4][1] // 2]
    idx = avi.read_index(cut)
    assert idx["frames"] == spans[:4] and idx["truncated"] is True
    # an interrupted recording: the size fields were never patched
    raw = bytearray(cut)
    raw[4:8] = struct.pack("<I", 0)
    movi = raw.index(b"movi")
    raw[movi - 4:movi] = struct.pack("<I", 0)
    idx = avi.read_index(bytes(raw))
    assert idx["frames"] == spans[:4] and idx["truncated"] is True


def test_read_index_refuses_other_codecs_and_opendml():
    from multitask_hydranet_amd import avi
    stored, _ = R.clip()
    data, _ = R.mux([(b"00dc", stored[0])], R.CLIP_W, R.CLIP_H, 10, 1, fourcc=b"XVID")
    with pytest.raises(ValueError, match="XVID"):
        avi.read_index(data)
    data, _ = R.mux([(b"00dc", stored[0])], R.CLIP_W, R.CLIP_H, 10, 1)
    ext = R.riff_list(b"movi", R.chunk(b"00dc", stored[1]))
    with pytest.raises(ValueError, match="AVIX"):
        avi.read_index(data + b"RIFF" + struct.pack("<I", 4 + len(ext)) + b"AVIX" + ext)
    with pytest.raises(ValueError):
        avi.read_index(b"RIFF\x04\0\0\0WAVE")


def test_writer_through_the_reference_walker(tmp_path):
    from multitask_hydranet_amd import avi
    stored, _ = R.clip()
    blobs = [stored[0], stored[1] + b"\0" if len(stored[1]) % 2 == 0 else stored[1], b"\xff\xd8\xff\xd9", stored[2][:-1] if len(stored[2]) % 2 == 0 else stored[2]]
    assert any(len(b) & 1 for b in blobs) and any(not len(b) & 1 for b in blobs)
    path = tmp_path / "out.avi"
    with avi.AviWriter(str(path), 1280, 720, fps=(30000, 1001)) as w:
        for b in blobs:
            w.write(b)
    data = path.read_bytes()
    got = R.walk(data)
    assert got["frames"] == blobs
    assert (got["width"], got["height"], got["avih_wh"], got["rate"], got["scale"]) == (1280, 720, (1280, 720), 30000, 1001)
    assert got["handler"] == b"MJPG" and got["compression"] == b"MJPG" and got["bit_count"] == 24 and got["streams"] == 1
    assert got["avih_frames"] == got["strh_length"] == len(blobs) and got["usec"] == 33367
    # size fields: the RIFF chunk is the whole file, the walk of its children ends exactly there, movi ends where idx1 begins
    assert got["riff_size"] + 8 == len(data) == got["end"]
    assert data[got["movi_pos"] + got["movi_size"]:][:4] == b"idx1"
    # idx1: one entry per frame, offsets relative to the 'movi' fourcc, pointing at the chunk headers
    assert len(got["idx1"]) == len(blobs)
    for (cid, flags, off, size), pos, b in zip(got["idx1"], got["chunk_pos"], blobs):
        assert cid == b"00dc" and flags & 0x10 and got["movi_pos"] + off == pos and size == len(b)
    # and our own reader agrees with the walker
    idx = avi.read_index(data)
    assert frames_of(idx, data) == blobs and not idx["truncated"]
    # the default rate is the reference's 10 fps; close() twice is harmless; write() after close() is an error
    w = avi.AviWriter(str(tmp_path / "d.avi"), 8, 8)
    w.close()
    w.close()
    with pytest.raises(ValueError):
        w.write(b"x")
    d = R.walk((tmp_path / "d.avi").read_bytes())
    assert (d["rate"], d["scale"], d["avih_frames"], d["frames"]) == (10, 1, 0, [])


def test_writer_raises_before_two_gib(tmp_path, monkeypatch):
    from multitask_hydranet_amd import avi
    monkeypatch.setattr(avi, "MAX_FILE_BYTES", 4096)
    with avi.AviWriter(str(tmp_path / "big.avi"), 8, 8) as w:
        w.write(b"\0" * 3000)
        with pytest.raises(ValueError, match="2 GiB"):
            w.write(b"\0" * 1000)
    got = R.walk((tmp_path / "big.avi").read_bytes())                    # the file that was closed is whole
    assert len(got["frames"]) == 1 and got["riff_size"] + 8 <= 4096
    assert avi.MAX_FILE_BYTES == 4096


def test_frame_bytes_splices_the_standard_tables():
    from multitask_hydranet_amd import avi
    stored, full = R.clip()
    data, _ = R.mux([(b"00dc", f) for f in stored], R.CLIP_W, R.CLIP_H, 10, 1)
    idx = avi.read_index(data)
    for t in range(5):
        got = avi.frame_bytes(idx, data, t)
        if t in R.CLIP_STRIPPED:
            assert got != stored[t] and avi.has_dht(got) is None and avi.has_dht(stored[t]) is not None
            assert np.array_equal(C.pil_bgr(got), C.pil_bgr(full[t]))            # exactly the pixels of the frame that kept its tables
        else:
            assert got == stored[t] == full[t]                                # a frame with its own DHT: byte for byte


def test_standard_tables_agree_with_the_library():
    """avi.py restates Annex K.3; csrc/hn_jpeg_tables.h is the library's statement.  Held together through the header's text and through
    the DHT segments the library's own JPEG writer emits."""
    from multitask_hydranet_amd import avi, jpeg_encode
    src = open(os.path.join(os.path.dirname(os.path.abspath(avi.__file__)), "csrc", "hn_jpeg_tables.h")).read()

    def table(name):
        body = re.search(r"\b%s\b[^=]*=\s*(\{.*?\});" % name, src, flags=re.S).group(1)
        return [int(v, 0) for v in re.findall(r"0x[0-9a-fA-F]+|\d+", body)]

    assert table("k_dc_bits") == list(avi.STD_DC_BITS[0] + avi.STD_DC_BITS[1])
    assert table("k_dc_vals") == list(avi.STD_DC_VALS)
    assert table("k_ac_bits") == list(avi.STD_AC_BITS[0] + avi.STD_AC_BITS[1])
    assert table("k_ac_vals") == list(avi.STD_AC_VALS[0] + avi.STD_AC_VALS[1])
    seg = avi.std_dht_segment()
    assert len(seg) == 2 + 418 and seg[:4] == b"\xff\xc4\x01\xa2"
    head = jpeg_encode.write_header(jpeg_encode.make_head(16, 16, 90, "4:2:2"))
    ours = {}
    pos = 4
    while pos < len(seg):
        n = sum(seg[pos + 1:pos + 17])
        ours[seg[pos]] = seg[pos + 1:pos + 17 + n]
        pos += 17 + n
    theirs = {}
    pos = 2
    while pos < len(head):                                               # SOI, then marker segments up to and including SOS
        assert head[pos] == 0xFF
        ln = struct.unpack_from(">H", head, pos + 2)[0]
        if head[pos + 1] == 0xC4:
            assert ln == 3 + 16 + sum(head[pos + 5:pos + 21])             # the library writes one table per segment
            theirs[head[pos + 4]] = head[pos + 5:pos + 2 + ln]
        pos += 2 + ln
    assert ours == theirs and sorted(ours) == [0x00, 0x01, 0x10, 0x11]
