"""CPU: the host share of the device's JPEG scan decode (hn_jpeg_scan_prepare through multitask_hydranet_amd/jpeg.py) and the Python
restatement of the device stage in its parallel formulation (tests/jpeg_scan_ref.py) against the host's entropy stage, exactly;
MultitaskData(decode="device-entropy"); the header and the library's exports.

Serial decoding with the record's tables runs in Python, so it covers the streams up to 157x66 and two of 640x360; for EVERY stream of the
matrix the record's tables are also compared with tables built here from the stream's own DHT segments, and its scan extent with the file."""
import re

import numpy as np
import pytest

from multitask_hydranet_amd import dataset as D
from multitask_hydranet_amd import jpeg
from multitask_hydranet_amd._lib import HEADER, lib
from tests import jpeg_cases as C
from tests import jpeg_scan_ref as SR

SMALL = [c for c in C.MATRIX if c[3][0] * c[3][1] <= 157 * 66]
# found by search over the matrix at S = 128: the first has an FF 00 pair and an RSTn marker astride subsequence boundaries and is longer
# than one window of 256 subsequences; the second is the 4:4:4 stream with the same properties bar the restart markers
LARGE = [("4:2:0", 50, True, (640, 360), 4), ("4:4:4", 50, True, (640, 360), 0)]
ROUNDS = {}


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _S():
    return int(lib().query("hn_jpeg_scan_subseq_bytes"))


def _dht_tables(data):
    """{(class, id): (look_n, look_v, maxcode, valoff, vals)} from the DHT segments before the scan, built with numpy"""
    out, pos = {}, 2
    while data[pos + 1] != 0xDA:
        m, ln = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        if m == 0xC4:
            d = data[pos + 4:pos + 2 + ln]
            o = 0
            while o < len(d):
                bits = np.frombuffer(d[o + 1:o + 17], dtype=np.uint8).astype(int)
                vals = np.zeros(256, dtype=np.uint8)
                vals[:bits.sum()] = np.frombuffer(d[o + 17:o + 17 + bits.sum()], dtype=np.uint8)
                look_n, look_v = np.zeros(512, dtype=np.uint8), np.zeros(512, dtype=np.uint8)
                maxcode, valoff = np.zeros(17, dtype=np.int32), np.zeros(17, dtype=np.int32)
                code = k = 0
                for length in range(1, 17):
                    valoff[length] = k - code
                    for i in range(bits[length - 1]):
                        if length <= 9:
                            first = (code + i) << (9 - length)
                            look_n[first:first + (1 << (9 - length))] = length
                            look_v[first:first + (1 << (9 - length))] = vals[k + i]
                    k += bits[length - 1]
                    code += bits[length - 1]
                    maxcode[length] = code - 1 if bits[length - 1] else -1
                    code <<= 1
                out[(d[o] >> 4, d[o] & 15)] = (look_n, look_v, maxcode, valoff, vals)
                o += 17 + bits.sum()
        pos += 2 + ln
    sos = data[pos + 4:pos + 2 + ((data[pos + 2] << 8) | data[pos + 3])]
    sel = [(sos[2 + 2 * c] >> 4, sos[2 + 2 * c] & 15) for c in range(sos[0])]
    return out, sel


@pytest.mark.parametrize("case", C.MATRIX, ids=C.case_id)
def test_scan_record_tables_and_extent(case):
    data = C.encode(case)
    head = jpeg.parse(data)
    rec = jpeg.scan_prepare(data, head)
    assert rec.dtype == jpeg.SCAN_DTYPE and rec.shape == (1,) and rec.nbytes == 8576
    r = rec[0]
    assert int(r["scan_offset"]) == head["scan_offset"] and int(r["scan_offset"] + r["scan_bytes"]) == len(data) and data[-2:] == b"\xff\xd9"
    assert [int(r[k]) for k in ("ncomp", "hs", "vs", "mcus_x", "mcus_y", "restart_interval")] == \
        [head[k] for k in ("ncomp", "hs", "vs", "mcus_x", "mcus_y", "restart_interval")]
    tabs, sel = _dht_tables(data)
    for c, (td, ta) in enumerate(sel):
        for got, want in ((r["dc"][r["td"][c]], tabs[(0, td)]), (r["ac"][r["ta"][c]], tabs[(1, ta)])):
            assert 0 <= r["td"][c] < 3 and 0 <= r["ta"][c] < 3
            assert np.array_equal(got["look_n"], want[0]) and np.array_equal(got["look_v"][want[0] > 0], want[1][want[0] > 0])
            assert np.array_equal(got["maxcode"][1:], want[2][1:]) and np.array_equal(got["valoff"][1:], want[3][1:])
            assert np.array_equal(got["vals"], want[4])


@pytest.mark.parametrize("case", SMALL + LARGE, ids=C.case_id)
def test_restatement_equals_the_host_entropy_stage(case):
    """serially with the record's tables, and in the device's parallel formulation: jpeg.entropy_decode's coefficients, exactly"""
    data = C.encode(case)
    head = jpeg.parse(data)
    rec = jpeg.scan_prepare(data, head)
    want = jpeg.entropy_decode(data, head)
    if case in SMALL:
        got, status = SR.decode_serial(data, head, rec)
        assert status == 0 and np.array_equal(got, want)
    got, status, rounds = SR.decode(data, head, rec, _S())
    assert status == 0 and got.dtype == want.dtype and np.array_equal(got, want)
    assert max(rounds) <= SR.T
    ROUNDS[C.case_id(case)] = rounds
    print("rounds per window:", rounds)


def test_boundary_cases_are_in_the_tested_set():
    """runs after the parametrised test above (file order) only to print the largest round count; the coverage itself is asserted here"""
    S = _S()
    seen = {"ff00": [], "rst": [], "short": [], "windows": []}
    for case in SMALL + LARGE:
        data = C.encode(case)
        for k, v in SR.straddles(data, jpeg.scan_prepare(data, jpeg.parse(data)), S).items():
            if v:
                seen[k].append(C.case_id(case))
    assert all(seen.values()), {k: len(v) for k, v in seen.items()}
    assert C.case_id(LARGE[0]) in seen["ff00"] and C.case_id(LARGE[0]) in seen["rst"] and C.case_id(LARGE[0]) in seen["windows"]
    assert any(n.endswith("-1x1") for n in seen["short"])
    if ROUNDS:
        print("largest round count of a window: %d (bound %d)" % (max(max(r) for r in ROUNDS.values()), SR.T))


def test_scan_prepare_refuses_foreign_heads_and_unsupported_streams():
    from PIL import Image
    import io
    a = C.encode(("4:2:0", 75, False, (157, 66), 4))
    b = C.encode(("4:2:0", 75, False, (17, 33), 0))
    with pytest.raises(jpeg.JpegError):
        jpeg.scan_prepare(a, jpeg.parse(b))
    bio = io.BytesIO()
    Image.fromarray(C.seeded_image(96, 64, 3)).save(bio, "JPEG", quality=80, progressive=True)
    rec = np.zeros(1, dtype=jpeg.SCAN_DTYPE)
    raw = lib().raw("hn_jpeg_scan_prepare")
    assert raw(bio.getvalue(), len(bio.getvalue()), jpeg.parse(a)["rec"].ctypes.data, rec.ctypes.data) == 3
    png = b"\x89PNG\r\n\x1a\n" + bytes(64)
    assert raw(png, len(png), jpeg.parse(a)["rec"].ctypes.data, rec.ctypes.data) == 1
    assert jpeg.stream_stage(bio.getvalue())[0] is None
    # a truncated stream: the scan runs to the end of the data
    cut = a[:len(a) - 40]
    r = jpeg.scan_prepare(cut, jpeg.parse(cut))[0]
    assert int(r["scan_offset"] + r["scan_bytes"]) == len(cut)


def test_pack_streams_layout():
    streams = [C.encode(("4:2:0", 75, False, (157, 66), 4)), C.encode(("grey", 50, True, (17, 33), 0))]
    frame = C.seeded_image(37, 21, 1)
    items = [jpeg.stream_stage(streams[0]), (None, frame), jpeg.stream_stage(streams[1])]
    pk = jpeg.pack_streams(items)
    assert pk["data"].dtype.is_floating_point is False and pk["data"].numel() % 16 == 0
    assert pk["offsets"].tolist()[1] == -1 and all(o % 16 == 0 for o in pk["offsets"].tolist() if o >= 0)
    assert [h is None for h in pk["heads"]] == [False, True, False] and np.array_equal(pk["frames"][1], frame)
    for i, k in ((0, 0), (2, 1)):
        o = int(pk["offsets"][i])
        assert pk["data"].numpy()[o:o + len(streams[k])].tobytes() == streams[k]
        assert int(pk["scans"]["stream_off"][k]) == o and int(pk["scans"]["coef_off"][k]) % 16 == 0
    assert int(pk["scans"]["coef_off"][1]) == items[0][0]["coef_bytes"] and pk["coef_bytes"] == sum(it[0]["coef_bytes"] for it in (items[0], items[2]))


def test_multitask_data_device_entropy(tmp_path):
    import io
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(C.seeded_image(96, 64, 3)).save(bio, "JPEG", quality=80, progressive=True)
    prog = bio.getvalue()
    ok = C.encode(("4:2:0", 75, False, (157, 66), 0))
    grey = C.encode(("grey", 75, True, (157, 66), 4))
    cfgs = C.write_tree(str(tmp_path), [("a.jpg", ok), ("b.jpg", prog), ("c.jpg", grey)], (64, 96))
    ds = D.MultitaskData(cfgs, "train", base_seed=3, decode="device-entropy")
    items = [ds[i] for i in range(3)]
    host = [D.MultitaskData(cfgs, "train", base_seed=3)[i] for i in range(3)]
    for i, data in ((0, ok), (2, grey)):
        assert set(items[i]) - set(host[i]) == {"src_stream", "jpeg_head", "jpeg_scan"} and set(host[i]) - set(items[i]) == {"src_frame"}
        assert items[i]["src_stream"].dtype == np.uint8 and items[i]["src_stream"].tobytes() == data
        assert items[i]["jpeg_head"]["width"] == 157 and items[i]["jpeg_scan"].dtype == jpeg.SCAN_DTYPE
        assert items[i]["aug_plan"] == host[i]["aug_plan"] and items[i]["src_image_shape"] == host[i]["src_image_shape"]
    assert list(items[1]) == list(host[1]) and np.array_equal(items[1]["src_frame"], C.pil_bgr(prog))
    b = ds.collate_fn(items)
    assert "src_frames" not in b and "src_coefs" not in b and list(b)[0] == "src_streams"
    pk = b["src_streams"]
    assert sorted(pk) == ["coef_bytes", "data", "frames", "heads", "lengths", "offsets", "scans"]
    assert [h is None for h in pk["heads"]] == [False, True, False] and pk["offsets"].tolist()[1] == -1
    assert np.array_equal(pk["frames"][1], items[1]["src_frame"]) and pk["lengths"].tolist() == [len(ok), 0, len(grey)]
    for i, data in ((0, ok), (2, grey)):
        o = int(pk["offsets"][i])
        assert pk["data"].numpy()[o:o + len(data)].tobytes() == data
    assert b["src_image_shape"][1] == dict(width=96, height=64, channel=3)
    small = C.write_tree(str(tmp_path / "s"), [("a.jpg", C.encode(("4:2:0", 75, False, (17, 33), 0)))], (64, 96))
    with pytest.raises(ValueError):                                   # the size check against the network input uses the header
        D.MultitaskData(small, "train", decode="device-entropy")[0]
    with pytest.raises(ValueError, match="device-entropy"):
        D.MultitaskData(cfgs, "train", decode="gpu")


def test_other_decode_modes_keep_their_items(tmp_path):
    imgs = [("a.jpg", C.encode(("4:2:0", 95, False, (157, 66), 0)))]
    cfgs = C.write_tree(str(tmp_path), imgs, (64, 96))
    tail = ["src_image_shape", "src_image_path", "lane_raw", "annot_lane_path", "aug_plan", "src_seg", "det_raw"]
    assert list(D.MultitaskData(cfgs, "train", base_seed=7, decode="host")[0]) == ["src_frame"] + tail
    assert list(D.MultitaskData(cfgs, "train", base_seed=7, decode="device")[0]) == ["src_coefs", "jpeg_head"] + tail
    bkeys = ["aug_plans", "src_image_shape", "src_image_path", "net_input_image_shape", "net_input_hw", "lane_raw", "annot_lane_path", "src_segs",
             "det_raw"]
    for mode, first, inner in (("host", "src_frames", ["data", "offsets", "shapes"]), ("device", "src_coefs", ["data", "frames", "heads", "offsets"])):
        ds = D.MultitaskData(cfgs, "train", base_seed=7, decode=mode)
        b = ds.collate_fn([ds[0]])
        assert list(b) == [first] + bkeys and sorted(b[first]) == inner


def test_header_declares_and_library_exports_the_scan_functions():
    txt = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name in ("hn_jpeg_scan_prepare", "hn_jpeg_scan_ws_bytes", "hn_jpeg_scan_subseq_bytes", "hn_jpeg_scan_decode"):
        assert re.search(r"\b(int|long)\s+%s\s*\(" % name, txt), name
        assert name in lib().symbols() and lib().raw(name) is not None
    S = _S()
    assert S in (64, 128, 256)
    q = lambda *a: int(lib().query("hn_jpeg_scan_ws_bytes", *a))
    assert q(3, 1000, 10) == 3 * ((1000 + S - 1) // S) * 16 and q(0, 1000, 10) == -1 and q(1, 0, 10) == -1
