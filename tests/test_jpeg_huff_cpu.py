"""The JPEG encode's entropy stage in its parallel formulation, without a GPU: tests/jpeg_huff_ref.py -- per-block bit
strings with the geometric predecessor, concatenation by prefix sum, one-padding, stuffing by count and scatter -- against the host
stage hn_jpeg_entropy_encode, which tests/test_jpeg_encode_cpu.py pins to PIL: header + restated scan + EOI equals its stream byte for
byte.  hn_jpeg_write_header against that stream's prefix.  The case set's own coverage is asserted, not assumed."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import jpeg_enc_ref as E
from tests import jpeg_huff_ref as H
from tests.test_jpeg_encode_cpu import GOLDEN_FRAMES, MATRIX, SUBSAMPLINGS, case_id, case_image, golden_bgr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOI = b"\xff\xd9"


@pytest.fixture(scope="module")
def JE():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import jpeg_encode
    return jpeg_encode


def planes(head):
    """[(first block, blocks per column, blocks per row, own blocks per column, own blocks per row)] of every component plane"""
    out, first = [], 0
    for c in range(head["ncomp"]):
        hs, vs = (head["hs"], head["vs"]) if c == 0 else (1, 1)
        bh, bw = head["mcus_y"] * vs, head["mcus_x"] * hs
        rw, rh = E.real_blocks(head, c)
        out.append((first, bh, bw, rh, rw))
        first += bh * bw
    return out


def hand_cases():
    """(name, width, height, sub-sampling, int16 [blocks, 64]) built by hand.  The blocks that only fill an MCU hold 30000, which no table
    can code: neither stage may read them."""
    rng = np.random.default_rng(7)
    zz = H.ZIGZAG
    out = []
    for ss, (w, h) in (("4:2:0", (33, 17)), ("4:2:2", (33, 17)), ("4:4:4", (17, 9)), ("grey", (33, 17)), ("4:2:0", (1, 1)), ("grey", (1, 1)),
                       ("4:2:0", (200, 120))):
        head = E.head_for(w, h, ss, 95)
        n = head["coef_bytes"] // 128
        tag = "%s-%dx%d" % (ss.replace(":", ""), w, h)
        zero = np.zeros((n, 64), np.int16)
        dc = zero.copy()
        for first, bh, bw, rh, rw in planes(head):
            y, x = np.mgrid[0:bh, 0:bw]
            dc[first:first + bh * bw, 0] = np.where((x + y) % 2 == 0, -1024, 1023).reshape(-1)     # differences of 0 and +-2047
        ac = zero.copy()
        ac[:, zz[1:]] = np.where(rng.integers(0, 2, (n, 63)) == 0, -1023, 1023) * (rng.integers(0, 12, (n, 63)) == 0)
        ac[0::3, zz[1:63]] = 0
        ac[0::3, zz[63]] = 1023                                          # a run of 62 zeros: three ZRL
        ac[1::3, zz[1:40]] = 0                                           # runs over 15 at varying places
        dense = rng.integers(-1023, 1024, (n, 64)).astype(np.int16)
        dense[:, 0] = rng.integers(-1024, 1024, n)
        for name, co in (("zero", zero), ("dc-alternating", dc), ("ac-1023", ac), ("dense", dense)):
            co = co.copy()
            for first, bh, bw, rh, rw in planes(head):
                p = co[first:first + bh * bw].reshape(bh, bw, 64)
                p[rh:] = 30000
                p[:, rw:] = 30000
            out.append(("%s-%s" % (name, tag), w, h, ss, co))
    return out


HAND = hand_cases()


def check(JE, w, h, ss, q, co):
    """-> (host stream, header length): the restated scan between the header and EOI equals the host stage's stream"""
    head = JE.make_head(w, h, q, ss)
    host = JE.entropy_encode(co, head)
    header = JE.write_header(head)
    assert host.startswith(header) and header[:2] == b"\xff\xd8" and header[-3:] == b"\x00\x3f\x00"        # ... the SOS segment's last bytes
    sos = header.rindex(b"\xff\xda")
    assert sos + 2 + ((header[sos + 2] << 8) | header[sos + 3]) == len(header)                              # nothing after the SOS segment
    scan = H.scan_bytes(head, co)
    same = header + scan + EOI == host
    print("restated scan %d bytes, host scan %d bytes, equal %s" % (len(scan), len(host) - len(header) - 2, same))
    assert same
    return host, len(header)


@pytest.mark.parametrize("case", MATRIX, ids=case_id)
def test_restatement_equals_host_stream(case, JE):
    ss, q, (w, h) = case
    check(JE, w, h, ss, q, E.encode_coefs(case_image(case), ss, q)[1])


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
@pytest.mark.parametrize("ss", SUBSAMPLINGS)
def test_restatement_equals_host_stream_on_committed_frames(name, ss, JE):
    bgr = golden_bgr(name)
    check(JE, bgr.shape[1], bgr.shape[0], ss, 95, E.encode_coefs(bgr, ss, 95)[1])


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_restatement_equals_host_stream_on_hand_made_coefficients(case, JE):
    name, w, h, ss, co = case
    check(JE, w, h, ss, 95, co)


def test_write_header_capacity_is_reported_and_respected(JE):
    from multitask_hydranet_amd._lib import lib
    fn = lib().raw("hn_jpeg_write_header")
    for ss, size in (("4:2:0", (157, 66)), ("grey", (17, 33))):
        head = JE.make_head(size[0], size[1], 75, ss)
        full = JE.write_header(head)
        assert len(full) == (623 if ss != "grey" else 328)               # SOI 2, APP0 18, DQT 69 each, SOF0 10 + 3 nc, DHT 33 + 183 per pair, SOS 8 + 2 nc
        for cap in (0, 1, 100, len(full) // 2, len(full) - 1):
            buf = np.full(len(full) + 64, 0xA5, dtype=np.uint8)
            assert fn(head["rec"].ctypes.data, buf.ctypes.data, cap) == JE.CAPACITY_TOO_SMALL, cap
            assert (buf[cap:] == 0xA5).all(), cap                        # nothing written at or past the capacity
            assert bytes(buf[:cap]) == full[:cap]
        buf = np.full(len(full) + 64, 0xA5, dtype=np.uint8)
        assert fn(head["rec"].ctypes.data, buf.ctypes.data, len(full)) == len(full)                       # the exact capacity is enough
        assert bytes(buf[:len(full)]) == full and (buf[len(full):] == 0xA5).all()
    bad = JE.make_head(16, 16, 75, "4:2:0")
    bad["rec"]["mcus_x"] = 7
    assert fn(bad["rec"].ctypes.data, buf.ctypes.data, 1024) == -1


@pytest.mark.parametrize("ss", ("4:2:0", "grey"))
def test_values_outside_the_tables_are_refused_by_both(ss, JE):
    head = JE.make_head(24, 24, 75, ss)
    n = head["coef_bytes"] // 128
    out = np.empty(1 << 16, np.uint8)
    ok = np.zeros((n, 64), np.int16)
    ok[:, 0] = 1023
    ok[:, 5] = -1023
    assert JE.entropy_status(ok, head, out) > 0
    H.scan_bytes(head, ok)
    for what, (b, k, v) in (("AC 1024", (1, 5, 1024)), ("AC -1024", (1, 63, -1024)), ("DC step 2048", (1, 0, -1025)), ("DC step -2048", (0, 0, 2048))):
        co = ok.copy()
        co[b, k] = v
        assert JE.entropy_status(co, head, out) == -1, what
        with pytest.raises(ValueError):
            H.scan_bytes(head, co)
    edge = ok.copy()
    edge[1, 0] = -1024                                                   # a step of exactly 2047: category 11, coded
    assert JE.entropy_status(edge, head, out) > 0
    assert JE.write_header(head) + H.scan_bytes(head, edge) + EOI == JE.entropy_encode(edge, head)


def coverage(JE, w, h, ss, q, co):
    """what the case exercises, from the host stream and the coefficients"""
    head = JE.make_head(w, h, q, ss)
    host = JE.entropy_encode(co, head)
    scan = host[len(JE.write_header(head)):-2]
    comp, real, blk, prev = H.scan_blocks(head)
    z = np.asarray(co).reshape(-1, 64).astype(np.int64)[blk[real]][:, H.ZIGZAG]
    nz = z[:, 1:] != 0
    k = np.arange(1, 64)[None, :]
    last = np.maximum.accumulate(np.where(nz, k, 0), axis=1)
    run = k - np.concatenate([np.zeros((len(z), 1), np.int64), last[:, :-1]], axis=1) - 1
    pred = np.where(prev[real] >= 0, np.asarray(co).reshape(-1, 64).astype(np.int64)[np.maximum(prev[real], 0), 0], 0)
    first, bh, bw, rh, rw = planes(head)[0]
    got = set()
    if b"\xff\x00" in scan: got.add("stuffed FF00")
    if (nz & (run > 15)).any(): got.add("ZRL")
    if (nz & (run > 47)).any(): got.add("three ZRL")
    if (H.bit_size(np.abs(z[:, 0] - pred)) == 11).any(): got.add("DC category 11")
    if (H.bit_size(np.abs(z[:, 1:])) == 10).any(): got.add("AC size 10")
    if (last[:, -1] == 63).any(): got.add("no EOB")
    if rw < bw: got.add("fill right %s" % ss)
    if rh < bh: got.add("fill below %s" % ss)
    if rw < bw and rh < bh: got.add("fill corner %s" % ss)
    if ss == "grey": got.add("greyscale")
    if (w, h) == (1, 1): got.add("1x1")
    if len(scan) > 2 * 4096: got.add("several stuffing chunks")
    if comp.size > 2 * 128: got.add("several tiles")
    return got


def test_the_case_set_covers_what_it_claims(JE):
    """4:2:2 has one luma block row per MCU row, so it has filling blocks to the right only"""
    got = set()
    for case in MATRIX:
        ss, q, (w, h) = case
        got |= coverage(JE, w, h, ss, q, E.encode_coefs(case_image(case), ss, q)[1])
    in_matrix = set(got)
    for name, w, h, ss, co in HAND:
        got |= coverage(JE, w, h, ss, 95, co)
    need = {"stuffed FF00", "ZRL", "three ZRL", "DC category 11", "AC size 10", "no EOB", "fill right 4:2:0", "fill below 4:2:0", "fill corner 4:2:0",
            "fill right 4:2:2", "greyscale", "1x1", "several stuffing chunks", "several tiles"}
    print("covered by MATRIX alone: %s" % sorted(in_matrix & need))
    print("covered only with the hand-made arrays: %s" % sorted((got - in_matrix) & need))
    assert not need - got, "the case set no longer exercises: %s" % sorted(need - got)


def test_header_declares_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hydranet_hip.h")).read(), flags=re.S)
    for decl in (r"long\s+hn_jpeg_write_header\s*\(", r"long\s+hn_jpeg_huff_ws_bytes\s*\(", r"int\s+hn_jpeg_huff_encode\s*\("):
        assert re.search(decl, txt), decl
    from multitask_hydranet_amd._lib import parse_header
    sig = parse_header()
    assert sig["hn_jpeg_huff_encode"][2] and not sig["hn_jpeg_write_header"][2]                            # the device stage takes a stream


def test_entropy_option_defaults_to_host(JE):
    from multitask_hydranet_amd import demo
    for fn in (JE.encode_batch, JE.imwrite, demo.Demo.process_device, demo.run_images):
        p = inspect.signature(fn).parameters
        assert "entropy" in p and p["entropy"].default == "host", fn
    assert inspect.signature(JE.entropy_encode_device).parameters["capacity"].default is None
    with pytest.raises(ValueError):
        JE.encode_batch([np.zeros((8, 8, 3), np.uint8)], entropy="gpu")  # refused before anything touches a device
