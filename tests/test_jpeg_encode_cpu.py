"""JPEG encode without a GPU: the integer restatement of the device stage (tests/jpeg_enc_ref.py) against PIL's own
encoder -- exact equality of the decoded pixels, of the quantisation tables and, through the host entropy stage, of every coefficient
block including the MCU-filling ones -- and the host entropy stage's stream (hn_jpeg_entropy_encode) against jpeg.parse /
jpeg.entropy_decode and PIL's decoder.  No tolerance anywhere."""
import io
import zlib

import numpy as np
import pytest

from tests import jpeg_enc_ref as E
from tests import jpeg_ref as R
from tests.jpeg_cases import GOLDEN_FRAMES, SIZES, golden_bytes, pil_bgr, seeded_image

SUBSAMPLINGS = ("4:4:4", "4:2:2", "4:2:0", "grey")
QUALITIES = (50, 75, 95, 100)
ENC_SIZES = tuple(SIZES) + ((9, 7), (33, 17))
MATRIX = [(ss, q, size) for ss in SUBSAMPLINGS for q in QUALITIES for size in ENC_SIZES]


def case_id(case):
    ss, q, (w, h) = case
    return "%s-q%d-%dx%d" % (ss.replace(":", ""), q, w, h)


def case_image(case):
    ss, q, (w, h) = case
    return np.ascontiguousarray(seeded_image(w, h, zlib.crc32(case_id(case).encode()))[..., ::-1])      # BGR


def pil_encode(bgr, ss, q):
    """PIL's stream of the BGR frame at the same settings (standard Huffman tables); grey takes channel 0"""
    from PIL import Image
    im = Image.fromarray(bgr[..., 0] if ss == "grey" else np.ascontiguousarray(bgr[..., ::-1]))
    kw = dict(quality=q, optimize=False)
    if ss != "grey":
        kw["subsampling"] = ss
    bio = io.BytesIO()
    im.save(bio, "JPEG", **kw)
    return bio.getvalue()


def golden_bgr(name):
    return pil_bgr(golden_bytes(name))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def jpeg_mods(built):
    from multitask_hydranet_amd import jpeg, jpeg_encode
    return jpeg, jpeg_encode


@pytest.mark.parametrize("quality", (1, 10, 30, 49) + QUALITIES)
def test_quality_scaled_tables_equal_pils(quality, jpeg_mods):
    from PIL import Image
    _, JE = jpeg_mods
    data = pil_encode(seeded_image(16, 16, 1), "4:2:0", quality)
    with Image.open(io.BytesIO(data)) as im:
        tabs = [np.array(im.quantization[i]) for i in sorted(im.quantization)]
    ours = E.quant_tables(quality)
    assert len(tabs) == 2 and np.array_equal(ours[0], tabs[0]) and np.array_equal(ours[1], tabs[1])
    lib_t = JE.quant_tables(quality)
    assert np.array_equal(lib_t[0], tabs[0]) and np.array_equal(lib_t[1], tabs[1]) and np.array_equal(lib_t[2], tabs[1])


def _check_restatement(bgr, ss, q):
    head, co = E.encode_coefs(bgr, ss, q)
    got = R.decode(head, E.fill_padding(head, co))
    want = pil_bgr(pil_encode(bgr, ss, q))
    assert got.shape == want.shape
    bad = int((got != want).sum())
    print("restatement vs PIL: %s q%d %dx%d mismatching samples %d" % (ss, q, bgr.shape[1], bgr.shape[0], bad))
    assert bad == 0


@pytest.mark.parametrize("case", MATRIX, ids=case_id)
def test_restatement_decodes_to_pils_pixels(case):
    _check_restatement(case_image(case), case[0], case[1])


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
@pytest.mark.parametrize("ss", SUBSAMPLINGS)
def test_restatement_decodes_to_pils_pixels_on_committed_frames(name, ss):
    _check_restatement(golden_bgr(name), ss, 95)


def _check_entropy_stage(jpeg, JE, bgr, ss, q):
    head, co = E.encode_coefs(bgr, ss, q)
    lib_head = JE.make_head(bgr.shape[1], bgr.shape[0], q, ss)
    for k in ("width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "coef_bytes"):
        assert lib_head[k] == head[k], k
    assert np.array_equal(lib_head["qt"], head["qt"])
    ours = JE.entropy_encode(co, lib_head)
    assert ours[:2] == b"\xff\xd8" and ours[-2:] == b"\xff\xd9"
    theirs = pil_encode(bgr, ss, q)
    h1, h2 = jpeg.parse(ours), jpeg.parse(theirs)
    assert h1 is not None and h2 is not None
    for k in ("width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "restart_interval", "coef_bytes"):
        assert h1[k] == h2[k], k
    assert np.array_equal(h1["qt"][:h1["ncomp"]], h2["qt"][:h2["ncomp"]])
    c1, c2 = jpeg.entropy_decode(ours, h1), jpeg.entropy_decode(theirs, h2)
    bad = int((c1 != c2).any(axis=1).sum())
    print("entropy stage vs PIL: %s q%d %dx%d blocks %d differing %d" % (ss, q, bgr.shape[1], bgr.shape[0], c1.shape[0], bad))
    assert bad == 0                                                      # every block, the MCU-filling ones included
    assert np.array_equal(c1, E.fill_padding(head, co))
    assert np.array_equal(pil_bgr(ours), pil_bgr(theirs))                # PIL opens our bytes and decodes the same pixels


@pytest.mark.parametrize("case", MATRIX, ids=case_id)
def test_entropy_stage_stream_equals_pils_coefficients(case, jpeg_mods):
    _check_entropy_stage(*jpeg_mods, case_image(case), case[0], case[1])


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
def test_entropy_stage_on_committed_frames(name, jpeg_mods):
    _check_entropy_stage(*jpeg_mods, golden_bgr(name), "4:2:0", 95)


def test_standard_huffman_tables_are_pils(jpeg_mods):
    """the DHT payloads we write are the Annex K tables libjpeg writes without optimize"""
    def dht(data):
        out, pos = {}, 2
        while data[pos + 1] != 0xDA:
            ln = (data[pos + 2] << 8) | data[pos + 3]
            if data[pos + 1] == 0xC4:
                seg, o = data[pos + 4:pos + 2 + ln], 0
                while o < len(seg):
                    n = sum(seg[o + 1:o + 17])
                    out[seg[o]] = bytes(seg[o:o + 17 + n])
                    o += 17 + n
            pos += 2 + ln
        return out
    _, JE = jpeg_mods
    bgr = np.ascontiguousarray(seeded_image(24, 24, 5)[..., ::-1])
    head, co = E.encode_coefs(bgr, "4:2:0", 75)
    a, b = dht(JE.entropy_encode(co, JE.make_head(24, 24, 75, "4:2:0"))), dht(pil_encode(bgr, "4:2:0", 75))
    assert sorted(a) == [0x00, 0x01, 0x10, 0x11] and a == b


@pytest.mark.parametrize("size", ((1, 1), (17, 33), (157, 66)))
def test_capacity_too_small_is_reported_and_respected(size, jpeg_mods):
    _, JE = jpeg_mods
    w, h = size
    bgr = np.ascontiguousarray(seeded_image(w, h, 3)[..., ::-1])
    head, co = E.encode_coefs(bgr, "4:2:0", 95)
    lib_head = JE.make_head(w, h, 95, "4:2:0")
    full = JE.entropy_encode(co, lib_head)
    for cap in (0, 1, 100, 622, len(full) // 2, len(full) - 1):
        buf = np.full(len(full) + 64, 0xA5, dtype=np.uint8)
        view = buf[:cap]
        assert JE.entropy_status(co, lib_head, view) == JE.CAPACITY_TOO_SMALL, cap
        assert (buf[cap:] == 0xA5).all(), cap                            # nothing written past the capacity
        assert bytes(buf[:cap]) == full[:cap] or cap == 0
    buf = np.full(len(full) + 64, 0xA5, dtype=np.uint8)
    assert JE.entropy_status(co, lib_head, buf[:len(full)]) == len(full)  # the exact capacity is enough
    assert bytes(buf[:len(full)]) == full and (buf[len(full):] == 0xA5).all()


def test_entropy_stage_rejects_bad_arguments(jpeg_mods):
    _, JE = jpeg_mods
    bgr = np.ascontiguousarray(seeded_image(16, 16, 3)[..., ::-1])
    head, co = E.encode_coefs(bgr, "4:4:4", 75)
    lib_head = JE.make_head(16, 16, 75, "4:4:4")
    out = np.empty(4096, np.uint8)
    assert JE.entropy_status(co[:-1], lib_head, out) == -1               # fewer coefficients than the header states
    big = co.copy()
    big[0, 5] = 2000                                                     # an AC value of 11 bits: no baseline code
    assert JE.entropy_status(big, lib_head, out) == -1
    with pytest.raises(ValueError):
        JE.entropy_encode(big, lib_head)
