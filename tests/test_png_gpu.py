"""GPU: the PNG label decode on the device (hn_png.hip through multitask_hydranet_amd/png.py) against dataset.imread_label, element for
element: the whole case matrix in ragged batches, two 1080x1920 files written by PIL's encoder, a fixed list of damaged streams (one per
status code) next to intact neighbours, the per-image PIL fallback, and MultitaskData(decode_labels="device") -> HydraTrainer.to_gpu
against decode_labels="host".  Integer throughout: no tolerance."""
import zlib

import numpy as np
import pytest
import torch

from multitask_hydranet_amd import dataset as D
from multitask_hydranet_amd import png
from multitask_hydranet_amd._lib import lib
from tests import png_cases as C
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 8192                            # bytes behind out and behind ws


def decode_guarded(items):
    """hn_png_decode on one batch of (head, zlib stream) into sentinel-filled out / ws with a guard band behind each and a status array
    longer than the batch -> (per-image maps, status words).  Asserts the guards."""
    pk = png.pack_streams(items)
    desc, idx, offs, shapes, max_idat, max_raw = png.describe_batch(pk)
    n = len(items)
    assert idx == list(range(n))
    ob = int(offs[-1])
    out = torch.full((ob + GUARD,), SENT, dtype=torch.uint8, device="cuda:0")
    wsb = int(lib().query("hn_png_ws_bytes", n, max_idat, max_raw))
    assert wsb > 0
    ws = torch.full((wsb + GUARD,), SENT, dtype=torch.uint8, device="cuda:0")
    status = torch.full((n + 16,), 77, dtype=torch.int32, device="cuda:0")
    data = pk["data"].to("cuda:0")
    desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to("cuda:0")
    lib().call("hn_png_decode", data.data_ptr(), int(data.numel()), desc_d.data_ptr(), n, max_idat, max_raw, ws.data_ptr(), wsb,
               out.data_ptr(), ob, status.data_ptr())
    torch.cuda.synchronize()
    flat, st = out.cpu().numpy(), status.cpu().numpy()
    assert (flat[ob:] == SENT).all(), "the decode wrote past the label buffer"
    assert (ws[wsb:] == SENT).all().item(), "the decode wrote past the workspace"
    assert (st[n:] == 77).all(), "the decode wrote past the status words"
    maps = [flat[int(offs[i]):int(offs[i + 1])].reshape(int(shapes[i, 0]), int(shapes[i, 1])) for i in range(n)]
    return maps, st[:n]


def test_matrix_decodes_to_imread_label():
    """all 168 cases in eight ragged batches (case k goes to batch k mod 8): every map equals PIL's, every status is 0"""
    files = [C.encode(case) for case in C.MATRIX]
    wrong, checked = [], 0
    for b in range(8):
        sel = list(range(b, len(files), 8))
        items = [png.stream_stage(files[k]) for k in sel]
        assert all(it[0] is not None for it in items)
        maps, st = decode_guarded(items)
        for k, m, s in zip(sel, maps, st):
            want = C.expected(files[k])
            checked += 1
            if s != 0 or m.shape != want.shape or not np.array_equal(m, want):
                wrong.append((C.case_id(C.MATRIX[k]), int(s), int((m != want).sum()) if m.shape == want.shape else -1))
    assert checked == 168
    assert not wrong, "device maps differ (case, status, pixels off): %s" % wrong[:12]


def test_1080x1920_files_written_by_pil():
    big = C.big_files()
    want = [C.expected(d) for d in big]
    maps, st = decode_guarded([png.stream_stage(big[k % 2]) for k in range(16)])
    assert (st == 0).all(), st
    for k, m in enumerate(maps):
        assert np.array_equal(m, want[k % 2]), k


class BitWriter:
    def __init__(self):
        self.bits = []

    def lsb(self, v, n):                 # header fields and extra bits: least significant bit first
        self.bits += [(v >> i) & 1 for i in range(n)]
        return self

    def code(self, v, n):                # Huffman codes: most significant bit first
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + j] << j for j in range(8)) for i in range(0, len(b), 8))


def _head(w, h, bpp=1):
    return {"width": w, "height": h, "color_type": 0 if bpp == 1 else 2, "bpp": bpp, "raw_bytes": h * (1 + w * bpp), "idat": [], "file": b""}


STORED = ("grey", "f2", "stored", 0, (97, 61), "stripe3", 72)
DYNAMIC = ("grey", "f1", "l9", 0, (5, 129), "poly", 64)
FIXED = ("grey", "f0", "fixed", 7, (97, 61), "stripe2", 104)


def damaged():
    """the fixed list: (name, expected status, (head, stream)), each a deterministic edit of a named case of the matrix"""
    out = []
    for case in (STORED, DYNAMIC, FIXED):
        assert case in C.MATRIX
    head, s = png.stream_stage(C.encode(STORED))
    assert C.first_block_type(s) == 0
    out.append(("reserved block type", 1, (head, s[:2] + bytes([s[2] | 0x06]) + s[3:])))
    out.append(("LEN/NLEN mismatch", 2, (head, s[:5] + bytes([s[5] ^ 0xFF]) + s[6:])))
    out.append(("Adler-32 trailer patched", 9, (head, s[:-1] + bytes([s[-1] ^ 0x01]))))
    out.append(("zlib header patched", 10, (head, bytes([0x79]) + s[1:])))
    raw = bytearray(C.raw_scanlines(STORED))
    raw[0] = 7
    out.append(("filter byte 7", 8, (head, zlib.compress(bytes(raw), 6))))
    hd, d = png.stream_stage(C.encode(DYNAMIC))
    assert C.first_block_type(d) == 2
    out.append(("HLIT patched to 288 codes", 3, (hd, d[:2] + bytes([d[2] | 0xF8]) + d[3:])))
    out.append(("truncated in the middle", 6, (hd, d[:len(d) // 2])))
    out.append(("one row more than the stream holds", 7, (dict(hd, height=hd["height"] + 1, raw_bytes=hd["raw_bytes"] + 1 + hd["width"]), d)))
    out.append(("one row fewer than the stream holds", 7, (dict(hd, height=hd["height"] - 1, raw_bytes=hd["raw_bytes"] - 1 - hd["width"]), d)))
    hf, f = png.stream_stage(C.encode(FIXED))
    assert C.first_block_type(f) == 1
    # the case's fixed block replaced by hand-written ones: litlen symbol 286 (8 bits, 11000110), which no length belongs to
    out.append(("litlen symbol 286", 4, (hf, f[:2] + BitWriter().lsb(1, 1).lsb(1, 2).code(0b11000110, 8).bytes() + bytes(4))))
    # distance symbol 30 (5 bits, 11110) behind literal 0 (00110000) and length symbol 257 (0000001)
    out.append(("distance symbol 30", 4, (hf, f[:2] + BitWriter().lsb(1, 1).lsb(1, 2).code(0b00110000, 8).code(1, 7).code(30, 5).bytes() + bytes(4))))
    # distance 2 (symbol 1) with one byte of output
    out.append(("distance before the output", 5, (hf, f[:2] + BitWriter().lsb(1, 1).lsb(1, 2).code(0b00110000, 8).code(1, 7).code(1, 5).bytes() + bytes(4))))
    return out


def test_damaged_streams_report_their_status_and_spare_their_neighbours():
    """input validation: every damaged stream ends as its status word, its intact neighbours are exact, nothing is written out of bounds"""
    bad = damaged()
    assert sorted(set(code for _, code, _ in bad)) == list(range(1, 11))
    good = [C.encode(c) for c in (C.MATRIX[70], C.MATRIX[24], C.MATRIX[129])]
    items, roles = [], []
    for k, (name, code, it) in enumerate(bad):
        items.append(png.stream_stage(good[k % 3]))
        roles.append(("good", k % 3))
        items.append(it)
        roles.append((name, code))
    items.append(png.stream_stage(good[0]))
    roles.append(("good", 0))
    maps, st = decode_guarded(items)
    want = [C.expected(g) for g in good]
    got = {}
    for (name, code), m, s in zip(roles, maps, st):
        if name == "good":
            assert s == 0 and np.array_equal(m, want[code])
        else:
            got[name] = int(s)
    assert got == {name: code for name, code, _ in bad}


def _extra_rows_file():
    """a file whose stream holds one row more than its IHDR says: the device rejects it (status 7), PIL stops at the last row it needs"""
    case = C.MATRIX[24]
    w, h = case[4]
    raw = C.raw_scanlines(case)
    return C.write_png(w, h, 0, zlib.compress(raw + bytes(1 + w), 6))


def test_decode_batch_falls_back_to_pil_per_image():
    from tests.test_png_cpu import _variant
    sixteen = _variant(depth=16, w=9, h=7)
    extra = _extra_rows_file()
    files = [C.encode(C.MATRIX[70]), sixteen, C.encode(C.MATRIX[129]), extra, C.encode(C.MATRIX[45])]
    want = [C.expected(f) for f in files]                                # PIL decodes every one of them
    assert png.parse(sixteen) is None and png.parse(extra) is not None
    got = png.imread_label_device(files, device="cuda:0")
    assert got["status"][:4].cpu().tolist() == [0, 0, 7, 0]              # one word per stream: the 16-bit file has none
    flat = got["data"].cpu().numpy()
    for i, w_ in enumerate(want):
        assert tuple(got["shapes"][i]) == w_.shape
        o = int(got["offsets"][i])
        assert np.array_equal(flat[o:o + w_.size].reshape(w_.shape), w_), i
    # a file neither decodes: PIL's error propagates
    s = bytearray(C.encode(C.MATRIX[24]))
    head = png.parse(bytes(s))
    o, n = head["idat"][0]
    broken = C.write_png(63, 5, 0, bytes(s[o:o + n // 2]))
    assert png.parse(broken) is not None
    with pytest.raises(Exception):
        C.expected(broken)
    with pytest.raises(Exception):
        png.imread_label_device([files[0], broken], device="cuda:0")


def test_trainer_device_labels_equal_host_labels(tmp_path):
    """to_gpu's batch from decode_labels="device" equals the decode_labels="host" one bit for bit: augmentation on and off, under
    decode="host" and decode="device-entropy" """
    from multitask_hydranet_amd.train import HydraTrainer
    from tests import jpeg_cases as J
    cfgs = load_cfg("hydranet_tiny.yml")
    dl = cfgs["dataloader"]
    tree = J.write_tree(str(tmp_path), [(n, J.golden_bytes(n)) for n in J.GOLDEN_FRAMES], (dl["network_input_height"], dl["network_input_width"]))
    dl.update(tree["dataloader"])
    torch.manual_seed(0)
    tr = HydraTrainer(cfgs, iters_per_epoch=10)
    for aug in (True, False):
        dl["with_aug"] = aug
        for decode in ("host", "device-entropy"):
            got = {}
            for labels in ("host", "device"):
                ds = D.MultitaskData(cfgs, "train", base_seed=4, decode=decode, decode_labels=labels)
                ds.set_epoch(3)
                batch = ds.collate_fn([ds[i] for i in range(len(ds))])
                assert ("src_seg_streams" in batch) == (labels == "device") and ("src_segs" in batch) == (labels == "host")
                assert ("src_streams" in batch) == (decode == "device-entropy")
                got[labels] = tr.to_gpu(batch)
            torch.cuda.synchronize()
            if aug:
                assert any(p["augmented"] and (p["photo"] or p["geom"]) for p in batch["aug_plans"])
            for k in ("image", "gt_seg", "gt_det", "gt_cls", "gt_loc"):
                a, b = got["host"][k], got["device"][k]
                assert a.is_cuda and b.is_cuda and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (aug, decode, k)
            assert got["device"]["gt_seg"].float().sum().item() > 0
            assert "src_seg_streams" not in got["device"] and "src_segs" not in got["device"]
