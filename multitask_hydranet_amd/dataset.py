"""The reference's MultitaskData over its data-list layout (model/dataset/dataloader.py:164-426, dataset/utility.py:235-257), split for
device augmentation: a DataLoader worker only decodes the files (PIL, swapped to BGR as cv2.imread delivers), parses the labels, samples the
image's augmentation plan (augment.sample_plan; with dataloader.do_split from the split ratio of the source lanes, by the split rule given
at construction, e.g. augment.cal_split) and packs the batch's host buffers.  The batch carries `src_frames` / `src_segs` (packed uint8),
the parsed labels and `aug_plans` instead of `image`; HydraTrainer.to_gpu runs augment.augment_batch on it, which returns the Collater
contract.  Workers never touch the GPU.  With decode="device" a worker stops after the JPEG's entropy stage (jpeg.py: host functions of the
library) and the batch carries `src_coefs`, which to_gpu decodes on the device into the same packed frames.  With decode="device-entropy" a
worker only reads the file and parses its header: the batch carries the files' bytes (`src_streams`) and the device decodes the scans too.
With decode_labels="device" (independent of `decode`) a worker does not decode the label PNG either: it walks the chunk list (png.py) and
the batch carries the zlib streams (`src_seg_streams`), which to_gpu inflates and unfilters on the device into the packed label maps.

    ds = MultitaskData(cfgs, "train")                 # with dataloader.do_split: MultitaskData(cfgs, "train", split_rule=augment.cal_split)
    loader = DataLoader(ds, batch_size=16, shuffle=True, num_workers=8, collate_fn=ds.collate_fn, pin_memory=True)
    for epoch in ...: ds.set_epoch(epoch); trainer.train_one_epoch(epoch)

With dataloader.allow_missing_labels (default False: a missing label file raises FileNotFoundError, as ever) an image may lack the label
file of some trained tasks: every item carries `task_valid`, (seg, det, lane) as 0 / 1, the batch a uint8 [3, N] array of them, and the
losses are masked with it (HydraNet.cal_loss).  A missing label is replaced by a stand-in of the right shape -- an all-255
label map, no boxes, no lines -- so that packing, augmentation and the lane encoder run unchanged; the stand-ins only fill shapes, the
masks decide what is trained.  Images without a label for any trained task are dropped at construction (`unlabelled` counts them).
"""
from __future__ import annotations

import json
import os
from typing import Callable, Optional

import numpy as np

from .augment import identity_plan, pack, sample_plan


def load_img_list(path):
    with open(path) as f:
        return list(map(str.strip, f))


def create_subset(data_list, with_lane=False, with_seg=False, with_detect=False):
    """utility.py:235-257: every image path of the list and its label files (images -> labels_lane / labels_segmentation / labels_object)"""
    pairs = []
    for p in load_img_list(data_list):
        if not p:
            continue
        d = dict(image_path=p)
        if with_lane:
            d["annot_path_lane"] = p.replace(".jpg", ".json").replace("images", "labels_lane")
        if with_seg:
            d["annot_path_seg"] = p.replace(".jpg", ".png").replace("images", "labels_segmentation")
        if with_detect:
            d["annot_path_detect"] = p.replace(".jpg", ".txt").replace("images", "labels_object")
        pairs.append(d)
    return pairs


def parse_own_label(labels):
    """labelme json -> {"Lines": [[{"x", "y"}, ...]], "Labels": [...]} (dataloader.py:383-393)"""
    out = {"Lines": [], "Labels": []}
    for shape in labels["shapes"]:
        out["Lines"].append([{"x": pt[0], "y": pt[1]} for pt in shape["points"]])
        out["Labels"].append(shape["label"])
    return out


def load_detect_annot(path):
    """x1,y1,x2,y2,id lines -> [k, 5] x1, y1, x2, y2, id - 1 (float64); boxes narrower or lower than 1 px dropped (dataloader.py:395-426)"""
    rows = []
    with open(path) as f:
        for line in f.readlines():
            v = line.strip("\n").split(",")
            if len(v) < 5:
                continue
            x1, y1, x2, y2, cid = (int(v[i]) for i in range(5))
            if x2 - x1 < 1 or y2 - y1 < 1:
                continue
            rows.append([x1, y1, x2, y2, cid - 1])
    return np.array(rows, dtype=np.float64).reshape(-1, 5)


def imread_bgr(path):
    from PIL import Image
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[..., ::-1])


def imread_label(path):
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.ndim == 3:                                   # cv2.IMREAD_UNCHANGED of a colour png: the reference keeps channel 0 after imgaug
        a = a[..., 0]
    return np.ascontiguousarray(a.astype(np.uint8))


class MultitaskData:
    """torch Dataset (map style) of the reference's layout; items are host-side only"""

    def __init__(self, cfgs, mode, base_seed: int = 0, split_rule: Optional[Callable] = None, decode: str = "host",
                 decode_labels: str = "host"):
        """split_rule: (parsed lanes, source width, source height) -> (split possible, ratio), the rule that dataloader.do_split draws
        its split crops from; augment.cal_split is the reference's (MultitaskData.cal_split, its quirks kept).  A training set with
        augmentation and do_split needs one, and lane labels to apply it to.
        decode: "host" -- the worker decodes the JPEG with PIL (`src_frame`); "device" -- the worker runs only the entropy stage
        (jpeg.parse + jpeg.entropy_decode: `src_coefs` + `jpeg_head`) and HydraTrainer.to_gpu finishes the decode on the device
        (jpeg.decode_batch); "device-entropy" -- the worker only reads the file, parses its header and prepares its scan (jpeg.parse +
        jpeg.scan_prepare: `src_stream`, the file's bytes, + `jpeg_head` + `jpeg_scan`) and the device runs the Huffman stage too; a file
        outside jpeg.py's supported set is decoded with PIL as before, that image only.
        decode_labels: "host" -- the worker decodes the label PNG with PIL (`src_seg`); "device" -- the worker only parses the file
        (png.stream_stage: `src_seg_stream`, the zlib stream, + `png_head`) and HydraTrainer.to_gpu decodes it on the device
        (png.decode_batch); a file outside png.py's supported set is decoded with PIL as before, that image only."""
        if decode not in ("host", "device", "device-entropy"):
            raise ValueError("decode should be one of ('host', 'device', 'device-entropy')")
        if decode_labels not in ("host", "device"):
            raise ValueError("decode_labels should be one of ('host', 'device')")
        self.decode, self.decode_labels = decode, decode_labels
        dl = cfgs["dataloader"]
        self.cfgs, self.mode, self.base_seed, self.epoch = cfgs, mode, int(base_seed), 0
        self.network_input_width, self.network_input_height = dl["network_input_width"], dl["network_input_height"]
        self.with_aug = bool(dl.get("with_aug", False)) and mode != "val"
        self.do_flip = bool(dl.get("do_flip", False))
        self.do_split = bool(dl.get("do_split", False)) and self.with_aug
        self.split_rule = split_rule
        t = cfgs["train"]
        self.train_lane, self.train_seg, self.train_detect = t["train_lane"], t["train_seg"], t["train_detect"]
        if self.do_split and not self.train_lane:
            raise ValueError("dataloader.do_split needs train.train_lane: the split ratio is computed from the lane labels")
        if self.do_split and split_rule is None:
            raise NotImplementedError("dataloader.do_split without a split rule: construct MultitaskData(..., split_rule=augment.cal_split) "
                                      "for the reference's split ratio")
        if not (self.train_lane or self.train_seg or self.train_detect):
            raise ValueError("must train at least one header")
        if mode not in ("train", "val"):
            raise NotImplementedError("mode should be one of ('train', 'val')")
        lst = os.path.join(dl["data_list"], "train.txt" if mode == "train" else "valid.txt")
        self.image_annot_path_pairs = create_subset(lst, with_lane=self.train_lane, with_seg=self.train_seg, with_detect=self.train_detect)
        # dataloader.allow_missing_labels: every derived label path is checked once, here; an item then knows which labels it has
        self.allow_missing_labels = bool(dl.get("allow_missing_labels", False))
        self.unlabelled = 0
        if self.allow_missing_labels:
            kept = []
            for pair in self.image_annot_path_pairs:
                pair["task_valid"] = tuple(int(key in pair and os.path.isfile(pair[key]))
                                           for key in ("annot_path_seg", "annot_path_detect", "annot_path_lane"))
                if any(pair["task_valid"]):
                    kept.append(pair)
                else:
                    self.unlabelled += 1
            self.image_annot_path_pairs = kept

    def set_epoch(self, epoch: int):
        """plans are seeded from (base_seed, epoch, index): call before every epoch's iteration"""
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.image_annot_path_pairs)

    def __getitem__(self, idx):
        pair = self.image_annot_path_pairs[idx]
        head = scan = None
        if self.decode == "device-entropy":
            from . import jpeg
            if not os.path.exists(pair["image_path"]):
                raise FileNotFoundError(pair["image_path"])
            staged = jpeg.stream_stage(jpeg.read_bytes(pair["image_path"]))      # (header, scan record, bytes) or (None, PIL's frame)
            head = staged[0]
            if head is not None:
                scan, img = staged[1], np.frombuffer(staged[2], dtype=np.uint8)
            else:
                img = staged[1]
            h, w = (head["height"], head["width"]) if head is not None else img.shape[:2]
        elif self.decode == "device":
            from . import jpeg
            if not os.path.exists(pair["image_path"]):
                raise FileNotFoundError(pair["image_path"])
            head, img = jpeg.host_stage(jpeg.read_bytes(pair["image_path"]))       # (header, coefficients) or (None, PIL's frame)
            h, w = (head["height"], head["width"]) if head is not None else img.shape[:2]
        else:
            img = imread_bgr(pair["image_path"])
            h, w = img.shape[:2]
        if h < self.network_input_height or w < self.network_input_width:
            raise ValueError("%s: %dx%d is smaller than the network input %dx%d (INTER_AREA does not upscale)"
                             % (pair["image_path"], w, h, self.network_input_width, self.network_input_height))
        if scan is not None:
            item = dict(src_stream=img, jpeg_head=head, jpeg_scan=scan, src_image_shape=dict(width=w, height=h, channel=3),
                        src_image_path=pair["image_path"])
        elif head is not None:
            item = dict(src_coefs=img, jpeg_head=head, src_image_shape=dict(width=w, height=h, channel=3), src_image_path=pair["image_path"])
        else:
            item = dict(src_frame=img, src_image_shape=dict(width=w, height=h, channel=3), src_image_path=pair["image_path"])
        has_seg, has_det, has_lane = pair.get("task_valid", (1, 1, 1))       # (without allow_missing_labels: every file is opened)
        if self.allow_missing_labels:
            item["task_valid"] = np.array(pair["task_valid"], dtype=np.uint8)
        if self.train_lane:
            if has_lane:
                with open(pair["annot_path_lane"]) as f:
                    item["lane_raw"] = parse_own_label(json.load(f))
            else:
                item["lane_raw"] = {"Lines": [], "Labels": []}             # stand-in: no lines
            item["annot_lane_path"] = pair["annot_path_lane"]
        if not self.with_aug:
            item["aug_plan"] = identity_plan()
        elif self.do_split:                                   # dataloader.py:300-304: the ratio from the source lanes at source size
            ok, ratio = self.split_rule(item["lane_raw"], w, h) if has_lane else (False, None)     # no lane label: not split
            item["aug_plan"] = sample_plan(self.base_seed, self.epoch, idx, do_flip=self.do_flip, do_split=True, split_ratio=ratio if ok else None)
        else:
            item["aug_plan"] = sample_plan(self.base_seed, self.epoch, idx, do_flip=self.do_flip)
        if self.train_seg:
            phead = None
            if not has_seg:
                seg = np.full((h, w), 255, dtype=np.uint8)              # stand-in: every pixel ignored (the already-decoded slot of either path)
            elif self.decode_labels == "device":
                from . import png
                phead, seg = png.stream_stage(png.read_bytes(pair["annot_path_seg"]))   # (head, zlib stream) or (None, PIL's map)
            else:
                seg = imread_label(pair["annot_path_seg"])
            shape = (phead["height"], phead["width"]) if phead is not None else seg.shape
            if shape != (h, w):
                raise ValueError("%s: label map %s does not match the frame %s" % (pair["annot_path_seg"], shape, (h, w)))
            if phead is not None:
                item["src_seg_stream"], item["png_head"] = np.frombuffer(seg, dtype=np.uint8), phead
            else:
                item["src_seg"] = seg
        if self.train_detect:
            item["det_raw"] = load_detect_annot(pair["annot_path_detect"]) if has_det else np.zeros((0, 5), dtype=np.float64)
        return item

    def collate_fn(self, batch):
        return collate(batch, self.network_input_height, self.network_input_width)


def collate(batch, net_h, net_w):
    """host half of the Collater: the frames (and label maps) packed into one uint8 buffer each; labels and plans as lists.  A batch with
    entropy-decoded items (decode="device") carries `src_coefs` instead of `src_frames`: jpeg.pack_coefs' buffers, the PIL-decoded frames of
    its unsupported files among them; one with items of decode="device-entropy" carries `src_streams`, jpeg.pack_streams' buffers, likewise.
    A batch with items of decode_labels="device" carries `src_seg_streams` (png.pack_streams' buffers, the PIL-decoded maps of its
    unsupported files among them) in place of `src_segs`.  Items of dataloader.allow_missing_labels carry `task_valid`: the batch's is the
    uint8 [3, N] array of them (rows seg, det, lane), which HydraTrainer.to_gpu copies to the device."""
    if any("src_stream" in b for b in batch):
        from .jpeg import pack_streams
        src = dict(src_streams=pack_streams([(b["jpeg_head"], b["jpeg_scan"], b["src_stream"]) if "src_stream" in b else (None, b["src_frame"])
                                             for b in batch]))
    elif any("src_coefs" in b for b in batch):
        from .jpeg import pack_coefs
        src = dict(src_coefs=pack_coefs([(b["jpeg_head"], b["src_coefs"]) if "src_coefs" in b else (None, b["src_frame"]) for b in batch]))
    else:
        src = dict(src_frames=pack([b["src_frame"] for b in batch]))
    out = dict(**src, aug_plans=[b["aug_plan"] for b in batch],
               src_image_shape=[b["src_image_shape"] for b in batch], src_image_path=[b["src_image_path"] for b in batch],
               net_input_image_shape=[json.dumps(dict(width=net_w, height=net_h, channel=3))] * len(batch), net_input_hw=(net_h, net_w))
    if "lane_raw" in batch[0]:
        out["lane_raw"] = [b["lane_raw"] for b in batch]
        out["annot_lane_path"] = [b["annot_lane_path"] for b in batch]
    if any("src_seg_stream" in b for b in batch):
        from .png import pack_streams as pack_png
        out["src_seg_streams"] = pack_png([(b["png_head"], b["src_seg_stream"]) if "src_seg_stream" in b else (None, b["src_seg"]) for b in batch])
    elif "src_seg" in batch[0]:
        out["src_segs"] = pack([b["src_seg"] for b in batch])
    if "det_raw" in batch[0]:
        out["det_raw"] = [b["det_raw"] for b in batch]
    if "task_valid" in batch[0]:
        out["task_valid"] = np.ascontiguousarray(np.stack([b["task_valid"] for b in batch], axis=1).astype(np.uint8))
    return out
