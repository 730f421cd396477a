"""demo.py of the reference (model/demo.py:52-261) on the HIP path: frame -> pre-processing -> HydraNet forward -> the three decodes.

    python -m multitask_hydranet_amd.demo [--cfg cfgs/hydranet_big.yml] [--weights ckpt.pth] --video IN.avi --out OUT.avi [--batch N] [--size WxH] [--max-frames N]
    python -m multitask_hydranet_amd.demo [--cfg cfgs/hydranet_big.yml] [--weights ckpt.pth] --images DIR --out DIR_VIS [--save-seg DIR_SEG [--seg-palette] [--seg-huffman dynamic]]
    python -m multitask_hydranet_amd.demo [--cfg cfgs/hydranet_big.yml] [--weights ckpt.pth] [--frames frames.npy] [--out demo_out]

What is kept: the configuration handling (network input size, which heads run, lane codec geometry, colour table), `module.`-prefixed
checkpoints (deparallel_model, demo.py:33-50), the per-frame sequence BGR -> RGB -> resize -> imagenet_normalize -> forward ->
laneheader.decode + scale_to_org, segheader.decode, detectheader.decode, and the thresholds demo.py hard-codes (lane 0.90 / 80, detection
0.4 / 0.3).  Every stage runs on the device (hn_preprocess_bgr, the folded-BatchNorm inference forward, hn_lane_decode_nms,
hn_seg_overlay, hn_det_postprocess).
--images is the reference's image-folder mode (demo.py:136-160, 260-261): every *.jpg / *.jpeg of DIR in sorted order is decoded onto the
device (jpeg.imread_bgr_device), runs the sequence above, is DRAWN in the reference's order -- laneheader.visual, the seg overlay,
detectheader.display (draw.py) -- and is written as a JPEG of the same name into --out (jpeg_encode); the frame stays on the device from
decode to encode (Demo.process_device).
--video is the reference's default mode (demo.py:64, 155-160, 178, 251-255: cv2.VideoCapture in, cv2.VideoWriter out) for a Motion-JPEG AVI: the
container is read and written by avi.py, the frames are the JPEGs the project decodes and encodes itself, taken in groups of --batch
through the same stages with one launch sequence and one host synchronisation per group (Demo.process_device_batch), resized to --size on
the device when one is given (hn_resize_bgr8), and written at the input's frame rate, with OUT.avi.results.json beside it (run_video).
What is not: cv2 (absent from this image), so no window, and no video codec other than Motion-JPEG.  Without --images / --video the frames
come from a .npy array [T, H, W, 3] uint8 BGR or are synthesised, the blended frames are returned without drawing (and written as .npy by the command line) and
the decoded lanes and boxes are returned as data (Demo.process).
--save-seg DIR (with --images / --video) also keeps what the seg head predicted, not only its colour blend: the arg-max class map the overlay
is painted from, nearest-resized to the frame's original size and written as an 8-bit label PNG per frame (<image stem>.png, or
frame_%06d.png for a video) -- the format MultitaskData reads its seg labels from.  Filter and deflate run on the device (png_encode,
hn_png_enc.hip); --seg-palette writes colour type 3 with the demo's colours instead of grey, the same index bytes; --seg-huffman dynamic
deflates with a Huffman code per block instead of the fixed one: the same pixels, smaller files.
--lane-seg-filter [--lane-top-k N --lane-seg-ratio R --lane-seg-width T --lane-seg-class C] (any mode) adds the one step of the reference's
deploy path that uses two heads together (deploy/src/model/hydranet_model.cpp:546-607): the lanes the NMS leaves are capped at 14 and each
is kept only when more than 1 % of its pixels, painted 20 wide, lie on the seg arg-max map's class 2 (marking_area).  It runs on the device
between the lane decode and its readback (hn_lane_seg_filter); only the survivors are drawn and results.json gains every
selected lane's score, painted area, overlap and verdict.  Off by default."""
from __future__ import annotations

import argparse
import os
import time
from typing import Dict, List, Optional

import numpy as np
import torch
import yaml

SEG_CLASS_COLOR_ID = {0: (0, 0, 0), 1: (128, 0, 128), 2: (255, 255, 255), 3: (0, 255, 255), 4: (0, 255, 0)}    # demo.py:91-96


def seg_palette(colors: dict) -> dict:
    """the demo's colour table (BGR, as it is painted into BGR frames) -> a PNG palette {id: (r, g, b)}"""
    return {int(k): (int(c[2]), int(c[1]), int(c[0])) for k, c in colors.items()}


class Demo:
    """the state demo.py sets up before its frame loop (demo.py:68-134)"""

    def __init__(self, cfgs: dict, weights: Optional[str] = None, device="cuda:0", fold_batchnorm: bool = True, lane_seg_filter=None,
                 det_nms=None):
        """det_nms: a postprocess.NmsOptions -- the suppression rule every process* call decodes its boxes with; None: the
        rule of the cfg's detection.nms_* keys, the reference's hard NMS without them.
        lane_seg_filter: True (the deploy header's constants) or a lane_codec.LaneSegFilter -- every process* call then caps the decoded
        lanes and filters them by the seg head's marking class on the device; each call's own lane_seg_filter argument
        overrides it (False: off for that call).  Needs a configuration that runs the seg head and the lane head."""
        from . import HydraNet
        from .lane_codec import LaneCodec
        self.cfgs = cfgs
        dl = cfgs["dataloader"]
        self.net_w, self.net_h = dl["network_input_width"], dl["network_input_height"]
        tr = cfgs["train"]
        self.train_detect, self.train_seg, self.train_lane = tr["train_detect"], tr["train_seg"], tr["train_lane"]
        self.obj_list = cfgs["detection"]["class_list"][1:]
        lane = cfgs["lane"]
        self.lane_coder = LaneCodec(input_width=self.net_w, input_height=self.net_h, anchor_stride=lane["anchor_stride"],
                                    points_per_line=int(self.net_h / lane["interval"]), do_interpolate=lane["interpolate"],
                                    anchor_lane_num=lane["anchor_lane_num"], scale_invariance=lane["scale_invariance"])
        self.colors = dict(SEG_CLASS_COLOR_ID)
        self.lane_conf, self.lane_nms = 0.90, 80          # demo.py:212-213 (hard-coded there, not the cfg's values)
        self.det_conf, self.det_iou = 0.4, 0.3            # demo.py:241
        self.lane_seg_filter = self._lane_filter(lane_seg_filter, None)
        self.device = torch.device(device)
        self.net = HydraNet(cfgs=cfgs, onnx_export=False).to(self.device)
        if weights:
            self.net.load_state_dict(torch.load(weights, map_location="cpu"))    # (`module.` prefixes are stripped by load_state_dict)
        self.net.eval()
        from .postprocess import NmsOptions
        if det_nms is not None and not isinstance(det_nms, NmsOptions):
            raise ValueError("det_nms is a postprocess.NmsOptions or None, not %r" % (det_nms,))
        self.det_nms = det_nms if det_nms is not None else getattr(self.net, "det_nms", None)
        if fold_batchnorm:
            self.net.prepare_inference()

    def _det_nms_kw(self):
        """detectheader.decode's nms argument: only when a rule is set, so that without one the call is what it always was"""
        return {} if self.det_nms is None else {"nms": self.det_nms}

    def _lane_filter(self, asked, default):
        """the LaneSegFilter a call runs with: its own argument (True: the deploy defaults, False: none), else the constructor's"""
        from .lane_codec import LaneSegFilter
        if asked is None:
            return default
        if asked is False:
            return None
        flt = LaneSegFilter() if asked is True else asked
        if not isinstance(flt, LaneSegFilter):
            raise ValueError("lane_seg_filter is True or a LaneSegFilter, not %r" % (asked,))
        if not (self.train_seg and self.train_lane):
            raise ValueError("the lane seg filter needs the seg head and the lane head, but this configuration runs train_seg=%s, "
                             "train_lane=%s" % (self.train_seg, self.train_lane))
        return flt

    @torch.no_grad()
    def process(self, input_img: np.ndarray, lane_seg_filter=None) -> Dict[str, object]:
        """one iteration of demo.py's loop (demo.py:176-246) for one BGR frame [H, W, 3] uint8.  lane_seg_filter: see __init__;
        "lane_filter" then holds the selected lanes' statistics and "lanes" only the survivors."""
        from .preprocess import preprocess_bgr
        net = self.net
        flt = self._lane_filter(lane_seg_filter, self.lane_seg_filter)
        org_h, org_w = input_img.shape[:2]
        org_size = (org_w, org_h)
        tic = time.time()
        img = preprocess_bgr(input_img, (self.net_h, self.net_w), device=self.device)       # demo.py:186-196
        outputs = net(img)                                                                    # demo.py:201
        res: Dict[str, object] = {"org_size": org_size}
        imgs: List[np.ndarray] = [input_img]
        if self.train_lane:                                                                   # demo.py:209-228
            cls_preds, loc_preds = outputs["lane"]["predict_cls"], outputs["lane"]["predict_loc"]
            lanes = []
            mask = self._seg_mask(outputs["seg"]) if flt is not None else None
            for b in range(len(imgs)):
                if flt is None:
                    nms_set = net.laneheader.decode(cls_preds[b], loc_preds[b], self.lane_coder, self.lane_conf, self.lane_nms, False)
                else:
                    nms_set, stats = net.laneheader.decode(cls_preds[b], loc_preds[b], self.lane_coder, self.lane_conf, self.lane_nms, False,
                                                           seg_mask=mask[b], seg_filter=flt, return_stats=True)
                    res.setdefault("lane_filter", []).append(stats)
                lanes.append(net.laneheader.scale_to_org(nms_set, self.net_w, self.net_h, org_size[0], org_size[1])["Lines"])
            res["lanes"] = lanes
        if self.train_seg:                                                                    # demo.py:230-233
            imgs = net.segheader.decode(imgs, outputs["seg"], org_size, self.colors)
        if self.train_detect:                                                                 # demo.py:236-242
            det = outputs["detection"]
            res["detections"] = net.detectheader.decode(img, det["regression"], det["classification"], det["anchors"], conf_thres=self.det_conf,
                                                        iou_thres=self.det_iou, **self._det_nms_kw())
        torch.cuda.synchronize(self.device)
        res["visual"] = imgs[0]
        res["ms"] = 1000.0 * (time.time() - tic)
        return res


    @torch.no_grad()
    def _need_seg(self):
        if not self.train_seg:
            raise ValueError("seg class maps were asked for, but this configuration runs no seg head (train.train_seg is off)")

    def _seg_mask(self, seg):
        """the arg-max class map [N, H, W] int64 the overlay is painted from (the deploy forward already returns it)"""
        from . import ops as K
        return K.argmax_channels(seg.detach().float()) if seg.dim() == 4 else seg

    @torch.no_grad()
    def process_device(self, frames: dict, quality: int = 95, subsampling: str = "4:2:0", entropy: str = "host", seg_png: bool = False,
                       seg_palette: Optional[dict] = None, seg_huffman: str = "fixed", lane_seg_filter=None) -> Dict[str, object]:
        """the same iteration for ONE frame that is already on the device in the packed layout of jpeg.imread_bgr_device, with the
        reference's drawing (demo.py:230, 235, 244) and its cv2.imwrite (demo.py:261): "jpeg" holds the annotated frame's JFIF bytes,
        "visual" the annotated frame in the packed device layout.  The frame is not copied to the host.  entropy: "host" | "device", where
        the Huffman stage of the encode runs (jpeg_encode.encode_batch); the bytes are the same.  seg_png: "seg_png" holds the PNG file
        bytes of the arg-max class map at the frame's original size (png_encode.encode_batch; colour type 3 with seg_palette = {id: (r, g,
        b)}, grey without; seg_huffman: "fixed" | "dynamic", png_encode's huffman -- the same pixels in a smaller file); everything else is
        what the call gives without it.  lane_seg_filter: see __init__ -- the lanes are capped and filtered by the arg-max map this call
        paints its overlay from, before the one readback of the decode; "lanes" holds the survivors, "lane_filter" the statistics."""
        from . import draw, jpeg_encode, png_encode
        if seg_png:
            self._need_seg()
        flt = self._lane_filter(lane_seg_filter, self.lane_seg_filter)
        from .preprocess import preprocess_bgr
        from .visual import seg_decode_device
        net = self.net
        assert len(frames["shapes"]) == 1, "one frame per call"
        org_h, org_w = (int(v) for v in frames["shapes"][0])
        org_size = (org_w, org_h)
        nbytes = org_h * org_w * 3
        tic = time.time()
        off = int(frames["offsets"][0])
        frame = frames["data"][off:off + nbytes].view(1, org_h, org_w, 3)
        img = preprocess_bgr(frame, (self.net_h, self.net_w), device=self.device)
        outputs = net(img)
        res: Dict[str, object] = {"org_size": org_size}
        if self.train_lane:
            cls_preds, loc_preds = outputs["lane"]["predict_cls"], outputs["lane"]["predict_loc"]
            if flt is None:
                nms_set = net.laneheader.decode(cls_preds[0], loc_preds[0], self.lane_coder, self.lane_conf, self.lane_nms, False)
            else:
                mask = self._seg_mask(outputs["seg"])
                nms_set, stats = net.laneheader.decode(cls_preds[0], loc_preds[0], self.lane_coder, self.lane_conf, self.lane_nms, False,
                                                       seg_mask=mask[0], seg_filter=flt, return_stats=True)
                res["lane_filter"] = [stats]
            res["lanes"] = [net.laneheader.scale_to_org(nms_set, self.net_w, self.net_h, org_w, org_h)["Lines"]]
            frames = net.laneheader.visual(frames, res["lanes"], org_w, filter_vertical=True)
        if self.train_seg:
            seg = mask if flt is not None else self._seg_mask(outputs["seg"]) if seg_png else outputs["seg"]
            blended = seg_decode_device(frame, seg, self.colors)
            frames = {"data": blended.view(-1), "offsets": np.zeros(1, np.int64), "shapes": np.array([[org_h, org_w]], np.int64)}
            if seg_png:
                res["seg_png"] = png_encode.encode_batch(seg, out_sizes=(org_h, org_w), palette=seg_palette, device=self.device,
                                                           huffman=seg_huffman)[0]
        if self.train_detect:
            det = outputs["detection"]
            res["detections"] = net.detectheader.decode(img, det["regression"], det["classification"], det["anchors"], conf_thres=self.det_conf,
                                                        iou_thres=self.det_iou, **self._det_nms_kw())
            frames = net.detectheader.display(res["detections"], frames, self.obj_list, org_size, (self.net_w, self.net_h))
        res["jpeg"] = jpeg_encode.encode_batch(frames, quality, subsampling, entropy)[0]
        res["visual"] = frames
        res["ms"] = 1000.0 * (time.time() - tic)
        return res


    @torch.no_grad()
    def process_device_batch(self, frames: dict, quality: int = 95, subsampling: str = "4:2:0", entropy: str = "host", out_hw=None,
                             seg_png: bool = False, seg_palette: Optional[dict] = None, seg_huffman: str = "fixed",
                             lane_seg_filter=None) -> Dict[str, object]:
        """process_device for the B frames of a packed batch that all have one size (a video's): one preprocess_bgr and one forward over
        the batch, the lane and box decodes of the batch read back at ONE point (the drawing primitives are built from them on the host),
        one draw_packed per drawing stage, one seg overlay, an optional resize_bgr of the annotated frames to out_hw = (height, width),
        one encode_batch.  "jpeg", "lanes" and "detections" hold one entry per frame -- for every frame what process_device gives for
        that frame alone, as long as the forward's arithmetic for an image does not depend on the batch it runs in --
        and "visual" the annotated (and resized) frames in the packed device layout.  Like process_device it paints into `frames`.
        seg_png: "seg_png" holds one PNG file per frame, the arg-max class maps at the frames' ORIGINAL size (out_hw does not apply),
        encoded for the whole batch in one png_encode.encode_batch (seg_huffman: its huffman).  lane_seg_filter: see __init__ -- the
        filter's launches follow the lane decode's and its results come back at the same one point; "lanes" holds every frame's
        survivors, "lane_filter" every frame's statistics."""
        from . import jpeg_encode, png_encode
        if seg_png:
            self._need_seg()
        flt = self._lane_filter(lane_seg_filter, self.lane_seg_filter)
        from .postprocess import postprocess, postprocess_device
        from .preprocess import preprocess_bgr, resize_bgr
        from .visual import seg_decode_device
        net = self.net
        shapes = np.asarray(frames["shapes"], dtype=np.int64).reshape(-1, 2)
        offsets = np.asarray(frames["offsets"], dtype=np.int64).reshape(-1)
        B = len(shapes)
        assert B > 0 and bool((shapes == shapes[0]).all()), "the frames of a batch have one size"
        org_h, org_w = (int(v) for v in shapes[0])
        org_size = (org_w, org_h)
        nbytes = org_h * org_w * 3
        tic = time.time()
        if not np.array_equal(offsets, offsets[0] + nbytes * np.arange(B)):               # not back to back: make them so
            data = torch.cat([frames["data"][int(o):int(o) + nbytes] for o in offsets])
            offsets = nbytes * np.arange(B, dtype=np.int64)
            frames = {"data": data, "offsets": offsets, "shapes": shapes}
        off = int(offsets[0])
        batch = frames["data"][off:off + B * nbytes].view(B, org_h, org_w, 3)
        img = preprocess_bgr(batch, (self.net_h, self.net_w), device=self.device)
        outputs = net(img)
        res: Dict[str, object] = {"org_size": org_size}
        # the two decodes first, launched back to back and read back together: the one point where the host waits for the device
        if self.train_detect:
            det = outputs["detection"]
            det_args = ((img.shape[2], img.shape[3]), det["anchors"], det["regression"], det["classification"], self.det_conf, self.det_iou)
            launched = postprocess_device(*det_args, nms=self.det_nms)
        if self.train_lane:
            cls_preds, loc_preds = outputs["lane"]["predict_cls"], outputs["lane"]["predict_loc"]
            if flt is None:
                nms_sets = net.laneheader.decode_batch(cls_preds, loc_preds, self.lane_coder, self.lane_conf, self.lane_nms, False)
            else:
                mask = self._seg_mask(outputs["seg"])
                nms_sets, res["lane_filter"] = net.laneheader.decode_batch(cls_preds, loc_preds, self.lane_coder, self.lane_conf, self.lane_nms,
                                                                           False, seg_mask=mask, seg_filter=flt, return_stats=True)
            res["lanes"] = [net.laneheader.scale_to_org(s, self.net_w, self.net_h, org_w, org_h)["Lines"] for s in nms_sets]
        if self.train_detect:
            res["detections"] = postprocess(*det_args, nms=self.det_nms, launched=launched)
        # the drawing, in the reference's order: lanes, seg overlay, boxes
        if self.train_lane:
            frames = net.laneheader.visual(frames, res["lanes"], org_w, filter_vertical=True)
        if self.train_seg:
            seg = mask if flt is not None else self._seg_mask(outputs["seg"]) if seg_png else outputs["seg"]
            blended = seg_decode_device(batch, seg, self.colors)
            frames = {"data": blended.view(-1), "offsets": nbytes * np.arange(B, dtype=np.int64), "shapes": shapes.copy()}
            if seg_png:
                res["seg_png"] = png_encode.encode_batch(seg, out_sizes=(org_h, org_w), palette=seg_palette, device=self.device,
                                                           huffman=seg_huffman)
        if self.train_detect:
            frames = net.detectheader.display(res["detections"], frames, self.obj_list, org_size, (self.net_w, self.net_h))
        if out_hw is not None and (int(out_hw[0]), int(out_hw[1])) != (org_h, org_w):
            frames = resize_bgr(frames, out_hw)
        res["jpeg"] = jpeg_encode.encode_batch(frames, quality, subsampling, entropy)
        res["visual"] = frames
        res["ms"] = 1000.0 * (time.time() - tic)
        return res


def list_images(folder: str) -> List[str]:
    """the *.jpg / *.jpeg files of the folder, sorted by name"""
    return [os.path.join(folder, f) for f in sorted(os.listdir(folder)) if f.lower().endswith((".jpg", ".jpeg"))]


def run_images(demo: "Demo", folder: str, out_dir: str, quality: int = 95, subsampling: str = "4:2:0", entropy: str = "host",
               decode_entropy: str = "host", seg_dir: Optional[str] = None, seg_palette: Optional[dict] = None,
               seg_huffman: str = "fixed") -> List[dict]:
    """--images: folder of JPEGs -> annotated JPEGs of the same names in out_dir, plus results.json.  entropy / decode_entropy: where the
    Huffman stage of the encode / of the decode runs; the bytes written are the same.  seg_dir: every frame's class map goes there as
    <image stem>.png (Demo.process_device's seg_png)."""
    import json
    from . import jpeg
    if seg_dir is not None:
        demo._need_seg()
        os.makedirs(seg_dir, exist_ok=True)
    os.makedirs(out_dir, exist_ok=True)
    summary = []
    for t, path in enumerate(list_images(folder)):
        r = demo.process_device(jpeg.imread_bgr_device(path, device=demo.device, entropy=decode_entropy), quality, subsampling, entropy,
                                seg_png=seg_dir is not None, seg_palette=seg_palette, seg_huffman=seg_huffman)
        with open(os.path.join(out_dir, os.path.basename(path)), "wb") as f:
            f.write(r["jpeg"])
        if seg_dir is not None:
            with open(os.path.join(seg_dir, os.path.splitext(os.path.basename(path))[0] + ".png"), "wb") as f:
                f.write(r["seg_png"])
        nd = sum(len(d["rois"]) for d in r.get("detections", []) or [])
        nl = sum(len(l) for l in r.get("lanes", []))
        print("frame %d (%s): total process time is %i ms, %d lanes, %d boxes" % (t, os.path.basename(path), r["ms"], nl, nd))
        summary.append({"frame": t, "file": os.path.basename(path), "ms": r["ms"], "lanes": nl, "boxes": nd})
        if "lane_filter" in r:
            summary[-1]["lane_filter"] = r["lane_filter"][0]
    json.dump(summary, open(os.path.join(out_dir, "results.json"), "w"), indent=1)
    return summary


def parse_size(text: str):
    """"1920x1080" -> (1920, 1080)"""
    w, _, h = text.lower().partition("x")
    if not (w.isdigit() and h.isdigit() and int(w) > 0 and int(h) > 0):
        raise argparse.ArgumentTypeError("a frame size is WIDTHxHEIGHT, e.g. 1920x1080, not %r" % text)
    return int(w), int(h)


def run_video(demo: "Demo", src: str, dst: str, batch: int = 8, quality: int = 95, subsampling: str = "4:2:0", entropy: str = "host",
              decode_entropy: str = "host", size=None, max_frames: Optional[int] = None, seg_dir: Optional[str] = None,
              seg_palette: Optional[dict] = None, seg_huffman: str = "fixed") -> List[dict]:
    """--video: a Motion-JPEG AVI -> the annotated Motion-JPEG AVI `dst` of the input's frame rate, plus dst + ".results.json".  The frames
    are taken in file order in groups of `batch` (the last group is smaller), decoded (jpeg.imread_bgr_device), annotated
    (Demo.process_device_batch) and appended to an avi.AviWriter; size = (width, height) of the output frames, the input's without.  A
    zero-length chunk -- "repeat the previous frame" -- writes the previous annotated JPEG again (a leading one is skipped).  The bytes
    of the next group are read and completed (avi.frame_bytes) while the device works on the current one.  seg_dir: the class map of
    every output frame goes there as frame_%06d.png, at the INPUT's frame size (a repeated frame writes its map again)."""
    import json
    import mmap
    from . import avi, jpeg
    assert batch >= 1, batch
    if seg_dir is not None:
        demo._need_seg()
        os.makedirs(seg_dir, exist_ok=True)
    summary: List[dict] = []
    with open(src, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as data:
        index = avi.read_index(data)
        if index["truncated"]:
            print("%s is cut short: %d complete frames" % (src, len(index["frames"])))
        in_w, in_h = index["width"], index["height"]
        out_w, out_h = (int(size[0]), int(size[1])) if size else (in_w, in_h)
        # which coded frame every output frame shows: a repeat chunk shows the one before it
        plan, coded = [], []
        for i, (_, nbytes) in enumerate(index["frames"]):
            if max_frames is not None and len(plan) >= max_frames:
                break
            if nbytes:
                coded.append(i)
            if coded:
                plan.append(len(coded) - 1)
        groups = [coded[a:a + batch] for a in range(0, len(coded), batch)]
        read = lambda g: [avi.frame_bytes(index, data, i) for i in groups[g]] if g < len(groups) else None
        fps = (index["rate"], index["scale"]) if index["rate"] > 0 and index["scale"] > 0 else (10, 1)
        with avi.AviWriter(dst, out_w, out_h, fps) as out:
            nxt, done, p = read(0), 0, 0
            for g in range(len(groups)):
                frames = jpeg.imread_bgr_device(nxt, device=demo.device, entropy=decode_entropy)
                got = [tuple(int(v) for v in s) for s in frames["shapes"]]
                if got != [(in_h, in_w)] * len(got):
                    raise ValueError("%s: frames of %s in a stream whose header says %dx%d" % (src, sorted(set(got)), in_w, in_h))
                nxt = read(g + 1)                                        # the device is decoding: the host's share of the next group
                r = demo.process_device_batch(frames, quality, subsampling, entropy, out_hw=(out_h, out_w), seg_png=seg_dir is not None,
                                              seg_palette=seg_palette, seg_huffman=seg_huffman)
                B = len(groups[g])
                while p < len(plan) and plan[p] < done + B:
                    k = plan[p] - done
                    out.write(r["jpeg"][k])
                    if seg_dir is not None:
                        with open(os.path.join(seg_dir, "frame_%06d.png" % p), "wb") as f:
                            f.write(r["seg_png"][k])
                    nd = len(r["detections"][k]["rois"]) if "detections" in r else 0
                    nl = len(r["lanes"][k]) if "lanes" in r else 0
                    summary.append({"frame": p, "file": os.path.basename(src), "ms": r["ms"] / B, "lanes": nl, "boxes": nd})
                    if "lane_filter" in r:
                        summary[-1]["lane_filter"] = r["lane_filter"][k]
                    p += 1
                done += B
                print("frames %d-%d: total process time is %i ms" % (done - B, done - 1, r["ms"]))
    json.dump(summary, open(dst + ".results.json", "w"), indent=1)
    return summary


def synthetic_frames(n: int, h: int = 1080, w: int = 1920, seed: int = 0) -> np.ndarray:
    """road-like BGR frames: sky / ground gradient, two lane-ish bright bands, a few boxes, noise"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        base = np.where(yy < h * 0.45, 150 + 60 * yy / h, 70 + 40 * yy / h)
        img = np.stack([base * 1.05, base, base * 0.9], -1)
        for off in (-0.18 + 0.02 * i, 0.2 - 0.01 * i):
            cx = w * (0.5 + off * (yy - h * 0.45) / (h * 0.55))
            img[(np.abs(xx - cx) < 6 + 10 * yy / h) & (yy > h * 0.45)] = 235
        for _ in range(4):
            x0, y0 = rs.randint(0, w - 200), rs.randint(int(h * 0.4), h - 150)
            img[y0:y0 + rs.randint(40, 140), x0:x0 + rs.randint(60, 200)] = rs.randint(20, 230, size=3)
        out[i] = np.clip(img + rs.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    return out


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cfg", default=os.path.join(root, "cfgs", "hydranet_big.yml"))
    ap.add_argument("--weights", default=None, help="checkpoint written by train.py (module.-prefixed keys are accepted); random init without")
    ap.add_argument("--frames", default=None, help=".npy uint8 [T, H, W, 3] BGR frames; synthetic 1080p frames without")
    ap.add_argument("--images", default=None, help="folder of *.jpg / *.jpeg frames: each is annotated and written as a JPEG of the same name into --out")
    ap.add_argument("--video", default=None, help="Motion-JPEG AVI: every frame is annotated and written to the AVI --out (and --out.results.json)")
    ap.add_argument("--batch", type=int, default=8, help="frames per launch sequence (--video)")
    ap.add_argument("--size", type=parse_size, default=None, help="WIDTHxHEIGHT of the output video's frames (--video); the input's without")
    ap.add_argument("--max-frames", type=int, default=None, help="stop after this many frames (--video)")
    ap.add_argument("--quality", type=int, default=95, help="JPEG quality of the annotated frames (--images, --video)")
    ap.add_argument("--entropy", choices=("host", "device"), default="host", help="where the Huffman stage of the JPEG encode runs (--images, --video)")
    ap.add_argument("--decode-entropy", choices=("host", "device"), default="host", help="where the Huffman stage of the JPEG decode runs (--images, --video)")
    ap.add_argument("--save-seg", default=None, metavar="DIR", help="also write every frame's predicted class map as an 8-bit label PNG into DIR "
                    "(--images: <image stem>.png; --video: frame_%%06d.png); needs a configuration with the seg head")
    ap.add_argument("--seg-palette", action="store_true", help="write the class maps of --save-seg as palette PNGs with the demo's colours")
    ap.add_argument("--seg-huffman", choices=("fixed", "dynamic"), default=None, help="the deflate code of the --save-seg PNGs: fixed (the default), "
                    "or dynamic -- a Huffman code per block of 16 chunks, the same pixels in less than half the bytes")
    ap.add_argument("--lane-seg-filter", action="store_true", help="the deploy path's lane filter: at most --lane-top-k lanes, each kept when "
                    "more than --lane-seg-ratio of its painted pixels lie on the seg head's marking class; results.json gains the statistics")
    ap.add_argument("--lane-top-k", type=int, default=None, help="lanes kept after the NMS at most (--lane-seg-filter; 14)")
    ap.add_argument("--lane-seg-ratio", type=float, default=None, help="the overlap a lane needs, exclusive (--lane-seg-filter; 0.01)")
    ap.add_argument("--lane-seg-width", type=int, default=None, help="thickness the lanes are painted with, pixels (--lane-seg-filter; 20)")
    ap.add_argument("--lane-seg-class", type=int, default=None, help="the seg class id that counts as marking (--lane-seg-filter; 2)")
    ap.add_argument("--nms", choices=("hard", "diou", "soft_linear", "soft_gaussian"), default=None, help="the suppression rule of the box decode "
                    "(postprocess.NmsOptions); without any --nms* / --max-det flag: the cfg's detection.nms_* keys, else the reference's hard NMS")
    ap.add_argument("--nms-sigma", type=float, default=None, help="sigma of --nms soft_gaussian (0.5)")
    ap.add_argument("--max-det", type=int, default=None, help="boxes drawn per frame at most (0: no limit)")
    ap.add_argument("--nms-class-agnostic", action="store_true", help="boxes of different classes suppress each other")
    ap.add_argument("--count", type=int, default=4)
    ap.add_argument("--out", default=None, help="directory for the annotated JPEGs (--images) or frame_%%04d.npy (blended frames), and results.json; "
                    "the annotated AVI (--video)")
    args = ap.parse_args(argv)
    if args.video and not args.out:
        ap.error("--video needs --out")
    if args.save_seg and not (args.images or args.video):
        ap.error("--save-seg needs --images or --video")
    if args.seg_huffman and not args.save_seg:
        ap.error("--seg-huffman needs --save-seg")
    huffman = args.seg_huffman or "fixed"
    lane_opts = {"top_k": args.lane_top_k, "min_ratio": args.lane_seg_ratio, "line_width": args.lane_seg_width, "lane_class": args.lane_seg_class}
    lane_opts = {k: v for k, v in lane_opts.items() if v is not None}
    if lane_opts and not args.lane_seg_filter:
        ap.error("--lane-top-k / --lane-seg-ratio / --lane-seg-width / --lane-seg-class need --lane-seg-filter")
    lane_filter = None
    if args.lane_seg_filter:
        from .lane_codec import LaneSegFilter
        lane_filter = LaneSegFilter(**lane_opts)
    cfgs = yaml.safe_load(open(args.cfg))
    if args.save_seg and not cfgs["train"]["train_seg"]:
        raise ValueError("--save-seg: %s runs no seg head (train.train_seg is off)" % args.cfg)
    torch.manual_seed(0)
    det_nms = None
    if args.nms is not None or args.nms_sigma is not None or args.max_det is not None or args.nms_class_agnostic:
        from .postprocess import NmsOptions
        det_nms = NmsOptions(kind=args.nms or "hard", sigma=0.5 if args.nms_sigma is None else args.nms_sigma, max_det=args.max_det or 0,
                             class_agnostic=args.nms_class_agnostic)
    demo = Demo(cfgs, args.weights, lane_seg_filter=lane_filter, det_nms=det_nms)
    if not args.weights:
        # random initialisation: every anchor scores ~0.5, far more candidates than any real frame has (the device NMS holds 32 768)
        print("no --weights: random initialisation, detection threshold raised to 0.95 for this run")
        demo.det_conf = 0.95
    palette = seg_palette(demo.colors) if args.seg_palette else None
    if args.images:
        if not args.out:
            ap.error("--images needs --out")
        return run_images(demo, args.images, args.out, args.quality, entropy=args.entropy, decode_entropy=args.decode_entropy,
                          seg_dir=args.save_seg, seg_palette=palette, seg_huffman=huffman)
    if args.video:
        return run_video(demo, args.video, args.out, args.batch, args.quality, entropy=args.entropy, decode_entropy=args.decode_entropy, size=args.size,
                         max_frames=args.max_frames, seg_dir=args.save_seg, seg_palette=palette, seg_huffman=huffman)
    frames = np.load(args.frames) if args.frames else synthetic_frames(args.count)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    summary = []
    for t, frame in enumerate(frames):
        r = demo.process(frame)
        nd = sum(len(d["rois"]) for d in r.get("detections", []) or [])
        nl = sum(len(l) for l in r.get("lanes", []))
        print("frame %d: total process time is %i ms, %d lanes, %d boxes" % (t, r["ms"], nl, nd))
        summary.append({"frame": t, "ms": r["ms"], "lanes": nl, "boxes": nd})
        if "lane_filter" in r:
            summary[-1]["lane_filter"] = r["lane_filter"][0]
        if args.out:
            np.save(os.path.join(args.out, "frame_%04d.npy" % t), r["visual"])
    if args.out:
        import json
        json.dump(summary, open(os.path.join(args.out, "results.json"), "w"), indent=1)
    return summary


if __name__ == "__main__":
    main()
