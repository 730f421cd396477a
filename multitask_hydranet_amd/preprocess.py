"""Input pre-processing on the device (reference: demo.py:26-50,186-196 and dataset/utility.py:213-227): BGR uint8 frame(s) -> RGB ->
bilinear resize to the network input -> /255 -> ImageNet mean / std -> fp32 NCHW, one kernel launch (hn_preprocess_bgr).
cv2 is a third-party dependency of the reference that is absent here: its 8-bit INTER_LINEAR resize is restated from OpenCV's published
fixed-point algorithm (11-bit coefficients); frames that already have the network size take no resize and are bit-exact against the
reference's numpy arithmetic (evaluated in float64, then cast to float32, exactly as demo.py does)."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import lib


def preprocess_bgr(frames, out_hw, device=None) -> torch.Tensor:
    """frames: uint8 [H, W, 3] or [N, H, W, 3] (numpy array or torch tensor, BGR as cv2.imread delivers) -> fp32 [N, 3, out_h, out_w]"""
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dim() == 3:
        frames = frames[None]
    assert frames.dtype == torch.uint8 and frames.shape[-1] == 3, (frames.dtype, frames.shape)
    dev = torch.device(device) if device is not None else (frames.device if frames.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    src = frames.to(dev).contiguous()
    n, hs, ws, _ = src.shape
    hd, wd = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((n, 3, hd, wd), device=dev, dtype=torch.float32)
    lib().call("hn_preprocess_bgr", src.data_ptr(), n, hs, ws, out.data_ptr(), hd, wd)
    return out


RESIZE_SRC_DTYPE = np.dtype({"names": ["off", "H", "W"], "formats": ["<i8", "<i4", "<i4"], "offsets": [0, 8, 12], "itemsize": 16})    # hn_post.hip struct ResizeSrc


def resize_bgr(frames, out_hw) -> dict:
    """cv2.resize(frame, (out_w, out_h)) -- 8-bit INTER_LINEAR, the arithmetic of preprocess_bgr up to the 8-bit value -- for a batch in
    one launch (hn_resize_bgr8).  frames: the packed device layout of jpeg.imread_bgr_device ({"data", "offsets", "shapes"}, ragged) or a
    uint8 device tensor [N, H, W, 3]; -> packed frames of the one size out_hw = (out_h, out_w).  A frame of that size is copied."""
    hd, wd = int(out_hw[0]), int(out_hw[1])
    if isinstance(frames, dict):
        data = frames["data"]
        shapes = np.asarray(frames["shapes"], dtype=np.int64).reshape(-1, 2)
        offsets = np.asarray(frames["offsets"], dtype=np.int64).reshape(-1)
    else:
        assert torch.is_tensor(frames) and frames.dim() == 4 and frames.shape[3] == 3, "a packed dict or a [N, H, W, 3] tensor"
        data = frames.contiguous().view(-1)
        n, h, w, _ = frames.shape
        shapes = np.tile(np.array([[h, w]], np.int64), (n, 1))
        offsets = np.arange(n, dtype=np.int64) * (h * w * 3)
    n = len(shapes)
    assert data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous() and len(offsets) == n
    assert 0 < n <= 65535 and 0 < hd <= 65535 and 0 < wd, (n, hd, wd)
    desc = np.zeros(n, dtype=RESIZE_SRC_DTYPE)
    for i, e in enumerate(desc):
        h, w = int(shapes[i, 0]), int(shapes[i, 1])
        assert h > 0 and w > 0 and 0 <= offsets[i] and offsets[i] + h * w * 3 <= data.numel(), (i, h, w, int(offsets[i]))
        e["off"], e["H"], e["W"] = int(offsets[i]), h, w
    with torch.cuda.device(data.device):
        out = torch.empty((n * hd * wd * 3,), device=data.device, dtype=torch.uint8)
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(data.device)
        lib().call("hn_resize_bgr8", data.data_ptr(), int(data.numel()), desc_d.data_ptr(), n, out.data_ptr(), hd, wd)
    return {"data": out, "offsets": np.arange(n, dtype=np.int64) * (hd * wd * 3), "shapes": np.tile(np.array([[hd, wd]], np.int64), (n, 1))}
