"""The 8-bit bilinear resize (OpenCV's INTER_LINEAR on uint8 images: 11-bit fixed-point coefficients, its rounding) as the tests state it.
There is ONE statement: the oracle's resize_bilinear_u8, which tests/test_post_gpu.py already holds hn_preprocess_bgr and hn_seg_overlay
to; hn_resize_bgr8 (tests/test_resize_bgr_gpu.py) is held to the same function, so the kernels that share the device code also share
their reference."""
import numpy as np

from oracle.hydranet_oracle import preprocess_bgr, resize_bilinear_u8


def resize_bgr(frame: np.ndarray, out_hw) -> np.ndarray:
    """cv2.resize(frame, (out_w, out_h)) of a uint8 H x W x 3 frame; a frame of that size already is returned as a copy"""
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    return resize_bilinear_u8(frame, (int(out_hw[0]), int(out_hw[1])))


__all__ = ["resize_bgr", "preprocess_bgr"]
