"""GPU: preprocess.resize_bgr (hn_resize_bgr8) == the numpy statement of the fixed-point resize (tests/resize_ref.py), exactly: up- and
down-scaling, odd sizes and edge clamping, the copy of a frame that has the output size, a ragged pack in one launch, both store paths
(output rows of whole dwords and not), and preprocess_bgr(resize_bgr(x)) == preprocess_bgr(x), the two kernels sharing one resize."""
import numpy as np
import pytest
import torch

from tests import resize_ref as R

pytestmark = pytest.mark.gpu


def rand_frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def unpack(pk):
    data = pk["data"].cpu().numpy()
    return [data[int(o):int(o) + int(h) * int(w) * 3].reshape(int(h), int(w), 3) for o, (h, w) in zip(pk["offsets"], pk["shapes"])]


@pytest.mark.parametrize("src_hw,dst_hw", [((37, 53), (48, 64)), ((660, 1570), (1080, 1920)), ((1080, 1920), (360, 640)), ((64, 64), (64, 64)),
                                           ((37, 53), (45, 50)), ((5, 3), (1, 1)), ((1, 1), (7, 9))],
                         ids=["up_odd", "to_1080p", "integer_factor", "copy", "byte_stores_tail_quad", "to_one_pixel", "from_one_pixel"])
def test_resize_equals_the_fixed_point_statement(src_hw, dst_hw):
    from multitask_hydranet_amd.augment import pack
    from multitask_hydranet_amd.preprocess import resize_bgr
    frame = rand_frame(*src_hw, seed=src_hw[0] * 7 + dst_hw[1])
    pk = pack([frame])
    got = resize_bgr({"data": pk["data"].cuda(), "offsets": pk["offsets"], "shapes": pk["shapes"]}, dst_hw)
    assert got["data"].is_cuda and got["data"].dtype == torch.uint8 and got["shapes"].tolist() == [list(dst_hw)] and got["offsets"].tolist() == [0]
    want = R.resize_bgr(frame, dst_hw)
    out = unpack(got)[0]
    bad = np.argwhere(out != want)
    assert bad.size == 0, "%d of %d values differ, the first at (y, x, c) = %s: %d, not %d" % (len(bad), want.size, bad[0], out[tuple(bad[0])], want[tuple(bad[0])])
    if src_hw == dst_hw:
        assert np.array_equal(out, frame)


@pytest.mark.parametrize("dst_hw", [(45, 50), (48, 64), (90, 31)], ids=["byte_stores", "dword_stores", "one_is_a_copy"])
def test_ragged_pack_in_one_launch(dst_hw):
    from multitask_hydranet_amd.augment import pack
    from multitask_hydranet_amd.preprocess import resize_bgr
    frames = [rand_frame(37, 53, 1), rand_frame(90, 31, 2)]
    pk = pack(frames)
    assert pk["shapes"].tolist() == [[37, 53], [90, 31]]
    got = resize_bgr({"data": pk["data"].cuda(), "offsets": pk["offsets"], "shapes": pk["shapes"]}, dst_hw)
    n = dst_hw[0] * dst_hw[1] * 3
    assert got["offsets"].tolist() == [0, n] and got["shapes"].tolist() == [list(dst_hw)] * 2 and got["data"].numel() == 2 * n
    for out, frame in zip(unpack(got), frames):
        assert np.array_equal(out, R.resize_bgr(frame, dst_hw))


def test_tensor_batch_and_a_misaligned_source():
    """[N, H, W, 3] tensor input; and frames that start at odd byte offsets of the pack (the kernel reads bytes, so any offset is fine)"""
    from multitask_hydranet_amd.preprocess import resize_bgr
    frames = np.stack([rand_frame(33, 47, s) for s in (3, 4, 5)])
    got = resize_bgr(torch.from_numpy(frames).cuda(), (20, 28))
    for out, frame in zip(unpack(got), frames):
        assert np.array_equal(out, R.resize_bgr(frame, (20, 28)))
    flat = torch.cat([torch.zeros(5, dtype=torch.uint8), torch.from_numpy(frames).reshape(-1)]).cuda()
    offs = 5 + np.arange(3, dtype=np.int64) * frames[0].size
    got = resize_bgr({"data": flat, "offsets": offs, "shapes": np.array([[33, 47]] * 3)}, (20, 28))
    for out, frame in zip(unpack(got), frames):
        assert np.array_equal(out, R.resize_bgr(frame, (20, 28)))
    with pytest.raises(AssertionError):                                  # a frame that does not fit the buffer is refused on the host
        resize_bgr({"data": flat, "offsets": offs + 1, "shapes": np.array([[33, 47]] * 3)}, (20, 28))


@pytest.mark.parametrize("net_hw", [(128, 128), (384, 640)])
def test_preprocess_after_resize_is_preprocess(net_hw):
    """both kernels run one resize: resizing to the network size first and pre-processing without a resize == pre-processing with it"""
    from multitask_hydranet_amd.preprocess import preprocess_bgr, resize_bgr
    x = torch.from_numpy(np.stack([rand_frame(660, 1570, 11), rand_frame(660, 1570, 12)])).cuda()
    small = resize_bgr(x, net_hw)["data"].view(2, net_hw[0], net_hw[1], 3)
    a, b = preprocess_bgr(small, net_hw), preprocess_bgr(x, net_hw)
    assert torch.equal(a, b)
    assert np.array_equal(b[0].cpu().numpy(), R.preprocess_bgr(x[0].cpu().numpy(), net_hw))
