"""The destination layouts of HipTileDecoder.image_batch_device, derived from an array's strides without a GPU: u8_pixel_layout(batch=True)
for [F, rows, w, C] and u8_planar_batch_layout for [F, C, rows, w], on numpy and CPU torch arrays: shapes, pitches and rejections."""
import numpy as np
import pytest

from yaik_amd.encoder import u8_pixel_layout, u8_planar_batch_layout


def _torch():
    return pytest.importorskip("torch")


def _fields(lay):
    return (lay.frames, lay.channels, lay.rows, lay.w, lay.row_bytes, lay.plane_bytes, lay.frame_bytes)


def test_planar_batch_tight_numpy():
    assert _fields(u8_planar_batch_layout(np.zeros((5, 3, 40, 24), np.uint8))) == (5, 3, 40, 24, 24, 960, 2880)
    assert _fields(u8_planar_batch_layout(np.zeros((2, 4, 8, 16), np.uint8))) == (2, 4, 8, 16, 16, 128, 512)


def test_planar_batch_padded_rows_planes_and_frames_numpy():
    buf = np.zeros(3 * 5000 + 3, np.uint8)
    view = np.ndarray((3, 4, 16, 40), np.uint8, buf, 3, (5000, 1000, 48, 1))             # base offset 3: not 16-byte aligned
    assert _fields(u8_planar_batch_layout(view)) == (3, 4, 16, 40, 48, 1000, 5000)


def test_planar_batch_torch_window_of_a_larger_batch():
    torch = _torch()
    big = torch.zeros((6, 4, 20, 70), dtype=torch.uint8)
    assert _fields(u8_planar_batch_layout(big[1:4, :, 2:18, 3:67])) == (3, 4, 16, 64, 70, 1400, 5600)
    assert _fields(u8_planar_batch_layout(big[::2, :3])) == (3, 3, 20, 70, 70, 1400, 11200)  # every other frame, the first three planes


def test_single_frame_ignores_the_frame_stride():
    buf = np.zeros(4096, np.uint8)
    view = np.ndarray((1, 3, 8, 16), np.uint8, buf, 0, (7, 128, 16, 1))                  # the stride of a dimension of one element means nothing
    assert _fields(u8_planar_batch_layout(view)) == (1, 3, 8, 16, 16, 128, 384)


def test_hwc_batch_destination():
    torch = _torch()
    frames = torch.zeros((8, 16, 24, 4), dtype=torch.uint8)
    lay = u8_pixel_layout(frames, batch=True)
    assert (lay.frames, lay.rows, lay.w, lay.channels, lay.row_bytes, lay.frame_bytes) == (8, 16, 24, 4, 96, 1536)
    lay = u8_pixel_layout(torch.zeros((8, 20, 40, 3), dtype=torch.uint8)[2:5, 1:17, :24], batch=True)
    assert (lay.frames, lay.rows, lay.w, lay.channels, lay.row_bytes, lay.frame_bytes) == (3, 16, 24, 3, 120, 2400)


def test_planar_batch_refusals():
    torch = _torch()
    with pytest.raises(TypeError):
        u8_planar_batch_layout(np.zeros((2, 3, 8, 8), np.int32))
    with pytest.raises(TypeError):
        u8_planar_batch_layout(torch.zeros((2, 3, 8, 8), dtype=torch.float32))
    with pytest.raises(ValueError):
        u8_planar_batch_layout(np.zeros((3, 8, 8), np.uint8))                     # a single [C, rows, w] image
    with pytest.raises(ValueError):
        u8_planar_batch_layout(np.zeros((0, 3, 8, 8), np.uint8))                  # no frame
    with pytest.raises(ValueError):
        u8_planar_batch_layout(np.zeros((2, 2, 8, 8), np.uint8))                  # C = 2
    with pytest.raises(ValueError):
        u8_planar_batch_layout(np.zeros((2, 8, 8, 3), np.uint8).transpose(0, 3, 1, 2))   # NHWC memory seen as NCHW: pixel stride 3
    with pytest.raises(ValueError):
        u8_planar_batch_layout(np.zeros((2, 3, 8, 16), np.uint8)[..., ::2])       # pixel stride 2
    buf = np.zeros(1 << 16, np.uint8)
    with pytest.raises(ValueError):                                                # rows overlap
        u8_planar_batch_layout(np.ndarray((2, 3, 8, 16), np.uint8, buf, 0, (4096, 200, 8, 1)))
    with pytest.raises(ValueError):                                                # planes overlap
        u8_planar_batch_layout(np.ndarray((2, 3, 8, 16), np.uint8, buf, 0, (4096, 100, 16, 1)))
    with pytest.raises(ValueError):                                                # frames overlap
        u8_planar_batch_layout(np.ndarray((2, 3, 8, 16), np.uint8, buf, 0, (383, 128, 16, 1)))
    with pytest.raises(ValueError):                                                # one frame broadcast over the batch
        u8_planar_batch_layout(torch.zeros((1, 3, 8, 8), dtype=torch.uint8).expand(4, 3, 8, 8))


def test_hwc_batch_refusals():
    with pytest.raises(ValueError):
        u8_pixel_layout(np.zeros((8, 8, 3), np.uint8), batch=True)                # not [F, rows, w, C]
    buf = np.zeros(1 << 16, np.uint8)
    with pytest.raises(ValueError):                                                # frames overlap
        u8_pixel_layout(np.ndarray((2, 8, 16, 3), np.uint8, buf, 0, (383, 48, 3, 1)), batch=True)
