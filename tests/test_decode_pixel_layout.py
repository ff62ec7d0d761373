"""The destination layouts of HipTileDecoder.image_device, derived from an array's strides without a GPU: u8_pixel_layout for HWC
([rows, w, C], as the 8-bit encode input uses it) and u8_planar_layout for CHW ([C, rows, w]), on numpy and CPU torch arrays."""
import numpy as np
import pytest

from yaik_amd.encoder import u8_pixel_layout, u8_planar_layout


def _torch():
    return pytest.importorskip("torch")


def test_planar_tight_numpy():
    lay = u8_planar_layout(np.zeros((3, 40, 24), np.uint8))
    assert (lay.channels, lay.rows, lay.w, lay.row_bytes, lay.plane_bytes) == (3, 40, 24, 24, 960)


def test_planar_padded_rows_and_planes_numpy():
    buf = np.zeros(4 * 1000 + 3, np.uint8)
    view = np.ndarray((4, 16, 40), np.uint8, buf, 3, (1000, 48, 1))
    lay = u8_planar_layout(view)
    assert (lay.channels, lay.rows, lay.w, lay.row_bytes, lay.plane_bytes) == (4, 16, 40, 48, 1000)


def test_planar_torch_slices():
    torch = _torch()
    big = torch.zeros((2, 4, 20, 70), dtype=torch.uint8)
    lay = u8_planar_layout(big[1, :, 2:18, 3:67])                    # a frame of a batch, cropped rows and columns
    assert (lay.channels, lay.rows, lay.w, lay.row_bytes, lay.plane_bytes) == (4, 16, 64, 70, 1400)
    lay = u8_planar_layout(torch.zeros((16, 8, 3), dtype=torch.uint8).permute(2, 0, 1).contiguous())
    assert (lay.row_bytes, lay.plane_bytes) == (8, 128)


def test_hwc_destination_of_a_batch_frame():
    torch = _torch()
    frames = torch.zeros((8, 16, 24, 4), dtype=torch.uint8)
    lay = u8_pixel_layout(frames[5])
    assert (lay.rows, lay.w, lay.channels, lay.row_bytes) == (16, 24, 4, 96)
    padded = torch.zeros((16, 40, 3), dtype=torch.uint8)[:, :24]
    lay = u8_pixel_layout(padded)
    assert (lay.rows, lay.w, lay.channels, lay.row_bytes) == (16, 24, 3, 120)


def test_planar_refusals():
    torch = _torch()
    with pytest.raises(TypeError):
        u8_planar_layout(np.zeros((3, 8, 8), np.int32))
    with pytest.raises(TypeError):
        u8_planar_layout(torch.zeros((3, 8, 8), dtype=torch.float32))
    with pytest.raises(ValueError):
        u8_planar_layout(np.zeros((8, 8), np.uint8))                   # not [C, rows, w]
    with pytest.raises(ValueError):
        u8_planar_layout(np.zeros((2, 8, 8), np.uint8))                # C = 2
    with pytest.raises(ValueError):
        u8_planar_layout(np.zeros((5, 8, 8), np.uint8))
    with pytest.raises(ValueError):
        u8_planar_layout(np.zeros((8, 8, 3), np.uint8).transpose(2, 0, 1))     # HWC memory seen as CHW: pixel stride 3
    with pytest.raises(ValueError):
        u8_planar_layout(np.zeros((3, 8, 16), np.uint8)[:, :, ::2])            # pixel stride 2
    buf = np.zeros(4096, np.uint8)
    with pytest.raises(ValueError):                                                # rows overlap
        u8_planar_layout(np.ndarray((3, 8, 16), np.uint8, buf, 0, (200, 8, 1)))
    with pytest.raises(ValueError):                                                # planes overlap
        u8_planar_layout(np.ndarray((3, 8, 16), np.uint8, buf, 0, (100, 16, 1)))
    with pytest.raises(ValueError):
        u8_planar_layout(torch.zeros((3, 8, 8), dtype=torch.uint8).expand(3, 8, 8).as_strided((3, 8, 8), (0, 8, 1)))


def test_hwc_refusals_for_a_destination():
    with pytest.raises(ValueError):
        u8_pixel_layout(np.zeros((8, 8, 2), np.uint8))
    with pytest.raises(ValueError):
        u8_pixel_layout(np.zeros((3, 8, 8), np.uint8).transpose(1, 2, 0))     # CHW memory seen as HWC
