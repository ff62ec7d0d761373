"""CPU suite: how HipTileEncoder.set_image_u8 / set_batch_u8 read 8-bit interleaved pixels (yaik_amd.encoder.u8_pixel_layout): shape,
channels, row pitch and frame stride from the array's strides, so padded or row-sliced numpy views go to the library without a copy."""
import numpy as np
import pytest

from yaik_amd.encoder import PixelLayout, u8_pixel_layout


def _view(buf, shape, strides, offset=0):
    return np.ndarray(shape, np.uint8, buf, offset, strides)


def test_tight_rows():
    img = np.zeros((40, 72, 4), np.uint8)
    assert u8_pixel_layout(img) == PixelLayout(frames=1, rows=40, w=72, channels=4, n_planes=4, row_bytes=288, frame_bytes=40 * 288)
    rgb = np.zeros((40, 72, 3), np.uint8)
    assert u8_pixel_layout(rgb) == PixelLayout(1, 40, 72, 3, 3, 216, 40 * 216)


def test_rgba_into_three_planes():
    lay = u8_pixel_layout(np.zeros((16, 8, 4), np.uint8), n_planes=3)
    assert (lay.channels, lay.n_planes, lay.row_bytes) == (4, 3, 32)


def test_padded_rows_and_unaligned_base():
    buf = np.zeros(1 + 40 * 229, np.uint8)
    v = _view(buf, (40, 72, 3), (229, 3, 1), offset=1)
    lay = u8_pixel_layout(v)
    assert (lay.rows, lay.w, lay.row_bytes) == (40, 72, 229)
    assert v.ctypes.data == buf.ctypes.data + 1                  # what set_image_u8 hands over: the view's first byte


def test_row_sliced_views():
    img = np.zeros((64, 72, 4), np.uint8)
    lay = u8_pixel_layout(img[8:24])
    assert (lay.rows, lay.row_bytes, lay.frame_bytes) == (16, 288, 16 * 288)
    lay = u8_pixel_layout(img[::2])                             # every other row: a pitch of two rows
    assert (lay.rows, lay.row_bytes) == (32, 576)


def test_batch_of_frames():
    frames = np.zeros((4, 16, 8, 4), np.uint8)
    assert u8_pixel_layout(frames, batch=True) == PixelLayout(4, 16, 8, 4, 4, 32, 16 * 32)
    buf = np.zeros(4 * 1024, np.uint8)
    v = _view(buf, (4, 16, 8, 3), (1024, 48, 3, 1))             # padded rows and padded frames
    lay = u8_pixel_layout(v, batch=True)
    assert (lay.frames, lay.row_bytes, lay.frame_bytes) == (4, 48, 1024)


def test_wrong_dtype():
    for dt in (np.int32, np.uint16, np.float32, np.int8):
        with pytest.raises(TypeError):
            u8_pixel_layout(np.zeros((16, 8, 4), dt))


def test_wrong_channel_count():
    for c in (1, 2, 5):
        with pytest.raises(ValueError):
            u8_pixel_layout(np.zeros((16, 8, c), np.uint8))
    with pytest.raises(ValueError):                             # 3 channels cannot fill 4 planes
        u8_pixel_layout(np.zeros((16, 8, 3), np.uint8), n_planes=4)
    with pytest.raises(ValueError):
        u8_pixel_layout(np.zeros((16, 8, 4), np.uint8), n_planes=2)


def test_wrong_rank():
    with pytest.raises(ValueError):
        u8_pixel_layout(np.zeros((16, 32), np.uint8))
    with pytest.raises(ValueError):
        u8_pixel_layout(np.zeros((16, 8, 4), np.uint8), batch=True)
    with pytest.raises(ValueError):
        u8_pixel_layout(np.zeros((2, 16, 8, 4), np.uint8))


def test_non_unit_pixel_or_channel_stride():
    img = np.zeros((16, 16, 4), np.uint8)
    with pytest.raises(ValueError):
        u8_pixel_layout(img[:, ::2])                            # every other pixel: pixel stride 8 bytes
    with pytest.raises(ValueError):
        u8_pixel_layout(img[..., ::-1])                         # channels reversed: channel stride -1
    with pytest.raises(ValueError):
        u8_pixel_layout(np.zeros((4, 16, 16), np.uint8).transpose(1, 2, 0))     # planar memory seen as [rows, w, C]


def test_overlapping_rows_or_frames():
    buf = np.zeros(4096, np.uint8)
    with pytest.raises(ValueError):
        u8_pixel_layout(_view(buf, (16, 8, 4), (16, 4, 1)))   # a row pitch shorter than a row
    with pytest.raises(ValueError):
        u8_pixel_layout(_view(buf, (2, 16, 8, 4), (256, 32, 4, 1)), batch=True)  # a frame stride shorter than a frame
