"""The gradient passes of the fused encode kernel with the deciding pixel at every column and row of a cell (tests/gradfit_columns_cases.py;
tests/test_gradfit_columns_cases.py shows from the reference alone that every case holds what it claims).

The kernel holds the pixels of the gradient phase in stream layout: channel 2 of two neighbouring columns shares a register and the Round6P
stream of channel 2 walks both at once, with a row step per column.  tests/test_gpu_gradfit_directed.py decides its tiles in columns 0 and 3 of
a cell; here every shape, path and kind has a tile decided at each of the sixteen pixels of its first and of its last cell, both signs, accepted
at rf and rejected at rf + 1 (all but the corner TL: kc.UNREALISED).  Bitmaps, counts, coverage, corner streams and range streams are compared
bit for bit with the CPU oracle, on kernel version 2 and once more as batches of three frames."""
import numpy as np
import pytest

from tests import gradfit_columns_cases as kc
from tests.test_gpu_gradfit_directed import _same_gradient, _same_range

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_v2():
    from tests.parity import encoder_for_kernel_version
    e = encoder_for_kernel_version(2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hip():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


def test_nothing_but_the_corner_is_left_out():
    assert set(kc.UNREALISED) == set(kc.CORNER_REQUESTS) and all("/first-cell/col0/row0/" in n for n in kc.UNREALISED)


@pytest.mark.parametrize("name", kc.ALL_NAMES)
def test_against_the_oracle(hip_v2, oracle_built, name):
    c = kc.case(name)
    hip_v2.set_image(c["planes"])
    hip_v2.encode(c["rf"], False, False)
    _same_gradient(hip_v2, c, name)
    _same_range(hip_v2, c, name)


@pytest.mark.parametrize("names", kc.BATCHES, ids=["+".join(b) for b in kc.BATCHES])
def test_batch_of_three(hip, oracle_built, names):
    """the fused kernel's frame-strided form: three different frames of one shape, each compared with its own oracle run"""
    import torch
    cases = [kc.case(n) for n in names]
    frames = torch.from_numpy(np.ascontiguousarray(np.stack([c["planes"] for c in cases]))).cuda()
    hip.set_batch(frames)
    hip.encode_batch(cases[0]["rf"], False)
    for f, c in enumerate(cases):
        hip.select_frame(f)
        _same_gradient(hip, c, (names, "frame", f))
        _same_range(hip, c, (names, "frame", f))
