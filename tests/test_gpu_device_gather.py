"""yk_device_gather (HipTileEncoder.gather): segments anywhere in device memory into one buffer with one launch.  The whole destination, padding
and the bytes behind the total included, is compared with a numpy model over a sentinel fill."""
import ctypes as C

import numpy as np
import pytest

from yaik_amd._lib import lib
from yaik_amd.encoder import HipTileEncoder, gather_layout

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG, YK_ERR_RANGE = -2, -5
SENTINEL = 0xA5
LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 70001, 1000003]               # around the 16-byte lane and the 4 KB piece, and many pieces


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def enc():
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool():
    """one source buffer in HBM and its host copy: segments are cut out of it at any byte offset"""
    torch = _torch()
    host = np.random.default_rng(11).integers(0, 256, 4 << 20, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    return host, dev


def _run(enc, pool, segs, tail=256):
    """segs: (byte offset in the pool, length); gathers, and compares the whole destination with the model"""
    torch = _torch()
    host, dev = pool
    lens = [n for _, n in segs]
    offs, total = gather_layout(lens)
    q_offs, q_total = enc.gather([0] * len(segs), lens, None)               # the size query needs no sources
    assert q_total == total and np.array_equal(q_offs, offs)
    out = torch.full((total + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
    ptrs = [dev.data_ptr() + o if n else 0 for o, n in segs]
    g_offs, g_total = enc.gather(ptrs, lens, out)
    enc.synchronize()
    assert g_total == total and np.array_equal(g_offs, offs)
    want = np.full(total + tail, SENTINEL, np.uint8)
    for (o, n), d in zip(segs, offs):
        want[d:d + n] = host[o:o + n]
    np.testing.assert_array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_lengths_in_shuffled_orders_at_every_source_alignment(enc, pool, seed):
    rng = np.random.default_rng(seed)
    lens = [LENGTHS[i] for i in rng.permutation(len(LENGTHS))]
    segs, at = [], 0
    for i, n in enumerate(lens):
        at = (at + 15) & ~15
        segs.append((at + (i * 5 + seed * 7) % 16, n))                       # source bases at byte offsets 0..15
        at += n + 16
    assert at < pool[0].size and len({o % 16 for o, _ in segs}) >= 5
    _run(enc, pool, segs)


def test_every_source_offset_for_every_short_length(enc, pool):
    segs = [(1024 * k + a, n) for k, (a, n) in enumerate((a, n) for a in range(16) for n in (1, 15, 16, 17, 33, 4097))]
    _run(enc, pool, segs)


def test_a_thousand_small_segments(enc, pool):
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 41, 1000)
    at = np.cumsum(lens + rng.integers(0, 5, 1000)) + 3
    _run(enc, pool, [(int(a), int(n)) for a, n in zip(at, lens)])


def test_a_single_segment(enc, pool):
    _run(enc, pool, [(7, 70001)])
    _run(enc, pool, [(0, 16)])
    _run(enc, pool, [(5, 0)])                                                # nothing but an empty segment: nothing is launched


def test_gather_layout_is_the_c_layout(enc):
    lens = [0, 1, 15, 16, 17, 4095, 4096, 4097, 70001, 1000003, 0, 3]
    offs, total = gather_layout(lens)
    c_offs, c_total = enc.gather([0] * len(lens), lens, None)
    assert np.array_equal(offs, c_offs) and total == c_total
    assert offs.tolist()[:6] == [0, 0, 16, 32, 48, 80] and total % 16 == 0 and total == offs[-1] + 16


def _refused(h, rc, code, word):
    assert rc == code, (rc, code, word)
    msg = lib().yk_last_error(h).decode()
    assert word in msg, (word, msg)


def test_refusals_leave_the_destination_alone(enc, pool):
    torch = _torch()
    L = lib()
    host, dev = pool
    n = 3
    lens = (C.c_size_t * n)(100, 0, 5000)
    src = (C.c_void_p * n)(dev.data_ptr() + 3, None, dev.data_ptr() + 4096)
    offs, total = (C.c_size_t * n)(), C.c_size_t()
    out = torch.full((8192,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dst, cap = C.c_void_p(out.data_ptr()), out.numel()
    _refused(enc._h, L.yk_device_gather(enc._h, None, lens, n, dst, cap, offs, C.byref(total)), YK_ERR_BAD_ARG, "NULL")
    _refused(enc._h, L.yk_device_gather(enc._h, src, None, n, dst, cap, offs, C.byref(total)), YK_ERR_BAD_ARG, "NULL")
    _refused(enc._h, L.yk_device_gather(enc._h, src, lens, n, dst, cap, None, C.byref(total)), YK_ERR_BAD_ARG, "NULL")
    _refused(enc._h, L.yk_device_gather(enc._h, src, lens, n, dst, cap, offs, None), YK_ERR_BAD_ARG, "NULL")
    for bad in (0, -1, 262145):
        _refused(enc._h, L.yk_device_gather(enc._h, src, lens, bad, dst, cap, offs, C.byref(total)), YK_ERR_BAD_ARG, "1..262144")
    holes = (C.c_void_p * n)(dev.data_ptr(), dev.data_ptr(), None)
    _refused(enc._h, L.yk_device_gather(enc._h, holes, lens, n, dst, cap, offs, C.byref(total)), YK_ERR_BAD_ARG, "NULL pointer")
    for a in (1, 8, 15):
        _refused(enc._h, L.yk_device_gather(enc._h, src, lens, n, C.c_void_p(out.data_ptr() + a), cap - 16, offs, C.byref(total)), YK_ERR_BAD_ARG, "multiple of 16")
    want_total = 112 + 5008
    for short in (0, want_total - 1):
        _refused(enc._h, L.yk_device_gather(enc._h, src, lens, n, dst, short, offs, C.byref(total)), YK_ERR_RANGE, "too small")
        assert total.value == want_total and list(offs) == [0, 112, 112]
    enc.synchronize()
    assert bool((out == SENTINEL).all())
    assert L.yk_device_gather(enc._h, src, lens, n, dst, want_total, offs, C.byref(total)) == 0     # an exact capacity, and the handle still works
    enc.synchronize()
    got = out.cpu().numpy()
    want = np.full(8192, SENTINEL, np.uint8)
    want[0:100] = host[3:103]
    want[112:5112] = host[4096:9096]
    np.testing.assert_array_equal(got, want)
