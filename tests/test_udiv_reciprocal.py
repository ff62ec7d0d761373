"""The multiply-and-shift division of the fused encode kernel's unit decode (yaik_amd/csrc/yk_udiv.h), on the CPU, through
yaik_amd/host/udiv_tool, which compiles the very functions the library uses (yk_udiv_make on the host when the image or batch is set,
yk_udiv in the kernel).

The bound.  yk_udiv is exact for every divisor d >= 1 and every numerator n < YK_UDIV_LIMIT = 2^29 (the proof is in the header).  A launch
divides block indices L < nB by xBB64 (blocks per block row, at most 512: sides are at most 32760 pixels) and by nBf (blocks per frame, at
most 512 * 512); nB = nBf * nFrames with at most 1024 frames, and the grid is rounded up to 128 blocks: L < 2^28 + 128 < 2^29.
yk_launch_encode2 refuses a launch beyond the limit."""
import json
import os
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yaik_amd", "host")
LIMIT = 1 << 29
MAX_SIDE, MAX_FRAMES, GROUP = 32760, 1024, 128                    # yk_set_image, yk_set_batch, the grid's rounding (8 * YK2_RUN blocks)
MAX_XBB64 = (MAX_SIDE + 63) // 64
MAX_NBF = MAX_XBB64 * MAX_XBB64


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", HOST, "udiv_tool"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "udiv_tool")


def _run(tool, *args):
    r = subprocess.run([tool, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode in (0, 1), r.stderr
    return json.loads(r.stdout)


def test_every_block_count_to_1024_with_every_index_below_1024_rows(tool):
    """d in 1..1024, L in [0, d * 1024): every quotient equals L / d"""
    out = _run(tool, "all", 1024, 1024)
    assert out["checked"] == 1024 * sum(range(1, 1025))
    assert out["mismatches"] == 0, out["firstBad"]
    assert out["maxNumerator"] == 1024 * 1024 - 1 < out["limit"] == LIMIT


def test_blocks_per_frame_up_to_the_largest_frame(tool):
    """nBf in 1..512*512: the end points of the quotient ranges (k d - 1 and k d for the first frames, for frames 1023..1025 and for the
    last quotient below the limit), 0, 1, the limit's last numerators, and 64 seeded numerators in [0, 2^29) each"""
    assert MAX_NBF == 512 * 512
    out = _run(tool, "ranges", MAX_NBF, 20261, 64)
    assert out["checked"] >= MAX_NBF * (64 + 4 + 8)               # a few end points fall beyond the limit for the largest divisors
    assert out["mismatches"] == 0, out["firstBad"]
    assert out["maxNumerator"] == LIMIT - 1


def test_a_launch_stays_below_the_limit():
    assert MAX_NBF * MAX_FRAMES + GROUP <= LIMIT
    src = open(os.path.join(os.path.dirname(HOST), "csrc", "yk_encode2.hip")).read()
    assert "> (long long)YK_UDIV_LIMIT) return yk_fail" in src    # the host's own check in yk_launch_encode2
    api = open(os.path.join(os.path.dirname(HOST), "csrc", "yk_api.hip")).read()
    assert "fullW > 32760 || fullH > 32760" in api and "nFrames > 1024" in api


def test_the_formula_as_written_down():
    """an independent spelling of the header's formula: shift = floor(log2 d), mul = ceil(2^(31 + shift) / d), q = ((2 n + 1) mul) >> (32 + shift)"""
    import random
    rng = random.Random(5)
    for d in [1, 2, 3, 5, 7, 64, 127, 128, 129, 511, 512, 1023, 1024, MAX_NBF - 1, MAX_NBF] + [rng.randrange(1, MAX_NBF + 1) for _ in range(200)]:
        shift = d.bit_length() - 1
        mul = -((-(1 << (31 + shift))) // d)
        assert (1 << 30) < mul <= (1 << 31)
        for n in [0, 1, d - 1, d, d + 1, 1024 * d - 1, 1024 * d, LIMIT - 1] + [rng.randrange(LIMIT) for _ in range(50)]:
            if 0 <= n < LIMIT:
                assert (((2 * n + 1) * mul) >> (32 + shift)) == n // d, (d, n)
