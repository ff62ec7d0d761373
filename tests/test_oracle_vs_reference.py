"""CPU suite: the oracle restatement against the unmodified reference (oracle/_ref/ref_driver), through the digests of the reference's
outputs committed in tests/golden/reference_digests.json; where the reference build exists, each digest is also checked against a live run."""
import pytest

from oracle.refrun import run_reference
from tests.blobs import compare_digest, oracle_blobs, reference_digest, reference_view
from tests.images import edge_image, lineart_image, natural_photo, synth_planes

CASES = {
    "synth128_rgb": lambda: synth_planes(128, n_planes=3),
    "synth256_rgba": lambda: synth_planes(256, n_planes=4),
    "noise64_rgb": lambda: edge_image(64, 64, "noise", 3),
    "flat128_rgba": lambda: edge_image(128, 128, "flat", 4),
    "smooth128_rgba": lambda: edge_image(128, 128, "smooth", 4),
    "white128_rgb": lambda: edge_image(128, 128, "white", 3),
    "dark64_rgb": lambda: edge_image(64, 64, "dark", 3),
    "twocolor256_rgba": lambda: edge_image(256, 256, "twocolor", 4),
    "mixed200x136_rgb": lambda: edge_image(200, 136, "mixed", 3),
    "photo256_rgba": lambda: edge_image(256, 256, "photo", 4),
    "photo192x128_rgb": lambda: edge_image(192, 128, "photo", 3, seed=11),
    "lineart512_rgba": lambda: lineart_image(512, 4),            # drawn illustration, anti-aliased edges, alpha surround
    "photo_astronaut256_rgb": natural_photo,                     # natural photograph
}


def reference_case(name):
    planes = CASES[name]()
    n, h, w = planes.shape
    return reference_view(run_reference(planes), decode_ok=(w % 16 == 0 and h % 16 == 0))


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_reference(oracle_built, name):
    ref = reference_digest("oracle_vs_reference", name, reference_case)
    bad = compare_digest(ref, oracle_blobs(CASES[name]()))
    assert not bad, bad


FUZZ_SEEDS = [1000, 1003, 1004, 1007, 1009, 1014]


def fuzz_planes(seed):
    from tests.test_gpu_fuzz_parity import _image
    size = 256 if seed % 2 else 128                     # the reference's RGBA path needs >= 256 (bad_alloc below)
    return _image(seed, size, 4 if seed % 2 else 3)


def reference_fuzz_case(seed):
    return reference_view(run_reference(fuzz_planes(int(seed))))


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_oracle_equals_reference_on_fuzz_regimes(oracle_built, seed):
    """The tile regimes of tests/test_gpu_fuzz_parity.py (ranges around 16, values >= 223, zeros, two-level tiles, accept-boundary
    gradients): the oracle must agree with the unmodified reference there too, so the GPU fuzz test is anchored."""
    ref = reference_digest("oracle_vs_reference_fuzz", str(seed), reference_fuzz_case)
    bad = compare_digest(ref, oracle_blobs(fuzz_planes(seed)))
    assert not bad, bad
