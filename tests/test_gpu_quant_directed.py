"""Directed tests of the 8x8 range quantiser's mode selection (the range phase of yk_encode2_kernel in yk_encode2.hip) and of the first-generation
cross-check kernel (tests/csrc/yk_encode_v1.hip) on tiles whose two best modes tie, nearly tie, or are told apart only by the order in which the
reference adds its float terms (tests/quant_cases.py; tests/test_quant_cases.py shows from the reference alone that every case holds what it
claims and that the cases catch the wrong pickers one by one).  Every comparison is exact, against the CPU oracle.

Each case runs in the shipped instantiation (want_dst False: the `spread` path for strips of at most four valid cells, the wide stores of strips
of whole tiles, WHOLE for frames whose sides are multiples of 64) and in the test-only one (want_dst True), with both start modes.  On top of
the stream comparison the mode of every tile that is not `sure` is read from its definition word, so a failure names the tile, its class and
both modes.  Which path a tile took is not observed: it follows from the inputs (see classify() in tests/quant_cases.py)."""
import numpy as np
import pytest

from tests import quant_cases as qc
from tests.parity import compare_encode

pytestmark = pytest.mark.gpu
COMBOS = [(want_dst, m3) for want_dst in (False, True) for m3 in (False, True)]


@pytest.fixture(scope="module", params=[2, 1], ids=["kernel_v2", "kernel_v1"])
def hip_gen(request):
    from tests.parity import encoder_for_kernel_version
    e = encoder_for_kernel_version(request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hooked():
    """a handle of the test build of the library: the same kernel source with the ablation switches"""
    from yaik_amd._lib import test_lib
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0, hooks=True)
    yield e
    test_lib().yk_set_ablation(e._h, 0)
    e.close()


@pytest.fixture(scope="module")
def hip():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


def _wrong_modes(e, c, m3):
    """The tiles that are not `sure` and the tiles of the case's targets, one by one: the definition word, and the index nibbles, which tell the
    kernel's mode even where the reference's word loses the mode's low bit (range << 7 reaches bit 13).  Returns a line per wrong tile."""
    cs = c["census"][m3]
    named = {t["tile"]: t["name"] for t in c["targets"]}
    out = []
    for p in range(3):
        defs, nib, nn = e.range_streams(p)
        want_defs, _, want_nn = cs["streams"][p]
        if defs.size != want_defs.size or nn != want_nn:
            return [f"plane {p}: {defs.size} definitions and {nn} nibbles, the oracle has {want_defs.size} and {want_nn}"]
        codes = np.stack([nib & 15, nib >> 4], 1).ravel()
        for (q, ty, tx), rec in cs["tiles"].items():
            if q != p or (rec["cls"] == "sure" and (q, ty, tx) not in named):
                continue
            r = rec["model"]
            got = codes[rec["nib0"]: rec["nib0"] + rec["n"]]
            if int(defs[rec["k"]]) != r["def"] or not np.array_equal(got, r["codes"][r["pick"]]):
                fits = [m for m in range(r["start"], 6) if np.array_equal(got, r["codes"][m])]
                out.append(f"plane {p} tile ({ty}, {tx}) [{named.get((q, ty, tx))}] classes {sorted(rec['flags'])}, valid cells {rec['quads']}, min {rec['mn']} max {rec['mx']}: "
                           f"oracle mode {r['pick']} word {r['def']:#06x}; kernel word {int(defs[rec['k']]):#06x}, its indices are those of mode(s) {fits}")
    return out


def _run(e, c, what, combos=COMBOS):
    for want_dst, m3 in combos:
        bad = compare_encode(c["planes"], e, m3, want_dst=want_dst)
        wrong = _wrong_modes(e, c, m3)
        head = f"{what}: want_dst {want_dst}, start mode {3 if m3 else 0}"
        assert not wrong, "\n".join([head, f"{len(wrong)} tiles with another mode than the oracle's:"] + [str(w) for w in wrong[:8]] + ["streams:"] + bad)
        assert not bad, "\n".join([head] + bad)


@pytest.mark.parametrize("name", qc.NAMES)
def test_against_the_oracle(hip_gen, oracle_built, name):
    """product kernel (its own choice of instantiation: WHOLE for the 64-multiple RGB cases when want_dst is False) and the v1 cross-check"""
    _run(hip_gen, qc.case(name), name)


@pytest.mark.parametrize("name", qc.NAMES)
def test_exact_path_for_every_tile(hooked, oracle_built, name):
    """yk_set_ablation 16: every tile-plane goes through the wave-wide re-summation in the reference's order"""
    from yaik_amd._lib import test_lib
    assert test_lib().yk_set_ablation(hooked._h, 16) == 0
    _run(hooked, qc.case(name), (name, "exact path forced"))


@pytest.mark.parametrize("name", qc.WHOLE_NAMES)
def test_whole_and_general_instantiation(hooked, oracle_built, name):
    """frames whose sides are multiples of 64: the test build's own choice (WHOLE), the general instantiation forced (32), and that with the
    exact path forced as well"""
    from yaik_amd._lib import test_lib
    c = qc.case(name)
    assert c["planes"].shape[1] % 64 == 0 and c["planes"].shape[2] % 64 == 0
    for flag in (0, 32, 48):
        assert test_lib().yk_set_ablation(hooked._h, flag) == 0
        _run(hooked, c, (name, "ablation", flag), [(False, False), (False, True)])


def _noise(shape, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).integers(0, 256, shape), np.int32)


@pytest.mark.parametrize("name", ["full128x64", "part72x40_a", "part72x40_b", "spread72x40_order_s0_0a", "five72x40_part14_tie_diff"])
@pytest.mark.parametrize("m3", [False, True])
def test_batch_frame_1_of_3(hip, oracle_built, name, m3):
    """yk_encode_batch: the directed image between two frames of noise; every frame's range streams against the oracle, the directed
    frame's modes tile by tile"""
    import torch
    from oracle.pyoracle import PASSES, OracleEncoder
    c = qc.case(name)
    frames = [_noise(c["planes"].shape, 1), np.asarray(c["planes"]), _noise(c["planes"].shape, 2)]
    hip.set_batch(torch.from_numpy(np.ascontiguousarray(np.stack(frames))).cuda())
    hip.encode_batch(3, m3)
    for f, planes in enumerate(frames):
        hip.select_frame(f)
        if f == 1:
            wrong = _wrong_modes(hip, c, m3)
            assert not wrong, "\n".join([f"{name}: frame 1, {len(wrong)} tiles with another mode than the oracle's:"] + [str(w) for w in wrong[:8]])
        ora = OracleEncoder(planes)
        for sx, sy in PASSES:
            ora.fitting_quad_smooth(sx, sy)
        for p in range(3):
            defs, nib, nn, _ = ora.dynamic_tile_encode(p, m3)
            d2, n2, nn2 = hip.range_streams(p)
            assert nn2 == nn and np.array_equal(d2, defs) and np.array_equal(n2, nib), (name, "frame", f, "plane", p, nn2, nn)
