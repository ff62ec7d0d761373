"""CPU only: the directed 1-D decode cases of tests/dec1d_cases.py hold what they claim, shown from the oracle and the model alone.

* the two references agree on every case: OracleDecoder (the gradient chunk first, split_masks and the plane-subset chunks where the case calls for
  them, then decode_1d on the streams zero-extended to full length) == model_decode, planes, tile4x4Mask and bytes consumed; a mismatch here is
  about the oracle or the model and is settled before any GPU test is trusted;
* the claims, from the model's census and the cases themselves (every mask at every quad position, wrapping and non-wrapping pixels, the scan
  blocks, the byte lanes, the cut points, the differing plane masks, the batches);
* every deliberate defect of the model changes the planes of a case named here.

No case is skipped or expected to fail.
"""
import numpy as np
import pytest

from tests import dec1d_cases as DC
from tests import graddec_cases as GC


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_built):
    pass


# ---- agreement of the two references --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.ALL_NAMES)
def test_oracle_equals_model(name):
    c, o, m = DC.case(name), DC.oracle_run(name), DC.model(name)
    assert o["consumed"] == m["consumed"] == (c["full_typ"].size, c["full_pix"].size), (name, o["consumed"], m["consumed"])
    assert np.array_equal(o["tile4"], m["tile4"]), name
    assert np.array_equal(o["planes"], m["planes"]), (name, DC.story(name, o["planes"], m["planes"]))


def test_the_oracle_alone_cannot_judge_a_long_cut():
    """decode_1d pads 64 zero bytes: the cuts of more than 64 bytes are judged by the zero-extended streams only"""
    for n in ("cut_typ_far", "cut_pix_far", "cut_typ_in0", "cut_pix_in0"):
        c = DC.case(n)
        assert c["full_typ"].size - c["typ"].size > 64 or c["full_pix"].size - c["pix"].size > 64, n


# ---- the stream builder ---------------------------------------------------------------------------------------------------------------------------
def test_streams_follow_the_stated_order():
    """one tile, mask 0x6 (top right and bottom left filled): the top half holds its left quadrant's four rows, the bottom half its right one's"""
    c = DC.case("tile_8x8_m6")
    L = c["L"]
    for p in range(3):
        assert c["full_typ"][3 * p:3 * p + 3].tolist() == [int(c["color0"][p, 0]), int(c["base"][p, 0]), int(c["delta"][p, 0])]
        assert np.array_equal(c["full_pix"][32 * p:32 * p + 32], np.concatenate([L[p, :4, :4].ravel(), L[p, 4:, 4:].ravel()]))
    c = DC.case("tile_8x8_m0")                                                  # nothing filled: rows of [left 4][right 4] = the tile row-major
    assert np.array_equal(c["full_pix"][:64], c["L"][0].ravel()) and c["full_pix"].size == 192 and c["full_typ"].size == 9
    c = DC.case("tile_16x8_m0")                                                 # tiles row-major (the second has mask 0x3: its bottom half only), planes one after the other
    assert c["masks"][0].tolist() == [0, 3]
    assert np.array_equal(c["full_pix"][64:96], c["L"][0, 4:, 8:].ravel()) and np.array_equal(c["full_pix"][96:160], c["L"][1, :, :8].ravel())
    for name in DC.ALL_NAMES:
        c = DC.case(name)
        q = c["masks"]
        pops = (q & 1) + (q >> 1 & 1) + (q >> 2 & 1) + (q >> 3 & 1)
        assert c["full_typ"].size == 3 * int((q != 15).sum()) and c["full_pix"].size == int((16 * (4 - pops)).sum()), name


def test_marks_come_from_hand_built_chunks_and_the_gradient_pixels_survive():
    for name in ("masks_136x72", "blocks_520x264", "tile_8x8_m9", "split_136x72", "batch_r7_1"):
        c, m = DC.case(name), DC.model(name)
        st = DC.gradient_state(c)
        w, h = c["w"], c["h"]
        marked = np.zeros((3, h, w), dtype=bool)
        for p in range(3):
            for cx, cy in DC.cells_of(c["masks"][p], w):
                marked[p, 4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4] = True
        mt = DC._tiled(marked.astype(np.uint8)).astype(bool)
        assert mt.any() and not mt.all(), name
        assert np.array_equal(m["planes"][mt], st["planes"][mt]) and st["planes"][mt].any(), name      # the 1-D call leaves marked quadrants alone
        if c["gtil"] is not None:
            (sx, sy, bm, raw), = c["gtil"]["chunks"]
            assert (sx, sy) == (2, 2) and np.array_equal(bm, GC.bitmap_of(2, 2, w, h, DC.cells_of(c["masks"][0], w)))
            assert np.array_equal(raw, GC.raw_stream(raw.size, 0)) and raw.size == c["gtil"]["need"][0]


# ---- the claims ---------------------------------------------------------------------------------------------------------------------------------
def test_values_cases_hold_every_delta_and_L_and_both_regimes():
    assert DC.VALUE_NAMES == tuple(f"values_r{r}" for r in (1, 2, 3, 7, 8, 15, 16, 17, 128, 255))
    for name in DC.VALUE_NAMES:
        c, m = DC.case(name), DC.model(name)
        assert (c["w"], c["h"]) == (256, 256) and not c["masks"].any() and c["gtil"] is None
        assert m["blocks"] == [[1024]] * 3 and m["consumed"] == (3 * 3072, 3 * 65536)     # one full scan block: the limit of the 11 + 17 bit packing
        tiled = DC._tiled(c["L"]).reshape(3, 1024, 64)
        pairs = {(int(d), int(l)) for d, row in zip(c["delta"][0], tiled[0]) for l in row}
        top = 128 if c["range"] == 1 else 256
        assert pairs == {(d, l) for d in range(top) for l in range(256)}, name
        assert (c["base"][0] == 0).all() and (c["base"][1] == 255).all() and np.array_equal(c["base"][2], (73 * c["delta"][2] + 41) % 256)
        wraps, decoded = m["wrap"]
        assert 0 < wraps < decoded, (name, m["wrap"])
        free = clash = 0
        for p in range(3):
            for t in range(0, 1024, 4):
                dec = DC.decodable(int(c["base"][p, t]), int(c["delta"][p, t]), c["range"])
                if int(c["color0"][p, t]) in dec:
                    clash += 1
                    assert len(dec) == 256                                       # color0 is decodable only where every value is
                else:
                    free += 1
        assert free > clash or c["range"] <= 2, (name, free, clash)
    # delta2 passes 2^21 below range 8: the bound is 2^24 (range 1, delta 255: 255 * 65536 + 1), and 8355841 at range 2
    assert ((255 * ((1 << 24) // 8)) >> 8) + 1 < 1 << 21 <= ((255 * ((1 << 24) // 7)) >> 8) + 1
    assert ((255 * ((1 << 24) // 2)) >> 8) + 1 == 8355841 and ((255 * (1 << 24)) >> 8) + 1 < 1 << 24


def test_lane_cases_hold_every_dword():
    dw = DC.lane_dwords()
    assert len({tuple(r) for r in dw.tolist()}) == 625 and set(dw.ravel().tolist()) == {0, 1, 0x7F, 0x80, 0xFF}
    for name, rng in (("lanes_r15", 15), ("lanes_r2", 2)):
        c = DC.case(name)
        assert (c["w"], c["h"], c["range"]) == (64, 40, rng) and not c["masks"].any()
        for p in range(3):
            got = {tuple(r) for r in c["full_pix"][2560 * p:2560 * p + 2560].reshape(-1, 4).tolist()}       # 16-byte aligned: these are the kernel's dwords
            assert got == {tuple(r) for r in dw.tolist()}, (name, p)
        assert (c["color0"] != c["base"]).all()                                 # L == 1 decodes to base: a 0x01 taken for a zero shows


def test_mask_cases_hold_every_mask_at_every_quad_position():
    want = {(q, k) for q in range(15) for k in range(4)}
    for name in ("masks_136x72", "blocks_520x264", "split_136x72", "split_520x264", "batch_r15_0", "batch_r7_2"):
        assert DC.model(name)["mask_at"] == want, name
    c = DC.case("masks_136x72")
    q = c["masks"][0]
    assert (c["w"], c["h"], q.size) == (136, 72, 153)
    assert {(int(v), i & 3) for i, v in enumerate(q)} == {(v, k) for v in range(16) for k in range(4)}       # the fully marked tile too
    assert (q[1:] != q[:-1]).all() and (q[17:] != q[:-17]).all()                # no tile has the mask of its left or upper neighbour
    for a in ("color0", "base", "delta"):
        assert (c[a][:, 1:] != c[a][:, :-1]).all() and (c[a][1:] != c[a][:-1]).all()
    assert (c["L"][:, 1:] != c["L"][:, :-1]).all() and (c["L"][:, :, 1:] != c["L"][:, :, :-1]).all() and (c["L"] == 0).any()
    # the bottom half's offset 16 * nTop behind every mask of the top half, with something to read there
    assert {(int(v) & 3) for v in q if (int(v) >> 2) != 3} == {0, 1, 2, 3}


def test_scan_block_case():
    c, m = DC.case("blocks_520x264"), DC.model("blocks_520x264")
    q = c["masks"][0]
    assert (c["w"] >> 3, c["h"] >> 3, q.size) == (65, 33, 2145) and q.size % 64 == 33 and -(-q.size // 1024) == 3
    assert not q[:1024].any() and (q[1024:1101] == 15).all() and q[1023] != 15 and q[1101] != 15
    assert m["blocks"][0][0] == 1024 and 0 < m["blocks"][0][1] < 1024 - 77 + 1 and 0 < m["blocks"][0][2] <= 97
    assert (q[1101:] == 15).any() and (q[2048:] != 15).any()
    assert 16 * 4 * 1024 == 65536                                               # block 0's pixel bytes: the 17-bit field's limit


def test_one_tile_cases():
    assert len(DC.TILE_NAMES) == 32
    for w in (8, 16):
        assert {int(DC.case(f"tile_{w}x8_m{q}")["masks"][0, 0]) for q in range(16)} == set(range(16))
    assert {int(DC.case(f"tile_16x8_m{q}")["masks"][0, 1]) for q in range(16)} == set(range(16))
    c = DC.case("tile_8x8_m15")
    assert c["typ"].size == 0 and c["pix"].size == 0                             # mask 0xF everywhere: empty streams, the planes keep the gradient pixels
    assert np.array_equal(DC.model("tile_8x8_m15")["planes"], DC.gradient_state(c)["planes"]) and DC.gradient_state(c)["planes"].any()
    assert DC.case("tile_16x8_m15")["masks"][0].tolist() == [15, 12] and DC.case("tile_16x8_m6")["masks"][0].tolist() == [6, 13]


def test_cut_cases():
    full = DC.case("masks_136x72")
    nt, npx = full["full_typ"].size // 3, full["full_pix"].size // 3
    pts = DC.cut_points()
    assert tuple(pts) == DC.CUT_NAMES
    for name, cut in pts.items():
        c = DC.case(name)
        (which, n), = cut.items()
        other = "pix" if which == "typ" else "typ"
        assert c[which].size == n and n % (3 if which == "typ" else 4) == 0 and c[other].size == full["full_" + other].size
        assert np.array_equal(c["full_" + which], full["full_" + which]) and np.array_equal(c["masks"], full["masks"])
        assert not np.array_equal(DC.model(name)["planes"], DC.model("masks_136x72")["planes"]), name    # the missing bytes are seen
    per = {"typ": nt, "pix": npx}
    for which in ("typ", "pix"):
        n = per[which]
        assert 0 < pts[f"cut_{which}_in0"][which] < n == pts[f"cut_{which}_at1"][which] and 2 * n < pts[f"cut_{which}_in2"][which] < 3 * n - 64
        assert 3 * n - pts[f"cut_{which}_far"][which] > 64 and pts[f"cut_{which}_0"][which] == 0
    assert pts["cut_pix_in0"]["pix"] % 16 == 4 and pts["cut_pix_in2"]["pix"] % 16 == 12        # a cut inside a lane's 16 bytes


def test_split_cases_have_three_different_masks():
    for name in DC.SPLIT_NAMES:
        c = DC.case(name)
        q = c["masks"]
        assert c["gtil"] is None and [m for m, _, _ in c["plane_chunks"]] == [3, 1, 2, 4]
        assert (q[0] != q[1]).any() and (q[1] != q[2]).any() and (q[0] != q[2]).any()
        counts = [int((q[p] != 15).sum()) for p in range(3)]
        assert DC.model(name)["consumed"][0] == 3 * sum(counts)
        assert DC.oracle_run(name)["tile4"].size == 3 * ((c["w"] + 15) >> 4) * (c["h"] >> 3)
    assert len(DC.model("split_520x264")["blocks"][0]) == 3


def test_batches_share_a_shape_and_differ_in_everything_else():
    assert set(DC.BATCHES) == {"batch_r15", "batch_r7"}
    for key, names in DC.BATCHES.items():
        cs = [DC.case(n) for n in names]
        assert len({(c["w"], c["h"], c["range"]) for c in cs}) == 1 and (cs[0]["w"], cs[0]["h"]) == (136, 72)
        assert len({c["masks"].tobytes() for c in cs}) == 3 and len({c["full_typ"].tobytes() for c in cs}) == 3
        assert [c["typ"].size > 0 for c in cs] == [True, False, True] and [c["pix"].size > 0 for c in cs] == [True, False, True]
        assert cs[1]["full_typ"].size and cs[1]["gtil"] is not None
    assert DC.case("batch_r7_0")["range"] == 7 and DC.case("batch_r15_0")["range"] == 15


# ---- sensitivity: every defect is seen by a named case -------------------------------------------------------------------------------------------
SEES = {
    "saturate": ("values_r15", "values_r2", "lanes_r15", "masks_136x72"),
    "no_plus_one": ("values_r15", "values_r255", "masks_136x72"),
    "l_times": ("values_r15", "values_r1", "lanes_r2"),
    "l0_base": ("values_r15", "lanes_r15", "masks_136x72"),
    "borrow_zero": ("lanes_r15", "lanes_r2", "values_r15"),
    "quadrant_major": ("masks_136x72", "blocks_520x264", "tile_8x8_m0", "tile_8x8_m12", "tile_8x8_m3"),
    "bottom_32": ("masks_136x72", "tile_8x8_m1", "tile_8x8_m3", "tile_16x8_m2"),
    "full_consumes": ("masks_136x72", "blocks_520x264", "tile_16x8_m15"),
    "planes_at_0": ("masks_136x72", "values_r15", "tile_8x8_m0", "split_136x72"),
    "block_base": ("blocks_520x264", "split_520x264"),
    "range_15": ("values_r7", "values_r16", "values_r1", "lanes_r2", "batch_r7_0", "batch_r7_2"),
}


@pytest.mark.parametrize("defect", DC.DEFECTS)
def test_every_defect_changes_a_named_case(defect):
    assert set(SEES) == set(DC.DEFECTS)
    for name in SEES[defect]:
        good, bad = DC.model(name), DC.model_decode(DC.case(name), defect=defect)
        assert not np.array_equal(good["planes"], bad["planes"]), f"{defect} is invisible in {name}"


def test_defects_are_blind_where_their_mechanism_is_absent():
    """what makes each of these a defect of its own"""
    for defect, name in (("block_base", "masks_136x72"), ("full_consumes", "values_r15"), ("quadrant_major", "tile_8x8_m6"), ("bottom_32", "tile_8x8_m0"),
                         ("range_15", "values_r15"), ("borrow_zero", "tile_8x8_m15")):
        assert np.array_equal(DC.model(name)["planes"], DC.model_decode(DC.case(name), defect=defect)["planes"]), (defect, name)
