"""CPU only: the directed gradient-decode cases of tests/graddec_cases.py hold what they claim, shown from the oracle and the model alone.

* the two references agree on every case: OracleDecoder.gradient chunk by chunk == model_decode (planes, tile4x4Mask, the corner lattice, the
  bytes consumed per chunk); a mismatch here is about the oracle or the model and is settled before any GPU test is trusted;
* the claims, from the model's census (tuples, byte values, corners per workgroup, block spans, loaded subsets, overlaps, edge bits, isolation);
* every deliberate defect of the model changes the planes or the marks of a case named here.

Run time of the whole file, measured on one CPU core: 8.7 s (122 tests; building the cases and the model's run of each take most of it).
"""
import numpy as np
import pytest

from tests import graddec_cases as GC


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_built):
    pass


# ---- the helpers themselves ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shp", list(GC.SHAPES))
@pytest.mark.parametrize("w,h", [(8, 8), (72, 40), (192, 128), (200, 136)])
def test_tile_bit_and_its_inverse(shp, w, h):
    sx, sy = GC.SHAPES[shp]
    g = GC.geo(sx, sy, w, h)
    nbits = g["nbytes"] * 8
    assert nbits == g["xbb"] * g["ybb"] * g["bit_count"] and g["bit_count"] % 8 == 0
    seen = set()
    for bit in range(nbits):
        tx, ty = GC.bit_tile(sx, sy, w, bit)
        assert GC.tile_bit(sx, sy, w, tx, ty) == bit
        seen.add((tx, ty))
    assert len(seen) == nbits                                                  # a bijection onto the tiles of the padded image
    assert seen == {(tx, ty) for tx in range(g["xbb"] * g["tpr"]) for ty in range(nbits // (g["xbb"] * g["tpr"]))}
    # swizzle order: tiles row-major inside a block, blocks row-major
    assert GC.bit_tile(sx, sy, w, 1) == (1, 0) and GC.bit_tile(sx, sy, w, g["tpr"]) == (0, 1)
    if g["xbb"] > 1:
        assert GC.bit_tile(sx, sy, w, g["bit_count"]) == (g["tpr"], 0)


def test_streams_follow_the_stated_rule():
    for name in GC.ALL_NAMES:
        c = GC.case(name)
        if c["group"] == "a":
            continue
        for ci, ((sx, sy, bm, raw), need) in enumerate(zip(c["chunks"], c["need"])):
            cut = c["short"].get(ci, 0)
            assert raw.size == (0 if cut == "all" else need - cut), (name, ci)
            assert np.array_equal(raw, (37 * np.arange(raw.size) + 11 + 5 * ci) % 251) and (raw.size == 0 or raw.max() <= 250)
            assert bm.size == GC.geo(sx, sy, c["w"], c["h"])["nbytes"]           # no bitmap is shorter than its pass needs
    s = GC.raw_stream(753, 0)
    assert set(s.tolist()) == set(range(251))
    assert (s[3:].reshape(-1, 3) != s[:-3].reshape(-1, 3)).any(axis=1).all()    # no two consecutive triples are equal


# ---- agreement of the two references --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.ALL_NAMES)
def test_oracle_equals_model(name):
    o, m = GC.oracle_run(name), GC.model(name)
    assert o["consumed"] == m["consumed"], (name, o["consumed"], m["consumed"])
    assert np.array_equal(o["lattice"], m["lattice"]), name
    assert np.array_equal(o["tile4"], m["tile4"]), name
    assert np.array_equal(o["planes"], m["planes"]), (name, GC.story(name, o["planes"], m["planes"]))


def test_model_remap_is_the_oracles():
    from oracle.pyoracle import palette_remap
    v = np.arange(251, dtype=np.uint8)
    assert np.array_equal(GC.model_remap(v, 250), palette_remap(v, 250))
    assert GC.model_remap(v, 250)[250] == 254 and GC.model_remap(v, 250, "remap_div")[250] == 255


# ---- the claims ---------------------------------------------------------------------------------------------------------------------------------
def _tile_set(name, ci=0):
    c = GC.case(name)
    sx, sy, bm, _ = c["chunks"][ci]
    return {(tx, ty) for _, tx, ty in GC.set_tiles(sx, sy, c["w"], bm)}


@pytest.mark.parametrize("name", GC.INTERP_NAMES)
def test_interpolation_cases_hold_every_tuple_in_isolated_tiles(name):
    c, m = GC.case(name), GC.model(name)
    sx, sy = c["chunks"][0][:2]
    tiles = _tile_set(name)
    assert len(tiles) == 432 and not m["skipped"] and c["remap"] == 0
    for tx, ty in tiles:                                                       # no set neighbour in the 8-neighbourhood: all four corners are free
        assert not {(tx + i, ty + j) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)} & tiles
    assert all(t[4] == 15 for t in m["tiles"]) and m["consumed"] == [432 * 12]
    lat = m["lattice"].reshape(c["h"] // 4 + 1, c["w"] // 4 + 1, 3)
    dx, dy = 1 << (sx - 2), 1 << (sy - 2)
    seen = set()
    for _, _, tx, ty, _, _ in m["tiles"]:
        ly, lx = (ty << sy) >> 2, (tx << sx) >> 2
        for ch in range(3):
            seen.add((int(lat[ly, lx, ch]), int(lat[ly, lx + dx, ch]), int(lat[ly + dy, lx, ch]), int(lat[ly + dy, lx + dx, ch])))
    assert seen == set(GC.interp_tuples()) and len(seen) == 1296
    assert (c["w"], c["h"]) == (44 << sx, 40 << sy) and (name != "interp_16x16" or (c["w"], c["h"]) == (704, 640))


@pytest.mark.parametrize("name", GC.BYTES_NAMES)
def test_bytes_cases_hold_all_256_byte_values(name):
    c = GC.case(name)
    bm = c["chunks"][0][2]
    assert bm.size == 256 and set(bm.tolist()) == set(range(256))
    if name.endswith("_perm"):
        assert np.array_equal(bm, (167 * np.arange(256)) % 256) and not np.array_equal(bm, np.arange(256))
    else:
        assert np.array_equal(bm, np.arange(256))
    assert (c["w"], c["h"]) == GC.BYTES_SIZES[name.split("_")[1]] and not GC.model(name)["skipped"]
    assert GC.model(name)["consumed"][0] == c["chunks"][0][3].size > 0


def test_bytes_cases_cover_every_shape_both_ways():
    assert {n.split("_")[1] for n in GC.BYTES_NAMES} == set(GC.SHAPES) and len(GC.BYTES_NAMES) == 14
    assert max(GC.case(n)["w"] for n in GC.ALL_NAMES) == 1024 and max(GC.case(n)["h"] for n in GC.ALL_NAMES) == 640


def test_word_halves():
    """w = 192: three 64-pixel blocks a row, two bytes a block, so word 1 of the 16x16 bitmap holds block 2 of row 0 and block 0 of row 1.  At
    192 x 128 the bitmap has 12 bytes (six blocks): the size at which it is no multiple of 4 is 192 x 192 (18 bytes), a case of its own."""
    got = set()
    for lo in (0, 1):
        for hi in (0, 1):
            name = f"word_halves_192x128_{lo}{hi}"
            c = GC.case(name)
            sx, sy, bm, _ = c["chunks"][0]
            assert (c["w"], c["h"], sx, sy, bm.size) == (192, 128, 4, 4, 12)
            assert GC.bit_tile(4, 4, 192, 32) == (8, 0) and GC.bit_tile(4, 4, 192, 48) == (0, 4)      # low half: block 2 of row 0; high half: block 0 of row 1
            word1 = int(bm[4:8].view("<u4")[0])
            got.add((word1 & 0xFFFF, word1 >> 16))
            assert bm[:4].all() and bm[8:].all()                                # the neighbouring words are not empty
    assert got == {(0, 0), (0, 0xFFFF), (0xFFFF, 0), (0xFFFF, 0xFFFF)}
    c = GC.case("word_halves_192x192")
    sx, sy, bm, _ = c["chunks"][1]
    assert (sx, sy, bm.size) == (4, 4, 18) and bm.size % 4 == 2 and bm[16] and bm[17] == 0xFF     # the last word: two bytes of bitmap, two behind its end
    assert any(t[0] == 1 and t[1] >= 128 and t[4] for t in GC.model("word_halves_192x192")["tiles"])   # tiles of that word own corners


def test_cap_cases_lie_on_both_sides_of_8192():
    counts = [GC.model(n)["blocks"][0] for n in GC.CAP_NAMES]
    assert counts == [[8385], [8125], [8385, 8256]], counts
    assert 8125 <= 8192 < 8256
    for n in GC.CAP_NAMES:
        assert (GC.case(n)["chunks"][0][2] == 0xFF).all() and GC.case(n)["chunks"][0][2].size % 1024 == 0
    sk = GC.model("cap_under_496x256")["skipped"]
    assert len(sk) == 4 * 64 and all(GC.bit_tile(2, 2, 496, b)[0] * 4 >= 496 for _, b in sk)       # the tiles at x >= 496 are set and skipped
    assert not GC.model("cap_over_512x256")["skipped"]


def test_offsets_case_has_multi_block_passes_that_are_not_first():
    c, m = GC.case("offsets_1024x512"), GC.model("offsets_1024x512")
    assert [GC.shape_name(sx, sy) for sx, sy, _, _ in c["chunks"]] == ["8x4", "4x4", "4x8"]
    assert [len(b) for b in m["blocks"]] == [2, 4, 2]
    late = [ci for ci in (1, 2) if len(m["blocks"][ci]) >= 2 and all(v > 0 for v in m["blocks"][ci])]
    assert late == [1, 2], m["blocks"]                                           # every 1024-byte block of the later passes owns corners
    assert all(raw.size == need for (_, _, _, raw), need in zip(c["chunks"], c["need"]))            # every stream is complete
    assert all(0.4 < np.unpackbits(bm).mean() < 0.6 for _, _, bm, _ in c["chunks"])


def test_reuse_lattice_has_all_15_loaded_subsets():
    m = GC.model("reuse_lattice")
    subsets = set()
    for ci, _, _, _, owned, loaders in m["tiles"]:
        if ci == 1:
            loaded = sum(1 << q for q in range(4) if loaders[q] == 0)
            assert loaded | owned == 15 and not loaded & owned
            subsets.add(loaded)
    assert subsets == set(range(1, 16))
    assert {bin(s).count("1") for s in subsets} == {1, 2, 3, 4}


def test_overlaps_exist_in_both_orders():
    c, m = GC.case("overlap_later_wins"), GC.model("overlap_later_wins")
    shapes = [GC.shape_name(sx, sy) for sx, sy, _, _ in c["chunks"]]
    pairs = {(shapes[a], shapes[b]) for a, b in m["overlaps"]}
    assert {("16x16", "4x4"), ("16x16", "8x4"), ("4x4", "16x16"), ("8x4", "16x16")} <= pairs, pairs
    for name in ("file_order_reversed", "eight_chunks"):
        assert GC.model(name)["overlaps"], name
    assert [GC.shape_name(sx, sy) for sx, sy, _, _ in GC.case("file_order_reversed")["chunks"]] == list(GC.SHAPES)[::-1]
    e = GC.case("eight_chunks")["chunks"]
    assert len(e) == 8 and e[7][:2] == (2, 2) and e[6][:2] == (2, 2) and not np.array_equal(e[6][2], e[7][2]) and GC.model("eight_chunks")["consumed"][7] > 0
    b = GC.case("empty_between")
    assert not b["chunks"][1][2].any() and b["chunks"][1][3].size == 0 and b["chunks"][0][3].size and b["chunks"][2][3].size
    assert len(GC.case("single_chunk")["chunks"]) == 1 and (GC.case("single_chunk")["w"], GC.case("single_chunk")["h"]) == (64, 64)


def test_short_streams():
    for n, cut in (("short_1", 1), ("short_2", 2), ("short_3", 3), ("short_7", 7)):
        c = GC.case(n)
        last = len(c["chunks"]) - 1
        assert c["need"][last] - c["chunks"][last][3].size == cut and all(c["need"][i] == c["chunks"][i][3].size for i in range(last))
        full = GC.model_decode(c, streams=[GC.raw_stream(k, i) for i, k in enumerate(c["need"])])
        assert not np.array_equal(full["planes"], GC.model(n)["planes"]), n     # the missing bytes are seen
    c = GC.case("short_empty")
    assert c["chunks"][1][3].size == 0 and c["need"][1] > 0 and c["chunks"][1][2].any()


def test_edge_cases_set_bits_outside_the_image():
    for name, (w, h) in (("edge_80x48", (80, 48)), ("edge_72x40", (72, 40)), ("edge_8x8", (8, 8))):
        c, m = GC.case(name), GC.model(name)
        assert (c["w"], c["h"]) == (w, h)
        for ci, (sx, sy, bm, _) in enumerate(c["chunks"]):
            outside = [b for b, tx, ty in GC.set_tiles(sx, sy, w, bm) if ((tx + 1) << sx) > w or ((ty + 1) << sy) > h]
            every = [b for b in range(bm.size * 8) if ((GC.bit_tile(sx, sy, w, b)[0] + 1) << sx) > w or ((GC.bit_tile(sx, sy, w, b)[1] + 1) << sy) > h]
            assert outside == every and outside, (name, ci)                     # every tile of the partial swizzle blocks past the edges
            assert [b for k, b in m["skipped"] if k == ci] == outside
    m = GC.model("edge_72x40")
    straddle = [(ci, b) for ci, b in m["skipped"] if ci == 0 and GC.bit_tile(4, 4, 72, b) == (4, 0)]
    assert straddle                                                             # a 16x16 tile whose left half lies inside the image (x = 64 of 72)
    c, m = GC.case("corner_tiles"), GC.model("corner_tiles")
    assert len(c["chunks"]) == 7 and not m["skipped"]
    for ci, (sx, sy, bm, _) in enumerate(c["chunks"]):
        assert {(tx, ty) for _, tx, ty in GC.set_tiles(sx, sy, 96, bm)} == {(0, 0), ((96 >> sx) - 1, 0), (0, (80 >> sy) - 1), ((96 >> sx) - 1, (80 >> sy) - 1)}
    first = [t for t in m["tiles"] if t[0] == 0]
    assert all(t[4] == 15 for t in first)                                       # the last lattice row and column are popped by the first pass ...
    lat = m["lattice"].reshape(21, 25, 3)
    assert lat[20, 24].any() and lat[20, 0].any() and lat[0, 24].any()


def test_batches_share_a_shape_and_differ_in_everything_else():
    for key, names in GC.BATCHES.items():
        cs = [GC.case(n) for n in names]
        assert len(cs) == 3 and len({(c["w"], c["h"]) for c in cs}) == 1
        assert len({tuple(ch[:2] for ch in c["chunks"]) for c in cs}) == 1 and len(cs[0]["chunks"]) <= 7
        for p in range(len(cs[0]["chunks"])):
            assert len({c["chunks"][p][2].tobytes() for c in cs}) > 1, (key, p)
        assert len({tuple(ch[3].size for ch in c["chunks"]) for c in cs}) == 3
        assert len({tuple(sorted(c["short"].items())) for c in cs}) >= 2
    over = [GC.model(n)["blocks"][0][0] for n in GC.BATCHES["b512x256"]]
    assert over[0] > 8192 >= over[1] > 0 and over[2] == 0


# ---- sensitivity: every defect is seen by a named case -------------------------------------------------------------------------------------------
SEES = {
    "pop_order": ("interp_8x8", "bytes_16x16_seq", "single_chunk"),
    "repop": ("bytes_4x4_seq", "reuse_lattice", "cap_over_512x256"),
    "round": ("interp_16x16", "interp_4x4", "interp_8x4"),
    "earlier_wins": ("overlap_later_wins", "file_order_reversed"),
    "edge_consumes": ("edge_80x48", "edge_72x40", "cap_under_496x256"),
    "remap_div": ("bytes_8x8_perm", "single_chunk"),
    "upright": ("bytes_16x16_seq", "bytes_16x8_perm"),
}


@pytest.mark.parametrize("defect", GC.DEFECTS)
def test_every_defect_changes_a_named_case(defect):
    assert set(SEES) == set(GC.DEFECTS)
    for name in SEES[defect]:
        good, bad = GC.model(name), GC.model_decode(GC.case(name), defect=defect)
        assert not (np.array_equal(good["planes"], bad["planes"]) and np.array_equal(good["tile4"], bad["tile4"])), f"{defect} is invisible in {name}"


def test_the_upright_defect_is_blind_outside_two_row_bytes():
    """what makes `upright` a defect of its own: shapes with eight tiles a row never take that branch"""
    good, bad = GC.model("bytes_8x8_seq"), GC.model_decode(GC.case("bytes_8x8_seq"), defect="upright")
    assert np.array_equal(good["planes"], bad["planes"]) and good["consumed"] == bad["consumed"]
