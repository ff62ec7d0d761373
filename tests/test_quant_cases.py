"""The directed inputs of the range quantiser (tests/quant_cases.py) hold what they claim, shown on the CPU from the oracle alone: the model of
the stage equals the oracle on every case, every tile sits in the class and in the context it was built for, the counts the cases promise are
met, and each of a set of wrong pickers disagrees with the oracle somewhere: the cases tell the mistakes apart."""
import collections

import numpy as np
import pytest

from tests import quant_cases as qc


@pytest.mark.parametrize("name", qc.NAMES)
def test_model_equals_the_oracle(oracle_built, name):
    """tile definitions (mode, range, base), index nibbles and their count of the three planes, both start modes"""
    c = qc.case(name)
    ora, _, _ = qc.oracle_state(c["planes"])
    for m3 in (False, True):
        for p in range(3):
            defs, nib, nn, _ = ora.dynamic_tile_encode(p, m3)
            d2, n2, nn2 = c["census"][m3]["streams"][p]
            assert nn2 == nn and defs.size == d2.size, (name, m3, p, "counts", nn2, nn, d2.size, defs.size)
            if not np.array_equal(d2, defs):
                k = int(np.nonzero(d2 != defs)[0][0])
                tile = next(t for t, r in c["census"][m3]["tiles"].items() if t[0] == p and r["k"] == k)
                raise AssertionError((name, m3, "definition", k, "tile", tile, "model", int(d2[k]) >> 13, "oracle", int(defs[k]) >> 13))
            assert np.array_equal(n2, nib), (name, m3, p, "index nibbles")


@pytest.mark.parametrize("name", qc.NAMES)
def test_every_tile_is_what_it_was_built_for(oracle_built, name):
    c = qc.case(name)
    seen = 0
    for m3 in (False, True):
        for t, rec in qc.claims(c, m3):
            assert rec is not None, (name, t["name"], t["tile"], "is not coded")
            assert rec["quads"] == t["quads"] and rec["n"] == 16 * bin(t["quads"]).count("1"), (name, t["name"], t["tile"], "valid cells", rec["quads"], t["quads"])
            if t["flag"] is not None:
                assert t["flag"] in rec["flags"], (name, t["name"], t["tile"], "start mode", 3 if m3 else 0, t["flag"], sorted(rec["flags"]))
            if t["name"] in qc.REGIMES:
                assert (rec["mn"], rec["mx"]) == qc.REGIMES[t["name"]], (name, t["name"], rec["mn"], rec["mx"])
            assert rec["mn"] < 254, "a minimum of 254 or 255 is the reference's out-of-bounds read: not pinned"
            seen += 1
    assert seen >= 1, name


def test_contexts(oracle_built):
    cells = lambda c, y0, y1, x0, x1: int(c["census"][False]["cells"][y0 // 4: y1 // 4, x0 // 4: x1 // 4].sum())
    # (a) strips of whole tiles only; a strip with a partly covered neighbour
    for name in ("full128x64", "noise72x40"):
        c = qc.case(name)
        assert all(r["quads"] == 15 for r in c["census"][False]["tiles"].values()) and c["census"][False]["cells"].all(), name
    c = qc.case("full64x64")
    p = c["image"].partly
    assert c["census"][False]["tiles"][(0,) + p]["quads"] == 7 and sum(r["quads"] != 15 for r in c["census"][False]["tiles"].values()) == 3
    assert {t["tile"][1] for t in c["targets"] if "neighbour" in t["ctx"]} == {p[0]}       # the same tile row, so the same strip
    # (b) one, two (both diagonals, the four halves) and three cells covered, and a covered cell whose value lies outside the valid pixels' range
    parts = collections.Counter()
    for name in ("part72x40_a", "part72x40_b", "part128x64"):
        for t in qc.case(name)["targets"]:
            parts[t["quads"]] += 1
    assert set(parts) == {14, 13, 11, 7, 6, 9, 3, 12, 5, 10, 8, 1}
    t = next(t for t in qc.case("part72x40_b")["targets"] if t["cover"] is not None)
    rec = qc.case("part72x40_b")["census"][True]["tiles"][t["tile"]]
    assert not rec["mn"] <= t["cover"] <= rec["mx"] and (rec["values"][~rec["valid"]] == t["cover"]).all()
    # (c) at most four valid cells in the strip, and five
    counts = set()
    for name in qc.NAMES:
        if name.startswith(("spread", "five")):
            c = qc.case(name)
            n = cells(c, *c["image"].strip)
            assert n == c["image"].cells and n == int(c["census"][False]["cells"].sum()), (name, n)
            assert (n == 5) == name.startswith("five")
            counts.add(n)
    assert counts == {1, 2, 3, 4, 5}
    # (d) the last tile column and row of 72 x 40
    edge = {t["tile"][1:] for t in qc.case("noise72x40")["targets"]}
    assert {(ty, 8) for ty in range(5)} | {(4, tx) for tx in range(8)} <= edge
    # (e) a shrunken box and a rejected 16x16 tile beside the tiles
    c = qc.case("rgba64x64")
    assert c["census"][False]["bounds"].tolist() == [16, 16, 64, 64]
    assert not any(t[1] in (4, 5) and t[2] in (4, 5) for t in c["census"][False]["tiles"]) and (0, 4, 3) in c["census"][False]["tiles"]
    # (f) four tiles that need the exact path in ONE plane of ONE wave's strip (64 x 16 pixels): side by side, one above the other, far apart
    c = qc.case("full128x64")
    need = {"order", "float_decides", "tie_diff", "near"}
    for start, names in qc.SERIAL.items():
        tiles = [t["tile"] for t in c["targets"] if t["ctx"].startswith("f: four") and t["start"] == start]
        assert len(tiles) == 4 and all(c["census"][start == 3]["tiles"][t]["flags"] & need for t in tiles), (start, tiles)
        assert len({(p, ty // 2, tx // 8) for p, ty, tx in tiles}) == 1
        assert {(ty % 2, tx % 8) for _, ty, tx in tiles} == {(0, 0), (0, 1), (1, 0), (1, 7)}
    # (g) one tile in all three planes; three planes of one tile in three classes
    for n in qc.TRI_SAME:
        tiles = [t["tile"] for t in c["targets"] if t["name"] == n and "three planes" in t["ctx"]]
        assert len(tiles) == 3 and len({t[1:] for t in tiles}) == 1, n
    ty, tx = c["image"].mixed
    assert len({c["census"][False]["tiles"][(p, ty, tx)]["cls"] for p in range(3)}) == 3


def _classes():
    """{class: {tile name: [contexts]}} over every claim that the census confirms"""
    out = collections.defaultdict(lambda: collections.defaultdict(set))
    for name in qc.NAMES:
        c = qc.case(name)
        for m3 in (False, True):
            for t, rec in qc.claims(c, m3):
                for f in rec["flags"]:
                    key = f if f != "tie_same" else ("tie_same<=7" if rec["mx"] - rec["mn"] <= qc.SHORTCUT_SPAN else "tie_same>7")
                    out[key][t["name"]].add(t["ctx"][0])
    return out


def test_counts(oracle_built):
    cl = _classes()
    for k in sorted(cl):
        print(f"{k}: {len(cl[k])} tiles;", ", ".join(f"{n} [{''.join(sorted(ctx))}]" for n, ctx in sorted(cl[k].items())))
    assert len(cl["tie_diff"]) >= 4 and len(cl["float_decides"]) >= 4
    assert len(cl["near"]) >= 1                                           # the directed search finds them: the class is not empty
    # order pairs: two arrangements of the same values, both coded whole in a case, two different picks by the oracle
    pairs = collections.Counter()
    c = qc.case("full128x64")
    where = {t["name"]: t["tile"] for t in c["targets"]}
    for n in qc.TILES:
        if n.startswith("order_") and n.endswith("a"):
            a, b = qc.TILES[n], qc.TILES[n[:-1] + "b"]
            assert sorted(a["v"]) == sorted(b["v"]) and a["start"] == b["start"]
            m3 = a["start"] == 3
            ra, rb = (c["census"][m3]["tiles"][where[x]] for x in (n, n[:-1] + "b"))
            assert ra["pick"] != rb["pick"] and "order" in ra["flags"] and "order" in rb["flags"], n
            pairs[a["start"]] += 1
    assert pairs[0] >= 2 and pairs[3] >= 2, pairs
    spans = {}
    for n, t in qc.made_tiles().items():
        if t["flag"] == "tie_same":
            r = qc.tile_model(t["v"], qc.valid_of(15), 0)
            spans[n] = r["mx"] - r["mn"]
    assert {0, 1, 7, 8} <= set(spans.values()) and max(spans.values()) > 32
    assert spans["zeros_tie"] > 7 and min(qc.tile("zeros_tie")["v"]) == 0 and min(qc.tile("zeros")["v"]) == 0
    assert set(qc.REGIMES) <= {t["name"] for t in c["targets"]}
    mn_mx = {n: (min(qc.tile(n)["v"]), max(qc.tile(n)["v"])) for n in qc.REGIMES}
    assert mn_mx["hi224"][0] >= 224 and mn_mx["max255"][1] == 255 and mn_mx["max255"][0] <= 253
    assert [mn_mx[n][1] - mn_mx[n][0] for n in ("span_lt16", "span16_31", "span32", "span223")] == [10, 24, 32, 223]


def test_the_cases_separate_the_mistakes(oracle_built):
    """every wrong picker disagrees with the oracle's tile definition on a committed case; the picker built like the kernel's rule agrees everywhere"""
    caught = collections.defaultdict(list)
    for name in qc.NAMES:
        c = qc.case(name)
        for m3 in (False, True):
            for tile, rec in c["census"][m3]["tiles"].items():
                want = rec["model"]["def"]                                 # the oracle's: test_model_equals_the_oracle
                assert qc._def_of(qc.kernel_rule(rec), rec["mn"], rec["mx"]) == want, (name, m3, tile, "the kernel's rule as modelled")
                if rec["cls"] == "sure" and rec["quads"] == 15 and rec["mn"] > 0:
                    continue
                for mutant, fn in qc.MUTANTS.items():
                    if fn(rec) != want:
                        caught[mutant].append((name, 3 if m3 else 0, tile, rec["cls"]))
    for mutant in qc.MUTANTS:
        print(f"{mutant}: caught {len(caught[mutant])} times, first by", caught[mutant][:3])
    missed = [m for m in qc.MUTANTS if not caught[m]]
    assert not missed, ("no committed case catches", missed)
