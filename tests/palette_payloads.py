"""Hand-made 'GTIL' colour payloads for the PaletteDecompressor tests (tests/test_palette_decode_layout.py on the CPU, tests/test_gpu_palette_decode.py
on the GPU): a builder of token streams, the corpus of valid and malformed payloads, and the oracle's verdict on a payload.  The oracle
(pyoracle.palette_decompress) decides what a payload decodes to and whether it is accepted; `valid` below is what the corpus EXPECTS, and the CPU
test asserts that the oracle agrees on every single item.

CB and CC are the chunk sizes of yaik_amd/csrc/yk_palette_dec.hip (PD_CB token bytes, PD_CC colours); token-byte chunks are counted from the first
token byte, hdr = 1 + 3 * codeBookSize + 3."""
from typing import NamedTuple

import numpy as np

CB = 64
CC = 1024
COLOUR_COUNTS = [1, 2, 3, 64, 65, 66, 67, CC - 1, CC, CC + 1, CC + 64, CC + 65, 4 * CC + 1]
HEADER_ONLY = np.array([0, 10, 20, 30], np.uint8)       # codeBookSize 0 and the first colour: every further colour is a code token 0 from the zero slack


class Item(NamedTuple):
    name: str
    payload: np.ndarray
    out_bytes: int
    valid: bool


class Builder:
    """A payload under construction: header (codeBookSize, rows, first colour) and tokens.  `colours` counts what the tokens wrote so far."""

    def __init__(self, rows, first=(0, 0, 0), code_book_size=None):
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3) & 255
        self.cbs = len(rows) if code_book_size is None else code_book_size
        self.b = [self.cbs] + rows.reshape(-1).tolist() + [int(v) & 255 for v in first]
        self.hdr = len(self.b)
        self.colours = 1

    def __len__(self):
        return len(self.b)

    def code(self, idx):
        assert 0 <= idx < 128
        self.b.append(idx); self.colours += 1
        return self

    def back(self, d):
        assert 0 <= d < 64
        self.b.append(0xC0 | d)
        return self

    def explicit(self, absolute, mask, values):
        assert 0 <= mask < 8 and len(values) == bin(mask).count("1")
        self.b += [(0x88 if absolute else 0x80) | mask] + [int(v) & 255 for v in values]
        self.colours += 1
        return self

    def raw(self, *bytes_):
        self.b += [int(v) & 255 for v in bytes_]
        return self

    def payload(self):
        return np.array(self.b, dtype=np.uint8)

    def item(self, name, valid=True, colours=None):
        return Item(name, self.payload(), 3 * (self.colours if colours is None else colours), valid)


def _rows(rng, n):
    return rng.integers(0, 256, size=(n, 3))


def random_stream(colours, seed, rows=None):
    """A valid stream of `colours` colours that mixes every token kind: codes (also indices beyond the book), both explicit kinds with every mask,
    back-references (single, stacked twice and three times) in front of any writing token."""
    rng = np.random.default_rng(seed)
    b = Builder(_rows(rng, int(rng.integers(0, 24)) if rows is None else rows), rng.integers(0, 256, 3))
    while b.colours < colours:
        n = b.colours
        if n >= 2 and rng.random() < 0.3:
            for _ in range(int(rng.integers(1, 4))):
                b.back(int(rng.integers(0, min(63, n - 2) + 1)))
        k = rng.random()
        if k < 0.5:
            b.code(int(rng.integers(0, 128)) if rng.random() < 0.1 else int(rng.integers(0, min(max(b.cbs, 1), 128))))
        else:
            mask = int(rng.integers(0, 8))
            b.explicit(k < 0.7, mask, rng.integers(0, 256, bin(mask).count("1")))
    return b


def _distinct_head(b, n, rng):
    for _ in range(n - b.colours):
        b.explicit(True, 7, rng.integers(0, 256, 3))


def valid_items():
    out = []
    rng = np.random.default_rng(1)
    # both explicit kinds with every mask, wrap-around included (0xF0 + 0x20, 0x10 + 0xF0)
    for absolute in (False, True):
        b = Builder(_rows(rng, 3), (0xF0, 0x10, 0x80))
        for mask in range(1, 8):
            for v in (0x20, 0xF0, 0xFF, 0x01, 0x80):
                b.explicit(absolute, mask, [v] * bin(mask).count("1"))
            b.code(1)
        out.append(b.item("explicit_abs" if absolute else "explicit_delta"))
    # back-references: every distance, stacked, in front of each explicit kind, reaching exactly colour 0
    b = Builder(_rows(rng, 5), (1, 2, 3))
    _distinct_head(b, 70, rng)
    for d in range(64):
        b.back(d).code(d % 5)
    out.append(b.item("backref_every_distance"))
    b = Builder(_rows(rng, 5), (9, 8, 7))
    _distinct_head(b, 40, rng)
    b.back(3).back(30).code(2)
    b.back(3).back(30).back(7).code(4)
    b.back(11).explicit(False, 5, [3, 250]).back(12).explicit(True, 2, [77]).back(0).explicit(False, 0, []).back(5).explicit(True, 0, [])
    out.append(b.item("backref_stacked_and_before_explicit"))
    for n in (1, 2, 30, 65):                               # colour n refers to colour 0: d + 2 == n
        if n == 1:
            continue                                        # d + 2 >= 2: colour 1 cannot name colour 0 by a back-reference (it is its default parent)
        b = Builder(_rows(rng, 4), (200, 100, 50))
        _distinct_head(b, n, rng)
        b.back(n - 2).code(1).back(min(b.colours - 2, 63)).explicit(False, 7, [1, 2, 3])
        out.append(b.item(f"backref_to_colour0_at_{n}"))
    # code indices from codeBookSize up to 127 read token bytes, and slack near the end of a short payload
    b = Builder(_rows(rng, 4), (5, 6, 7))
    for idx in range(4, 128):
        b.code(idx)
    out.append(b.item("codes_beyond_the_book_long"))
    b = Builder(_rows(rng, 2), (5, 6, 7))
    for idx in (2, 3, 4, 5, 127, 100, 9, 8):
        b.code(idx)
    out.append(b.item("codes_beyond_the_book_into_slack"))
    for cbs in (0, 1, 128, 255):
        b = random_stream(90, 40 + cbs, rows=cbs)
        out.append(b.item(f"codebook_{cbs}"))
    for n in COLOUR_COUNTS:
        out.append(random_stream(n, 100 + n).item(f"colours_{n}"))
    # a 4-byte token at each of its four alignments across the first, second and last chunk boundary (boundaries lie at hdr + k * CB)
    for k, total in ((1, 5), (2, 5), (4, 5)):
        for a in range(4):
            b = Builder(_rows(rng, 2), (50, 60, 70))
            while len(b) < b.hdr + k * CB - a:
                b.code(len(b) & 1)
            assert len(b) == b.hdr + k * CB - a
            b.explicit(True, 7, [k, a, 99])
            while len(b) < b.hdr + total * CB - CB // 2:
                b.code(1) if len(b) % 7 else b.explicit(False, 3, [2, 3])
            out.append(b.item(f"straddle_boundary{k}_align{a}"))
    # dependency shapes
    b = Builder([(1, 255, 3), (0, 2, 250), (7, 7, 7)], (10, 20, 30))
    for i in range(4999):
        b.code(i % 3)
    out.append(b.item("one_chain_5000"))
    b = Builder(_rows(rng, 6), (1, 1, 1))
    _distinct_head(b, 65, rng)
    for i in range(3 * CC - 65):
        b.back(63).code(i % 6)
    out.append(b.item("65_interleaved_chains"))
    b = Builder(_rows(rng, 6), (3, 2, 1))
    roots = {CC // 3: 1, 2 * (CC // 3) + 5: 2, CC + 17: 4, CC + 17 + CC // 3: 1, 2 * CC + 3: 2, 2 * CC + 3 + CC // 3: 4}
    while b.colours < 3 * CC:
        n = b.colours
        if n in roots:
            b.explicit(True, roots[n], [n & 255])
        elif n % 5 == 0:
            b.explicit(False, 1 + n % 7, [n] * bin(1 + n % 7).count("1"))
        else:
            b.code(n % 6)
    out.append(b.item("channel_roots"))
    # long runs of back-references: whole chunks of them, runs that end exactly on, one before and one behind a chunk boundary; the LAST one names
    # the parent, every one is checked
    b = Builder(_rows(rng, 5), (4, 5, 6))
    _distinct_head(b, 70, rng)
    for run in (CB - 1, CB, CB + 1, 4 * CB + 3, 300, 2 * CB, 7):
        for i in range(run):
            b.back(int(rng.integers(0, 64)))
        b.code(run % 5) if run % 2 else b.explicit(False, 7, [run, 2, 3])
    while (len(b) - b.hdr) % CB:                                           # a run that starts exactly at a chunk boundary and fills two chunks
        b.code(1)
    for i in range(2 * CB):
        b.back(i % 64)
    b.code(3)
    out.append(b.item("backref_long_runs"))
    b = Builder(_rows(rng, 3), (7, 7, 7))
    _distinct_head(b, 12, rng)
    for i in range(5000):                                                   # the largest distance the run may name at colour 12 is d = 10
        b.back(i % 11)
    b.code(2)
    out.append(b.item("backref_run_5000_all_within_reach"))
    # malformed bytes BEHIND the token that writes the last colour are never looked at
    b = random_stream(20, 7).raw(0x90)
    out.append(b.item("extension_one_beyond"))
    b = random_stream(5, 8).back(40).code(0)
    out.append(b.item("backref_before_0_one_beyond", colours=5))
    b = Builder(_rows(rng, 5), (1, 2, 3))
    out.append(Item("header_exactly_fits", b.payload()[:16], 3 * 9, True))      # 1 + 3 * 5 == n: the first colour and all tokens are slack
    out.append(Item("header_only_2", HEADER_ONLY, 3 * 2, True))
    out.append(Item("header_only_385", HEADER_ONLY, 3 * 385, True))
    return out


def malformed_items():
    """The first token can be an extension code or a back-reference before colour 0; it cannot be out of input: a payload that passes the header check
    has hdr = 4 + 3 * codeBookSize <= n + 3 < n + 385."""
    out = []
    rng = np.random.default_rng(2)
    b = Builder(_rows(rng, 5), (1, 2, 3))
    out.append(Item("header_too_long_by_1", b.payload()[:15], 3 * 4, False))
    out.append(Item("header_255_in_4_bytes", np.array([255, 1, 2, 3], np.uint8), 3, False))
    for ext in (0x90, 0x97, 0x98, 0xA0, 0xBF):
        out.append(Builder(_rows(rng, 3), (4, 4, 4)).raw(ext, 1, 2, 3).item(f"extension_{ext:02x}_first_token", False, colours=2))
    b = random_stream(50, 9).raw(0xB0)
    out.append(b.item("extension_at_last_colour", False, colours=51))
    b = random_stream(50, 10).back(3).raw(0x91)
    out.append(b.item("extension_behind_backref_at_last_colour", False, colours=51))
    out.append(Builder(_rows(rng, 3), (4, 4, 4)).back(0).code(0).item("backref_before_0_first_token", False))
    b = random_stream(10, 11).back(20).code(0)
    out.append(b.item("backref_before_0_at_last_colour", False))
    b = random_stream(10, 12).back(20).back(3).code(0)                     # every stacked back-reference is checked, not only the last
    out.append(b.item("backref_before_0_stacked_under_a_good_one", False))
    for where in (0, 1, CB, 2500, 4999):                                    # one back-reference too far, anywhere in a run of 5000 good ones
        b = Builder(_rows(rng, 3), (7, 7, 7))
        _distinct_head(b, 12, rng)
        for i in range(5000):
            b.back(11 if i == where else i % 11)
        b.code(2)
        out.append(b.item(f"backref_before_0_at_{where}_of_a_run_of_5000", False))
    b = random_stream(2 * CC + 10, 13)
    b.back(5).code(0)
    bad = b.payload().copy()
    out.append(Item("backref_fine_far_in", bad, 3 * b.colours, True))       # the same shape deep in a stream is fine ...
    out.append(Item("input_exhausted_long", b.payload(), 3 * (b.colours + 400), False))     # ... and 400 colours more than tokens + slack can give
    return out


def corpus():
    return valid_items() + malformed_items()


def oracle_decode(payload, out_bytes, remap_range=250):
    """(accepted, bytes) by the CPU oracle.  remap_range 0 = the bytes as decoded: PaletteFullRangeRemapping(255) multiplies by exactly 1."""
    from oracle.pyoracle import palette_decompress
    try:
        return True, palette_decompress(payload, out_bytes, 255 if remap_range == 0 else remap_range)
    except RuntimeError:
        return False, None


def truncation_boundary():
    """The largest colour count the oracle accepts for HEADER_ONLY (every colour beyond the first is a code token read from the zero slack)."""
    n = 385
    assert oracle_decode(HEADER_ONLY, 3 * n)[0]
    while oracle_decode(HEADER_ONLY, 3 * (n + 1))[0]:
        n += 1
        assert n < 400
    return n
