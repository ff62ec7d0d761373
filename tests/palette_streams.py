"""Hand-made colour streams for the PaletteCompressor tests (tests/test_palette_layout.py on the CPU, tests/test_gpu_palette.py on the GPU), the
oracle's payloads for them, and a reader of the payload that counts token kinds.  Streams are uint8 arrays of 3 bytes per colour."""
import numpy as np

WG = 256                                            # colours per workgroup of yk_palette.hip
LENGTHS = [1, 2, 3, 63, 64, 65, 66, 67, 127, 128, 129, WG - 1, WG, WG + 1, WG + 64, WG + 65, 4 * WG - 1, 4 * WG + 1]


def _u8(a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.uint8)


def constant(n, colour=(17, 200, 3)):
    return _u8(np.tile(np.array(colour, np.int64), (n, 1)))


def ramp(n):
    k = np.arange(n, dtype=np.int64)
    return _u8(np.stack([k % 251, (k // 2) % 251, (k // 3) % 251], axis=1))


def ramp_noise(n, seed=1):
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.int64)
    base = np.stack([(k // 4) % 240, (k // 8) % 240, (k // 16) % 240], axis=1) + 4
    return _u8(base + rng.integers(-3, 4, size=(n, 3)))


def noise(n, seed=2, hi=251):
    return _u8(np.random.default_rng(seed).integers(0, hi, size=(n, 3)))


def alternating(n):
    return _u8(np.array([(10, 20, 30), (200, 100, 0)], np.int64)[np.arange(n) % 2])


def channel_noise(n, mask, seed=3):
    """only the channels of `mask` change, by anything in -255..255: explicit tokens of that mask, both kinds"""
    v = np.random.default_rng(seed + mask).integers(0, 256, size=(n, 3))
    for c in range(3):
        if not (mask >> c) & 1:
            v[:, c] = 77
    return _u8(v)


def explicit_masks(mask, seed=4):
    """300 colours of noise in the channels NOT in `mask` fill rows 1..63 (one vote each: registration order), then 20 colours that change only
    the channels of `mask`, by more than 127 and by a different amount every time: absolute explicit tokens of exactly that mask."""
    rng = np.random.default_rng(seed + mask)
    head = np.full((300, 3), 90, np.int64)
    k = np.arange(20)
    seq = np.where(k % 2 == 0, 5 * (k // 2), 200 + 5 * (k // 2) + (k // 2) % 3)
    tail = np.full((20, 3), 90, np.int64)
    for c in range(3):
        if (mask >> c) & 1:
            tail[:, c] = seq + c
        else:
            head[:, c] = rng.integers(0, 256, size=300)
    return _u8(np.concatenate([head, tail]))


def periodic(period, n=None):
    """Colours repeat with `period`; inside a period they are distinct and alternate between two distant clusters, so that the nearest earlier
    colour is rarely the one just before: from the second period on a colour is reached by the zero delta from `period` colours back."""
    k = np.arange(period, dtype=np.int64)
    a = np.stack([10 + (k * 7) % 49, 20 + (k * 11) % 50, 30 + (k * 13) % 51], axis=1)
    b = np.stack([240 - (k * 7) % 49, 230 - (k * 11) % 50, 220 - (k * 13) % 51], axis=1)
    cols = np.where((k % 2 == 0)[:, None], a, b)
    assert len({tuple(c) for c in cols.tolist()}) == period
    n = n or 3 * period + 5
    return _u8(cols[np.arange(n) % period])


def vote_tie(swap=False):
    """(5,0,0) and (0,7,0) get two votes each: registration order decides their rows"""
    d = [(0, 7, 0), (5, 0, 0)] if swap else [(5, 0, 0), (0, 7, 0)]
    c, out = np.array([10, 10, 10]), []
    out.append(c.copy())
    for k in range(4):
        c = c + np.array(d[k % 2]); out.append(c.copy())
    return _u8(out)


def equal_minima():
    """colour 2 is equally far from colours 0 and 1: the first wins, so (5,0,0) is voted and (-5,0,0) is not"""
    return _u8([(10, 10, 10), (20, 10, 10), (15, 10, 10), (60, 90, 10), (65, 90, 10), (70, 90, 10)])


def _oracle():
    from oracle.pyoracle import OracleEncoder
    return OracleEncoder(np.zeros((3, 8, 8), np.int32))


def oracle_payloads(streams, chain, enc=None):
    """PaletteCompressor of the CPU oracle over the streams in order.  chain = K > 0: a fresh oracle encoder per run of K streams; chain = 0: one
    encoder (the caller's `enc`, to continue across calls).  Empty streams are skipped and give an empty payload."""
    out = []
    for i, s in enumerate(streams):
        if chain > 0 and i % chain == 0:
            enc = _oracle()
        elif enc is None:
            enc = _oracle()
        out.append(enc.palette_compress(s).copy() if s.size else np.zeros(0, np.uint8))
    return out


def book_rows(payload):
    """the header's rows as signed triples (only unambiguous while every delta lies in -128..127)"""
    fc = int(payload[0])
    return payload[1:1 + 3 * fc].astype(np.int8).astype(np.int64).reshape(fc, 3)


def stale_pair(seed=5):
    """(A, B, C): A has more than 64 rows (deltas within +-120, so the header shows them exactly).  B has few rows of its own and is built from
    A's book: its colour 1 votes A's row 45 (a CURRENT row of B with a stale duplicate above it: the lower one must win) and later colours sit
    exactly one of A's rows 40..63 behind their predecessor while a nearer colour takes their vote (a hit on a row only the stale part holds).
    C is shorter still: its stale rows come from B and, above those, from A."""
    a = noise(400, seed=seed, hi=121)
    rows = book_rows(oracle_payloads([a], 1)[0])
    assert len(rows) == 128
    base = np.array([128, 128, 128])
    b = [base, base + rows[45]]
    for k in (40, 50, 63, 45):
        s = rows[k]
        assert np.abs(s).sum() > 3
        b += [base + s - np.array([1, 0, 0]), base, base + s]
    c = [base, base + rows[60], base + rows[60] - np.array([0, 1, 0]), base, base + rows[12]]
    return a, _u8(b), _u8(c)


def cases():
    """(name, streams, chain) of every hand-made call"""
    out = []
    for name, mk in (("constant", constant), ("ramp", ramp), ("ramp_noise", ramp_noise), ("noise", noise), ("alternating", alternating)):
        out.append((name, [mk(n) for n in LENGTHS], 1))
    out.append(("channel_noise", [channel_noise(600, m) for m in range(1, 8)], 1))
    out.append(("explicit_masks", [explicit_masks(m) for m in range(1, 7)], 1))
    out.append(("periodic", [periodic(p) for p in range(2, 68)], 1))
    out.append(("ties", [vote_tie(False), vote_tie(True), equal_minima()], 1))
    a, b, c = stale_pair()
    out.append(("stale_chain", [a, b, c], 3))
    out.append(("stale_reset", [a, b, c], 1))
    out.append(("empty_in_chain", [a, np.zeros(0, np.uint8), b, np.zeros(0, np.uint8), c], 5))
    seven = [noise(300, 11), ramp(70), np.zeros(0, np.uint8), ramp_noise(WG + 3, 12), b, constant(5), noise(90, 13)]
    out.append(("two_frames", seven + [ramp_noise(100, 14), a, b, c, alternating(33), np.zeros(0, np.uint8), noise(WG, 15)], 7))
    rng = np.random.default_rng(21)
    short = []
    for r in range(33):
        for p in range(7):
            n = int(rng.integers(0, 40))
            short.append(noise(n, 100 + r * 7 + p, hi=60) if p % 2 else ramp_noise(n, 100 + r * 7 + p))
    out.append(("33_runs_of_7", short, 7))
    return out


def token_kinds(payload, entries):
    """Walks a payload like PaletteDecompressor does and counts what it holds."""
    fc = int(payload[0])
    pos = 1 + 3 * fc + 3
    k = {"code": 0, "backref": 0, "explicit_delta": 0, "explicit_abs": 0, "stale_hit": 0, "rows": fc,
         "distances": set(), "masks_delta": set(), "masks_abs": set()}
    for _ in range(entries - 1):
        b = int(payload[pos]); pos += 1
        if b < 0x80:
            k["code"] += 1
            k["stale_hit"] += b >= fc
        elif b >= 0xC0:
            k["backref"] += 1
            k["distances"].add(b & 0x3F)
            k["stale_hit"] += int(payload[pos]) >= fc
            pos += 1
        else:
            kind, mask = (b >> 3) & 7, b & 7
            assert kind in (0, 1) and mask
            k["explicit_delta" if kind == 0 else "explicit_abs"] += 1
            k["masks_delta" if kind == 0 else "masks_abs"].add(mask)
            pos += bin(mask).count("1")
    assert pos == payload.size, (pos, payload.size)
    return k
