"""numpy restatement of yk_decode_compare_* (include/yaik_hip.h): decoded pixels against source pixels, everything in int64.

compare(dec, src) takes two [h, w, C] arrays (C = 3 or 4, any integer dtype, samples 0..255) and returns the four statistics per channel plus
the 8x8 tile map: {"sse": [C], "sad": [C], "n_diff": [C], "max_abs": [C], "n_samples": h * w, "tile_sse": int64 [h/8, w/8]} -- tile_sse is the
SSE over all C channels of every 8x8 tile, row-major.  Written from the definitions, sharing nothing with the kernels."""
import numpy as np


def compare(dec: np.ndarray, src: np.ndarray) -> dict:
    dec, src = np.asarray(dec).astype(np.int64), np.asarray(src).astype(np.int64)
    if dec.shape != src.shape or dec.ndim != 3 or dec.shape[2] not in (3, 4) or dec.shape[0] % 8 or dec.shape[1] % 8:
        raise ValueError(f"two [h, w, C] arrays with C = 3 or 4 and sides that are multiples of 8 expected, got {dec.shape} and {src.shape}")
    h, w, c = dec.shape
    d = dec - src
    sq = d * d
    return {
        "sse": [int(sq[:, :, k].sum()) for k in range(c)],
        "sad": [int(np.abs(d[:, :, k]).sum()) for k in range(c)],
        "n_diff": [int(np.count_nonzero(d[:, :, k])) for k in range(c)],
        "max_abs": [int(np.abs(d[:, :, k]).max()) for k in range(c)],
        "n_samples": h * w,
        "tile_sse": sq.reshape(h // 8, 8, w // 8, 8, c).sum(axis=(1, 3, 4)),
    }
