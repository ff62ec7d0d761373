"""Round-trip quality figures: the host side of yk_decode_compare_* (include/yaik_hip.h).

The GPU returns exact integers per frame and channel (yk_quality: sse, sad, nDiff, maxAbs over nSamples = w * h samples); this module mirrors the
struct, turns it into a dict and computes PSNR.  Pure host code: no GPU, no torch.
"""
from __future__ import annotations

import ctypes as C
import math

CHANNEL_NAMES = ("r", "g", "b", "a")
PEAK = 255


class YkQuality(C.Structure):
    """yk_quality of include/yaik_hip.h"""
    _fields_ = [("sse", C.c_uint64 * 4), ("sad", C.c_uint64 * 4), ("nDiff", C.c_uint64 * 4), ("maxAbs", C.c_uint32 * 4), ("nSamples", C.c_uint64)]


def psnr_db(sse: int, n: int) -> float:
    """10 log10(255^2 n / sse) in float64 for a sum of squared errors over n 8-bit samples; inf when sse == 0."""
    sse, n = int(sse), int(n)
    if sse < 0 or n <= 0:
        raise ValueError(f"sse >= 0 and n > 0 expected, got sse = {sse}, n = {n}")
    if sse == 0:
        return math.inf
    return 10.0 * math.log10(float(PEAK * PEAK) * float(n) / float(sse))


def quality_dict(q: YkQuality, channels: int) -> dict:
    """One frame's yk_quality as a dict: sse, sad, n_diff, max_abs and psnr_db are lists of `channels` entries (R, G, B[, A]), n_samples = w * h,
    psnr_db_all the PSNR over all compared samples (the channels' sse summed, channels * n_samples samples)."""
    if channels not in (3, 4):
        raise ValueError(f"channels must be 3 or 4, got {channels}")
    n = int(q.nSamples)
    sse = [int(q.sse[k]) for k in range(channels)]
    return {
        "channels": channels,
        "n_samples": n,
        "sse": sse,
        "sad": [int(q.sad[k]) for k in range(channels)],
        "n_diff": [int(q.nDiff[k]) for k in range(channels)],
        "max_abs": [int(q.maxAbs[k]) for k in range(channels)],
        "psnr_db": [psnr_db(s, n) for s in sse],
        "psnr_db_all": psnr_db(sum(sse), n * channels),
    }
