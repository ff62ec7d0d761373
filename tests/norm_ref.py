"""The reference of the normalised outputs (include/yaik_hip.h) in numpy, on top of the oracle's crop.

For a decoded byte v of channel k:   f = fp32(fp32(v) * scale[k]) + bias[k]    (float32 multiply, then float32 add: two roundings, never an fma)
    float32: f;   float16: f.astype(float16) (IEEE round-to-nearest-even, overflow to inf, subnormals kept);
    bfloat16: integer round-to-nearest-even on the bit pattern of f.
Mirror: [:, ::-1] of the crop.  Every comparison made with these is on BIT PATTERNS (bits()): the arithmetic is fully defined, so the tolerance is
zero.  bfloat16 has no numpy dtype: its values travel as uint16 bit patterns throughout.
"""
import numpy as np

DTYPES = ("float16", "bfloat16", "float32")
ELEM_BYTES = {"float16": 2, "bfloat16": 2, "float32": 4}


def four(v):
    a = np.atleast_1d(np.asarray(v, dtype=np.float32))
    return np.full(4, a[0], np.float32) if a.size == 1 else a.astype(np.float32)


def _imagenet():
    from yaik_amd.encoder import norm_params
    mean = np.array([0.485, 0.456, 0.406, 0.5], np.float64) * 255
    std = np.array([0.229, 0.224, 0.225, 0.25], np.float64) * 255
    return norm_params(mean, std)


def parameter_sets() -> dict:
    """name -> (scale[4], bias[4]) float32: the sets A..G of the tests"""
    sb = _imagenet()
    return {
        "A": (four(1 / 255), four(0)),                # the plain unit range
        "B": (sb[0], sb[1]),                          # norm_params of the ImageNet means and stds x 255, (0.5, 0.25) x 255 for alpha: fused != unfused
        "C": (four(1), four(0)),                      # the bytes themselves
        "D": (four(2.0 ** -20), four(0)),             # fp16 subnormals
        "E": (four(300), four(0)),                    # fp16 goes to inf from v = 219
        "F": (four(1), four(0.5)),                    # every v >= 128 is a bf16 tie, both parities
        "G": (four(1), four(0.0625)),                 # every v >= 128 is an fp16 tie
    }


def affine_f32(v, scale, bias):
    """float32 array of v's shape [..., C]: the two-rounding result"""
    c = v.shape[-1]
    m = v.astype(np.float32) * four(scale)[:c]        # float32 * float32 -> float32, rounded once
    return (m + four(bias)[:c]).astype(np.float32)    # and once more


def affine_fused_f32(v, scale, bias):
    """what a contracted fma would give: one rounding of the exact v * scale + bias (exact in float64: a 24-bit by 8-bit product and one add)"""
    c = v.shape[-1]
    return (v.astype(np.float64) * four(scale)[:c].astype(np.float64) + four(bias)[:c].astype(np.float64)).astype(np.float32)


def bf16_bits(f32):
    """uint16 bit patterns of round-to-nearest-even(f32) in bfloat16 (no NaN input here)"""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def convert_bits(f32, dtype: str):
    """the bit patterns (uint16 / uint32) of f32 stored as `dtype`"""
    if dtype == "float32":
        return np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(f32.astype(np.float16)).view(np.uint16)
    if dtype == "bfloat16":
        return bf16_bits(f32)
    raise ValueError(dtype)


def norm_ref(pixels, dtype: str, scale, bias, mirror=False):
    """bit patterns [h, w, C] of the normalised output of uint8 pixels [h, w, C] (the oracle's crop, alpha as channel 3)"""
    p = pixels[:, ::-1] if mirror else pixels
    return convert_bits(affine_f32(np.ascontiguousarray(p), scale, bias), dtype)


def bits(t):
    """a torch tensor of float16 / bfloat16 / float32 as its numpy bit patterns (uint16 / uint32)"""
    import torch
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)
