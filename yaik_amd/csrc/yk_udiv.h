// Division of a small unsigned number by a divisor that stays the same for a whole launch, as one multiplication and one shift.
// The host computes the pair when the image or the batch is set (yk_udiv_make); the fused encode kernel, whose every wave used to run
// the runtime's integer division for its unit decode, then needs s_mul_hi_u32 and a shift (yk_udiv).  Plain C++: host, device and the
// CPU-only check (yaik_amd/host/udiv_tool.cpp) share this file.
//
//   q = ((2 n + 1) * mul) >> (32 + shift),   shift = floor(log2 d),   mul = ceil(2^(31 + shift) / d)   (2^30 < mul <= 2^31)
//
// Exactness.  Write mul * d = 2^(31 + shift) + e with 0 <= e < d.  Then (2 n + 1) * mul / 2^(32 + shift)
//   = (2 n + 1) / (2 d) + (2 n + 1) e / (d 2^(32 + shift)).
// The first term is n / d + 1 / (2 d): it has the floor of n / d and stays at least 1 / (2 d) below the next integer.  The second term is
// smaller than that margin when (2 n + 1) e < 2^(31 + shift); e < d < 2^(shift + 1) makes (2 n + 1) < 2^30 sufficient.  So the quotient
// is exact for EVERY divisor d >= 1 and every n < YK_UDIV_LIMIT = 2^29, and 2 n + 1 does not overflow 32 bits.
// (The doubled numerator is what lets d = 1 through: ceil(2^32 / 1) would not fit a 32-bit multiplier.)
#pragma once
#include <cstdint>

#define YK_UDIV_LIMIT (1u << 29)        // numerators below this are divided exactly, whatever the divisor

struct YkUdiv { uint32_t mul, shift; };

inline YkUdiv yk_udiv_make(uint32_t d) {
    YkUdiv r = { 0u, 0u };
    if (d == 0) return r;                                       // no divisor: every quotient 0
    while ((d >> r.shift) > 1u) r.shift++;
    r.mul = (uint32_t)((((uint64_t)1 << (31 + r.shift)) + d - 1) / d);
    return r;
}

#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t yk_udiv(uint32_t n, uint32_t mul, uint32_t shift) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(2u * n + 1u, mul) >> shift;
#else
    return (uint32_t)(((uint64_t)(2u * n + 1u) * mul) >> 32) >> shift;
#endif
}
