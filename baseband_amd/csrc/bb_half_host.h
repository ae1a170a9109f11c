// float32 -> float16 / bfloat16 bit patterns, round to nearest even, on the host.
// The ONE place where the 16-bit output types are rounded: the level tables of
// bb_init / bb_get_levels_as and the fill values of a launch go through here;
// the kernels (k_half.h) only move the patterns.  Same results as
// numpy.ndarray.astype(float16) and torch.Tensor.to(bfloat16) for every input
// (overflow -> inf, float16 subnormals, NaN stays NaN).
#pragma once
#include <stdint.h>
#include <string.h>

inline uint16_t bb_f32_to_f16(float x)
{
    uint32_t f; memcpy(&f, &x, 4);
    const uint16_t sgn = (uint16_t)((f & 0x80000000u) >> 16);
    const uint32_t f_exp = f & 0x7f800000u;
    uint32_t f_sig;
    if (f_exp >= 0x47800000u) {                       // |x| >= 2^16, inf or NaN
        if (f_exp == 0x7f800000u && (f & 0x007fffffu)) {
            uint16_t ret = (uint16_t)(0x7c00u + ((f & 0x007fffffu) >> 13));
            if (ret == 0x7c00u) ++ret;                // keep it a NaN
            return (uint16_t)(sgn + ret);
        }
        return (uint16_t)(sgn + 0x7c00u);
    }
    if (f_exp <= 0x38000000u) {                       // |x| < 2^-14: float16 subnormal or zero
        if (f_exp < 0x33000000u) return sgn;          // below half the smallest subnormal
        const uint32_t e = f_exp >> 23;
        f_sig = 0x00800000u + (f & 0x007fffffu);
        const uint32_t shift = 113 - e;               // 1 .. 11; 13 + shift bits are dropped in all
        const uint32_t lost = f_sig & ((1u << shift) - 1);
        f_sig >>= shift;
        // nearest even on the 13 bits below the float16 mantissa, `lost` is sticky
        if ((f_sig & 0x00003fffu) != 0x00001000u || lost) f_sig += 0x00001000u;
        return (uint16_t)(sgn + (f_sig >> 13));
    }
    const uint16_t h_exp = (uint16_t)((f_exp - 0x38000000u) >> 13);
    f_sig = f & 0x007fffffu;
    if ((f_sig & 0x00003fffu) != 0x00001000u) f_sig += 0x00001000u;
    return (uint16_t)(sgn + h_exp + (uint16_t)(f_sig >> 13));   // (a mantissa carry raises the exponent)
}

inline uint16_t bb_f32_to_bf16(float x)
{
    uint32_t f; memcpy(&f, &x, 4);
    if ((f & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;         // NaN
    return (uint16_t)((f + 0x7fffu + ((f >> 16) & 1u)) >> 16);
}
