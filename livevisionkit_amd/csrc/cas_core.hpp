// The per-channel arithmetic of the CAS filter (FidelityFX CasFilter with CAS_SLOW and CAS_BETTER_DIAGONALS; specification: tests/np_cas.py,
// DESIGN.md section 14), written once for the kernels of cas.hip (packed 3- and 4-channel frames) and cas_gray.hip (one channel), and the byte
// <-> unit conversions they share with the FSR kernels (fsr_core.hpp).  Every operation is rounded on its own (-ffp-contract=off); the fused
// multiply-adds are spelled out.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ffx {

__device__ __forceinline__ float as_f(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t as_u(float f) { return __float_as_uint(f); }

// correctly rounded u / 255: q = u * (1 / 255), then one exact-residual correction (Markstein); checked for all 256 values by
// tests/test_cas_spec.py against the exact rational quotient
__device__ __forceinline__ float unit_of(float u)
{
    const float c = 1.0f / 255.0f;
    const float q = u * c;
    return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, u), c, q);
}

__device__ __forceinline__ float sat(float v) { return __builtin_fminf(__builtin_fmaxf(v, 0.0f), 1.0f); }

// the store of both filters: rint(v * 255) of a v in [0, 1]
__device__ __forceinline__ uint32_t to_byte(float v) { return (uint32_t)rintf(v * 255.0f); }

// One channel of CasFilter: the nine neighbours in the order a b c / d e f / g h i.
__device__ __forceinline__ float cas_channel(float a, float b, float c, float d, float e, float f, float g, float h, float i, float peak)
{
    float mn = __builtin_fminf(__builtin_fminf(d, e), __builtin_fminf(f, __builtin_fminf(b, h)));
    float mx = __builtin_fmaxf(__builtin_fmaxf(d, e), __builtin_fmaxf(f, __builtin_fmaxf(b, h)));
    mn = mn + __builtin_fminf(__builtin_fminf(mn, a), __builtin_fminf(c, __builtin_fminf(g, i)));
    mx = mx + __builtin_fmaxf(__builtin_fmaxf(mx, a), __builtin_fmaxf(c, __builtin_fmaxf(g, i)));
    const float lo_rcp_mx = as_f(0x7ef07ebbu - as_u(mx));
    const float amp = as_f((as_u(sat(__builtin_fminf(mn, 2.0f - mx) * lo_rcp_mx)) >> 1) + 0x1fbc4639u);
    const float w = amp * peak;
    const float wt = 1.0f + 4.0f * w;
    const float r = as_f(0x7ef19fffu - as_u(wt));
    const float med_rcp = r * ((-r) * wt + 2.0f);
    return sat(((((b * w + d * w) + f * w) + h * w) + e) * med_rcp);
}

} // namespace ffx
