// What the kernels that read the planes of an I420 / NV12 frame directly share (deblock_420.hip, scaling_420.hip): the planes as kernel arguments, the
// exact 2x chroma up-sampling of the ingest in its closed form, the load of four chroma samples, and the host's checks of plane ranges and alignment.
//
// up() is the exact 2x chroma up-sampling of the ingest; its closed form is derived in the comment above k_ingest_yuv420_x2 (ingest.hip) and restated
// here.  For luma column x with c = x / 2 the horizontal sum is t = 3 C[c] + C[f], f = c - 1 for an even x and c + 1 for an odd one; for luma row y
// with k = y / 2 the value is (((3 t_k) >> 2) + (t_g >> 2) + 2) >> 2, g = k - 1 for an even y and k + 1 for an odd one; f and g are clamped to the
// plane (the edge sample replicated, coefficients unchanged).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace yuv420 {

struct Planes { const uint8_t* y; const uint8_t* u; const uint8_t* v; int ys, us, vs; };     // NV12: u is the UV plane, v unused
struct PlanesOut { uint8_t* y; uint8_t* u; uint8_t* v; int ys, us, vs; };

__device__ __forceinline__ int up_v(int t_near, int t_far) { return (((3 * t_near) >> 2) + (t_far >> 2) + 2) >> 2; }

struct __attribute__((packed, aligned(1))) P4 { uint32_t w; };
struct __attribute__((packed, aligned(1))) P8 { uint32_t w[2]; };

// chroma columns c0 - 1 .. c0 + 2 of one chroma row, one sample per byte (su: U, sv: V), columns clamped to the plane.  Inside the plane: one
// unaligned dword per plane (NV12: one 8-byte load, de-interleaved with v_perm_b32), as the ingest reads them.
template <bool NV12>
__device__ __forceinline__ void load_chroma4(const uint8_t* __restrict__ urow, const uint8_t* __restrict__ vrow, int c0, int cc, uint32_t& su, uint32_t& sv)
{
    if (c0 >= 1 && c0 + 2 < cc)
    {
        if constexpr (NV12)
        {
            const P8 a = *reinterpret_cast<const P8*>(urow + 2 * (c0 - 1));
            su = __builtin_amdgcn_perm(a.w[1], a.w[0], 0x06040200u); sv = __builtin_amdgcn_perm(a.w[1], a.w[0], 0x07050301u);
        }
        else
        {
            su = reinterpret_cast<const P4*>(urow + c0 - 1)->w;
            sv = reinterpret_cast<const P4*>(vrow + c0 - 1)->w;
        }
        return;
    }
    constexpr int PIX = NV12 ? 2 : 1;
    su = sv = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
    {
        const int c = min(max(c0 - 1 + j, 0), cc - 1);
        su |= (uint32_t)urow[c * PIX] << (8 * j);
        sv |= (uint32_t)(NV12 ? urow[c * PIX + 1] : vrow[c * PIX]) << (8 * j);
    }
}

// [first byte, one past the last byte) of a plane of `prows` rows of `row` bytes at pitch `step`
struct Span { uintptr_t lo, hi; };

inline Span span_of(const void* p, int step, int prows, int row)
{
    const uintptr_t lo = (uintptr_t)p;
    return {lo, lo + (uintptr_t)(prows - 1) * (uintptr_t)step + (uintptr_t)row};
}

inline bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

inline bool aligned_to(const void* p, int step, unsigned a) { return (((uintptr_t)p | (uintptr_t)step) & (a - 1)) == 0; }

} // namespace yuv420
