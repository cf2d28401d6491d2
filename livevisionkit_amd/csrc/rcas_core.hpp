// The arithmetic of FSR's robust contrast adaptive sharpening (RCAS; the OpenCL kernel `rcas`, LiveVisionKit/Functions/OpenCL/Sources/FSR.cl:460-535), written
// once for the kernels of sharpen.hip (packed 8UC3 frames), scaling_420.hip (the planes of an I420 / NV12 frame) and scaling_obs.hip (the planes of the
// other OBS video formats): the pixel, its unpacking, the two limiter tables and the rows of a packed frame as a thread of four columns reads them.
//
// Arithmetic contract (must stay in lock-step with the specification the tests check against): binary32 IEEE ops, no implicit contraction, fused
// multiply-adds exactly where written as fma(), native_recip = v_rcp_f32 as in the reference's compiled kernel (see fill_tables), min/max with fmin/fmax
// semantics (a NaN operand loses), truncating byte conversion.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rcas {

constexpr int RCAS_PXT = 4, RCAS_STRIP_W = 64 * RCAS_PXT;

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ float min_(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ float max_(float a, float b) { return __builtin_fmaxf(a, b); }

struct __attribute__((packed, aligned(1))) U12B { uint32_t w[3]; };
struct __attribute__((packed, aligned(1))) U4B { uint32_t w; };

struct Px { float c[3]; };

__device__ __forceinline__ Px unpack(uint32_t lo_bytes)
{
    const float norm_factor = 0.00392156862f;               // FSR.cl:484
    Px r;
    r.c[0] = (float)(lo_bytes & 0xffu) * norm_factor;
    r.c[1] = (float)((lo_bytes >> 8) & 0xffu) * norm_factor;
    r.c[2] = (float)((lo_bytes >> 16) & 0xffu) * norm_factor;
    return r;
}

// One source row as a thread sees it: the pixel left of its four, its four, and the pixel right of them.
struct RawRow { uint32_t w0, w1, w2, wl, wr; };
struct Row { Px p[RCAS_PXT + 2]; };

// Unconditional loads (no branches, so that all rows of a thread are in flight together): the row index is clamped into the image
// and the two side loads fall back to in-row addresses at the frame edge -- whatever they return there belongs to border pixels,
// which are copied.  Requires x0 + 4 <= cols.
__device__ __forceinline__ RawRow load_row(const uint8_t* __restrict__ src, int step, int y, int rows, int x0, int cols)
{
    const uint8_t* rp = src + (long)min(max(y, 0), rows - 1) * step + 3 * (long)x0;
    const U12B v = *reinterpret_cast<const U12B*>(rp);
    RawRow r;
    r.w0 = v.w[0]; r.w1 = v.w[1]; r.w2 = v.w[2];
    r.wl = reinterpret_cast<const U4B*>(x0 > 0 ? rp - 4 : rp)->w >> 8;                        // bytes -3..-1
    r.wr = reinterpret_cast<const U4B*>(x0 + RCAS_PXT < cols ? rp + 11 : rp + 8)->w >> 8;     // bytes 12..14
    return r;
}

__device__ __forceinline__ Row unpack_row(const RawRow& r)
{
    Row o;
    o.p[0] = unpack(r.wl);
    o.p[1] = unpack(r.w0);
    o.p[2] = unpack((r.w0 >> 24) | (r.w1 << 8));
    o.p[3] = unpack((r.w1 >> 16) | (r.w2 << 16));
    o.p[4] = unpack(r.w2 >> 8);
    o.p[5] = unpack(r.wr);
    return o;
}

// The limiter reciprocals of the 256 possible ring extrema (FSR.cl:513-518, "these need to be high precision RCPs"), one entry per thread of a
// 256-thread block; the caller synchronises the block before it reads them.
__device__ __forceinline__ void fill_tables(float* __restrict__ s_rmin, float* __restrict__ s_rmax)
{
    const float v = (float)threadIdx.x * 0.00392156862f;
    // What the reference's kernel computes when it is compiled for this device: LLVM folds `-hitMin` into
    // min * (-1.0f / (4 mx4)), a correctly rounded divide; the hitMax reciprocal stays the device's v_rcp_f32.
    s_rmin[threadIdx.x] = 1.0f / (4.0f * v);                                   // native_recip(4 * mx4), negation folded in
    s_rmax[threadIdx.x] = __builtin_amdgcn_rcpf(fma_(4.0f, v, -4.0f));         // native_recip(4 * mn4 + peakC.y)
}

// FSR.cl:486-534 for one pixel: b above, h below, d left, f right, e centre.  Returns 0x00ZZYYXX.
__device__ __forceinline__ uint32_t rcas_pixel(const Px& b, const Px& d, const Px& e, const Px& f, const Px& h, float sharp,
                                               const float* __restrict__ s_rmin, const float* __restrict__ s_rmax)
{
    float lobe_c[3];
#pragma unroll
    for (int c = 0; c < 3; c++)                              // FSR.cl:503-521
    {
        const float mn4 = min_(b.c[c], min_(d.c[c], min_(f.c[c], h.c[c])));
        const float mx4 = max_(b.c[c], max_(d.c[c], max_(f.c[c], h.c[c])));
        // Byte offset 4 k of an extremum k * norm_factor in the tables, without a conversion or a left shift (both half-rate VALU
        // classes on gfx950, scripts/valu_peak.hip): 1020 (k norm) + 2 = 4 k + 2 - 8e-9 k, and adding 2^23 leaves that integer,
        // rounded to 4 k + 2 for every k in 0..255, in the low mantissa bits.
        const uint32_t omx = __float_as_uint(fma_(mx4, 1020.0f, 8388610.0f)) & 0x3fcu;
        const uint32_t omn = __float_as_uint(fma_(mn4, 1020.0f, 8388610.0f)) & 0x3fcu;
        const float hitMin = min_(mn4, e.c[c]) * *reinterpret_cast<const float*>(reinterpret_cast<const char*>(s_rmin) + omx);
        const float hitMax = (1.0f - max_(mx4, e.c[c])) * *reinterpret_cast<const float*>(reinterpret_cast<const char*>(s_rmax) + omn);
        lobe_c[c] = max_(-hitMin, hitMax);
    }
    const float lobe = min_(max_(max_(lobe_c[2], max_(lobe_c[1], lobe_c[0])), -0.1875f), 0.0f) * sharp;   // FSR.cl:525
    const float a = fma_(4.0f, lobe, 1.0f);                  // FSR.cl:528, APrxMedRcpF1 (FSR.cl:70)
    const float rb = __uint_as_float(0x7ef19fffu - __float_as_uint(a));
    const float rcpL = rb * fma_(-rb, a, 2.0f);
    uint32_t px = 0;
#pragma unroll
    for (int c = 0; c < 3; c++)                              // FSR.cl:529-531
    {
        const float v = fma_(((b.c[c] + d.c[c]) + h.c[c]) + f.c[c], lobe, e.c[c]) * rcpL;
        px |= ((uint32_t)(int)(v * 255.0f) & 0xffu) << (8 * c);
    }
    return px;
}

__device__ __forceinline__ uint32_t load_px_raw(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

} // namespace rcas
