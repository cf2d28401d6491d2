// What the units that read or write the planes of an I420 / NV12 frame directly share.  The planes as a kernel argument, the
// description an entry builds once from its C arguments and the host's rules about it are plain C++ in planes420.hpp; here are the device side -- the
// exact 2x chroma up-sampling of the ingest in its closed form, the load of four chroma samples, the store of a thread's luma and chroma samples with
// the flags that choose its wide forms -- and the one out-of-place refusal of the entries (require_out_of_place).
//
// up() is the exact 2x chroma up-sampling of the ingest; its closed form is derived in the comment above k_ingest_yuv420_x2 (ingest.hip) and restated
// here.  For luma column x with c = x / 2 the horizontal sum is t = 3 C[c] + C[f], f = c - 1 for an even x and c + 1 for an odd one; for luma row y
// with k = y / 2 the value is (((3 t_k) >> 2) + (t_g >> 2) + 2) >> 2, g = k - 1 for an even y and k + 1 for an odd one; f and g are clamped to the
// plane (the edge sample replicated, coefficients unchanged).
#pragma once

#include "lvk_hip_internal.hpp"

namespace yuv420 {

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

// which of the wide accesses the planes' bases and pitches allow: the Y input as dwords, the Y output as dwords, the chroma output as one dword
// (NV12) or one 16-bit word per plane (I420)
constexpr int kYInDw = 1, kYOutDw = 2, kChromaWide = 4;

// in: nullptr where the kernel reads no planes
inline int access_flags(const PlaneSet* in, const PlaneSet& out)
{
    const Planes& o = out.p;
    return (in && aligned_to(in->p.y, in->p.ys, 4) ? kYInDw : 0) | (aligned_to(o.y, o.ys, 4) ? kYOutDw : 0)
         | ((out.nv12 ? aligned_to(o.u, o.us, 4) : aligned_to(o.u, o.us, 2) && aligned_to(o.v, o.vs, 2)) ? kChromaWide : 0);
}

// The stores of a thread that owns four luma columns of a row pair (two where `half`: the row's last two columns of a frame with cols % 4 == 2) and
// their chroma samples.  The callers hand the values over as the arrays they hold and the predicate as `half`, not as its negation: in this form the
// helpers inline to the instruction streams the kernels had with the stores written out.
//
// four pixels of a luma row to p, each the low byte of its word (the first two where `half`): one dword where flags has kYOutDw
__device__ __forceinline__ void store_luma4(uint8_t* p, const uint32_t (&y)[4], bool half, int flags)
{
    if (!half && (flags & kYOutDw)) *reinterpret_cast<uint32_t*>(p) = (y[0] & 0xffu) | ((y[1] & 0xffu) << 8) | ((y[2] & 0xffu) << 16) | (y[3] << 24);
    else
    {
        p[0] = (uint8_t)y[0]; p[1] = (uint8_t)y[1];
        if (!half) { p[2] = (uint8_t)y[2]; p[3] = (uint8_t)y[3]; }
    }
}

// the chroma samples (c0, k) = (u[0], v[0]) and (c0 + 1, k) = (u[1], v[1]) (the first alone where `half`): where flags has kChromaWide, NV12 one
// dword and I420 one 16-bit word per plane
template <bool NV12>
__device__ __forceinline__ void store_chroma2(const PlanesOut& out, int k, int c0, const uint32_t (&u)[2], const uint32_t (&v)[2], bool half, int flags)
{
    if constexpr (NV12)
    {
        uint8_t* p = out.u + (size_t)k * out.us + 2 * c0;
        if (!half && (flags & kChromaWide)) *reinterpret_cast<uint32_t*>(p) = u[0] | (v[0] << 8) | (u[1] << 16) | (v[1] << 24);
        else
        {
            p[0] = (uint8_t)u[0]; p[1] = (uint8_t)v[0];
            if (!half) { p[2] = (uint8_t)u[1]; p[3] = (uint8_t)v[1]; }
        }
    }
    else
    {
        uint8_t* pu = out.u + (size_t)k * out.us + c0;
        uint8_t* pv = out.v + (size_t)k * out.vs + c0;
        if (!half && (flags & kChromaWide))
        {
            *reinterpret_cast<uint16_t*>(pu) = (uint16_t)(u[0] | (u[1] << 8));
            *reinterpret_cast<uint16_t*>(pv) = (uint16_t)(v[0] | (v[1] << 8));
        }
        else
        {
            pu[0] = (uint8_t)u[0]; pv[0] = (uint8_t)v[0];
            if (!half) { pu[1] = (uint8_t)u[1]; pv[1] = (uint8_t)v[1]; }
        }
    }
}

// An entry that reads neighbours is out of place: no byte of the `n_in` input spans may be an output byte, and no output byte another plane's
inline int require_out_of_place(lvk_hip_ctx* ctx, const char* name, const Span* in, int n_in, const PlaneSet& out)
{
    const Spans o = spans_of(out);
    if (!clear_of(in, n_in, o)) return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": an output plane overlaps an input (the call is out of place)");
    if (!disjoint(o)) return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": two output planes overlap");
    return LVK_HIP_OK;
}

} // namespace yuv420

// lvk::ScalingFilter on 4:2:0 planes (scaling_420.hip): lvk_hip_scale_yuv420 behind its entry guard, shared with lvk_hip_scale_obs; `name` is the entry's
int lvk_scale_420(lvk_hip_ctx* ctx, const char* name, const yuv420::PlaneSet& src, const yuv420::PlaneSet& dst, float sharpness);

// lvk::CASFilter on 4:2:0 planes (cas_420.hip): lvk_hip_cas_yuv420 behind its entry guard, shared with lvk_hip_cas_obs; `name` is the entry's
int lvk_cas_420(lvk_hip_ctx* ctx, const char* name, const yuv420::PlaneSet& src, const yuv420::PlaneSet& dst, float sharpness);

// lvk::FSRFilter on 4:2:0 planes (fsr_420.hip): lvk_hip_fsr_yuv420 behind its entry guard, shared with lvk_hip_fsr_obs; `name` is the entry's
int lvk_fsr_420(lvk_hip_ctx* ctx, const char* name, const yuv420::PlaneSet& src, const int region_xywh[4], const yuv420::PlaneSet& dst);
