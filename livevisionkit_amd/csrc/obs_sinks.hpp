// What the units that write the planes of an OBS video format outside 4:2:0 from a kernel share (remap_obs.hip, scaling_obs.hip, deblock_obs.hip, and lens_filter.hip for
// the checks): the per-format plane sinks -- planar or packed 4:2:2, planar 4:4:4, AYUV -- as FrameIngest::to_obs would write the frame (reference:
// Modules/OBS-Plugin/Interop/FrameIngest.cpp:526-557 I4XXIngest, :640-666 P422Ingest, :690-703 P444Ingest), the one format -> sink switch (with_obs_sink) and
// the one check of a frame's output planes (obs_outputs_ok).  A sink takes a thread's four horizontally adjacent packed pixels:
//     sink.store(x0, y, npx, px, active, parity)
#pragma once

#include "remap_core.hpp"
#include "obs_planes.hpp"

namespace {

using namespace obs;

__device__ __forceinline__ uint32_t half_even_u32(uint32_t s) { return (s + ((s >> 1) & 1u)) >> 1; }      // cvRound(s * 0.5f)

// LAYOUT 0: planes Y, U, V (I422 / I42A); 1 YUY2 (Y U Y V); 2 YVYU; 3 UYVY.  A thread holds 4 horizontally adjacent pixels = 2 chroma pairs; the frame's
// width is even, so a thread at the right edge holds 2 or 4.
template <int LAYOUT>
struct Sink422
{
    uint8_t* __restrict__ p0; int s0; uint8_t* __restrict__ p1; int s1; uint8_t* __restrict__ p2; int s2;
    __device__ __forceinline__ void store(int x0, int y, int npx, const uint32_t px[PXT], bool active, int /*parity*/) const
    {
        if (!active) return;
        const uint32_t u0 = half_even_u32(((px[0] >> 8) & 0xffu) + ((px[1] >> 8) & 0xffu)), u1 = half_even_u32(((px[2] >> 8) & 0xffu) + ((px[3] >> 8) & 0xffu));
        const uint32_t v0 = half_even_u32(((px[0] >> 16) & 0xffu) + ((px[1] >> 16) & 0xffu)), v1 = half_even_u32(((px[2] >> 16) & 0xffu) + ((px[3] >> 16) & 0xffu));
        const uint32_t y0 = px[0] & 0xffu, y1 = px[1] & 0xffu, y2 = px[2] & 0xffu, y3 = px[3] & 0xffu;
        if (LAYOUT == 0)
        {
            uint8_t* yr = p0 + (__umul24((uint32_t)y, (uint32_t)s0) + (uint32_t)x0);
            uint8_t* ur = p1 + (__umul24((uint32_t)y, (uint32_t)s1) + (uint32_t)(x0 >> 1));
            uint8_t* vr = p2 + (__umul24((uint32_t)y, (uint32_t)s2) + (uint32_t)(x0 >> 1));
            const uint32_t yy = y0 | (y1 << 8) | (y2 << 16) | (y3 << 24);
            if (npx == PXT && ((reinterpret_cast<uintptr_t>(yr) & 3u) == 0)) LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(yr), yy);
            else for (int p = 0; p < npx; p++) yr[p] = (uint8_t)(yy >> (8 * p));
            ur[0] = (uint8_t)u0; vr[0] = (uint8_t)v0;
            if (npx > 2) { ur[1] = (uint8_t)u1; vr[1] = (uint8_t)v1; }
        }
        else
        {
            const uint32_t f0 = LAYOUT != 2 ? u0 : v0, g0 = LAYOUT != 2 ? v0 : u0, f1 = LAYOUT != 2 ? u1 : v1, g1 = LAYOUT != 2 ? v1 : u1;
            const uint32_t a = LAYOUT == 3 ? (f0 | (y0 << 8) | (g0 << 16) | (y1 << 24)) : (y0 | (f0 << 8) | (y1 << 16) | (g0 << 24));
            const uint32_t b = LAYOUT == 3 ? (f1 | (y2 << 8) | (g1 << 16) | (y3 << 24)) : (y2 | (f1 << 8) | (y3 << 16) | (g1 << 24));
            uint8_t* d = p0 + (__umul24((uint32_t)y, (uint32_t)s0) + 2u * (uint32_t)x0);
            if ((reinterpret_cast<uintptr_t>(d) & 3u) == 0)
            {
                LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(d), a);
                if (npx > 2) LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(d) + 1, b);
            }
            else
                for (int k = 0; k < 2 * npx; k++) d[k] = (uint8_t)((k < 4 ? a : b) >> (8 * (k & 3)));
        }
    }
};

// LAYOUT 0: planes Y, U, V (I444 / YUVA); 1: A Y U V with A = 255 (AYUV)
template <int LAYOUT>
struct Sink444
{
    uint8_t* __restrict__ p0; int s0; uint8_t* __restrict__ p1; int s1; uint8_t* __restrict__ p2; int s2;
    __device__ __forceinline__ void store(int x0, int y, int npx, const uint32_t px[PXT], bool active, int /*parity*/) const
    {
        if (!active) return;
        if (LAYOUT == 0)
        {
            uint8_t* r[3] = {p0 + (__umul24((uint32_t)y, (uint32_t)s0) + (uint32_t)x0), p1 + (__umul24((uint32_t)y, (uint32_t)s1) + (uint32_t)x0),
                             p2 + (__umul24((uint32_t)y, (uint32_t)s2) + (uint32_t)x0)};
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
            {
                const uint32_t w = ((px[0] >> (8 * ch)) & 0xffu) | (((px[1] >> (8 * ch)) & 0xffu) << 8) | (((px[2] >> (8 * ch)) & 0xffu) << 16) | (((px[3] >> (8 * ch)) & 0xffu) << 24);
                if (npx == PXT && ((reinterpret_cast<uintptr_t>(r[ch]) & 3u) == 0)) LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(r[ch]), w);
                else for (int p = 0; p < npx; p++) r[ch][p] = (uint8_t)(w >> (8 * p));
            }
        }
        else
        {
            uint8_t* d = p0 + (__umul24((uint32_t)y, (uint32_t)s0) + 4u * (uint32_t)x0);
            const bool al = (reinterpret_cast<uintptr_t>(d) & 3u) == 0;
            for (int p = 0; p < npx; p++)
            {
                const uint32_t w = 255u | (px[p] << 8);
                if (al) LVK_STREAM_STORE(reinterpret_cast<uint32_t*>(d) + p, w);
                else { d[4 * p] = 255; d[4 * p + 1] = (uint8_t)px[p]; d[4 * p + 2] = (uint8_t)(px[p] >> 8); d[4 * p + 3] = (uint8_t)(px[p] >> 16); }
            }
        }
    }
};

// A thread's finished row of four pixels goes to the sink (scaling_obs.hip, deblock_obs.hip).  AYUV alone has a wider form here: four whole pixels whose 16
// bytes lie on a 16-byte boundary leave as ONE store, as k_egress_444_dw writes them (ingest.hip) -- the sink's four dword stores, 16 bytes apart across the
// wave, cost the 4K frame 20 us.  Everything else, and every other row of an AYUV plane, is the sink's own store.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <class Sink>
__device__ __forceinline__ void store_row(const Sink& sink, int x0, int y, int npx, const uint32_t (&px)[PXT])
{
    sink.store(x0, y, npx, px, true, 0);
}

__device__ __forceinline__ void store_row(const Sink444<1>& sink, int x0, int y, int npx, const uint32_t (&px)[PXT])
{
    uint8_t* d = sink.p0 + (__umul24((uint32_t)y, (uint32_t)sink.s0) + 4u * (uint32_t)x0);
    if (npx == PXT && (reinterpret_cast<uintptr_t>(d) & 15u) == 0)
    {
        const u32x4 w = {255u | (px[0] << 8), 255u | (px[1] << 8), 255u | (px[2] << 8), 255u | (px[3] << 8)};
        __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(d));
    }
    else sink.store(x0, y, npx, px, true, 0);
}

// The sink of `video_format` over the caller's planes, checked, handed to launch(sink): the one switch of the two launchers below.  Plane i holds
// rows x `c` samples of `bpp` bytes; 4:2:2 has an even width.
template <class Launch>
int with_obs_sink(lvk_hip_ctx* ctx, const char* who, int video_format, int rows, int cols, void* const planes[3], const int steps[3], const Launch& launch)
{
    uint8_t* p0 = (uint8_t*)planes[0]; uint8_t* p1 = (uint8_t*)planes[1]; uint8_t* p2 = (uint8_t*)planes[2];
    auto plane_ok = [&](int i, int c, int bpp) { return remap_plane_ok(planes[i], steps[i], rows, c, bpp); };
    switch (video_format)
    {
    case LVK_VIDEO_FORMAT_I422: case LVK_VIDEO_FORMAT_I42A:
        LVK_HIP_REQUIRE(ctx, (cols & 1) == 0 && plane_ok(0, cols, 1) && plane_ok(1, cols / 2, 1) && plane_ok(2, cols / 2, 1));
        return launch(Sink422<0>{p0, steps[0], p1, steps[1], p2, steps[2]});
    case LVK_VIDEO_FORMAT_YUY2:
        LVK_HIP_REQUIRE(ctx, (cols & 1) == 0 && plane_ok(0, cols, 2));
        return launch(Sink422<1>{p0, steps[0], p0, 0, p0, 0});
    case LVK_VIDEO_FORMAT_YVYU:
        LVK_HIP_REQUIRE(ctx, (cols & 1) == 0 && plane_ok(0, cols, 2));
        return launch(Sink422<2>{p0, steps[0], p0, 0, p0, 0});
    case LVK_VIDEO_FORMAT_UYVY:
        LVK_HIP_REQUIRE(ctx, (cols & 1) == 0 && plane_ok(0, cols, 2));
        return launch(Sink422<3>{p0, steps[0], p0, 0, p0, 0});
    case LVK_VIDEO_FORMAT_I444: case LVK_VIDEO_FORMAT_YUVA:
        LVK_HIP_REQUIRE(ctx, plane_ok(0, cols, 1) && plane_ok(1, cols, 1) && plane_ok(2, cols, 1));
        return launch(Sink444<0>{p0, steps[0], p1, steps[1], p2, steps[2]});
    case LVK_VIDEO_FORMAT_AYUV:
        LVK_HIP_REQUIRE(ctx, plane_ok(0, cols, 4));
        return launch(Sink444<1>{p0, steps[0], p0, 0, p0, 0});
    }
    return ctx->fail(LVK_HIP_ERR_ARG, std::string(who) + ": no fused sink for video format " + std::to_string(video_format));
}

// The output planes of one frame (cols even on 4:2:2: the caller has checked): every plane there, its row inside its pitch, addressable by the sinks; clear
// of the `n_in` input spans and of one another
int obs_outputs_ok(lvk_hip_ctx* ctx, const char* name, int vf, void* const o_planes[3], const int o_steps[3], int rows, int cols, const Span* in, int n_in)
{
    const ObsRows t = obs_rows(vf, cols);
    if (t.n == 0) return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": video format " + std::to_string(vf) + " is not one FrameIngest::Select knows");
    Spans out{{}, t.n};
    for (int i = 0; i < t.n; i++)
    {
        LVK_HIP_REQUIRE(ctx, remap_plane_ok(o_planes[i], o_steps[i], rows, t.bytes[i], 1));
        out.s[i] = span_of(o_planes[i], o_steps[i], rows, t.bytes[i]);
    }
    LVK_HIP_REQUIRE(ctx, !is_direct4(vf) || o_steps[0] == 4 * cols);
    if (!clear_of(in, n_in, out)) return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": an output plane overlaps an input (the call is out of place)");
    if (!disjoint(out)) return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": two output planes overlap");
    return LVK_HIP_OK;
}

} // namespace
