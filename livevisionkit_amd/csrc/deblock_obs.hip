// lvk::DeblockingFilter on the planes of EVERY video format FrameIngest::Select accepts, out of place, in one call: lvk_hip_deblock_apply_obs (DESIGN.md
// section 31).  The output planes are, byte for byte, those of
//   lvk_hip_ingest_obs -> lvk_hip_deblock_apply(format = lvk_hip_obs_frame_format(fmt)) -> lvk_hip_egress_obs
// (Y800: lvk_hip_deblock_apply_gray).  Routes, chosen by the host (obs::deblock_route):
//   I420 / I40A / NV12              the body of lvk_hip_deblock_apply_yuv420 (deblock::apply_420, deblock_420.hip)
//   4:2:2, 4:4:4, AYUV              four launches, no packed frame:
//                                     the block statistics of the luma -- k_deblock_stats<1> (deblock.hip) on a planar Y plane, k_deblock_stats_luma on the
//                                     luma bytes of a packed layout: the grey of a YUV frame is its channel 0
//                                     k_deblock_down_obs    k_deblock_down<3> (the shared down_pixel) with the pixel the ingest would write taken from the planes
//                                     k_deblock_median<3>   (deblock.hip) on the small frame
//                                     k_deblock_blend_obs   one thread per 4 x 2 pixels: forms the packed pixels, blends those inside the region as
//                                                           k_deblock_blend does, hands each row to the format's sink (obs_sinks.hpp), which does the egress
//   BGR3, RGBA / BGRA / BGRX        one 2-D copy of the used bytes into the output plane, then lvk_hip_deblock_apply in place on it (three-byte pixels: BGR3 at
//                                   its pitch, the 4-byte formats on DirectIngest's rows * cols * 3-byte view of pitch 3 * cols)
//   Y800                            a copy, then lvk_hip_deblock_apply_gray in place on the output plane
//
// The packed pixel of a 4:2:2 frame is (Y, up2x(U), up2x(V)), up2x in its closed form (other + 3 nearer + 2) >> 2 with the edge sample replicated
// (k_ingest_422, ingest.hip); of a 4:4:4 planar frame the three bytes; of an AYUV frame bytes 1 .. 3 of the pixel's four.
// No load touches a byte outside the used bytes of a plane row -- columns and pairs are clamped one by one, a partial group is read byte by byte --, and no
// store one outside those of an output row (the sinks store npx pixels).
#include "deblock_core.hpp"
#include "obs_sinks.hpp"

using namespace deblock;

namespace {

// The planes of a 4:2:2 or 4:4:4 frame as the source of packed pixels 0x00VVUUYY.
// CHROMA 422: LAYOUT 0 planes Y, U, V (I422 / I42A), 1 YUY2, 2 YVYU, 3 UYVY -- the layouts of Sink422.  CHROMA 444: LAYOUT 0 planes Y, U, V (I444 / YUVA),
// 1 AYUV -- those of Sink444.
template <int CHROMA, int LAYOUT>
struct ObsSrc
{
    const uint8_t* p0; int s0; const uint8_t* p1; int s1; const uint8_t* p2; int s2;
    struct Row { const uint8_t* a; const uint8_t* b; const uint8_t* c; };

    // byte offsets inside a packed 4:2:2 pixel pair (Y C Y C or C Y C Y)
    static constexpr int YOFF = LAYOUT == 3 ? 1 : 0, UOFF = LAYOUT == 1 ? 1 : LAYOUT == 2 ? 3 : 0, VOFF = LAYOUT == 1 ? 3 : LAYOUT == 2 ? 1 : 2;

    __device__ __forceinline__ Row row(int y) const
    {
        const bool planar = LAYOUT == 0;
        return {p0 + (size_t)y * s0, planar ? p1 + (size_t)y * s1 : nullptr, planar ? p2 + (size_t)y * s2 : nullptr};
    }

    // the pixel of column x of that row: what the ingest writes there (the downscale's fetch)
    __device__ __forceinline__ uint32_t pixel(const Row& r, int cols, int x) const
    {
        if constexpr (CHROMA == 444)
        {
            if constexpr (LAYOUT == 0) return (uint32_t)r.a[x] | ((uint32_t)r.b[x] << 8) | ((uint32_t)r.c[x] << 16);
            else return reinterpret_cast<const yuv420::P4*>(r.a + 4 * (size_t)x)->w >> 8;
        }
        else
        {
            const int cc = cols >> 1, c = x >> 1;
            const int cf = (x & 1) ? min(c + 1, cc - 1) : max(c - 1, 0);
            uint32_t y, un, uf, vn, vf;
            if constexpr (LAYOUT == 0) { y = r.a[x]; un = r.b[c]; uf = r.b[cf]; vn = r.c[c]; vf = r.c[cf]; }
            else
            {
                const uint8_t* n = r.a + 4 * (size_t)c;
                const uint8_t* f = r.a + 4 * (size_t)cf;
                y = r.a[2 * (size_t)x + YOFF]; un = n[UOFF]; uf = f[UOFF]; vn = n[VOFF]; vf = f[VOFF];
            }
            return y | (((uf + 3 * un + 2) >> 2) << 8) | (((vf + 3 * vn + 2) >> 2) << 16);
        }
    }

    // bytes x0 .. x0 + 3 of a plane row, each in its own word: one (unaligned) dword for a whole group, the first npx byte by byte else
    static __device__ __forceinline__ void bytes4(const uint8_t* __restrict__ row, int x0, int npx, uint32_t (&b)[PXT])
    {
        uint32_t w = 0;
        if (npx == PXT) w = reinterpret_cast<const yuv420::P4*>(row + x0)->w;
        else
            for (int j = 0; j < npx; j++) w |= (uint32_t)row[x0 + j] << (8 * j);
#pragma unroll
        for (int j = 0; j < PXT; j++) b[j] = (w >> (8 * j)) & 0xffu;
    }

    // the chroma of columns x0 .. x0 + 3 as 0x00VV00UU from the samples c0 - 1 .. c0 + 2 (x0 = 2 c0) by up2x's closed form: both halves at once, a sum
    // is at most 1022 and the two bits a right shift moves across are masked off
    static __device__ __forceinline__ void up4(const uint32_t (&s)[4], uint32_t (&uv)[PXT])
    {
        const uint32_t m1 = 3 * s[1] + 0x00020002u, m2 = 3 * s[2] + 0x00020002u;
        uv[0] = ((s[0] + m1) >> 2) & 0x00ff00ffu; uv[1] = ((s[2] + m1) >> 2) & 0x00ff00ffu;
        uv[2] = ((s[1] + m2) >> 2) & 0x00ff00ffu; uv[3] = ((s[3] + m2) >> 2) & 0x00ff00ffu;
    }

    // the pixels x0 .. x0 + npx - 1 of that row (x0 a multiple of 4; npx = 2 or 4 on 4:2:2): the blend's fetch.  px[npx ..] is made of bytes of the row.
    __device__ __forceinline__ void load4(const Row& r, int cols, int x0, int npx, uint32_t (&px)[PXT]) const
    {
        if constexpr (CHROMA == 444 && LAYOUT == 0)
        {
            uint32_t y[PXT], u[PXT], v[PXT];
            bytes4(r.a, x0, npx, y); bytes4(r.b, x0, npx, u); bytes4(r.c, x0, npx, v);
#pragma unroll
            for (int j = 0; j < PXT; j++) px[j] = y[j] | (u[j] << 8) | (v[j] << 16);
        }
        else if constexpr (CHROMA == 444)
        {
#pragma unroll
            for (int j = 0; j < PXT; j++) px[j] = reinterpret_cast<const yuv420::P4*>(r.a + 4 * (size_t)min(x0 + j, cols - 1))->w >> 8;    // A Y U V: the plane may start at any byte
        }
        else
        {
            const int cc = cols >> 1, c0 = x0 >> 1;
            uint32_t y[PXT], s[4], uv[PXT];
            if constexpr (LAYOUT == 0)
            {
                bytes4(r.a, x0, npx, y);
                uint32_t su, sv;
                yuv420::load_chroma4<false>(r.b, r.c, c0, cc, su, sv);
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) s[j] = __builtin_amdgcn_perm(sv, su, 0x0c040c00u + j * 0x00010001u);              // sample j as 0x00VV00UU
            }
            else
            {
                // the pixel pairs c0 - 1 .. c0 + 2, one dword each; clamping the pair index replicates the edge samples
                uint32_t w[4];
#pragma unroll
                for (int j = 0; j < 4; j++)
                {
                    w[j] = reinterpret_cast<const yuv420::P4*>(r.a + 4 * (size_t)min(max(c0 - 1 + j, 0), cc - 1))->w;
                    s[j] = ((w[j] >> (8 * UOFF)) & 0xffu) | (((w[j] >> (8 * VOFF)) & 0xffu) << 16);
                }
                y[0] = (w[1] >> (8 * YOFF)) & 0xffu; y[1] = (w[1] >> (8 * YOFF + 16)) & 0xffu;
                y[2] = (w[2] >> (8 * YOFF)) & 0xffu; y[3] = (w[2] >> (8 * YOFF + 16)) & 0xffu;
            }
            up4(s, uv);
#pragma unroll
            for (int j = 0; j < PXT; j++) px[j] = y[j] | ((uv[j] & 0xffu) << 8) | (uv[j] & 0xff0000u);
        }
    }
};

// the plane source that reads what `Sink` writes
template <class Sink> struct ObsSrcOf;
template <int L> struct ObsSrcOf<Sink422<L>> { using type = ObsSrc<422, L>; };
template <int L> struct ObsSrcOf<Sink444<L>> { using type = ObsSrc<444, L>; };

// k_deblock_stats<1> on the luma bytes of a packed YUV layout: the first at byte `first` of a row, the next `stride` bytes on (YUY2 / YVYU 0 and 2,
// UYVY 1 and 2, AYUV 1 and 4).  One wave per macroblock (4 per block of 256 threads along x), the two passes of block_stats.
__global__ __launch_bounds__(256)
void k_deblock_stats_luma(const uint8_t* __restrict__ plane, int step, int first, int stride, int bs, int ex, float inv_area, int levels, double level_step,
                          uint8_t* __restrict__ mean_out, uint8_t* __restrict__ grid_out, float* __restrict__ keep_out)
{
    const int lane = threadIdx.x & 63;
    const int bx = blockIdx.x * 4 + (threadIdx.x >> 6), by = blockIdx.y;
    if (bx >= ex) return;                       // whole waves only
    const uint8_t* base = plane + (size_t)by * bs * step + (size_t)bx * bs * stride + first;
    const int n = bs * bs;
    block_stats([&](auto f) {
                    for (int i = lane; i < n; i += 64)
                    {
                        const int py = i / bs, px = i - py * bs;
                        f((int)base[(size_t)py * step + (size_t)px * stride]);
                    }
                }, bs, inv_area, levels, level_step, lane, (size_t)by * ex + bx, mean_out, grid_out, keep_out);
}

// k_deblock_down<3> on the planes: one thread per pixel of the small frame (packed, three bytes)
template <class Src>
__global__ __launch_bounds__(256)
void k_deblock_down_obs(Src src, int cols, int rh, int rw, uint8_t* __restrict__ dst, int hs, int ws,
                        int iscale, float inv_area, const int2* __restrict__ xr, const AreaTabEntry* __restrict__ xt,
                        const int2* __restrict__ yr, const AreaTabEntry* __restrict__ yt)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ws || y >= hs) return;
    uint8_t* d = dst + ((size_t)y * ws + x) * 3;
    down_pixel<3>([&](int yy) { return src.row(yy); }, [&](const typename Src::Row& r, int xx) { return src.pixel(r, cols, xx); },
                  d, x, y, rh, rw, iscale, inv_area, xr, xt, yr, yt);
}

// One thread per group of 4 x 2 pixels (columns 4 g .. 4 g + 3, rows 2 k and 2 k + 1; the last group of a row holds 1 .. 4 columns -- 2 or 4 on 4:2:2 --,
// the last row pair of an odd height one row).  A pixel inside the region (x < rw, y < rh) is blended channel by channel as k_deblock_blend does it --
// `smooth` of the channel, then its blend --, a pixel outside keeps what the ingest makes of the planes; the sink then does the egress, so a 4:2:2 pair
// that straddles the region's edge averages a blended and an unblended value.  Row 1 reuses row 0's keep_block and median-frame loads where both rows
// interpolate between the same table rows, as in k_deblock_blend_420.
template <class Src, class Sink>
__global__ __launch_bounds__(256)
void k_deblock_blend_obs(Src src, Sink sink, int rows, int cols, int rh, int rw,
                         const float* __restrict__ keep_block, int ex, const LinTabEntry* __restrict__ kx, const LinTabEntry* __restrict__ ky,
                         const uint8_t* __restrict__ small, int ws, const Lin8Entry* __restrict__ sx, const Lin8Entry* __restrict__ sy)
{
    const int g = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y * 4 + threadIdx.y;
    const int x0 = g * PXT, ya = 2 * k;
    if (x0 >= cols || ya >= rows) return;
    const int npx = min(PXT, cols - x0);
    const bool two = ya + 1 < rows;

    uint32_t px[2][PXT];
    src.load4(src.row(ya), cols, x0, npx, px[0]);
    src.load4(src.row(two ? ya + 1 : ya), cols, x0, npx, px[1]);

    if (x0 < rw && ya < rh)
    {
        LinTabEntry tyk[2] = {};
        Lin8Entry tys[2] = {};
#pragma unroll
        for (int r = 0; r < 2; r++)
            if (ya + r < rh) { tyk[r] = ky[ya + r]; tys[r] = sy[ya + r]; }
        // (uniform over a wave: it depends on k alone)
        const bool both = ya + 1 < rh;
        const bool same_k = both && tyk[0].s0 == tyk[1].s0 && tyk[0].s1 == tyk[1].s1;
        const bool same_s = both && tys[0].s0 == tys[1].s0 && tys[0].s1 == tys[1].s1;
#pragma unroll
        for (int p = 0; p < PXT; p++)
        {
            const int x = x0 + p;
            if (x >= rw) continue;                          // rw <= cols: a pixel of the region is a pixel of the frame
            const LinTabEntry txk = kx[x];
            const Lin8Entry txs = sx[x];
            float kh0 = 0.f, kh1 = 0.f;                     // keep_at's horizontal pass over the two rows of keep_block
            uint32_t p00 = 0, p01 = 0, p10 = 0, p11 = 0;    // the four taps of `smooth`
#pragma unroll
            for (int r = 0; r < 2; r++)
            {
                if (ya + r >= rh) continue;                 // rh <= rows
                if (r == 0 || !same_k)
                {
                    const float* k0 = keep_block + (size_t)tyk[r].s0 * ex;
                    const float* k1 = keep_block + (size_t)tyk[r].s1 * ex;
                    kh0 = k0[txk.s0] * txk.a0 + k0[txk.s1] * txk.a1;
                    kh1 = k1[txk.s0] * txk.a0 + k1[txk.s1] * txk.a1;
                }
                const float keep = kh0 * tyk[r].a0 + kh1 * tyk[r].a1;
                const float deb = fabsf(keep - 1.0f);
                const float den = (keep + deb) + 1e-5f;
                if (r == 0 || !same_s)
                {
                    const size_t r0 = (size_t)tys[r].s0 * ws, r1 = (size_t)tys[r].s1 * ws;    // the two rows of `small`, in pixels
                    p00 = load_tap(small + (r0 + txs.s0) * 3); p01 = load_tap(small + (r0 + txs.s1) * 3);
                    p10 = load_tap(small + (r1 + txs.s0) * 3); p11 = load_tap(small + (r1 + txs.s1) * 3);
                }
                const uint32_t v = px[r][p];
                uint32_t out = 0;
#pragma unroll
                for (int c = 0; c < 3; c++)
                {
                    const int s = lin8(byte_of(p00, c), byte_of(p01, c), byte_of(p10, c), byte_of(p11, c), txs, tys[r].a0, tys[r].a1);
                    out |= (uint32_t)blend_px(byte_of(v, c), s, keep, deb, den) << (8 * c);
                }
                px[r][p] = out;
            }
        }
    }
    store_row(sink, x0, ya, npx, px[0]);
    if (two) store_row(sink, x0, ya + 1, npx, px[1]);
}

} // namespace

extern "C" int lvk_hip_deblock_apply_obs(lvk_hip_deblock* d, int video_format, const void* const d_planes[3], const int steps[3],
                                         void* const o_planes[3], const int o_steps[3], int rows, int cols, int region_xywh[4])
{
    if (!d) return LVK_HIP_ERR_ARG;
    lvk_hip_ctx* ctx = d->ctx;
    LVK_HIP_ENTRY(ctx);
    const char* name = "lvk_hip_deblock_apply_obs";
    const int vf = video_format;
    LVK_HIP_REQUIRE(ctx, d_planes != nullptr && steps != nullptr && o_planes != nullptr && o_steps != nullptr);
    const DeblockRoute route = deblock_route(vf);
    if (route == DeblockRoute::None) return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": video format " + std::to_string(vf) + " is not one FrameIngest::Select knows");
    if (route == DeblockRoute::Planes420)
        return apply_420(d, name, plane_set_420(vf, d_planes, steps, rows, cols), plane_set_420(vf, o_planes, o_steps, rows, cols), region_xywh);

    // ---- everything that can refuse the call, before anything is enqueued
    int rc = lvk_ingest_obs_check(ctx, vf, d_planes, steps, rows, cols);          // the planes in use, their pitches, the parity of the size, the format
    if (rc != LVK_HIP_OK) return rc;
    LVK_HIP_REQUIRE(ctx, obs_size_ok(vf, rows, cols));
    // out of place: the chroma up-sampling reads its neighbours, and the input planes are never written
    const Spans in = obs_spans(vf, d_planes, steps, rows, cols);
    if ((rc = obs_outputs_ok(ctx, name, vf, o_planes, o_steps, rows, cols, in.s, in.n)) != LVK_HIP_OK) return rc;
    Geometry g;
    if ((rc = geometry(ctx, d->settings, rows, cols, name, g)) != LVK_HIP_OK) return rc;

    if (route != DeblockRoute::Fused)
    {
        // BGR3, the DirectIngest formats and Y800 ARE packed frames -- BGR3 and Y800 at their own pitch, RGBA / BGRA / BGRX the first rows * cols * 3 bytes of
        // the tight plane, a frame of pitch 3 * cols (lvk_ingest_obs_check) --, so ingest and egress are copies: one of them remains, the apply runs in place
        const bool gray = route == DeblockRoute::Gray, tight = is_direct4(vf);
        const int bpp = gray ? 1 : 3;
        const int in_step = tight ? 3 * cols : steps[0], out_step = tight ? 3 * cols : o_steps[0];
        LVK_HIP_CHECK(ctx, hipMemcpy2DAsync(o_planes[0], (size_t)out_step, d_planes[0], (size_t)in_step, (size_t)bpp * (size_t)cols, (size_t)rows,
                                            hipMemcpyDeviceToDevice, ctx->stream));
        return gray ? lvk_hip_deblock_apply_gray(d, o_planes[0], out_step, rows, cols, region_xywh)
                    : lvk_hip_deblock_apply(d, o_planes[0], out_step, rows, cols, lvk_hip_obs_frame_format(vf), region_xywh);
    }

    return with_obs_sink(ctx, name, vf, rows, cols, o_planes, o_steps, [&](const auto& sink) {
        using Src = typename ObsSrcOf<std::decay_t<decltype(sink)>>::type;
        const Src src{(const uint8_t*)d_planes[0], steps[0], (const uint8_t*)d_planes[1], steps[1], (const uint8_t*)d_planes[2], steps[2]};
        const lvk_deblock_settings& s = d->settings;
        int rc;
        if ((rc = reserve(d, g, 3)) != LVK_HIP_OK) return rc;
        const LumaBytes luma = luma_bytes(vf);
        if (luma.stride == 1) rc = launch_stats_plane(d, src.p0, src.s0, g);
        else
        {
            const size_t cells = (size_t)g.ey * g.ex;
            hipLaunchKernelGGL(k_deblock_stats_luma, dim3((g.ex + 3) / 4, g.ey), dim3(256), 0, ctx->stream, src.p0, src.s0, luma.first, luma.stride, g.bs, g.ex,
                               1.0f / (float)((long long)g.bs * g.bs), (int)std::min<uint32_t>(s.detection_levels, 256u), 1.0 / (double)s.detection_levels,
                               d->d_grid, d->d_grid + cells, d->d_keep);
            LVK_HIP_CHECK(ctx, hipGetLastError());
        }
        if (rc != LVK_HIP_OK) return rc;
        {
            const float inv_area_s = g.fast ? 1.0f / (float)((long long)g.iscale * g.iscale) : 0.0f;
            hipLaunchKernelGGL(k_deblock_down_obs<Src>, dim3((g.ws + 63) / 64, (g.hs + 3) / 4), dim3(64, 4), 0, ctx->stream, src, cols, g.rh, g.rw,
                               d->d_small, g.hs, g.ws, g.fast ? g.iscale : 0, inv_area_s, (const int2*)d->d_xr, (const AreaTabEntry*)d->d_xt,
                               (const int2*)d->d_yr, (const AreaTabEntry*)d->d_yt);
            LVK_HIP_CHECK(ctx, hipGetLastError());
        }
        if ((rc = launch_median_c3(d, g)) != LVK_HIP_OK) return rc;

        d->rh = g.rh; d->rw = g.rw; d->ey = g.ey; d->ex = g.ex; d->hs = g.hs; d->ws = g.ws; d->have_maps = true;
        const LinTabEntry *kx, *ky;
        const Lin8Entry *sx, *sy;
        if ((rc = blend_tables(ctx, d, true, &kx, &ky, &sx, &sy)) != LVK_HIP_OK) return rc;
        hipLaunchKernelGGL((k_deblock_blend_obs<Src, std::decay_t<decltype(sink)>>), dim3(((cols + PXT - 1) / PXT + 63) / 64, ((rows + 1) / 2 + 3) / 4), dim3(64, 4), 0,
                           ctx->stream, src, sink, rows, cols, g.rh, g.rw, (const float*)d->d_keep, g.ex, kx, ky, (const uint8_t*)d->d_median, g.ws, sx, sy);
        LVK_HIP_CHECK(ctx, hipGetLastError());
        if (region_xywh) { region_xywh[0] = 0; region_xywh[1] = 0; region_xywh[2] = g.rw; region_xywh[3] = g.rh; }
        return (int)LVK_HIP_OK;
    });
}
