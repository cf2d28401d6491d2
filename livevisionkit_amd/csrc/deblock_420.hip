// lvk::DeblockingFilter on the planes of an I420 / NV12 frame, out of place: lvk_hip_deblock_apply_yuv420.  The output planes
// are, byte for byte, those of lvk_hip_ingest_yuv420 -> lvk_hip_deblock_apply(LVK_FORMAT_YUV) -> lvk_hip_egress_yuv420; the packed frame between
// them is never made.  Four launches on the context's stream:
//   k_deblock_stats<1>      (deblock.hip) on the Y plane: the grey of a YUV frame is its channel 0
//   k_deblock_down_420      k_deblock_down<3> (the shared down_pixel) with the pixel (Y, up(U), up(V)) taken from the planes
//   k_deblock_median<3>     (deblock.hip) on the small frame
//   k_deblock_blend_420     one thread per 4 x 2 luma pixels and their 2 chroma samples per plane: up-samples the chroma, blends the pixels inside
//                           the region as k_deblock_blend does, writes the luma and the (sum + 2) >> 2 of each 2 x 2 quad of chroma values
//
// up() is the exact 2x chroma up-sampling of the ingest in the closed form yuv420_core.hpp restates.
// No load touches a byte outside the cols (Y, NV12 UV) or cols / 2 (I420 chroma) bytes of a plane row, and no store one outside those of an
// output row.
#include "deblock_core.hpp"
#include "yuv420_core.hpp"

using namespace deblock;
using namespace yuv420;

namespace {

// Row y of the frame as the ingest makes it: the luma row and, per chroma plane, the row the up-sampling weighs 3 (n: k = y / 2) and the one it
// weighs 1 (f: k - 1 for an even y, k + 1 for an odd one, clamped to the plane)
struct Row420 { const uint8_t* y; const uint8_t* un; const uint8_t* uf; const uint8_t* vn; const uint8_t* vf; };

template <bool NV12>
__device__ __forceinline__ Row420 row_420(const Planes& in, int cr, int y)
{
    const int k = y >> 1;
    const int kf = (y & 1) ? min(k + 1, cr - 1) : max(k - 1, 0);
    Row420 r;
    r.y = in.y + (size_t)y * in.ys;
    r.un = in.u + (size_t)k * in.us; r.uf = in.u + (size_t)kf * in.us;
    r.vn = NV12 ? r.un + 1 : in.v + (size_t)k * in.vs; r.vf = NV12 ? r.uf + 1 : in.v + (size_t)kf * in.vs;
    return r;
}

// the pixel (Y, up(U), up(V)) of that row at column x, channels in bytes 0 .. 2: what the ingest writes there
template <bool NV12>
__device__ __forceinline__ uint32_t pixel_420(const Row420& r, int cc, int x)
{
    constexpr int PIX = NV12 ? 2 : 1;
    const int c = x >> 1;
    const int cf = (x & 1) ? min(c + 1, cc - 1) : max(c - 1, 0);
    const int u = up_v(3 * r.un[c * PIX] + r.un[cf * PIX], 3 * r.uf[c * PIX] + r.uf[cf * PIX]);
    const int v = up_v(3 * r.vn[c * PIX] + r.vn[cf * PIX], 3 * r.vf[c * PIX] + r.vf[cf * PIX]);
    return (uint32_t)r.y[x] | ((uint32_t)u << 8) | ((uint32_t)v << 16);
}

// the horizontal sums of the four luma columns 2 c0 .. 2 c0 + 3 from the samples c0 - 1 .. c0 + 2
__device__ __forceinline__ void up_h4(uint32_t w, int (&t)[4])
{
    const int s0 = (int)(w & 0xffu), s1 = (int)((w >> 8) & 0xffu), s2 = (int)((w >> 16) & 0xffu), s3 = (int)(w >> 24);
    const int m1 = 3 * s1, m2 = 3 * s2;
    t[0] = s0 + m1; t[1] = m1 + s2; t[2] = s1 + m2; t[3] = m2 + s3;
}

// k_deblock_down<3> on the planes: one thread per pixel of the small frame (packed, three bytes).  The default scale, 4, has a path of its own: a
// whole cell is 4 x 4 luma pixels, the columns 4 x .. 4 x + 3 of the rows 4 y .. 4 y + 3, whose chroma comes from the columns 2 x - 1 .. 2 x + 2 of the
// chroma rows 2 y - 1 .. 2 y + 2 -- one load per plane and row (load_chroma4) where the shared body reads two samples per plane and row for every
// pixel.  Same sums, same box_mean.  y_dw: the Y plane's base and pitch are multiples of 4.
template <bool NV12>
__global__ __launch_bounds__(256)
void k_deblock_down_420(Planes in, int rows, int cols, int rh, int rw, uint8_t* __restrict__ dst, int hs, int ws,
                        int iscale, float inv_area, const int2* __restrict__ xr, const AreaTabEntry* __restrict__ xt,
                        const int2* __restrict__ yr, const AreaTabEntry* __restrict__ yt, int y_dw)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ws || y >= hs) return;
    const int cc = cols >> 1, cr = rows >> 1;
    uint8_t* d = dst + ((size_t)y * ws + x) * 3;
    if (iscale == 4 && 4 * x + 4 <= rw && 4 * y + 4 <= rh)
    {
        int tu[4][4], tv[4][4];                             // horizontal sums of the chroma rows 2 y - 1 .. 2 y + 2
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            const int cy = min(max(2 * y - 1 + r, 0), cr - 1);
            uint32_t su, sv;
            load_chroma4<NV12>(in.u + (size_t)cy * in.us, NV12 ? nullptr : in.v + (size_t)cy * in.vs, 2 * x, cc, su, sv);
            up_h4(su, tu[r]); up_h4(sv, tv[r]);
        }
        int s[3] = {};
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const uint8_t* p = in.y + (size_t)(4 * y + j) * in.ys + 4 * x;
            const uint32_t yw = y_dw ? *reinterpret_cast<const uint32_t*>(p) : (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            const int n = 1 + (j >> 1), f = j == 0 ? 0 : j == 3 ? 3 : 3 - j;       // luma rows 4 y + (0, 1, 2, 3): chroma rows (1, 1, 2, 2) weigh 3, (0, 2, 1, 3) weigh 1
#pragma unroll
            for (int q = 0; q < 4; q++)
            {
                s[0] += byte_of(yw, q); s[1] += up_v(tu[n][q], tu[f][q]); s[2] += up_v(tv[n][q], tv[f][q]);
            }
        }
        store_pixel<3>(d, (uint32_t)box_mean(s[0], 4, inv_area) | ((uint32_t)box_mean(s[1], 4, inv_area) << 8) | ((uint32_t)box_mean(s[2], 4, inv_area) << 16));
        return;
    }
    down_pixel<3>([&](int yy) { return row_420<NV12>(in, cr, yy); }, [&](const Row420& r, int xx) { return pixel_420<NV12>(r, cc, xx); },
                  d, x, y, rh, rw, iscale, inv_area, xr, xt, yr, yt);
}

// One thread per group of 4 x 2 luma pixels (columns 4 g .. 4 g + 3, rows 2 k and 2 k + 1; the last group of a row holds 2 columns where
// cols % 4 == 2) and the chroma samples (c0, k), (c0 + 1, k), c0 = 2 g.  The chroma rows k - 1 .. k + 1 and columns c0 - 1 .. c0 + 2 are read once;
// the horizontal sums of row k serve both luma rows.  A pixel inside the region (x < rw, y < rh) is blended channel by channel as k_deblock_blend
// does it -- `smooth` of the channel, then its blend --, a pixel outside keeps (Y, up(U), up(V)); the chroma written is the egress's
// (sum + 2) >> 2 of the quad's four values, so a quad that straddles the region's edge mixes blended and unblended ones.
template <bool NV12>
__global__ __launch_bounds__(256)
void k_deblock_blend_420(Planes in, PlanesOut out, int rows, int cols, int rh, int rw,
                         const float* __restrict__ keep_block, int ex, const LinTabEntry* __restrict__ kx, const LinTabEntry* __restrict__ ky,
                         const uint8_t* __restrict__ small, int ws, const Lin8Entry* __restrict__ sx, const Lin8Entry* __restrict__ sy, int flags)
{
    const int g = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y * 4 + threadIdx.y;
    const int x0 = g * 4, cc = cols >> 1, cr = rows >> 1;
    if (x0 >= cols || k >= cr) return;
    const bool half = x0 + 4 > cols;                        // the row's last two columns
    const int c0 = x0 >> 1, ya = 2 * k;

    // chroma: rows k - 1, k, k + 1 (clamped), horizontal sums per row
    int tu[3][4], tv[3][4];
#pragma unroll
    for (int r = 0; r < 3; r++)
    {
        const int cy = min(max(k - 1 + r, 0), cr - 1);
        uint32_t su, sv;
        load_chroma4<NV12>(in.u + (size_t)cy * in.us, NV12 ? nullptr : in.v + (size_t)cy * in.vs, c0, cc, su, sv);
        up_h4(su, tu[r]); up_h4(sv, tv[r]);
    }
    // luma
    uint32_t yw[2];
#pragma unroll
    for (int r = 0; r < 2; r++)
    {
        const uint8_t* p = in.y + (size_t)(ya + r) * in.ys + x0;
        if (!half && (flags & kYInDw)) yw[r] = *reinterpret_cast<const uint32_t*>(p);
        else
        {
            yw[r] = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
            if (!half) yw[r] |= ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
    }
    // the group's pixels: Y in yw, up(U) / up(V) in U / V; row 0 = luma row 2 k (chroma rows k - 1, k), row 1 = 2 k + 1 (k, k + 1)
    int U[2][4], V[2][4];
#pragma unroll
    for (int p = 0; p < 4; p++)
    {
        U[0][p] = up_v(tu[1][p], tu[0][p]); U[1][p] = up_v(tu[1][p], tu[2][p]);
        V[0][p] = up_v(tv[1][p], tv[0][p]); V[1][p] = up_v(tv[1][p], tv[2][p]);
    }
    if (x0 < rw && ya < rh)
    {
        LinTabEntry tyk[2] = {};
        Lin8Entry tys[2] = {};
#pragma unroll
        for (int r = 0; r < 2; r++)
            if (ya + r < rh) { tyk[r] = ky[ya + r]; tys[r] = sy[ya + r]; }
        // Both luma rows of the group mostly interpolate between the same two rows of keep_block (a block is bs rows high) and of `small` (one row of
        // it covers filter_scaling luma rows): then row 1 reuses row 0's loads and horizontal passes, which are the same operations on the same
        // values.  Uniform over a wave (it depends on k alone).
        const bool both = ya + 1 < rh;
        const bool same_k = both && tyk[0].s0 == tyk[1].s0 && tyk[0].s1 == tyk[1].s1;
        const bool same_s = both && tys[0].s0 == tys[1].s0 && tys[0].s1 == tys[1].s1;
        uint32_t yo[2] = {yw[0], yw[1]};
#pragma unroll
        for (int p = 0; p < 4; p++)
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
                if (ya + r >= rh) continue;
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
                const int src[3] = {byte_of(yw[r], p), U[r][p], V[r][p]};
                int res[3];
#pragma unroll
                for (int c = 0; c < 3; c++)
                {
                    const int s = lin8(byte_of(p00, c), byte_of(p01, c), byte_of(p10, c), byte_of(p11, c), txs, tys[r].a0, tys[r].a1);
                    res[c] = blend_px(src[c], s, keep, deb, den);
                }
                yo[r] = (yo[r] & ~(0xffu << (8 * p))) | ((uint32_t)res[0] << (8 * p));
                U[r][p] = res[1]; V[r][p] = res[2];
            }
        }
        yw[0] = yo[0]; yw[1] = yo[1];
    }
    // luma out
#pragma unroll
    for (int r = 0; r < 2; r++)
    {
        const uint32_t y[4] = {yw[r], yw[r] >> 8, yw[r] >> 16, yw[r] >> 24};
        store_luma4(out.y + (size_t)(ya + r) * out.ys + x0, y, half, flags);
    }
    // chroma out: INTER_AREA 0.5 of each 2 x 2 quad
    const uint32_t u[2] = {(uint32_t)(U[0][0] + U[0][1] + U[1][0] + U[1][1] + 2) >> 2, (uint32_t)(U[0][2] + U[0][3] + U[1][2] + U[1][3] + 2) >> 2};
    const uint32_t v[2] = {(uint32_t)(V[0][0] + V[0][1] + V[1][0] + V[1][1] + 2) >> 2, (uint32_t)(V[0][2] + V[0][3] + V[1][2] + V[1][3] + 2) >> 2};
    store_chroma2<NV12>(out, k, c0, u, v, half, flags);
}

} // namespace

// lvk_hip_deblock_apply_yuv420 behind its entry guard: also the I420 / I40A / NV12 route of lvk_hip_deblock_apply_obs (deblock_obs.hip)
int deblock::apply_420(lvk_hip_deblock* d, const char* who, const PlaneSet& src, const PlaneSet& dst, int region_xywh[4])
{
    lvk_hip_ctx* ctx = d->ctx;
    const std::string name(who);
    const int nv12 = dst.nv12, rows = dst.rows, cols = dst.cols;
    LVK_HIP_REQUIRE(ctx, well_formed(src) && well_formed(dst));
    int rc;
    // out of place: the chroma up-sampling reads its neighbours
    const Spans src_spans = spans_of(src);
    if ((rc = require_out_of_place(ctx, name.c_str(), src_spans.s, src_spans.n, dst)) != LVK_HIP_OK) return rc;
    const lvk_deblock_settings& s = d->settings;
    Geometry g;
    if ((rc = geometry(ctx, s, rows, cols, name, g)) != LVK_HIP_OK) return rc;
    if ((rc = reserve(d, g, 3)) != LVK_HIP_OK) return rc;

    const Planes in = src.in();
    const PlanesOut out = dst.out();
    const int crows = rows / 2;
    if ((rc = launch_stats_plane(d, in.y, in.ys, g)) != LVK_HIP_OK) return rc;
    {
        const float inv_area_s = g.fast ? 1.0f / (float)((long long)g.iscale * g.iscale) : 0.0f;
        const dim3 grid((g.ws + 63) / 64, (g.hs + 3) / 4), block(64, 4);
        const int y_dw = aligned_to(in.y, in.ys, 4) ? 1 : 0;
        if (nv12)
            hipLaunchKernelGGL(k_deblock_down_420<true>, grid, block, 0, ctx->stream, in, rows, cols, g.rh, g.rw, d->d_small, g.hs, g.ws, g.fast ? g.iscale : 0,
                               inv_area_s, (const int2*)d->d_xr, (const AreaTabEntry*)d->d_xt, (const int2*)d->d_yr, (const AreaTabEntry*)d->d_yt, y_dw);
        else
            hipLaunchKernelGGL(k_deblock_down_420<false>, grid, block, 0, ctx->stream, in, rows, cols, g.rh, g.rw, d->d_small, g.hs, g.ws, g.fast ? g.iscale : 0,
                               inv_area_s, (const int2*)d->d_xr, (const AreaTabEntry*)d->d_xt, (const int2*)d->d_yr, (const AreaTabEntry*)d->d_yt, y_dw);
        LVK_HIP_CHECK(ctx, hipGetLastError());
    }
    if ((rc = launch_median_c3(d, g)) != LVK_HIP_OK) return rc;

    d->rh = g.rh; d->rw = g.rw; d->ey = g.ey; d->ex = g.ex; d->hs = g.hs; d->ws = g.ws; d->have_maps = true;
    const LinTabEntry *kx, *ky;
    const Lin8Entry *sx, *sy;
    if ((rc = blend_tables(ctx, d, true, &kx, &ky, &sx, &sy)) != LVK_HIP_OK) return rc;
    {
        const int flags = access_flags(&src, dst);
        const dim3 grid(((cols + 3) / 4 + 63) / 64, (crows + 3) / 4), block(64, 4);
        if (nv12)
            hipLaunchKernelGGL(k_deblock_blend_420<true>, grid, block, 0, ctx->stream, in, out, rows, cols, g.rh, g.rw, (const float*)d->d_keep, g.ex, kx, ky,
                               (const uint8_t*)d->d_median, g.ws, sx, sy, flags);
        else
            hipLaunchKernelGGL(k_deblock_blend_420<false>, grid, block, 0, ctx->stream, in, out, rows, cols, g.rh, g.rw, (const float*)d->d_keep, g.ex, kx, ky,
                               (const uint8_t*)d->d_median, g.ws, sx, sy, flags);
        LVK_HIP_CHECK(ctx, hipGetLastError());
    }
    if (region_xywh) { region_xywh[0] = 0; region_xywh[1] = 0; region_xywh[2] = g.rw; region_xywh[3] = g.rh; }
    return LVK_HIP_OK;
}

extern "C" int lvk_hip_deblock_apply_yuv420(lvk_hip_deblock* d, const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step,
                                            void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step,
                                            int nv12, int rows, int cols, int region_xywh[4])
{
    if (!d) return LVK_HIP_ERR_ARG;
    LVK_HIP_ENTRY(d->ctx);
    return apply_420(d, "lvk_hip_deblock_apply_yuv420", plane_set(d_y, y_step, d_u, u_step, d_v, v_step, nv12, rows, cols),
                     plane_set(o_y, oy_step, o_u, ou_step, o_v, ov_step, nv12, rows, cols), region_xywh);
}
