// lvk::ScalingFilter on the planes of EVERY video format FrameIngest::Select accepts, out of place, in one call: lvk_hip_scale_obs.
// The output planes are, byte for byte, those of lvk_hip_ingest_obs -> lvk_hip_upscale(yuv = the frame format is YUV) -> lvk_hip_sharpen -> lvk_hip_egress_obs.
// Routes, chosen by the host (obs::scale_route):
//   I420 / I40A / NV12              the body of lvk_hip_scale_yuv420 (lvk_scale_420, scaling_420.hip)
//   4:2:2, 4:4:4, AYUV, upscale     the ingest into a pooled packed frame, the YUV EASU kernel into a second one, then k_rcas_obs<PackedSrc, Sink> from
//                                   that frame into the format's planes: the sharpened packed frame and the egress launch are gone
//   the same, equal sizes           one launch, no scratch memory: k_rcas_obs<PlaneSrc, Sink> forms the packed pixel the ingest would write in registers
//   BGR3, RGBA / BGRA / BGRX        three-byte pixels as they are: [lvk_launch_upscale(yuv = 0) into a pooled frame,] lvk_launch_sharpen into the plane
//   Y800                            [the gray EASU into a pooled plane,] the gray RCAS
//
// k_rcas_obs has k_rcas<4>'s shape (sharpen.hip) and k_rcas_420's structure (scaling_420.hip): 256 threads, a thread owns 4 columns x 4 rows, all its
// source rows are in flight together, a rolling three-row window, the two LDS reciprocal tables, rcas_pixel of rcas_core.hpp; each finished row of four
// pixels goes to a sink of obs_sinks.hpp.  Sizes are not all even here: a thread at the right edge holds 1 .. 4 columns (2 or 4 on 4:2:2), the last row
// group 1 .. 4 rows.  No load touches a byte outside the used bytes of a plane row or the 3 cols bytes of a packed row -- rows and columns are clamped one
// by one --, and no store one outside those of an output row (the sinks store npx pixels).
#include "lvk_hip_internal.hpp"
#include "rcas_src.hpp"
#include "obs_sinks.hpp"
#include "yuv420_core.hpp"

#include <cmath>

namespace {

constexpr int NPX = rcas::RCAS_PXT;

// The planes of a 4:2:2 or 4:4:4 frame: the packed pixel the ingest would write (k_ingest_422 / k_ingest_444, ingest.hip) is formed in registers, one
// dword 0x00VVUUYY per pixel of the thread's 6 x 6: rows y0 - 1 .. y0 + 4, columns x0 - 1 .. x0 + 4, each clamped into the frame by itself, so that a pixel
// outside the frame -- it is only ever the neighbour of a border pixel, which is copied -- is made of bytes of the frame.
// CHROMA 422: LAYOUT 0 planes Y, U, V (I422 / I42A), 1 YUY2, 2 YVYU, 3 UYVY -- the layouts of Sink422.  The chroma columns c0 - 1 .. c0 + 2 (c0 = x0 / 2),
// clamped to the plane (the edge sample replicated), give the six columns by up2x's closed form (ingest.hip): (other + 3 nearer + 2) >> 2.
// CHROMA 444: LAYOUT 0 planes Y, U, V (I444 / YUVA): the three bytes; 1 AYUV: bytes 1 .. 3 of the pixel's four.
template <int CHROMA, int LAYOUT>
struct PlaneSrc
{
    const uint8_t* p0; int s0; const uint8_t* p1; int s1; const uint8_t* p2; int s2;
    struct Raw { uint32_t px[ROWS + 2][NPX + 2]; };

    // bytes x0 - 1 .. x0 + 4 of a plane row of `cols` bytes: inside the row one (unaligned) dword and the two sides, at its end byte by byte
    static __device__ __forceinline__ void load6(const uint8_t* __restrict__ row, int x0, int cols, uint32_t (&b)[NPX + 2])
    {
        uint32_t w;
        if (x0 + NPX <= cols) w = reinterpret_cast<const yuv420::P4*>(row + x0)->w;
        else
        {
            w = 0;
#pragma unroll
            for (int j = 0; j < NPX; j++) w |= (uint32_t)row[min(x0 + j, cols - 1)] << (8 * j);
        }
        b[0] = row[max(x0 - 1, 0)]; b[NPX + 1] = row[min(x0 + NPX, cols - 1)];
#pragma unroll
        for (int j = 0; j < NPX; j++) b[j + 1] = (w >> (8 * j)) & 0xffu;
    }

    // the chroma of columns x0 - 1 .. x0 + 4 as 0x00VV00UU from the samples c0 - 1 .. c0 + 2 in the same form: both halves at once, a sum is at most 1022
    // and the two bits a right shift moves across are masked off
    static __device__ __forceinline__ void up6(const uint32_t (&s)[4], uint32_t (&uv)[NPX + 2])
    {
        const uint32_t m0 = 3 * s[0] + 0x00020002u, m1 = 3 * s[1] + 0x00020002u, m2 = 3 * s[2] + 0x00020002u, m3 = 3 * s[3] + 0x00020002u;
        uv[0] = ((s[1] + m0) >> 2) & 0x00ff00ffu; uv[1] = ((s[0] + m1) >> 2) & 0x00ff00ffu; uv[2] = ((s[2] + m1) >> 2) & 0x00ff00ffu;
        uv[3] = ((s[1] + m2) >> 2) & 0x00ff00ffu; uv[4] = ((s[3] + m2) >> 2) & 0x00ff00ffu; uv[5] = ((s[2] + m3) >> 2) & 0x00ff00ffu;
    }

    __device__ __forceinline__ void load(Raw& raw, int x0, int y0, int rows, int cols, int) const
    {
#pragma unroll
        for (int r = 0; r < ROWS + 2; r++)
        {
            const size_t yy = (size_t)min(max(y0 - 1 + r, 0), rows - 1);
            uint32_t (&px)[NPX + 2] = raw.px[r];
            if constexpr (CHROMA == 444 && LAYOUT == 0)
            {
                uint32_t y[NPX + 2], u[NPX + 2], v[NPX + 2];
                load6(p0 + yy * s0, x0, cols, y); load6(p1 + yy * s1, x0, cols, u); load6(p2 + yy * s2, x0, cols, v);
#pragma unroll
                for (int j = 0; j < NPX + 2; j++) px[j] = y[j] | (u[j] << 8) | (v[j] << 16);
            }
            else if constexpr (CHROMA == 444)
            {
                const uint8_t* row = p0 + yy * s0;                             // A Y U V: the plane may start at any byte
#pragma unroll
                for (int j = 0; j < NPX + 2; j++) px[j] = reinterpret_cast<const yuv420::P4*>(row + 4 * (size_t)min(max(x0 - 1 + j, 0), cols - 1))->w >> 8;
            }
            else
            {
                const int cc = cols >> 1, c0 = x0 >> 1;
                uint32_t y[NPX + 2], s[4], uv[NPX + 2];
                if constexpr (LAYOUT == 0)
                {
                    load6(p0 + yy * s0, x0, cols, y);
                    uint32_t su, sv;
                    yuv420::load_chroma4<false>(p1 + yy * s1, p2 + yy * s2, c0, cc, su, sv);
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) s[j] = __builtin_amdgcn_perm(sv, su, 0x0c040c00u + j * 0x00010001u);      // sample j as 0x00VV00UU
                }
                else
                {
                    // the pixel pairs c0 - 1 .. c0 + 2, one dword each (Y C Y C or C Y C Y); clamping the pair index replicates the edge samples
                    const uint8_t* row = p0 + yy * s0;
                    constexpr int YS = LAYOUT == 3 ? 8 : 0, CS = LAYOUT == 3 ? 0 : 8;      // bit offset of the first luma / chroma byte of a pair
                    uint32_t w[4];
#pragma unroll
                    for (int j = 0; j < 4; j++)
                    {
                        w[j] = reinterpret_cast<const yuv420::P4*>(row + 4 * (size_t)min(max(c0 - 1 + j, 0), cc - 1))->w;
                        const uint32_t first = (w[j] >> CS) & 0xffu, second = (w[j] >> (CS + 16)) & 0xffu;
                        s[j] = LAYOUT != 2 ? first | (second << 16) : second | (first << 16);
                    }
                    y[0] = (w[0] >> (YS + 16)) & 0xffu; y[1] = (w[1] >> YS) & 0xffu; y[2] = (w[1] >> (YS + 16)) & 0xffu;
                    y[3] = (w[2] >> YS) & 0xffu; y[4] = (w[2] >> (YS + 16)) & 0xffu; y[5] = (w[3] >> YS) & 0xffu;
                }
                up6(s, uv);
#pragma unroll
                for (int j = 0; j < NPX + 2; j++) px[j] = y[j] | ((uv[j] & 0xffu) << 8) | (uv[j] & 0xff0000u);
            }
        }
    }
    __device__ __forceinline__ rcas::Row row(const Raw& raw, int r) const
    {
        rcas::Row o;
#pragma unroll
        for (int j = 0; j < NPX + 2; j++) o.p[j] = rcas::unpack(raw.px[r][j]);
        return o;
    }
    __device__ __forceinline__ void centre(const Raw& raw, int r, uint32_t (&c)[NPX]) const
    {
#pragma unroll
        for (int p = 0; p < NPX; p++) c[p] = raw.px[r][p + 1];
    }
};

// (a thread's finished row of four pixels goes to the sink through store_row of obs_sinks.hpp)
//
// lvk_hip_sharpen of the frame `src` describes, then lvk_hip_egress_obs of the result through `sink`, without that result: one thread per 4 x ROWS pixels.
template <class Src, class Sink>
__global__ __launch_bounds__(256)
void k_rcas_obs(Src src, Sink sink, int rows, int cols, float sharp)
{
    __shared__ float s_rmin[256], s_rmax[256];
    rcas::fill_tables(s_rmin, s_rmax);
    __syncthreads();

    const int x0 = (int)blockIdx.x * rcas::RCAS_STRIP_W + (int)(threadIdx.x & 63) * NPX;
    const int y0 = ((int)blockIdx.y * 4 + (int)(threadIdx.x >> 6)) * ROWS;
    if (x0 >= cols || y0 >= rows) return;
    const int npx = min(NPX, cols - x0);                    // the row's last 1 .. 3 columns

    typename Src::Raw raw;                                  // rows y0 - 1 .. y0 + ROWS, all in flight together
    src.load(raw, x0, y0, rows, cols, 0);
    rcas::Row win[3];
    win[0] = src.row(raw, 0);
    win[1] = src.row(raw, 1);
#pragma unroll
    for (int r = 0; r < ROWS; r++)
    {
        const int y = y0 + r;
        if (y >= rows) break;
        const rcas::Row& up = win[r % 3];
        const rcas::Row& mid = win[(r + 1) % 3];
        rcas::Row& down = win[(r + 2) % 3];
        down = src.row(raw, r + 2);
        uint32_t centre[NPX];
        src.centre(raw, r + 1, centre);
        const bool border_row = y == 0 || y >= rows - 1;
        uint32_t o[NPX];
#pragma unroll
        for (int p = 0; p < NPX; p++)
        {
            const int x = x0 + p;
            const bool border = border_row || x == 0 || x >= cols - 1;              // FSR.cl:475-481: copied
            const uint32_t px = rcas::rcas_pixel(up.p[p + 1], mid.p[p], mid.p[p + 1], mid.p[p + 2], down.p[p + 1], sharp, s_rmin, s_rmax);
            o[p] = border ? centre[p] : px;
        }
        store_row(sink, x0, y, npx, o);
    }
}

template <class Src, class Sink>
int launch_rcas_obs(lvk_hip_ctx* ctx, const Src& src, const Sink& sink, int rows, int cols, float sharp)
{
    const dim3 block(256), grid((unsigned)((cols + rcas::RCAS_STRIP_W - 1) / rcas::RCAS_STRIP_W), (unsigned)((rows + 4 * ROWS - 1) / (4 * ROWS)));
    hipLaunchKernelGGL((k_rcas_obs<Src, Sink>), grid, block, 0, ctx->stream, src, sink, rows, cols, sharp);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

// the plane source that reads what `Sink` writes
template <class Sink> struct PlaneSrcOf;
template <int L> struct PlaneSrcOf<Sink422<L>> { using type = PlaneSrc<422, L>; };
template <int L> struct PlaneSrcOf<Sink444<L>> { using type = PlaneSrc<444, L>; };

} // namespace

extern "C" int lvk_hip_scale_obs(lvk_hip_ctx* ctx, int video_format,
                                 const void* const d_planes[3], const int steps[3], int src_rows, int src_cols,
                                 void* const o_planes[3], const int o_steps[3], int dst_rows, int dst_cols, float sharpness)
{
    LVK_HIP_ENTRY(ctx);
    const char* name = "lvk_hip_scale_obs";
    const int vf = video_format;
    LVK_HIP_REQUIRE(ctx, d_planes != nullptr && steps != nullptr && o_planes != nullptr && o_steps != nullptr);
    const bool equal = dst_rows == src_rows && dst_cols == src_cols;
    const ScaleRoute route = scale_route(vf, equal);
    if (route == ScaleRoute::None) return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": video format " + std::to_string(vf) + " is not one FrameIngest::Select knows");
    if (route == ScaleRoute::Planes420)
        return lvk_scale_420(ctx, name, plane_set_420(vf, d_planes, steps, src_rows, src_cols), plane_set_420(vf, o_planes, o_steps, dst_rows, dst_cols), sharpness);

    // ---- everything that can refuse the call, before anything is enqueued
    int rc = lvk_ingest_obs_check(ctx, vf, d_planes, steps, src_rows, src_cols);  // the planes in use, their pitches, the parity of the size, the format
    if (rc != LVK_HIP_OK) return rc;
    LVK_HIP_REQUIRE(ctx, obs_size_ok(vf, dst_rows, dst_cols));
    LVK_HIP_REQUIRE(ctx, dst_cols >= src_cols && dst_rows >= src_rows);           // Image.cpp:157
    LVK_HIP_REQUIRE(ctx, sharpness >= 0.0f && sharpness <= 1.0f);                 // LVK_ASSERT_01, Image.cpp:210 (a NaN fails both)
    const ObsRows t = obs_rows(vf, src_cols);
    for (int i = 0; i < t.n; i++) LVK_HIP_REQUIRE(ctx, remap_plane_ok(d_planes[i], steps[i], src_rows, t.bytes[i], 1));
    // out of place: the sharpening and the chroma up-sampling read their neighbours
    const Spans in = obs_spans(vf, d_planes, steps, src_rows, src_cols);
    if ((rc = obs_outputs_ok(ctx, name, vf, o_planes, o_steps, dst_rows, dst_cols, in.s, in.n)) != LVK_HIP_OK) return rc;

    // The frames between the launches come from the context's pool and go back to it once the last kernel is enqueued: whoever is handed them next
    // enqueues behind that kernel on this context's stream (lvk_hip.h, lvk_hip_free), and the steady state allocates nothing.
    void *d_small = nullptr, *d_big = nullptr;

    if (route == ScaleRoute::Gray)                                                // a one-channel frame, plane to plane
    {
        if (equal) return lvk_hip_sharpen_gray(ctx, d_planes[0], steps[0], dst_rows, dst_cols, o_planes[0], o_steps[0], sharpness);
        const int g_step = (dst_cols + 3) & ~3;
        if ((rc = lvk_hip_malloc(ctx, (size_t)g_step * dst_rows, &d_big)) != LVK_HIP_OK) return rc;
        rc = lvk_hip_upscale_gray(ctx, d_planes[0], steps[0], src_rows, src_cols, d_big, g_step, dst_rows, dst_cols);
        if (rc == LVK_HIP_OK) rc = lvk_hip_sharpen_gray(ctx, d_big, g_step, dst_rows, dst_cols, o_planes[0], o_steps[0], sharpness);
        (void)lvk_hip_free(ctx, d_big);
        return rc;
    }

    const int s_step = (3 * src_cols + 3) & ~3, p_step = (3 * dst_cols + 3) & ~3;
    if (route == ScaleRoute::Bgr)
    {
        // BGR3 and the DirectIngest formats ARE packed three-byte frames -- BGR3 at its own pitch, RGBA / BGRA / BGRX the first rows * cols * 3 bytes of the
        // tight plane, a frame of pitch 3 * cols at its own size (lvk_ingest_obs_check) --, so ingest and egress are copies and the kernels run on the planes.
        const bool bgr3 = vf == LVK_VIDEO_FORMAT_BGR3;
        const int in_step = bgr3 ? steps[0] : 3 * src_cols, out_step = bgr3 ? o_steps[0] : 3 * dst_cols;
        if (equal) return lvk_launch_sharpen(ctx, ctx->stream, d_planes[0], in_step, dst_rows, dst_cols, o_planes[0], out_step, sharpness);
        if ((rc = lvk_hip_malloc(ctx, (size_t)p_step * dst_rows, &d_big)) != LVK_HIP_OK) return rc;
        rc = lvk_launch_upscale(ctx, ctx->stream, d_planes[0], in_step, src_rows, src_cols, d_big, p_step, dst_rows, dst_cols, 0);
        if (rc == LVK_HIP_OK) rc = lvk_launch_sharpen(ctx, ctx->stream, d_big, p_step, dst_rows, dst_cols, o_planes[0], out_step, sharpness);
        (void)lvk_hip_free(ctx, d_big);
        return rc;
    }

    const float sharp = exp2f(-2.0f * (1.0f - sharpness));                        // Image.cpp:227
    if (route == ScaleRoute::FusedPlanes)                   // lvk::upscale copies (Image.cpp:162-166): the sharpening reads the planes itself
        return with_obs_sink(ctx, name, vf, dst_rows, dst_cols, o_planes, o_steps, [&](const auto& sink) {
            using Src = typename PlaneSrcOf<std::decay_t<decltype(sink)>>::type;
            const Src src{(const uint8_t*)d_planes[0], steps[0], (const uint8_t*)d_planes[1], steps[1], (const uint8_t*)d_planes[2], steps[2]};
            return launch_rcas_obs(ctx, src, sink, dst_rows, dst_cols, sharp);
        });

    if ((rc = lvk_hip_malloc(ctx, (size_t)s_step * src_rows, &d_small)) != LVK_HIP_OK) return rc;
    if ((rc = lvk_hip_malloc(ctx, (size_t)p_step * dst_rows, &d_big)) == LVK_HIP_OK
        && (rc = lvk_launch_ingest_obs(ctx, ctx->stream, vf, d_planes, steps, src_rows, src_cols, d_small, s_step)) == LVK_HIP_OK
        && (rc = lvk_launch_upscale(ctx, ctx->stream, d_small, s_step, src_rows, src_cols, d_big, p_step, dst_rows, dst_cols, 1)) == LVK_HIP_OK)
        rc = with_obs_sink(ctx, name, vf, dst_rows, dst_cols, o_planes, o_steps, [&](const auto& sink) {
            return launch_rcas_obs(ctx, PackedSrc{(const uint8_t*)d_big, p_step}, sink, dst_rows, dst_cols, sharp);
        });
    (void)lvk_hip_free(ctx, d_small);
    (void)lvk_hip_free(ctx, d_big);
    return rc;
}
