// lvk::CASFilter on the planes of EVERY video format FrameIngest::Select accepts, out of place, in one call: lvk_hip_cas_obs.
// The output planes are, byte for byte, those of
//   lvk_hip_ingest_obs -> lvk_hip_cas(format = lvk_hip_obs_frame_format(fmt)) -> lvk_hip_egress_obs
// (Y800: lvk_hip_cas_gray).  Routes, chosen by the host (obs::cas_route), one launch each, no copy, no scratch memory:
//   I420 / I40A / NV12              the body of lvk_hip_cas_yuv420 (lvk_cas_420, cas_420.hip)
//   4:2:2, 4:4:4, AYUV              k_cas_obs<Src, Sink>: forms the packed pixels the ingest would write from the planes, sharpens the three channels with
//                                   cas_channel (cas_core.hpp), hands each row to the format's sink (obs_sinks.hpp), which does the egress
//   BGR3, RGBA / BGRA / BGRX        lvk_hip_cas on three-byte pixels from the input plane to the output plane: BGR3 at its pitches, the 4-byte formats on
//                                   DirectIngest's rows * cols * 3-byte view of pitch 3 * cols
//   Y800                            lvk_hip_cas_gray from plane to plane
//
// k_cas_obs has k_cas_gray's shape (cas_gray.hip): no LDS, 256 threads, a wave per band of kRows rows, a thread owns 4 columns x kRows rows (the last
// group of a row 1 .. 4 columns, 2 or 4 on 4:2:2; the last band 1 .. kRows rows), loads the kRows + 2 rows it needs at once and walks them with a rolling
// three-row window of u / 255 values in registers.
// TWO EDGE RULES meet here.  The packed pixel of a 4:2:2 frame is (Y, up2x(U), up2x(V)), up2x in its closed form (far + 3 near + 2) >> 2 with the edge
// sample REPLICATED (k_ingest_422, ingest.hip).  A CAS neighbour outside the frame reads as 0 in every channel.  So rows and columns are clamped into the
// frame one by one for the loads -- no load touches a byte outside the used bytes of a plane row --, and a pixel outside the frame is replaced by 0 when
// the window is unpacked.  The sinks store npx pixels: no store touches a byte outside those of an output row.
#include "lvk_hip_internal.hpp"
#include "cas_core.hpp"
#include "obs_sinks.hpp"
#include "yuv420_core.hpp"

using namespace ffx;

namespace {

constexpr int kRows = 4;                   // rows per thread
constexpr int kBlockH = 4 * kRows;         // rows per block: one band per wave
constexpr int kWin = PXT + 2;              // columns x0 - 1 .. x0 + PXT

// The planes of a 4:2:2 or 4:4:4 frame as the source of rows of packed pixels 0x00VVUUYY.
// CHROMA 422: LAYOUT 0 planes Y, U, V (I422 / I42A), 1 YUY2, 2 YVYU, 3 UYVY -- the layouts of Sink422.  CHROMA 444: LAYOUT 0 planes Y, U, V (I444 / YUVA),
// 1 AYUV -- those of Sink444.
template <int CHROMA, int LAYOUT>
struct CasSrc
{
    const uint8_t* p0; int s0; const uint8_t* p1; int s1; const uint8_t* p2; int s2;

    // bytes x0 - 1 .. x0 + 4 of a plane row of `cols` bytes: inside the row one (unaligned) dword and the two sides, at its end byte by byte
    static __device__ __forceinline__ void load6(const uint8_t* __restrict__ row, int x0, int cols, uint32_t (&b)[kWin])
    {
        uint32_t w;
        if (x0 + PXT <= cols) w = reinterpret_cast<const yuv420::P4*>(row + x0)->w;
        else
        {
            w = 0;
#pragma unroll
            for (int j = 0; j < PXT; j++) w |= (uint32_t)row[min(x0 + j, cols - 1)] << (8 * j);
        }
        b[0] = row[max(x0 - 1, 0)]; b[PXT + 1] = row[min(x0 + PXT, cols - 1)];
#pragma unroll
        for (int j = 0; j < PXT; j++) b[j + 1] = (w >> (8 * j)) & 0xffu;
    }

    // the chroma of columns x0 - 1 .. x0 + 4 as 0x00VV00UU from the samples c0 - 1 .. c0 + 2 (x0 = 2 c0) by up2x's closed form: both halves at once, a
    // sum is at most 1022 and the two bits a right shift moves across are masked off
    static __device__ __forceinline__ void up6(const uint32_t (&s)[4], uint32_t (&uv)[kWin])
    {
        const uint32_t m0 = 3 * s[0] + 0x00020002u, m1 = 3 * s[1] + 0x00020002u, m2 = 3 * s[2] + 0x00020002u, m3 = 3 * s[3] + 0x00020002u;
        uv[0] = ((s[1] + m0) >> 2) & 0x00ff00ffu; uv[1] = ((s[0] + m1) >> 2) & 0x00ff00ffu; uv[2] = ((s[2] + m1) >> 2) & 0x00ff00ffu;
        uv[3] = ((s[1] + m2) >> 2) & 0x00ff00ffu; uv[4] = ((s[3] + m2) >> 2) & 0x00ff00ffu; uv[5] = ((s[2] + m3) >> 2) & 0x00ff00ffu;
    }

    // The pixels x0 - 1 .. x0 + 4 of row yy (a row of the frame; x0 a multiple of 4 below cols): what the ingest writes there.  A column outside the
    // frame is made of bytes of the row -- the caller replaces it.
    __device__ __forceinline__ void load_row(int yy, int x0, int cols, uint32_t (&px)[kWin]) const
    {
        if constexpr (CHROMA == 444 && LAYOUT == 0)
        {
            uint32_t y[kWin], u[kWin], v[kWin];
            load6(p0 + (size_t)yy * s0, x0, cols, y); load6(p1 + (size_t)yy * s1, x0, cols, u); load6(p2 + (size_t)yy * s2, x0, cols, v);
#pragma unroll
            for (int j = 0; j < kWin; j++) px[j] = y[j] | (u[j] << 8) | (v[j] << 16);
        }
        else if constexpr (CHROMA == 444)
        {
            const uint8_t* row = p0 + (size_t)yy * s0;                         // A Y U V: the plane may start at any byte
#pragma unroll
            for (int j = 0; j < kWin; j++) px[j] = reinterpret_cast<const yuv420::P4*>(row + 4 * (size_t)min(max(x0 - 1 + j, 0), cols - 1))->w >> 8;
        }
        else
        {
            const int cc = cols >> 1, c0 = x0 >> 1;
            uint32_t y[kWin], s[4], uv[kWin];
            if constexpr (LAYOUT == 0)
            {
                load6(p0 + (size_t)yy * s0, x0, cols, y);
                uint32_t su, sv;
                yuv420::load_chroma4<false>(p1 + (size_t)yy * s1, p2 + (size_t)yy * s2, c0, cc, su, sv);
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) s[j] = __builtin_amdgcn_perm(sv, su, 0x0c040c00u + j * 0x00010001u);      // sample j as 0x00VV00UU
            }
            else
            {
                // the pixel pairs c0 - 1 .. c0 + 2, one dword each (Y C Y C or C Y C Y); clamping the pair index replicates the edge samples
                const uint8_t* row = p0 + (size_t)yy * s0;
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
            for (int j = 0; j < kWin; j++) px[j] = y[j] | ((uv[j] & 0xffu) << 8) | (uv[j] & 0xff0000u);
        }
    }
};

// the plane source that reads what `Sink` writes
template <class Sink> struct CasSrcOf;
template <int L> struct CasSrcOf<Sink422<L>> { using type = CasSrc<422, L>; };
template <int L> struct CasSrcOf<Sink444<L>> { using type = CasSrc<444, L>; };

// lvk_hip_cas(format = YUV) of the frame `src` describes, then lvk_hip_egress_obs of the result through `sink`, without either packed frame
template <class Src, class Sink>
__global__ __launch_bounds__(256)
void k_cas_obs(Src src, Sink sink, int rows, int cols, float peak)
{
    const int x0 = (int)blockIdx.x * STRIP_W + (int)(threadIdx.x & 63) * PXT;
    const int y0 = ((int)blockIdx.y * 4 + (int)(threadIdx.x >> 6)) * kRows;
    if (x0 >= cols || y0 >= rows) return;
    const int npx = min(PXT, cols - x0);                    // the row's last 1 .. 3 columns

    // Unconditional loads, so that all rows of a thread are in flight together, from rows clamped into the frame: a row above or below it is loaded from
    // its in-frame neighbour and replaced by 0 below.
    uint32_t raw[kRows + 2][kWin];                          // rows y0 - 1 .. y0 + kRows
#pragma unroll
    for (int r = 0; r < kRows + 2; r++) src.load_row(min(max(y0 - 1 + r, 0), rows - 1), x0, cols, raw[r]);

    bool cin[kWin];
#pragma unroll
    for (int j = 0; j < kWin; j++) cin[j] = x0 - 1 + j >= 0 && x0 - 1 + j < cols;

    float win[3][kWin][3];                                  // the rolling window: [row][column x0 - 1 .. x0 + PXT][channel]
    auto unpack = [&](int r, float (&o)[kWin][3]) {
        const int y = y0 - 1 + r;
        const bool rin = y >= 0 && y < rows;
#pragma unroll
        for (int j = 0; j < kWin; j++)
#pragma unroll
            for (int c = 0; c < 3; c++)
            {
                const float v = unit_of((float)((raw[r][j] >> (8 * c)) & 0xffu));
                o[j][c] = rin && cin[j] ? v : 0.0f;
            }
    };
    unpack(0, win[0]);
    unpack(1, win[1]);
#pragma unroll
    for (int r = 0; r < kRows; r++)
    {
        const int y = y0 + r;
        if (y >= rows) break;
        const float (&up)[kWin][3] = win[r % 3];
        const float (&mid)[kWin][3] = win[(r + 1) % 3];
        float (&down)[kWin][3] = win[(r + 2) % 3];
        unpack(r + 2, down);
        uint32_t o[PXT];
#pragma unroll
        for (int p = 0; p < PXT; p++)
        {
            o[p] = 0;
#pragma unroll
            for (int c = 0; c < 3; c++)
                o[p] |= to_byte(cas_channel(up[p][c], up[p + 1][c], up[p + 2][c], mid[p][c], mid[p + 1][c], mid[p + 2][c],
                                            down[p][c], down[p + 1][c], down[p + 2][c], peak)) << (8 * c);
        }
        store_row(sink, x0, y, npx, o);
    }
}

} // namespace

extern "C" int lvk_hip_cas_obs(lvk_hip_ctx* ctx, int video_format, const void* const d_planes[3], const int steps[3],
                               void* const o_planes[3], const int o_steps[3], int rows, int cols, float sharpness)
{
    LVK_HIP_ENTRY(ctx);
    const char* name = "lvk_hip_cas_obs";
    const int vf = video_format;
    LVK_HIP_REQUIRE(ctx, d_planes != nullptr && steps != nullptr && o_planes != nullptr && o_steps != nullptr);
    const CasRoute route = cas_route(vf);
    if (route == CasRoute::None) return ctx->fail(LVK_HIP_ERR_ARG, std::string(name) + ": video format " + std::to_string(vf) + " is not one FrameIngest::Select knows");
    if (route == CasRoute::Planes420)
        return lvk_cas_420(ctx, name, plane_set_420(vf, d_planes, steps, rows, cols), plane_set_420(vf, o_planes, o_steps, rows, cols), sharpness);

    // ---- everything that can refuse the call, before anything is enqueued
    int rc = lvk_ingest_obs_check(ctx, vf, d_planes, steps, rows, cols);          // the planes in use, their pitches, the parity of the size, the format
    if (rc != LVK_HIP_OK) return rc;
    LVK_HIP_REQUIRE(ctx, sharpness >= 0.0f && sharpness <= 1.0f);                 // CASEffect.cpp: LVK_ASSERT_01 (a NaN fails both)
    // out of place: the sharpening and the chroma up-sampling read their neighbours, and the input planes are never written
    const Spans in = obs_spans(vf, d_planes, steps, rows, cols);
    if ((rc = obs_outputs_ok(ctx, name, vf, o_planes, o_steps, rows, cols, in.s, in.n)) != LVK_HIP_OK) return rc;

    if (route == CasRoute::Gray) return lvk_hip_cas_gray(ctx, d_planes[0], steps[0], rows, cols, o_planes[0], o_steps[0], sharpness);
    if (route == CasRoute::Bgr)
    {
        // BGR3 and the DirectIngest formats ARE packed three-byte frames -- BGR3 at its own pitch, RGBA / BGRA / BGRX the first rows * cols * 3 bytes of the
        // tight plane, a frame of pitch 3 * cols (lvk_ingest_obs_check) --, so ingest and egress are copies and the kernel runs from plane to plane
        const bool tight = is_direct4(vf);
        return lvk_hip_cas(ctx, d_planes[0], tight ? 3 * cols : steps[0], rows, cols, lvk_hip_obs_frame_format(vf), o_planes[0], tight ? 3 * cols : o_steps[0],
                           sharpness);
    }

    float peak = 0.0f;
    lvk_hip_cas_const(sharpness, &peak);
    return with_obs_sink(ctx, name, vf, rows, cols, o_planes, o_steps, [&](const auto& sink) {
        using Sink = std::decay_t<decltype(sink)>;
        using Src = typename CasSrcOf<Sink>::type;
        const Src src{(const uint8_t*)d_planes[0], steps[0], (const uint8_t*)d_planes[1], steps[1], (const uint8_t*)d_planes[2], steps[2]};
        const dim3 block(256), grid((unsigned)((cols + STRIP_W - 1) / STRIP_W), (unsigned)((rows + kBlockH - 1) / kBlockH));
        hipLaunchKernelGGL((k_cas_obs<Src, Sink>), grid, block, 0, ctx->stream, src, sink, rows, cols, peak);
        LVK_HIP_CHECK(ctx, hipGetLastError());
        return (int)LVK_HIP_OK;
    });
}
