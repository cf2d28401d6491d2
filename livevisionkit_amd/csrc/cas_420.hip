// lvk::CASFilter on the planes of an I420 / NV12 frame, out of place, in one launch: lvk_hip_cas_yuv420.  The output planes are,
// byte for byte, those of lvk_hip_ingest_yuv420 -> lvk_hip_cas(format = YUV) -> lvk_hip_egress_yuv420, without the two packed frames between them.
//
// CAS sharpens every channel on its own (cas_channel of cas_core.hpp, specification tests/np_cas.py), so the packed pixel never exists: k_cas_420 forms
// the three channels (Y, up(U), up(V)) of the pixels it needs in registers, one channel at a time.  Shape: that of the equal-size kernel of
// scaling_420.hip with a 3 x 3 window.  256 threads, a wave per row pair, a thread owns the four luma columns x0 .. x0 + 3 of the rows 2 k and 2 k + 1:
//   luma     rows 2 k - 1 .. 2 k + 2, columns x0 - 1 .. x0 + 4: per row one (unaligned) dword inside the row and the byte on either side
//   chroma   rows k - 1 .. k + 1, columns c0 - 1 .. c0 + 2 (c0 = x0 / 2): one load_chroma4 per row, whose six horizontal sums serve the luma rows that
//            read the row; the vertical pass is yuv420::up_v on both planes at once
//   out      the luma of the eight pixels, and per plane the (sum + 2) >> 2 of each 2 x 2 quad of sharpened chroma values: the egress's INTER_AREA 0.5 x 0.5
// TWO EDGE RULES meet here.  The up-sampling replicates the edge sample: a chroma row or column beyond the plane is the clamped one.  A CAS neighbour
// outside the FRAME reads as 0 in every channel, which is not the replicated value: rows and columns are clamped for the loads and the pixels beyond the
// frame are replaced by 0 afterwards.  The chroma out is therefore not a function of the chroma in alone; the luma out is lvk_hip_cas_gray of the luma in.
// cols % 4 == 2 leaves the last thread of a row two columns.  No load touches a byte outside the cols (Y, NV12 UV) or cols / 2 (I420 chroma) bytes of a
// plane row, and no store one outside those of an output row.
#include "lvk_hip_internal.hpp"
#include "cas_core.hpp"
#include "yuv420_core.hpp"

using namespace ffx;
using namespace yuv420;

namespace {

constexpr int kPxt = 4;                    // luma columns per thread
constexpr int kStripW = 64 * kPxt;         // luma columns per wave

// the horizontal sums of the luma columns 2 c0 - 1 .. 2 c0 + 4 from the samples c0 - 1 .. c0 + 2 of both planes (U in the low, V in the high 16 bits):
// a sum is at most 1020
__device__ __forceinline__ void up_h6(uint32_t su, uint32_t sv, uint32_t (&t)[kPxt + 2])
{
    uint32_t s[4];                                     // sample j as 0x00VV00UU
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) s[j] = __builtin_amdgcn_perm(sv, su, 0x0c040c00u + j * 0x00010001u);
    const uint32_t m0 = 3 * s[0], m1 = 3 * s[1], m2 = 3 * s[2], m3 = 3 * s[3];
    t[0] = m0 + s[1]; t[1] = s[0] + m1; t[2] = m1 + s[2]; t[3] = s[1] + m2; t[4] = m2 + s[3]; t[5] = s[2] + m3;
}

// yuv420::up_v on both halves at once: 3 t <= 3060 stays inside its half, and the two bits a right shift moves across are masked off.  0x00VV00UU.
__device__ __forceinline__ uint32_t up_v2(uint32_t t_near, uint32_t t_far)
{
    return (((((3 * t_near) >> 2) & 0x3fff3fffu) + ((t_far >> 2) & 0x3fff3fffu) + 0x00020002u) >> 2) & 0x00ff00ffu;
}

// One channel of the thread's 2 x 4 pixels from its 4 x 6 window, into byte `ch` of the output pixels
__device__ __forceinline__ void sharpen_2x4(const float (&w)[4][kPxt + 2], float peak, int ch, uint32_t (&o)[2][kPxt])
{
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int p = 0; p < kPxt; p++)
            o[r][p] |= to_byte(cas_channel(w[r][p], w[r][p + 1], w[r][p + 2], w[r + 1][p], w[r + 1][p + 1], w[r + 1][p + 2],
                                           w[r + 2][p], w[r + 2][p + 1], w[r + 2][p + 2], peak)) << (8 * ch);
}

template <bool NV12>
__global__ __launch_bounds__(256)
void k_cas_420(Planes in, PlanesOut out, int rows, int cols, float peak, int flags)
{
    const int x0 = (int)blockIdx.x * kStripW + (int)(threadIdx.x & 63) * kPxt;
    const int k = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    const int ya = 2 * k;
    if (x0 >= cols || ya >= rows) return;
    const bool half = x0 + kPxt > cols;                     // the row's last two columns
    const int cc = cols >> 1, cr = rows >> 1, c0 = x0 >> 1;

    // ---- loads, all in flight together, from rows and columns clamped into the planes
    uint32_t yw[4], yl[4], yr[4];                           // luma rows ya - 1 .. ya + 2
    const int xl = max(x0 - 1, 0), xr = min(x0 + kPxt, cols - 1);
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        const uint8_t* p = in.y + (size_t)min(max(ya - 1 + r, 0), rows - 1) * in.ys;
        yw[r] = half ? (uint32_t)p[x0] | ((uint32_t)p[x0 + 1] << 8) : reinterpret_cast<const P4*>(p + x0)->w;
        yl[r] = p[xl]; yr[r] = p[xr];
    }
    uint32_t t[3][kPxt + 2];                                // the horizontal sums of the chroma rows k - 1 .. k + 1
#pragma unroll
    for (int j = 0; j < 3; j++)
    {
        const int cy = min(max(k - 1 + j, 0), cr - 1);
        uint32_t su, sv;
        load_chroma4<NV12>(in.u + (size_t)cy * in.us, NV12 ? nullptr : in.v + (size_t)cy * in.vs, c0, cc, su, sv);
        up_h6(su, sv, t[j]);
    }

    // ---- which of the 4 x 6 pixels lie in the frame: the others read as 0
    bool rin[4], cin[kPxt + 2];
#pragma unroll
    for (int r = 0; r < 4; r++) rin[r] = ya - 1 + r >= 0 && ya - 1 + r < rows;
#pragma unroll
    for (int j = 0; j < kPxt + 2; j++) cin[j] = x0 - 1 + j >= 0 && x0 - 1 + j < cols;

    uint32_t o[2][kPxt] = {};                               // 0x00VVUUYY
    float w[4][kPxt + 2];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int j = 0; j < kPxt + 2; j++)
        {
            const uint32_t y = j == 0 ? yl[r] : j == kPxt + 1 ? yr[r] : (yw[r] >> (8 * (j - 1))) & 0xffu;
            w[r][j] = rin[r] && cin[j] ? unit_of((float)y) : 0.0f;
        }
    sharpen_2x4(w, peak, 0, o);

    // luma row ya - 1 + r: chroma row n = (r + 1) / 2 of the three weighs 3, its outer neighbour f (also one of the three) weighs 1
    uint32_t uv[4][kPxt + 2];
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        const int n = (r + 1) >> 1, f = (r & 1) ? n - 1 : n + 1;
#pragma unroll
        for (int j = 0; j < kPxt + 2; j++) uv[r][j] = up_v2(t[n][j], t[f][j]);
    }
#pragma unroll
    for (int ch = 1; ch < 3; ch++)
    {
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int j = 0; j < kPxt + 2; j++)
                w[r][j] = rin[r] && cin[j] ? unit_of((float)((uv[r][j] >> (16 * (ch - 1))) & 0xffu)) : 0.0f;
        sharpen_2x4(w, peak, ch, o);
    }

    // ---- stores: the luma of both rows; the chroma is INTER_AREA 0.5 of each 2 x 2 quad of output pixels
    store_luma4(out.y + (size_t)ya * out.ys + x0, o[0], half, flags);
    store_luma4(out.y + (size_t)(ya + 1) * out.ys + x0, o[1], half, flags);
    uint32_t u[2], v[2];
#pragma unroll
    for (int q = 0; q < 2; q++)
    {
        const uint32_t a = o[0][2 * q], b = o[0][2 * q + 1], c = o[1][2 * q], d = o[1][2 * q + 1];
        u[q] = (((a >> 8) & 0xffu) + ((b >> 8) & 0xffu) + ((c >> 8) & 0xffu) + ((d >> 8) & 0xffu) + 2) >> 2;
        v[q] = (((a >> 16) & 0xffu) + ((b >> 16) & 0xffu) + ((c >> 16) & 0xffu) + ((d >> 16) & 0xffu) + 2) >> 2;
    }
    store_chroma2<NV12>(out, k, c0, u, v, half, flags);
}

} // namespace

// lvk_hip_cas_yuv420 behind its entry guard: also the I420 / I40A / NV12 route of lvk_hip_cas_obs (cas_obs.hip)
int lvk_cas_420(lvk_hip_ctx* ctx, const char* name, const PlaneSet& src, const PlaneSet& dst, float sharpness)
{
    LVK_HIP_REQUIRE(ctx, well_formed(src) && well_formed(dst, true));
    LVK_HIP_REQUIRE(ctx, sharpness >= 0.0f && sharpness <= 1.0f);                            // CASEffect.cpp: LVK_ASSERT_01 (a NaN fails both)
    // out of place: the sharpening and the chroma up-sampling read their neighbours
    const Spans src_spans = spans_of(src);
    const int rc = require_out_of_place(ctx, name, src_spans.s, src_spans.n, dst);
    if (rc != LVK_HIP_OK) return rc;
    float peak = 0.0f;
    lvk_hip_cas_const(sharpness, &peak);

    // (the flags choose the wide STORES only: the luma loads are unaligned dwords whatever the input planes' alignment is)
    const int rows = dst.rows, cols = dst.cols, flags = access_flags(nullptr, dst);
    const dim3 block(256), grid((unsigned)((cols + kStripW - 1) / kStripW), (unsigned)((rows / 2 + 3) / 4));
    if (dst.nv12) hipLaunchKernelGGL(k_cas_420<true>, grid, block, 0, ctx->stream, src.in(), dst.out(), rows, cols, peak, flags);
    else hipLaunchKernelGGL(k_cas_420<false>, grid, block, 0, ctx->stream, src.in(), dst.out(), rows, cols, peak, flags);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

extern "C" int lvk_hip_cas_yuv420(lvk_hip_ctx* ctx,
                                  const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step,
                                  void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step,
                                  int rows, int cols, int nv12, float sharpness)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_cas_420(ctx, "lvk_hip_cas_yuv420", plane_set(d_y, y_step, d_u, u_step, d_v, v_step, nv12, rows, cols),
                       plane_set(o_y, oy_step, o_u, ou_step, o_v, ov_step, nv12, rows, cols), sharpness);
}
