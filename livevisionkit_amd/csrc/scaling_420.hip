// lvk::ScalingFilter on the planes of an I420 / NV12 frame, out of place: lvk_hip_scale_yuv420.  The output planes are, byte for
// byte, those of lvk_hip_ingest_yuv420 -> lvk_hip_upscale(yuv = 1) -> lvk_hip_sharpen -> lvk_hip_egress_yuv420.  Two routes, chosen by the host:
//   equal sizes   one launch, no scratch memory: k_rcas_420<PlanarSrc> forms the packed pixel (Y, up(U), up(V)) in registers, sharpens it and writes
//                 the luma and the (sum + 2) >> 2 of each 2 x 2 quad of chroma values
//   upscale       the ingest into a packed source frame, the EASU kernel into a packed destination frame (both from the context's block pool, both
//                 given back as soon as the last kernel is enqueued), then k_rcas_420<PackedSrc> from that frame into the planes
//
// k_rcas_420 has k_rcas<4>'s shape (sharpen.hip): 256 threads, a thread owns 4 columns x 4 rows, all its source rows are in flight together, a rolling
// three-row window, the two LDS reciprocal tables, rcas_pixel of rcas_core.hpp.  A thread writes 4 luma rows and 2 chroma samples per plane and row pair.
// cols % 4 == 2 leaves the last thread of a row two columns, rows % 4 == 2 the last row group two rows.
// No load touches a byte outside the cols (Y, NV12 UV) or cols / 2 (I420 chroma) bytes of a plane row or the 3 cols bytes of a packed row, and no store
// one outside those of an output row.
#include "lvk_hip_internal.hpp"
#include "rcas_core.hpp"
#include "rcas_src.hpp"
#include "yuv420_core.hpp"

#include <cmath>

using namespace rcas;
using namespace yuv420;

namespace {

// The planes of an I420 / NV12 frame: the packed pixel (Y, up(U), up(V)) the ingest would write is formed in registers.  A thread's 6 x 6 pixels, rows
// y0 - 1 .. y0 + 4 and columns x0 - 1 .. x0 + 4, need the chroma rows k0 - 1 .. k0 + 2 (k0 = y0 / 2) and columns c0 - 1 .. c0 + 2 (c0 = x0 / 2): one
// load_chroma4 per chroma row, whose six horizontal sums serve every luma row that reads the row.  Rows and columns are clamped one by one, so that a
// pixel outside the frame -- it is only ever the neighbour of a border pixel, which is copied -- is made of bytes of the frame.
template <bool NV12>
struct PlanarSrc
{
    Planes in;
    // t: the horizontal sums of the four chroma rows, U's in the low and V's in the high 16 bits
    struct Raw { uint32_t yw[ROWS + 2], yl[ROWS + 2], yr[ROWS + 2], t[4][RCAS_PXT + 2]; };

    // the horizontal sums of the luma columns 2 c0 - 1 .. 2 c0 + 4 from the samples c0 - 1 .. c0 + 2 of both planes: a sum is at most 1020
    static __device__ __forceinline__ void up_h6(uint32_t su, uint32_t sv, uint32_t (&t)[RCAS_PXT + 2])
    {
        uint32_t s[4];                                     // sample j as 0x00VV00UU
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) s[j] = __builtin_amdgcn_perm(sv, su, 0x0c040c00u + j * 0x00010001u);
        const uint32_t m0 = 3 * s[0], m1 = 3 * s[1], m2 = 3 * s[2], m3 = 3 * s[3];
        t[0] = m0 + s[1]; t[1] = s[0] + m1; t[2] = m1 + s[2]; t[3] = s[1] + m2; t[4] = m2 + s[3]; t[5] = s[2] + m3;
    }
    // yuv420::up_v on both halves at once: 3 t <= 3060 stays inside its half, and the two bits a right shift moves across are masked off
    static __device__ __forceinline__ uint32_t up_v2(uint32_t t_near, uint32_t t_far)
    {
        return ((((3 * t_near) >> 2) & 0x3fff3fffu) + ((t_far >> 2) & 0x3fff3fffu) + 0x00020002u) >> 2;
    }

    __device__ __forceinline__ void load(Raw& raw, int x0, int y0, int rows, int cols, int flags) const
    {
        const int cc = cols >> 1, cr = rows >> 1, c0 = x0 >> 1, k0 = y0 >> 1;
        const bool dw = x0 + RCAS_PXT <= cols && (flags & kYInDw);
        const int xl = max(x0 - 1, 0), xr = min(x0 + RCAS_PXT, cols - 1);
#pragma unroll
        for (int r = 0; r < ROWS + 2; r++)
        {
            const uint8_t* p = in.y + (size_t)min(max(y0 - 1 + r, 0), rows - 1) * in.ys;
            if (dw) raw.yw[r] = *reinterpret_cast<const uint32_t*>(p + x0);
            else
            {
                raw.yw[r] = 0;
#pragma unroll
                for (int j = 0; j < RCAS_PXT; j++) raw.yw[r] |= (uint32_t)p[min(x0 + j, cols - 1)] << (8 * j);
            }
            raw.yl[r] = p[xl]; raw.yr[r] = p[xr];
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const int cy = min(max(k0 - 1 + j, 0), cr - 1);
            uint32_t su, sv;
            load_chroma4<NV12>(in.u + (size_t)cy * in.us, NV12 ? nullptr : in.v + (size_t)cy * in.vs, c0, cc, su, sv);
            up_h6(su, sv, raw.t[j]);
        }
    }
    // pixel j (column x0 - 1 + j) of row r (luma row y0 - 1 + r): chroma row n = (r + 1) / 2 of the four weighs 3, its outer neighbour f weighs 1
    __device__ __forceinline__ uint32_t pixel(const Raw& raw, int r, int j) const
    {
        const int n = (r + 1) >> 1, f = (r & 1) ? n - 1 : n + 1;
        const uint32_t y = j == 0 ? raw.yl[r] : j == RCAS_PXT + 1 ? raw.yr[r] : (raw.yw[r] >> (8 * (j - 1))) & 0xffu;
        const uint32_t uv = up_v2(raw.t[n][j], raw.t[f][j]);                     // 0x??VV??UU
        return y | ((uv & 0xffu) << 8) | (uv & 0xff0000u);
    }
    __device__ __forceinline__ Row row(const Raw& raw, int r) const
    {
        Row o;
#pragma unroll
        for (int j = 0; j < RCAS_PXT + 2; j++) o.p[j] = unpack(pixel(raw, r, j));
        return o;
    }
    __device__ __forceinline__ void centre(const Raw& raw, int r, uint32_t (&c)[RCAS_PXT]) const
    {
#pragma unroll
        for (int p = 0; p < RCAS_PXT; p++) c[p] = pixel(raw, r, p + 1);
    }
};

// lvk_hip_sharpen of the frame `src` describes, then lvk_hip_egress_yuv420 of the result, without that result: one thread per 4 x ROWS pixels.
template <class Src, bool NV12>
__global__ __launch_bounds__(256)
void k_rcas_420(Src src, PlanesOut out, int rows, int cols, float sharp, int flags)
{
    __shared__ float s_rmin[256], s_rmax[256];
    fill_tables(s_rmin, s_rmax);
    __syncthreads();

    const int x0 = (int)blockIdx.x * RCAS_STRIP_W + (int)(threadIdx.x & 63) * RCAS_PXT;
    const int y0 = ((int)blockIdx.y * 4 + (int)(threadIdx.x >> 6)) * ROWS;
    if (x0 >= cols || y0 >= rows) return;
    const bool half = x0 + RCAS_PXT > cols;                 // the row's last two columns

    typename Src::Raw raw;                                  // rows y0 - 1 .. y0 + ROWS, all in flight together
    src.load(raw, x0, y0, rows, cols, flags);
    Row win[3];
    win[0] = src.row(raw, 0);
    win[1] = src.row(raw, 1);
    uint32_t even[RCAS_PXT] = {};                           // the output pixels of the row pair's first row
#pragma unroll
    for (int r = 0; r < ROWS; r++)
    {
        const int y = y0 + r;
        if (y >= rows) break;
        const Row& up = win[r % 3];
        const Row& mid = win[(r + 1) % 3];
        Row& down = win[(r + 2) % 3];
        down = src.row(raw, r + 2);
        uint32_t centre[RCAS_PXT];
        src.centre(raw, r + 1, centre);
        const bool border_row = y == 0 || y >= rows - 1;
        uint32_t o[RCAS_PXT];
#pragma unroll
        for (int p = 0; p < RCAS_PXT; p++)
        {
            const int x = x0 + p;
            const bool border = border_row || x == 0 || x >= cols - 1;              // FSR.cl:475-481: copied
            const uint32_t px = rcas_pixel(up.p[p + 1], mid.p[p], mid.p[p + 1], mid.p[p + 2], down.p[p + 1], sharp, s_rmin, s_rmax);
            o[p] = border ? centre[p] : px;
        }
        // luma out
        store_luma4(out.y + (size_t)y * out.ys + x0, o, half, flags);
        if (!(r & 1))
        {
#pragma unroll
            for (int p = 0; p < RCAS_PXT; p++) even[p] = o[p];
            continue;
        }
        // chroma out: INTER_AREA 0.5 of each 2 x 2 quad of output pixels, border-copied ones included
        const int k = y >> 1, c0 = x0 >> 1;
        uint32_t u[2], v[2];
#pragma unroll
        for (int q = 0; q < 2; q++)
        {
            const uint32_t a = even[2 * q], b = even[2 * q + 1], c = o[2 * q], d = o[2 * q + 1];
            u[q] = (((a >> 8) & 0xffu) + ((b >> 8) & 0xffu) + ((c >> 8) & 0xffu) + ((d >> 8) & 0xffu) + 2) >> 2;
            v[q] = (((a >> 16) & 0xffu) + ((b >> 16) & 0xffu) + ((c >> 16) & 0xffu) + ((d >> 16) & 0xffu) + 2) >> 2;
        }
        if constexpr (NV12)
        {
            // (written out: through store_chroma2<true> this kernel's dword store comes out with the sources of one v_bitop3_b32 commuted, and the
            //  kernels' instruction streams are kept as they were -- DESIGN.md section 28)
            uint8_t* p = out.u + (size_t)k * out.us + 2 * c0;
            if (!half && (flags & kChromaWide)) *reinterpret_cast<uint32_t*>(p) = u[0] | (v[0] << 8) | (u[1] << 16) | (v[1] << 24);
            else
            {
                p[0] = (uint8_t)u[0]; p[1] = (uint8_t)v[0];
                if (!half) { p[2] = (uint8_t)u[1]; p[3] = (uint8_t)v[1]; }
            }
        }
        else store_chroma2<false>(out, k, c0, u, v, half, flags);
    }
}

template <class Src, bool NV12>
int launch_rcas_420(lvk_hip_ctx* ctx, const Src& src, const PlanesOut& out, int rows, int cols, float sharp, int flags)
{
    const dim3 block(256), grid((unsigned)((cols + RCAS_STRIP_W - 1) / RCAS_STRIP_W), (unsigned)((rows + 4 * ROWS - 1) / (4 * ROWS)));
    hipLaunchKernelGGL((k_rcas_420<Src, NV12>), grid, block, 0, ctx->stream, src, out, rows, cols, sharp, flags);
    LVK_HIP_CHECK(ctx, hipGetLastError());
    return LVK_HIP_OK;
}

} // namespace

// lvk_hip_scale_yuv420 behind its entry guard: also the I420 / I40A / NV12 route of lvk_hip_scale_obs (scaling_obs.hip)
int lvk_scale_420(lvk_hip_ctx* ctx, const char* name, const yuv420::PlaneSet& src, const yuv420::PlaneSet& dst, float sharpness)
{
    const int nv12 = dst.nv12, src_rows = src.rows, src_cols = src.cols, dst_rows = dst.rows, dst_cols = dst.cols;
    LVK_HIP_REQUIRE(ctx, well_formed(src) && well_formed(dst));
    LVK_HIP_REQUIRE(ctx, dst_cols >= src_cols && dst_rows >= src_rows);                      // Image.cpp:157
    LVK_HIP_REQUIRE(ctx, sharpness >= 0.0f && sharpness <= 1.0f);                            // LVK_ASSERT_01, Image.cpp:210 (a NaN fails both)
    int rc;
    // out of place: the sharpening and the chroma up-sampling read their neighbours
    const Spans src_spans = spans_of(src);
    if ((rc = require_out_of_place(ctx, name, src_spans.s, src_spans.n, dst)) != LVK_HIP_OK) return rc;
    const float sharp = exp2f(-2.0f * (1.0f - sharpness));                                   // Image.cpp:227
    const Planes in = src.in();
    const PlanesOut out = dst.out();

    if (dst_rows == src_rows && dst_cols == src_cols)       // lvk::upscale copies (Image.cpp:162-166): the sharpening reads the planes itself
    {
        const int flags = access_flags(&src, dst);
        return nv12 ? launch_rcas_420<PlanarSrc<true>, true>(ctx, PlanarSrc<true>{in}, out, dst_rows, dst_cols, sharp, flags)
                    : launch_rcas_420<PlanarSrc<false>, false>(ctx, PlanarSrc<false>{in}, out, dst_rows, dst_cols, sharp, flags);
    }
    const int out_flags = access_flags(nullptr, dst);

    // The two packed frames between the three launches come from the context's pool and go back to it once the last kernel is enqueued: whoever is
    // handed them next enqueues behind that kernel on this context's stream (lvk_hip.h, lvk_hip_free), and the steady state allocates nothing.
    const int s_step = (3 * src_cols + 3) & ~3, p_step = (3 * dst_cols + 3) & ~3;
    void *d_small = nullptr, *d_big = nullptr;
    if ((rc = lvk_hip_malloc(ctx, (size_t)s_step * src_rows, &d_small)) != LVK_HIP_OK) return rc;
    if ((rc = lvk_hip_malloc(ctx, (size_t)p_step * dst_rows, &d_big)) == LVK_HIP_OK
        && (rc = lvk_launch_ingest_yuv420(ctx, ctx->stream, in.y, in.ys, in.u, in.us, in.v, in.vs, nv12, src_rows, src_cols, d_small, s_step)) == LVK_HIP_OK
        && (rc = lvk_launch_upscale(ctx, ctx->stream, d_small, s_step, src_rows, src_cols, d_big, p_step, dst_rows, dst_cols, 1)) == LVK_HIP_OK)
    {
        const PackedSrc big{(const uint8_t*)d_big, p_step};
        rc = nv12 ? launch_rcas_420<PackedSrc, true>(ctx, big, out, dst_rows, dst_cols, sharp, out_flags)
                  : launch_rcas_420<PackedSrc, false>(ctx, big, out, dst_rows, dst_cols, sharp, out_flags);
    }
    (void)lvk_hip_free(ctx, d_small);
    (void)lvk_hip_free(ctx, d_big);
    return rc;
}

extern "C" int lvk_hip_scale_yuv420(lvk_hip_ctx* ctx,
                                    const void* d_y, int y_step, const void* d_u, int u_step, const void* d_v, int v_step, int src_rows, int src_cols,
                                    void* o_y, int oy_step, void* o_u, int ou_step, void* o_v, int ov_step, int dst_rows, int dst_cols,
                                    int nv12, float sharpness)
{
    LVK_HIP_ENTRY(ctx);
    return lvk_scale_420(ctx, "lvk_hip_scale_yuv420", plane_set(d_y, y_step, d_u, u_step, d_v, v_step, nv12, src_rows, src_cols),
                         plane_set(o_y, oy_step, o_u, ou_step, o_v, ov_step, nv12, dst_rows, dst_cols), sharpness);
}
