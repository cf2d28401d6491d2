// The tracker's chain optical flow -> fast_filter -> robust global motion as one launcher, and the diagnostics entry point over it.
//
// lvk_launch_track_chain is the chained block of FrameTracker::track (Vision/FrameTracker.cpp:140-168) as this library runs it: the flow kernel
// reads the points from device-visible host memory, fast_filter (Functions/Container.tpp:97-121) runs inside the RANSAC's first kernel for up to
// LVK_COMPACT_RANSAC_MAX points and as a kernel of its own beyond, the point count and the model choice may live on the device, and the last
// kernel may announce its results through a word in host memory.  lvk_hip_stab::track enqueues the chain through it; lvk_hip_track_chain lets a
// test select every one of these variants on inputs of its own.
#include "lvk_hip_internal.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>

int lvk_launch_track_chain(lvk_hip_ctx* ctx, const LvkTrackChain& c)
{
    int rc;
    const int n = c.n;
    if (c.prev_pyr &&
        (rc = lvk_launch_pyrlk(ctx, *c.prev_pyr, *c.next_pyr, c.h_pts, n, c.d_matched, c.d_status, c.win_w, c.win_h, c.max_count, c.epsilon, c.min_eig, c.d_pts,
                               c.d_und ? c.lens : nullptr, c.lens_sx, c.lens_sy, c.d_und, c.d_n)) != LVK_HIP_OK) return rc;
    const bool fused_compact = c.estimate && !c.separate_compact && n <= LVK_COMPACT_RANSAC_MAX;        // the RANSAC's first kernel compacts the flow result itself
    if (!fused_compact && (rc = lvk_launch_match_compact(ctx, c.d_pts, c.d_matched, c.d_status, n, c.d_p1, c.d_p2, c.d_count, c.h_count, c.h_matched, c.h_status,
                                                         c.d_und, (float)c.region_w, (float)c.region_h, c.d_n)) != LVK_HIP_OK) return rc;
    if (c.stage_boundary) c.stage_boundary(c.user);
    if (!c.estimate) return LVK_HIP_OK;
    if (fused_compact)
        return lvk_launch_compact_ransac(ctx, c.d_pts, c.d_matched, c.d_status, n, c.d_p1, c.d_p2, c.d_count, c.h_count, c.h_matched, c.h_status,
                                         c.d_und, (float)c.region_w, (float)c.region_h,
                                         c.threshold, (double)c.region_w, (double)c.region_h, c.full, c.d_ws, c.h_H, c.h_ninl, c.h_mask, c.d_n, c.d_full, c.done);
    return lvk_launch_ransac(ctx, c.d_p1, c.d_p2, n, c.threshold, (double)c.region_w, (double)c.region_h, c.full, c.d_ws, c.h_H, c.h_ninl, c.h_mask, c.d_count, c.d_full, c.done);
}

namespace {

// Every block of one lvk_hip_track_chain call; released together.
struct ChainBuffers
{
    std::vector<void*> dev, host;
    DevicePyramid P, N;
    template <class T> hipError_t device(T** p, size_t count) { hipError_t e = hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T)); if (e == hipSuccess) dev.push_back(*p); return e; }
    template <class T> hipError_t pinned(T** p, size_t count) { hipError_t e = hipHostMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocCoherent); if (e == hipSuccess) host.push_back(*p); return e; }
    ~ChainBuffers() { for (void* p : dev) (void)hipFree(p); for (void* p : host) (void)hipHostFree(p); P.release(); N.release(); }
};

} // namespace

extern "C" int lvk_hip_track_chain(lvk_hip_ctx* ctx, const lvk_track_chain_desc* d, lvk_track_chain_result* r)
{
    LVK_HIP_ENTRY(ctx);
    LVK_HIP_REQUIRE(ctx, d && r && d->prev && d->n_bound >= 1 && d->n_bound <= 4096 && d->region_w > 0 && d->region_h > 0);
    const bool flow = d->d_prev_img != nullptr;
    LVK_HIP_REQUIRE(ctx, flow ? (d->d_next_img && d->rows > 0 && d->cols > 0 && r->next_pts && r->flow_status && (!d->lens || r->flow_und))
                              : (d->matched && d->status && !d->lens));
    LVK_HIP_REQUIRE(ctx, r->mask && r->pairs_dev && r->mirror_matched && r->mirror_status);
    const int nb = d->n_bound, G = LVK_TRACK_CHAIN_GUARD;
    // where the kernels will put the count (the layout of a given `und` follows it: previous | matched, n_eff entries each)
    const int n_eff = d->count_on_device ? std::min(std::max(d->n_word, 0), nb) : nb;
    const bool with_und = flow ? d->lens != nullptr : d->und != nullptr;
    constexpr int FILL = LVK_TRACK_CHAIN_FILL;

    ChainBuffers b;
    hipStream_t st = ctx->stream;
    float2 *h_pts, *h_matched, *d_pts, *d_matched, *d_und, *d_p; uint8_t *h_status, *h_mask, *d_status; int *h_count, *h_ninl, *d_count, *d_words; double* h_H; unsigned* h_flag; void* d_ws;
    hipError_t e;
    if ((e = b.pinned(&h_pts, nb)) != hipSuccess || (e = b.pinned(&h_matched, nb)) != hipSuccess || (e = b.pinned(&h_status, nb)) != hipSuccess ||
        (e = b.pinned(&h_mask, nb)) != hipSuccess || (e = b.pinned(&h_count, 1)) != hipSuccess || (e = b.pinned(&h_ninl, 1)) != hipSuccess ||
        (e = b.pinned(&h_H, 9)) != hipSuccess || (e = b.pinned(&h_flag, 16)) != hipSuccess ||
        (e = b.device(&d_pts, nb)) != hipSuccess || (e = b.device(&d_matched, nb + 2 * G)) != hipSuccess || (e = b.device(&d_status, nb + 2 * G)) != hipSuccess ||
        (e = b.device(&d_und, 2 * nb + 2 * G)) != hipSuccess || (e = b.device(&d_p, 2 * nb)) != hipSuccess || (e = b.device(&d_count, 1)) != hipSuccess ||
        (e = b.device(&d_words, 2)) != hipSuccess || (e = hipMalloc(&d_ws, lvk_ransac_workspace_bytes(nb))) != hipSuccess)
        return ctx->fail(LVK_HIP_ERR_RUNTIME, hipGetErrorString(e));
    b.dev.push_back(d_ws);
    // everything the kernels may leave untouched carries the fill byte: what the caller reads back says which bytes a kernel wrote
    std::memcpy(h_pts, d->prev, (size_t)nb * sizeof(float2));
    std::memset(h_matched, FILL, (size_t)nb * sizeof(float2)); std::memset(h_status, FILL, nb); std::memset(h_mask, FILL, nb);
    *h_count = -1; *h_ninl = -1; *h_flag = 0;
    for (int q = 0; q < 9; q++) h_H[q] = 0.0;
    const int words[2] = {d->n_word, d->full_word};
    if ((e = hipMemsetAsync(d_pts, FILL, (size_t)nb * sizeof(float2), st)) != hipSuccess ||
        (e = hipMemsetAsync(d_matched, FILL, (size_t)(nb + 2 * G) * sizeof(float2), st)) != hipSuccess ||
        (e = hipMemsetAsync(d_status, FILL, (size_t)(nb + 2 * G), st)) != hipSuccess ||
        (e = hipMemsetAsync(d_und, FILL, (size_t)(2 * nb + 2 * G) * sizeof(float2), st)) != hipSuccess ||
        (e = hipMemsetAsync(d_p, FILL, (size_t)2 * nb * sizeof(float2), st)) != hipSuccess ||
        (e = hipMemsetAsync(d_count, FILL, sizeof(int), st)) != hipSuccess ||
        (e = hipMemcpyAsync(d_words, words, sizeof(words), hipMemcpyHostToDevice, st)) != hipSuccess)
        return ctx->fail(LVK_HIP_ERR_RUNTIME, hipGetErrorString(e));

    LvkTrackChain c;
    LensModel lens_model;
    if (flow)
    {
        int rc;
        if ((rc = b.P.allocate(ctx, d->rows, d->cols, d->max_level, d->win_w, d->win_h)) != LVK_HIP_OK || (rc = b.N.allocate(ctx, d->rows, d->cols, d->max_level, d->win_w, d->win_h)) != LVK_HIP_OK) return rc;
        if ((e = hipMemcpy2DAsync(const_cast<uint8_t*>(b.P.args.lv[0].img), b.P.args.lv[0].step, d->d_prev_img, d->prev_step, d->cols, d->rows, hipMemcpyDeviceToDevice, st)) != hipSuccess ||
            (e = hipMemcpy2DAsync(const_cast<uint8_t*>(b.N.args.lv[0].img), b.N.args.lv[0].step, d->d_next_img, d->next_step, d->cols, d->rows, hipMemcpyDeviceToDevice, st)) != hipSuccess)
            return ctx->fail(LVK_HIP_ERR_RUNTIME, hipGetErrorString(e));
        if ((rc = b.P.build(ctx)) != LVK_HIP_OK || (rc = b.N.build(ctx)) != LVK_HIP_OK) return rc;
        if (d->lens)
        {
            if (lvk_lens_model_build(*d->lens, d->lens_rows, d->lens_cols, lens_model) != LVK_HIP_OK) return ctx->fail(LVK_HIP_ERR_ARG, "invalid camera profile");
            c.lens = &lens_model; c.lens_sx = d->lens_sx; c.lens_sy = d->lens_sy;
        }
        c.prev_pyr = &b.P.args; c.next_pyr = &b.N.args; c.h_pts = h_pts;
        c.win_w = d->win_w; c.win_h = d->win_h; c.max_count = d->max_count; c.epsilon = d->epsilon; c.min_eig = d->min_eig;
    }
    else
    {
        // a flow result as the flow kernel leaves it: the device copy of the points, the matches, the flags, the corrected positions
        if ((e = hipMemcpyAsync(d_pts, d->prev, (size_t)nb * sizeof(float2), hipMemcpyHostToDevice, st)) != hipSuccess ||
            (e = hipMemcpyAsync(d_matched + G, d->matched, (size_t)nb * sizeof(float2), hipMemcpyHostToDevice, st)) != hipSuccess ||
            (e = hipMemcpyAsync(d_status + G, d->status, (size_t)nb, hipMemcpyHostToDevice, st)) != hipSuccess ||
            (d->und && n_eff > 0 && (e = hipMemcpyAsync(d_und + G, d->und, (size_t)2 * n_eff * sizeof(float2), hipMemcpyHostToDevice, st)) != hipSuccess))
            return ctx->fail(LVK_HIP_ERR_RUNTIME, hipGetErrorString(e));
    }
    c.n = nb; c.d_n = d->count_on_device ? d_words : nullptr;
    c.full = d->full != 0; c.d_full = d->model_on_device ? d_words + 1 : nullptr;
    c.d_pts = d_pts; c.d_matched = d_matched + G; c.d_status = d_status + G; c.d_und = with_und ? d_und + G : nullptr;
    c.d_p1 = d_p; c.d_p2 = d_p + nb; c.d_count = d_count; c.h_count = h_count; c.h_matched = h_matched; c.h_status = h_status;
    c.region_w = d->region_w; c.region_h = d->region_h; c.threshold = d->threshold;
    c.separate_compact = d->separate_compact != 0;
    c.d_ws = d_ws; c.h_H = h_H; c.h_ninl = h_ninl; c.h_mask = h_mask;
    if (d->host_signal) c.done = LvkHostSignal{h_flag, 0x5EED0001u};
    int rc = lvk_launch_track_chain(ctx, c);
    if (rc != LVK_HIP_OK) { (void)hipStreamSynchronize(st); return rc; }

    r->signalled = 0;
    if (c.done.flag)
    {
        // as lvk_hip_stab::track waits: spin on the word (acquire), bounded; the results and the mirrors are read BEFORE any stream wait
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 0;; spins++)
        {
            if (__atomic_load_n(c.done.flag, __ATOMIC_ACQUIRE) == c.done.seq) { r->signalled = 1; break; }
            if ((spins & 63u) == 63u && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
        }
    }
    if (!r->signalled)
    {
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return ctx->fail(LVK_HIP_ERR_RUNTIME, hipGetErrorString(e));
        if (c.done.flag && __atomic_load_n(c.done.flag, __ATOMIC_ACQUIRE) == c.done.seq) r->signalled = 1;      // (a machine busy enough to outlast the spin)
    }
    std::memcpy(r->H, h_H, 9 * sizeof(double));
    const int ninl = *h_ninl;
    r->count_host = *h_count;
    std::memcpy(r->mask, h_mask, nb);
    std::memcpy(r->mirror_matched, h_matched, (size_t)nb * sizeof(float2));
    std::memcpy(r->mirror_status, h_status, nb);
    // ... then device memory (these copies wait for the stream)
    r->count_dev = -1;
    if ((e = hipMemcpyAsync(&r->count_dev, d_count, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipMemcpyAsync(r->pairs_dev, d_p, (size_t)2 * nb * sizeof(float2), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (flow && ((e = hipMemcpyAsync(r->next_pts, d_matched, (size_t)(nb + 2 * G) * sizeof(float2), hipMemcpyDeviceToHost, st)) != hipSuccess ||
                  (e = hipMemcpyAsync(r->flow_status, d_status, (size_t)(nb + 2 * G), hipMemcpyDeviceToHost, st)) != hipSuccess)) ||
        (flow && r->flow_und && (e = hipMemcpyAsync(r->flow_und, d_und, (size_t)(2 * nb + 2 * G) * sizeof(float2), hipMemcpyDeviceToHost, st)) != hipSuccess) ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return ctx->fail(LVK_HIP_ERR_RUNTIME, hipGetErrorString(e));
    if (d->host_signal && !r->signalled) return ctx->fail(LVK_HIP_ERR_RUNTIME, "the chain completed without storing its host signal word");
    r->rc = ninl >= 0 ? ninl : -10 + ninl;
    return LVK_HIP_OK;
}
