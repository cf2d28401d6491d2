// Frames in HOST memory either side of the filter (the 4:2:0 path and, through lvk_hip_stab_push_obs_host, every other OBS format): staging planes, transfer streams, deferred downloads, upload look-ahead.
// Reference: FrameIngest::upload_planes / download_planes around to_ocl -> filter -> to_obs (Modules/OBS-Plugin/Interop/FrameIngest.cpp:415-474,
// 494-602, VisionFilter.cpp:151-212).
#include "stab_state.hpp"

using namespace lvkstab;

int lvk_hip_stab::ensure_hostio(int rows, int cols, size_t in_bytes)
{
    HostIO& h = hostio;
    const bool same = h.rows == rows && h.cols == cols && h.up;
    if (same && h.in_bytes >= in_bytes) return LVK_HIP_OK;
    // (an input slot only grows while the frame size stays: entries of different formats that alternate at one size do not rebuild the slots on every push)
    const size_t in_keep = same ? h.in_bytes : 0;
    LVK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (remap_stream) LVK_HIP_CHECK(ctx, hipStreamSynchronize(remap_stream));
    // (LVK_HIP_HOST_SINK=copy: the last emitted frame of the old size may not have been handed to the copy engine yet -- it was reported as
    //  produced, so it goes out before its staging planes are freed)
    { const int frc = flush_download(true); if (frc != LVK_HIP_OK) return frc; }
    free_hostio();
    const size_t bytes = (size_t)rows * cols + 2 * (size_t)((rows + 1) / 2) * ((cols + 1) / 2);
    const size_t in_cap = std::max(bytes, std::max(in_bytes, in_keep));
    for (auto& p : h.d_in) LVK_HIP_CHECK(ctx, hipMalloc(&p, in_cap));
    for (auto& p : h.d_out) LVK_HIP_CHECK(ctx, hipMalloc(&p, bytes));
    // The streams that exist are the streams that are used: every stream of the process is a queue the runtime maps onto its few hardware
    // queues, and a transfer stream that lands on the hardware queue of the caller's stream stalls the tracker's kernels behind its copies
    // (measured, 4K free running with look-ahead: 3 140-3 190 frames/s with ONE upload stream, 2 700-2 850 with two, 2 040-2 130 with a third
    // side stream next to them).  The second upload stream (chroma of a frame pushed without look-ahead) and the download streams
    // (LVK_HIP_HOST_SINK=copy) are made on first use.  [The mechanism was narrowed down with scripts/sdma_interference_probe.py and the timelines
    // G-H of profiles/r03_host_feed_timeline.txt: whichever kernel comes first on the tracking stream after a look-ahead upload has started
    // -- the downscale, the flow kernel, a 5 KB copy, even a kernel that only stores its arguments -- ends ~220 us after that upload began.]
    { const int rcs = host_stream(h.up); if (rcs != LVK_HIP_OK) return rcs; }
    ctx->sync_hooks.emplace_back((void*)this, [this]() { return flush_download(true); });          // lvk_hip_sync() covers the transfers
    for (int i = 0; i < HostIO::K_IN; i++)
    {
        LVK_HIP_CHECK(ctx, hipEventCreateWithFlags(&h.y_done[i], hipEventDisableTiming));
        LVK_HIP_CHECK(ctx, hipEventCreateWithFlags(&h.c_done[i], hipEventDisableTiming));
    }
    for (int i = 0; i < HostIO::K_OUT; i++)
    {
        LVK_HIP_CHECK(ctx, hipEventCreateWithFlags(&h.out_ready[i], hipEventDisableTiming));
        LVK_HIP_CHECK(ctx, hipEventCreateWithFlags(&h.down_done[i], hipEventDisableTiming));
        h.down_armed[i] = false;
    }
    h.rows = rows; h.cols = cols; h.in_bytes = in_cap; h.in_next = h.out_next = 0; h.last_down = -1; h.ahead.clear();
    return LVK_HIP_OK;
}

// the blocks lvk_hip_stab_push_gray_host still owns (the streams that read them have been synchronised by the caller)
void lvk_hip_stab::free_gray_host()
{
    for (void* p : gray_host_live) (void)lvk_hip_free(ctx, p);
    gray_host_live.clear();
    if (gray_up_done) { (void)hipEventDestroy(gray_up_done); gray_up_done = nullptr; }
    if (gray_fence) { (void)hipEventDestroy(gray_fence); gray_fence = nullptr; }
}

void lvk_hip_stab::free_hostio()
{
    HostIO& h = hostio;
    auto& aux = ctx->aux_streams;
    { auto& hooks = ctx->sync_hooks; hooks.erase(std::remove_if(hooks.begin(), hooks.end(), [this](const auto& kv) { return kv.first == (void*)this; }), hooks.end()); }
    h.pending.valid = false;
    for (hipStream_t s : {h.up, h.down, h.down2})
        if (s)
        {
            (void)hipStreamSynchronize(s);
            { std::lock_guard<std::mutex> alock(ctx->aux_mutex); aux.erase(std::remove(aux.begin(), aux.end(), s), aux.end()); }
            (void)hipStreamDestroy(s);
        }
    h.up = h.down = h.down2 = nullptr;
    for (auto& p : h.d_in) { if (p) (void)hipFree(p); p = nullptr; }
    for (auto& p : h.d_out) { if (p) (void)hipFree(p); p = nullptr; }
    for (auto* arr : {h.y_done, h.c_done}) for (int i = 0; i < HostIO::K_IN; i++) if (arr[i]) { (void)hipEventDestroy(arr[i]); arr[i] = nullptr; }
    for (auto* arr : {h.out_ready, h.down_done}) for (int i = 0; i < HostIO::K_OUT; i++) if (arr[i]) { (void)hipEventDestroy(arr[i]); arr[i] = nullptr; }
    h.rows = h.cols = 0; h.in_bytes = 0;
}

// The uploads of one host frame into staging slot k, on the upload stream.
//   * pushed now (the caller waits for this frame): luma, event, chroma, event -- the tracker starts on the luma plane while the chroma planes
//     are still on the link;
//   * announced ahead (the link is the bottleneck, not this frame's latency): ONE copy when the planes are contiguous.  A copy engine
//     that has to wait for anything but its own previous copy -- here: the event between the two copies -- is restarted by the
//     runtime's signal handler 60-80 us late (timeline in profiles/r03_host_feed_timeline.txt): 341 us of link time per frame instead of 265.
int lvk_hip_stab::host_upload(const HostPlane* pl, int n, int k, bool ahead)
{
    HostIO& io = hostio;
    // the slot holds the planes tight, one after the other (Y | U | V, Y | UV, or the one plane of a packed format)
    uint8_t* d[3] = {nullptr, nullptr, nullptr}; size_t total = 0;
    for (int i = 0; i < n; i++) { d[i] = (uint8_t*)io.d_in[k] + total; total += (size_t)pl[i].width * pl[i].rows; }
    LVK_HIP_REQUIRE(ctx, n >= 1 && n <= 3 && total <= io.in_bytes);
    // (the staging slot is free: the kernels that read it -- downscale, conversion -- were complete when the push that used it returned)
    auto copy_plane = [&](void* dst, const HostPlane& h, hipStream_t s) -> hipError_t {
        if (h.step == h.width) return hipMemcpyAsync(dst, h.p, (size_t)h.width * h.rows, hipMemcpyHostToDevice, s);
        return hipMemcpy2DAsync(dst, h.width, h.p, h.step, h.width, h.rows, hipMemcpyHostToDevice, s);
    };
    // planes i and i + 1 lie back to back in host memory, as in the slot
    auto follows = [&](int i) { return pl[i].step == pl[i].width && pl[i + 1].step == pl[i + 1].width &&
                                       (const uint8_t*)pl[i + 1].p == (const uint8_t*)pl[i].p + (size_t)pl[i].width * pl[i].rows; };
    bool contiguous = pl[0].step == pl[0].width;
    for (int i = 0; i + 1 < n; i++) contiguous = contiguous && follows(i);
    // ONE upload stream.  (hipMemcpyAsync blocks the host while an earlier copy of the same stream is still in flight, which two alternating
    // streams would avoid, but a second stream costs more than that wait: see ensure_hostio; 3 140-3 190 against 2 700-2 850 frames/s.)
    hipStream_t us = io.up;
    if (n == 1 || (ahead && contiguous))
    {
        // a packed format's one plane, or a whole frame announced ahead: one event covers it
        if (contiguous) LVK_HIP_CHECK(ctx, hipMemcpyAsync(d[0], pl[0].p, total, hipMemcpyHostToDevice, us));
        else LVK_HIP_CHECK(ctx, copy_plane(d[0], pl[0], us));
        LVK_HIP_CHECK(ctx, hipEventRecord(io.c_done[k], us));
        io.y_is_c[k] = true;
        return LVK_HIP_OK;
    }
    io.y_is_c[k] = false;
    LVK_HIP_CHECK(ctx, copy_plane(d[0], pl[0], us));                                 // luma and chroma of a frame pushed now: one stream, in order
    LVK_HIP_CHECK(ctx, hipEventRecord(io.y_done[k], us));
    if (n == 3 && follows(1))
    {
        LVK_HIP_CHECK(ctx, hipMemcpyAsync(d[1], pl[1].p, (size_t)pl[1].width * pl[1].rows + (size_t)pl[2].width * pl[2].rows, hipMemcpyHostToDevice, us));      // U | V contiguous: one copy
    }
    else for (int i = 1; i < n; i++) LVK_HIP_CHECK(ctx, copy_plane(d[i], pl[i], us));
    LVK_HIP_CHECK(ctx, hipEventRecord(io.c_done[k], us));
    return LVK_HIP_OK;
}

// ---- what lvk_hip_stab_push_yuv420_host and lvk_hip_stab_push_obs_host share around the push they wrap
// what a host entry hands to that push (events to wait for, the sink hints) never outlives the entry, whichever way it returns
struct HostPushHooks
{
    lvk_hip_stab* s;
    ~HostPushHooks() { s->remap_wait = nullptr; s->ingest_wait[0] = s->ingest_wait[1] = nullptr; s->host_free_running_hint = false; s->host_direct_now = false; }
};

int lvk_hip_stab::host_stage(const HostPlane* pl, int n, int* k)
{
    *k = hostio.in_next; hostio.in_next = (*k + 1) % HostIO::K_IN;
    return host_upload(pl, n, *k, false);
}

// direct: the wrapped push's kernels store into the caller's pinned planes themselves
int lvk_hip_stab::host_begin_push(int k, bool direct)
{
    HostIO& io = hostio;
    LVK_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, io.y_is_c[k] ? io.c_done[k] : io.y_done[k], 0));           // the tracker needs the luma plane only
    ingest_wait[0] = io.y_is_c[k] ? nullptr : io.y_done[k]; ingest_wait[1] = io.c_done[k];
    host_free_running_hint = caller_free_running_now() ||
                             (io.last_end.time_since_epoch().count() != 0 && std::chrono::steady_clock::now() - io.last_end < std::chrono::microseconds(15));
    if (direct)
    {
        // a download of an earlier frame may still be writing the caller's (possibly the same) host planes: the kernel's stores follow it
        const int rc = flush_download(true);
        if (rc != LVK_HIP_OK) return rc;
        if (io.last_down >= 0 && io.down_armed[io.last_down]) remap_wait = io.down_done[io.last_down];
    }
    return LVK_HIP_OK;
}

int lvk_hip_stab::host_end_push(int k)
{
    // "consumed on return": the conversion (which waited for both uploads) has finished in every mode by now; the event costs nothing then
    LVK_HIP_CHECK(ctx, hipEventSynchronize(hostio.c_done[k]));
    return LVK_HIP_OK;
}

// Deferred download (LVK_HIP_HOST_SINK=copy): the D2H copy of an emitted frame is handed to the runtime only once the remap that wrote the
// device planes is KNOWN to be complete, on a stream with nothing pending -- a copy that has to wait for a kernel is performed by the
// runtime with a blit kernel (which saturates the link's write queue and stalls every other kernel), an unencumbered one by a copy engine.
// wait = false: only if the remap has finished (polled at the start and at the end of the following push); true: wait for it.
int lvk_hip_stab::flush_download(bool wait)
{
    HostIO& io = hostio;
    if (!io.pending.valid) return LVK_HIP_OK;
    const int j = io.pending.slot;
    const hipError_t q = hipEventQuery(io.out_ready[j]);
    if (q == hipErrorNotReady) { (void)hipGetLastError(); if (!wait) return LVK_HIP_OK; LVK_HIP_CHECK(ctx, hipEventSynchronize(io.out_ready[j])); }
    else if (q != hipSuccess) return fail(LVK_HIP_ERR_RUNTIME, hipGetErrorString(q));
    const int rows = io.rows, cols = io.cols, nv12 = io.pending.nv12, crows = rows / 2, ccols = nv12 ? cols : cols / 2;
    uint8_t* o_y = (uint8_t*)io.d_out[j]; uint8_t* o_u = o_y + (size_t)rows * cols; uint8_t* o_v = nv12 ? o_u : o_u + (size_t)crows * ccols;
    { int rcs; if ((rcs = host_stream(io.down)) != LVK_HIP_OK || (rcs = host_stream(io.down2)) != LVK_HIP_OK) return rcs; }
    hipStream_t ds = (j & 1) ? io.down2 : io.down;           // (hipMemcpyAsync blocks the host while an earlier copy of the same stream is in flight)
    auto copy_plane = [&](void* dst, int dpitch, const void* src, int spitch, int width, int height) -> hipError_t {
        if (spitch == width && dpitch == width) return hipMemcpyAsync(dst, src, (size_t)width * height, hipMemcpyDeviceToHost, ds);
        return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, ds);
    };
    const auto& p = io.pending;
    {
        // a destination the previous download (on the other stream) may still be writing: order behind it
        const uint8_t* lo = (const uint8_t*)p.y; const uint8_t* hi = lo + (size_t)p.ys * rows;
        if (io.last_down >= 0 && io.last_down != j && io.down_armed[io.last_down] && io.last_dst_lo < hi && lo < io.last_dst_hi)
            LVK_HIP_CHECK(ctx, hipStreamWaitEvent(ds, io.down_done[io.last_down], 0));
        io.last_dst_lo = lo; io.last_dst_hi = hi;
    }
    const bool contiguous = p.ys == cols && p.us == ccols && (uint8_t*)p.u == (uint8_t*)p.y + (size_t)rows * cols &&
                            (nv12 || (p.vs == ccols && (uint8_t*)p.v == (uint8_t*)p.u + (size_t)crows * ccols));
    if (contiguous) LVK_HIP_CHECK(ctx, hipMemcpyAsync(p.y, o_y, (size_t)rows * cols + (size_t)(nv12 ? 1 : 2) * crows * ccols, hipMemcpyDeviceToHost, ds));
    else
    {
        LVK_HIP_CHECK(ctx, copy_plane(p.y, p.ys, o_y, cols, cols, rows));
        LVK_HIP_CHECK(ctx, copy_plane(p.u, p.us, o_u, ccols, ccols, crows));
        if (!nv12) LVK_HIP_CHECK(ctx, copy_plane(p.v, p.vs, o_v, ccols, ccols, crows));
    }
    LVK_HIP_CHECK(ctx, hipEventRecord(io.down_done[j], ds));
    io.down_armed[j] = true; io.last_down = j;
    io.pending.valid = false;
    return LVK_HIP_OK;
}

// Announced frames that will not be pushed (the caller stopped, seeked or restarted): their uploads are waited for -- the staging slots are
// rewritten by the next upload on the same stream anyway, but the caller's planes must not be read after this returns -- and forgotten.
int lvk_hip_stab::cancel_lookahead()
{
    HostIO& io = hostio;
    if (io.up) LVK_HIP_CHECK(ctx, hipStreamSynchronize(io.up));
    io.ahead.clear();
    for (hipEvent_t& e : ingest_wait) e = nullptr;
    return LVK_HIP_OK;
}

extern "C" {

// Look-ahead for streaming callers (the reader thread of VideoFilter::stream uploads frames ahead of the filter thread,
// Filters/VideoFilter.cpp:62-209): starts the upload of the planes that the NEXT lvk_hip_stab_push_yuv420_host call will push, so that the
// link is busy with frame n + 1 while frame n is tracked: announce frame n + 1, THEN push frame n.  Announced frames are pushed in order; at
// most two may be outstanding.  The planes stay the caller's until their push has returned.
int lvk_hip_stab_prefetch_yuv420_host(lvk_hip_stab* st, const void* h_y, int y_step, const void* h_u, int u_step, const void* h_v, int v_step, int nv12, int rows, int cols)
{
    if (!st) return LVK_HIP_ERR_ARG;
    lvk_device_guard device_guard(st->ctx);
    lvk_hip_ctx* ctx = st->ctx;
    LVK_HIP_REQUIRE(ctx, h_y && h_u && (nv12 || h_v) && rows > 0 && cols > 0 && rows % 2 == 0 && cols % 2 == 0);
    LVK_HIP_REQUIRE(ctx, y_step >= cols && u_step >= (nv12 ? cols : cols / 2) && (nv12 || v_step >= cols / 2));
    int rc;
    HostPlane in[3]; const int n_in = lvk_hip_stab::planes420(h_y, y_step, h_u, u_step, h_v, v_step, nv12, rows, cols, in);
    if ((rc = st->require_pinned_planes(in, n_in, "lvk_hip_stab_prefetch_yuv420_host")) != LVK_HIP_OK) return rc;
    if ((rc = st->ensure_hostio(rows, cols)) != LVK_HIP_OK) return rc;
    lvk_hip_stab::HostIO& io = st->hostio;
    // two staging slots: the frame being pushed and the one on the link -- at most two announced frames that have not been pushed yet
    LVK_HIP_REQUIRE(ctx, io.ahead.size() < (size_t)lvk_hip_stab::HostIO::K_IN);
    const int k = io.in_next; io.in_next = (k + 1) % lvk_hip_stab::HostIO::K_IN;
    if ((rc = st->host_upload(in, n_in, k, true)) != LVK_HIP_OK) return rc;
    io.ahead.push_back({k, {h_y, h_u, nv12 ? h_u : h_v}, rows, cols, nv12 ? 1 : 0});
    return LVK_HIP_OK;
}

// Host-resident frames: FrameIngest::upload_planes -> to_ocl -> StabilizationFilter::filter -> to_obs -> download_planes in one call
// (Modules/OBS-Plugin/Interop/FrameIngest.cpp:415-474,494-602, VisionFilter.cpp:151-212) -- SURVEY.md section 8d's metric ("p99 ms/frame
// including H2D of the input and D2H of the output when frames are host-resident").  h_* / oh_*: planes in PINNED host memory
// (lvk_hip_host_malloc, hipHostMalloc, hipHostRegister).  What the link gives (profiles/r03_pcie_probe.txt): 55 GB/s one way, 46.8 GB/s
// each way with ONE copy-engine stream per direction at once, 31 with two per direction -- so:
//   in:  one upload stream; the luma plane goes first and the tracker's stream waits for IT only (downscale, pyramid, flow and the motion
//        estimate run while the chroma planes are still on the link); the 4:2:0 conversion waits for both.  Planes that are contiguous in
//        host memory (the OBS frame layout, FrameIngest.cpp:441-453 "uploads are done in bulk") travel as one copy each.
//   out: a caller that waits for every frame gets the planes written by the remap kernel ITSELF into the pinned host planes (zero copy:
//        the stores go over the link as they are produced -- no remap -> download serialisation, ~0.1 ms less per frame); a caller that
//        runs free gets remap -> device planes -> one download on the download stream behind an event (a copy engine both ways is the
//        faster pair when the link is saturated: 46.8 vs 43 GB/s).  Same pixels either way.
// Input planes are consumed when the call returns; output planes are complete after lvk_hip_sync().
int lvk_hip_stab_push_yuv420_host(lvk_hip_stab* st, const void* h_y, int y_step, const void* h_u, int u_step, const void* h_v, int v_step, int nv12,
                                  int rows, int cols, uint64_t timestamp,
                                  void* oh_y, int oy_step, void* oh_u, int ou_step, void* oh_v, int ov_step, int o_rows,
                                  int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted)
{
    if (!st) return LVK_HIP_ERR_ARG;
    lvk_device_guard device_guard(st->ctx);
    lvk_hip_ctx* ctx = st->ctx;
    if (produced) *produced = 0;
    LVK_HIP_REQUIRE(ctx, h_y && h_u && (nv12 || h_v) && rows > 0 && cols > 0 && rows % 2 == 0 && cols % 2 == 0);
    LVK_HIP_REQUIRE(ctx, y_step >= cols && u_step >= (nv12 ? cols : cols / 2) && (nv12 || v_step >= cols / 2));
    int rc;
    HostPlane in[3]; const int n_in = lvk_hip_stab::planes420(h_y, y_step, h_u, u_step, h_v, v_step, nv12, rows, cols, in);
    if ((rc = st->require_pinned_planes(in, n_in, "lvk_hip_stab_push_yuv420_host")) != LVK_HIP_OK) return rc;
    // the frame this push emits is the DELAYED one, at its own size (frames queued before a resize leave at the old size): the output planes are
    // checked -- pitch, rows, pinned over their whole extent -- against THAT geometry
    QueuedFrame due{};
    const bool will_emit = st->next_output(QueuedFrame{nullptr, 3 * cols, rows, cols, timestamp, LVK_FORMAT_YUV}, &due);
    const int erows = will_emit ? due.rows : rows, ecols = will_emit ? due.cols : cols;
    // (planes given to a push that emits nothing are held to the incoming frame's geometry: pageable memory is refused whenever it is seen)
    if (oh_y && oh_u && (nv12 || oh_v))
    {
        if (!(oy_step >= ecols && ou_step >= (nv12 ? ecols : ecols / 2) && (nv12 || ov_step >= ecols / 2) && o_rows >= erows))
            return st->fail(LVK_HIP_ERR_ARG, "the output planes do not hold the frame this push emits: " + std::to_string(ecols) + " x " + std::to_string(erows) +
                                             " (the DELAYED frame's own size -- lvk_hip_stab_next_output); nothing was queued");
        HostPlane out[3]; const int n_out = lvk_hip_stab::planes420(oh_y, oy_step, oh_u, ou_step, oh_v, ov_step, nv12, erows, ecols, out);
        if ((rc = st->require_pinned_planes(out, n_out, "lvk_hip_stab_push_yuv420_host (output)")) != LVK_HIP_OK) return rc;
    }
    if ((rc = st->ensure_hostio(rows, cols)) != LVK_HIP_OK) return rc;
    lvk_hip_stab::HostIO& io = st->hostio;
    if ((rc = st->flush_download(false)) != LVK_HIP_OK) return rc;
    auto tr_last = std::chrono::steady_clock::now();
    auto tr_mark = [&](int k) { if (!st->trace.on) return; const auto now = std::chrono::steady_clock::now(); st->host_trace_acc[k] += std::chrono::duration<double, std::micro>(now - tr_last).count(); tr_last = now; };
    const int crows = rows / 2, ccols = nv12 ? cols : cols / 2;                     // chroma plane geometry (bytes per row)
    int k;
    if (!io.ahead.empty())
    {
        // its upload has been under way since the look-ahead call; look-ahead frames are pushed in the order they were announced
        const auto a = io.ahead.front();
        if (!(a.key[0] == h_y && a.key[1] == h_u && a.key[2] == (nv12 ? h_u : h_v) && a.rows == rows && a.cols == cols && a.nv12 == (nv12 ? 1 : 0)))
            return st->fail(LVK_HIP_ERR_ARG, "lvk_hip_stab_push_yuv420_host: another frame has been announced (lvk_hip_stab_prefetch_yuv420_host) and not pushed yet -- "
                                             "announced frames are pushed in the order announced, and a frame pushed while announcements are outstanding must be the oldest of them");
        io.ahead.pop_front();
        k = a.slot;
    }
    else
    {
        if ((rc = st->host_stage(in, n_in, &k)) != LVK_HIP_OK) return rc;
    }
    uint8_t* d_y = (uint8_t*)io.d_in[k];
    uint8_t* d_u = d_y + (size_t)rows * cols;
    uint8_t* d_v = nv12 ? d_u : d_u + (size_t)crows * ccols;
    tr_mark(0);
    HostPushHooks clear_hooks{st};

    // where the output planes are written: by the remap kernel itself, straight into the pinned host planes (measured, 4K, free running:
    // 2 800 frames/s against 2 490 for remap -> device planes -> download, whose D2H copy the runtime performs with a blit KERNEL that
    // saturates the link's write queue and stalls every other kernel's memory traffic while it runs -- timelines under profiles/).
    // LVK_HIP_HOST_SINK=copy keeps the download route for comparison.
    const bool have_out = oh_y && oh_u && (nv12 || oh_v);
    // (a frame of an EARLIER size -- the staging planes of the download route have the new one -- always leaves through the kernel's own stores)
    const bool direct = have_out && (st->host_sink_mode != 2 || erows != rows || ecols != cols);
    if ((rc = st->host_begin_push(k, direct)) != LVK_HIP_OK) return rc;
    const int j = io.out_next;
    uint8_t* o_y = nullptr; uint8_t* o_u = nullptr; uint8_t* o_v = nullptr;
    int oys = oy_step, ous = ou_step, ovs = ov_step;
    if (have_out && !direct)
    {
        o_y = (uint8_t*)io.d_out[j]; o_u = o_y + (size_t)rows * cols; o_v = nv12 ? o_u : o_u + (size_t)crows * ccols;
        oys = cols; ous = ccols; ovs = ccols;
        if (io.pending.valid && io.pending.slot == j) { if ((rc = st->flush_download(true)) != LVK_HIP_OK) return rc; }
        if (io.down_armed[j]) st->remap_wait = io.down_done[j];                      // the download that last read this slot
    }
    else if (have_out) { o_y = (uint8_t*)oh_y; o_u = (uint8_t*)oh_u; o_v = (uint8_t*)oh_v; }
    int prod = 0;
    tr_mark(1);
    st->host_direct_now = direct;
    rc = lvk_hip_stab_push_yuv420(st, d_y, cols, d_u, ccols, d_v, ccols, nv12, rows, cols, timestamp, o_y, oys, o_u, ous, o_v, ovs, direct ? o_rows : rows, &prod, out_timestamp, emitted);
    tr_mark(2);
    { const int erc = st->host_end_push(k); if (erc != LVK_HIP_OK) return erc; }
    tr_mark(3);
    if (rc != LVK_HIP_OK) return rc;
    if ((rc = st->flush_download(false)) != LVK_HIP_OK) return rc;                  // the previous frame's remap has usually finished by now
    if (prod && have_out && !direct)
    {
        if ((rc = st->flush_download(true)) != LVK_HIP_OK) return rc;               // (one deferred download at a time)
        io.out_next = (j + 1) % lvk_hip_stab::HostIO::K_OUT;
        hipStream_t os = (hipStream_t)lvk_hip_stab_output_stream(st);
        LVK_HIP_CHECK(ctx, hipEventRecord(io.out_ready[j], os));
        io.pending.valid = true; io.pending.slot = j; io.pending.y = oh_y; io.pending.u = oh_u; io.pending.v = oh_v;
        io.pending.ys = oy_step; io.pending.us = ou_step; io.pending.vs = ov_step; io.pending.nv12 = nv12 ? 1 : 0;
        io.down_armed[j] = false;
    }
    if (produced) *produced = prod;
    tr_mark(4); st->host_trace_n++;
    io.last_end = std::chrono::steady_clock::now();
    return LVK_HIP_OK;
}

// The host entry for EVERY three-channel OBS video format FrameIngest::Select accepts; Y800, a one-channel frame, goes through lvk_hip_stab_push_gray_host
// below.  It is lvk_hip_stab_push_obs with the planes in pinned host memory --
// what FrameIngest::upload_planes / download_planes do for every format alike (Modules/OBS-Plugin/Interop/FrameIngest.cpp:415-474).  I420 / I40A / NV12
// are lvk_hip_stab_push_yuv420_host's.  The other formats share its machinery:
//   in:  the planes go through the one upload stream into a staging slot sized for the format; planar formats luma first with its own event (the tracker
//        starts on it), packed formats one copy and one event; planes contiguous in host memory travel as one copy;
//   out: the fused remap + egress sinks (remap_obs.hip) store into the caller's pinned planes themselves; the formats without a fused sink (BGR3, RGBA,
//        BGRA, BGRX) take remap -> packed buffer -> egress, whose destination is the host planes.  No download route through device planes.
// Refused before anything changes: everything lvk_hip_stab_push_obs refuses, pageable planes, and a push while 4:2:0 look-ahead frames are outstanding.
int lvk_hip_stab_push_obs_host(lvk_hip_stab* st, int video_format, const void* const h_planes[3], const int steps[3], int rows, int cols, uint64_t timestamp,
                               void* const oh_planes[3], const int o_steps[3], int o_rows, int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted)
{
    if (!st) return LVK_HIP_ERR_ARG;
    if (produced) *produced = 0;
    const int vf = video_format;
    if (vf == LVK_VIDEO_FORMAT_I420 || vf == LVK_VIDEO_FORMAT_I40A || vf == LVK_VIDEO_FORMAT_NV12)
    {
        const int nv12 = vf == LVK_VIDEO_FORMAT_NV12 ? 1 : 0;
        if (!h_planes || !steps) return st->fail(LVK_HIP_ERR_ARG, "lvk_hip_stab_push_obs_host: no input planes");
        void* const none[3] = {nullptr, nullptr, nullptr}; const int zero[3] = {0, 0, 0};
        void* const* op = oh_planes && o_steps ? oh_planes : none; const int* os = oh_planes && o_steps ? o_steps : zero;
        return lvk_hip_stab_push_yuv420_host(st, h_planes[0], steps[0], h_planes[1], steps[1], nv12 ? h_planes[1] : h_planes[2], nv12 ? steps[1] : steps[2], nv12,
                                             rows, cols, timestamp, op[0], os[0], op[1], os[1], nv12 ? op[1] : op[2], nv12 ? os[1] : os[2], o_rows,
                                             produced, out_timestamp, emitted);
    }
    lvk_device_guard device_guard(st->ctx);
    lvk_hip_ctx* ctx = st->ctx;
    int rc, frame_format = 0;
    QueuedFrame due{}; bool will_emit = false;
    if ((rc = lvk_stab_check_in_planes(st, vf, h_planes, steps, rows, cols, &frame_format)) != LVK_HIP_OK) return rc;
    if ((rc = lvk_stab_check_due(st, vf, frame_format, rows, cols, timestamp, oh_planes, o_steps, o_rows, &due, &will_emit)) != LVK_HIP_OK) return rc;
    lvk_hip_stab::HostIO& io = st->hostio;
    if (!io.ahead.empty())
        return st->fail(LVK_HIP_ERR_ARG, "lvk_hip_stab_push_obs_host: frames announced through lvk_hip_stab_prefetch_yuv420_host have not been pushed yet -- push them "
                                         "(lvk_hip_stab_push_yuv420_host) or lvk_hip_stab_prefetch_cancel() first; nothing was queued");
    HostPlane in[3]; const int n_in = host_planes_of(vf, h_planes, steps, rows, cols, in);
    LVK_HIP_REQUIRE(ctx, n_in > 0);
    if ((rc = st->require_pinned_planes(in, n_in, "lvk_hip_stab_push_obs_host")) != LVK_HIP_OK) return rc;
    // the output planes are checked -- pinned over their whole extent -- against the geometry of the frame this push emits (the DELAYED one, which
    // lvk_stab_check_due has found them large enough for); planes given to a push that emits nothing are not touched, and are held to the incoming
    // frame's geometry when they have it: pageable memory is refused whenever it is seen
    const bool rgbx = vf == LVK_VIDEO_FORMAT_RGBA || vf == LVK_VIDEO_FORMAT_BGRA || vf == LVK_VIDEO_FORMAT_BGRX;
    const int erows = will_emit ? due.rows : rows, ecols = will_emit ? due.cols : cols;
    if (oh_planes && o_steps && oh_planes[0] && o_rows >= erows)
    {
        HostPlane out[3]; const int n_out = host_planes_of(vf, oh_planes, o_steps, erows, ecols, out);
        bool whole = true;
        for (int i = 0; i < n_out; i++) whole = whole && out[i].p && out[i].step >= out[i].width;
        // (DirectIngest's 4-byte formats are a tight byte stream by definition: the egress refuses another pitch -- here, before the frame is queued)
        if (rgbx && o_steps[0] != 4 * ecols) { if (will_emit) return st->fail(LVK_HIP_ERR_ARG, "lvk_hip_stab_push_obs_host: RGBA / BGRA / BGRX output planes are tight (o_steps[0] == 4 * cols of the emitted frame); nothing was queued"); whole = false; }
        if (whole && (rc = st->require_pinned_planes(out, n_out, "lvk_hip_stab_push_obs_host (output)")) != LVK_HIP_OK) return rc;
    }
    size_t in_bytes = 0;
    for (int i = 0; i < n_in; i++) in_bytes += (size_t)in[i].width * in[i].rows;
    if ((rc = st->ensure_hostio(rows, cols, in_bytes)) != LVK_HIP_OK) return rc;
    if ((rc = st->flush_download(false)) != LVK_HIP_OK) return rc;
    int k = 0;
    if ((rc = st->host_stage(in, n_in, &k)) != LVK_HIP_OK) return rc;
    // the staged planes, tight (the 4-byte formats: the 3 * cols bytes a row that were moved, under the pitch DirectIngest declares)
    const void* d_planes[3] = {nullptr, nullptr, nullptr}; int d_steps[3] = {0, 0, 0};
    { size_t off = 0; for (int i = 0; i < n_in; i++) { d_planes[i] = (const uint8_t*)io.d_in[k] + off; d_steps[i] = rgbx ? 4 * cols : in[i].width; off += (size_t)in[i].width * in[i].rows; } }
    HostPushHooks clear_hooks{st};
    // every emitted frame leaves through stores into the host planes; the remap itself crosses the link only where its sink is fused
    if ((rc = st->host_begin_push(k, will_emit)) != LVK_HIP_OK) return rc;
    st->host_direct_now = will_emit && lvk_remap_obs_fusable(vf);
    int prod = 0;
    rc = lvk_hip_stab_push_obs(st, vf, d_planes, d_steps, rows, cols, timestamp, oh_planes, o_steps, o_rows, &prod, out_timestamp, emitted);
    { const int erc = st->host_end_push(k); if (erc != LVK_HIP_OK) return erc; }
    if (rc != LVK_HIP_OK) return rc;
    if ((rc = st->flush_download(false)) != LVK_HIP_OK) return rc;
    if (produced) *produced = prod;
    io.last_end = std::chrono::steady_clock::now();
    return LVK_HIP_OK;
}

// The host entries for ONE packed plane of 1 (Y800 / VideoFrame::GRAY) or 4 (BGRA / RGBA) bytes per pixel: lvk_hip_stab_push_gray / lvk_hip_stab_push_c4 with
// the plane in pinned host memory, one plane each way.
//   in:  one copy on the upload stream into a block of the context's pool that the entry owns until its frame has been emitted (the queue holds whole
//        frames); the tracker's stream waits for the copy's event; the host plane is the caller's again when the call returns;
//   out: the remap stores into the caller's pinned plane itself (no download route).
// Refused before anything is uploaded or queued: what the device entry refuses (sizes, a short step, another pixel size in the queue, an output plane that
// does not hold the DELAYED frame), frames that the device entry borrowed still queued, pageable planes, outstanding 4:2:0 look-ahead.
static int lvk_stab_push_plain_host(lvk_hip_stab* st, int bpp, int format, const void* h_frame, int step, int rows, int cols, uint64_t timestamp,
                                    void* oh_out, int out_step, int out_rows, int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted)
{
    if (!st) return LVK_HIP_ERR_ARG;
    if (produced) *produced = 0;
    const std::string name_s = bpp == 1 ? "lvk_hip_stab_push_gray_host" : "lvk_hip_stab_push_c4_host";
    const char* name = name_s.c_str();
    lvk_device_guard device_guard(st->ctx);
    lvk_hip_ctx* ctx = st->ctx;
    LVK_HIP_REQUIRE(ctx, h_frame && rows > 0 && cols > 0 && step >= bpp * cols);
    if (!st->buffers_ok) return ctx->fail(LVK_HIP_ERR_RUNTIME, "the last configure() failed while allocating the tracker's buffers: configure again");
    int rc;
    QueuedFrame due{}; bool will_emit = false;
    // (the host plane is copied into a packed block of the library's own: only the output plane, which the remap writes, has an alignment rule)
    if ((rc = lvk_stab_check_plain(st, true, bpp, format, nullptr, 0, rows, cols, timestamp, oh_out, out_step, out_rows, &due, &will_emit)) != LVK_HIP_OK) return rc;
    if (!st->hostio.ahead.empty())
        return st->fail(LVK_HIP_ERR_ARG, name_s + ": frames announced through lvk_hip_stab_prefetch_yuv420_host have not been pushed yet -- push them "
                                                  "or lvk_hip_stab_prefetch_cancel() first; nothing was queued");
    const HostPlane in{h_frame, step, bpp * cols, rows};
    if ((rc = st->require_pinned_planes(&in, 1, name)) != LVK_HIP_OK) return rc;
    if (oh_out && out_step >= bpp * (will_emit ? due.cols : cols) && out_rows >= (will_emit ? due.rows : rows))
    {
        const HostPlane out{oh_out, out_step, bpp * (will_emit ? due.cols : cols), will_emit ? due.rows : rows};
        if ((rc = st->require_pinned_planes(&out, 1, (name_s + " (output)").c_str())) != LVK_HIP_OK) return rc;
    }
    // blocks whose frame left the queue outside a push (restart, a shrinking queue): nothing may still read them
    {
        bool synced = false;
        for (size_t i = 0; i < st->gray_host_live.size();)
        {
            void* p = st->gray_host_live[i];
            bool queued = p == st->pending_release;
            for (const QueuedFrame& q : st->queue) queued = queued || q.d_ptr == p;
            if (queued) { i++; continue; }
            if (!synced) { LVK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream)); if (st->remap_stream) LVK_HIP_CHECK(ctx, hipStreamSynchronize(st->remap_stream)); synced = true; }
            (void)lvk_hip_free(ctx, p);
            st->gray_host_live.erase(st->gray_host_live.begin() + (long)i);
        }
        st->orphaned.clear();                                  // (they were this entry's blocks, freed above)
    }
    if ((rc = st->host_stream(st->hostio.up)) != LVK_HIP_OK) return rc;
    if (!st->gray_up_done) LVK_HIP_CHECK(ctx, hipEventCreateWithFlags(&st->gray_up_done, hipEventDisableTiming));
    if (!st->gray_fence) LVK_HIP_CHECK(ctx, hipEventCreateWithFlags(&st->gray_fence, hipEventDisableTiming));
    void* d_frame = nullptr;
    const size_t row_bytes = (size_t)bpp * cols;
    if ((rc = lvk_hip_malloc(ctx, row_bytes * rows, &d_frame)) != LVK_HIP_OK) return rc;
    // the block may have been read last by a remap on the tracking stream that has not run yet (no overlap: a frame is released as soon as its remap is
    // enqueued): the upload follows whatever that stream holds.  In overlap mode a frame is released only after its remap has finished.
    hipStream_t up = st->hostio.up;
    hipError_t e = hipEventRecord(st->gray_fence, ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(up, st->gray_fence, 0);
    if (e == hipSuccess) e = (size_t)step == row_bytes ? hipMemcpyAsync(d_frame, h_frame, row_bytes * rows, hipMemcpyHostToDevice, up)
                                                       : hipMemcpy2DAsync(d_frame, row_bytes, h_frame, (size_t)step, row_bytes, (size_t)rows, hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = hipEventRecord(st->gray_up_done, up);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, st->gray_up_done, 0);
    if (e != hipSuccess) { (void)hipStreamSynchronize(up); (void)lvk_hip_free(ctx, d_frame); return ctx->fail(LVK_HIP_ERR_RUNTIME, hipGetErrorString(e)); }
    st->gray_host_live.push_back(d_frame);
    HostPushHooks clear_hooks{st};
    struct EntryFlag { lvk_hip_stab* s; ~EntryFlag() { s->gray_host_entry_now = false; } } entry_flag{st};
    st->gray_host_entry_now = true;
    st->host_direct_now = will_emit;                               // the remap's stores cross the host link
    int prod = 0; const void* released = nullptr;
    rc = bpp == 1 ? lvk_hip_stab_push_gray(st, d_frame, cols, rows, cols, timestamp, oh_out, out_step, out_rows, &prod, out_timestamp, &released, emitted)
                  : lvk_hip_stab_push_c4(st, d_frame, 4 * cols, rows, cols, timestamp, format, oh_out, out_step, out_rows, &prod, out_timestamp, &released, emitted);
    const hipError_t se = hipEventSynchronize(st->gray_up_done);    // "consumed on return": the host plane is the caller's again
    auto drop = [&](const void* p) {
        auto it = std::find(st->gray_host_live.begin(), st->gray_host_live.end(), p);
        if (it != st->gray_host_live.end()) { (void)lvk_hip_free(ctx, *it); st->gray_host_live.erase(it); }
    };
    if (rc == LVK_HIP_ERR_ARG) drop(d_frame);                       // (a refused push has queued nothing)
    if (released) drop(released);
    if (rc != LVK_HIP_OK) return rc;
    if (se != hipSuccess) return ctx->fail(LVK_HIP_ERR_RUNTIME, hipGetErrorString(se));
    if (produced) *produced = prod;
    st->hostio.last_end = std::chrono::steady_clock::now();
    return LVK_HIP_OK;
}

int lvk_hip_stab_push_gray_host(lvk_hip_stab* st, const void* h_frame, int step, int rows, int cols, uint64_t timestamp,
                                void* oh_out, int out_step, int out_rows, int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted)
{
    return lvk_stab_push_plain_host(st, 1, LVK_FORMAT_GRAY, h_frame, step, rows, cols, timestamp, oh_out, out_step, out_rows, produced, out_timestamp, emitted);
}

int lvk_hip_stab_push_c4_host(lvk_hip_stab* st, const void* h_frame, int step, int rows, int cols, uint64_t timestamp, int format,
                              void* oh_out, int out_step, int out_rows, int* produced, uint64_t* out_timestamp, lvk_frame_info* emitted)
{
    if (!st) return LVK_HIP_ERR_ARG;
    if (produced) *produced = 0;
    if (format != LVK_FORMAT_BGRA && format != LVK_FORMAT_RGBA)
        return st->fail(LVK_HIP_ERR_ARG, "lvk_hip_stab_push_c4_host: format is LVK_FORMAT_BGRA or LVK_FORMAT_RGBA; nothing was queued");
    return lvk_stab_push_plain_host(st, 4, format, h_frame, step, rows, cols, timestamp, oh_out, out_step, out_rows, produced, out_timestamp, emitted);
}

// Pinned host memory for the planes of lvk_hip_stab_push_yuv420_host (what obs_source_frame buffers would be registered as)
int lvk_hip_host_malloc(lvk_hip_ctx* ctx, size_t bytes, void** h_ptr)
{
    if (!ctx || !h_ptr) return LVK_HIP_ERR_ARG;
    LVK_HIP_REQUIRE(ctx, bytes > 0);
    lvk_device_guard device_guard(ctx);
    LVK_HIP_CHECK(ctx, hipHostMalloc(h_ptr, bytes, hipHostMallocDefault));
    return LVK_HIP_OK;
}

int lvk_hip_host_free(lvk_hip_ctx* ctx, void* h_ptr)
{
    if (!ctx) return LVK_HIP_ERR_ARG;
    lvk_device_guard device_guard(ctx);
    if (h_ptr) LVK_HIP_CHECK(ctx, hipHostFree(h_ptr));
    return LVK_HIP_OK;
}

} // extern "C"
