// The routing of lvk_hip_deblock_apply_obs and where a fused format keeps its luma (deblock_route, luma_bytes of livevisionkit_amd/csrc/obs_planes.hpp)
// on the CPU: g++ only, no HIP, built with -fsanitize=address,undefined by tests/test_deblock_route_check_cpp.py.
//
// 1. The route table: sixteen formats and four numbers that are none; a route is Fused exactly where the format has planes and is none of 4:2:0, Y800,
//    BGR3 and the 4-byte DirectIngest formats.
// 2. luma_bytes against the byte patterns of the layouts: a row of `cols` pixels is written out as letters (Y U Y V, Y V Y U, U Y V Y, A Y U V, or a
//    plane of Y), in a buffer of exactly the row's bytes -- a luma offset past the row is the sanitizer's to find --, and the strided walk must visit
//    every Y of the row, nothing else, `cols` times.
#include "obs_planes.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace obs;

namespace {

long long checked = 0;
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; if (failures < 20) std::printf("FAIL line %d: %s\n", __LINE__, #cond); } } while (0)

const int kAll[] = {LVK_VIDEO_FORMAT_I420, LVK_VIDEO_FORMAT_NV12, LVK_VIDEO_FORMAT_YVYU, LVK_VIDEO_FORMAT_YUY2, LVK_VIDEO_FORMAT_UYVY, LVK_VIDEO_FORMAT_RGBA,
                    LVK_VIDEO_FORMAT_BGRA, LVK_VIDEO_FORMAT_BGRX, LVK_VIDEO_FORMAT_Y800, LVK_VIDEO_FORMAT_I444, LVK_VIDEO_FORMAT_BGR3, LVK_VIDEO_FORMAT_I422,
                    LVK_VIDEO_FORMAT_I40A, LVK_VIDEO_FORMAT_I42A, LVK_VIDEO_FORMAT_YUVA, LVK_VIDEO_FORMAT_AYUV};

const char* pattern_of(int vf)             // the bytes of plane 0, repeated along a row
{
    switch (vf)
    {
    case LVK_VIDEO_FORMAT_YUY2: return "YUYV";
    case LVK_VIDEO_FORMAT_YVYU: return "YVYU";
    case LVK_VIDEO_FORMAT_UYVY: return "UYVY";
    case LVK_VIDEO_FORMAT_AYUV: return "AYUV";
    default: return "Y";                   // I422 / I42A / I444 / YUVA: plane 0 is the Y plane
    }
}

void routes()
{
    int fused = 0;
    for (int vf : kAll)
    {
        const DeblockRoute r = deblock_route(vf);
        if (is_420(vf)) EXPECT(r == DeblockRoute::Planes420);
        else if (vf == LVK_VIDEO_FORMAT_Y800) EXPECT(r == DeblockRoute::Gray);
        else if (vf == LVK_VIDEO_FORMAT_BGR3 || is_direct4(vf)) EXPECT(r == DeblockRoute::Bgr);
        else { EXPECT(r == DeblockRoute::Fused); fused++; }
        EXPECT(r != DeblockRoute::None && obs_rows(vf, 2).n > 0 == !is_420(vf));
        // the fused route is the one with a plane sink: 4:2:2 takes an even width, every other fused format any
        if (r == DeblockRoute::Fused) EXPECT(obs_size_ok(vf, 3, 5) == !is_422(vf) && obs_size_ok(vf, 3, 6));
        checked++;
    }
    EXPECT(fused == 8);
    for (int bad : {0, 17, -1, 99}) EXPECT(deblock_route(bad) == DeblockRoute::None);
}

void luma()
{
    for (int vf : kAll)
    {
        if (deblock_route(vf) != DeblockRoute::Fused) continue;
        const char* pat = pattern_of(vf);
        const int period = (int)std::strlen(pat);
        const LumaBytes l = luma_bytes(vf);
        EXPECT(l.stride >= 1 && l.first >= 0 && l.first < l.stride);
        for (int cols = 1; cols <= 40; cols++)
        {
            if (!obs_size_ok(vf, 1, cols)) continue;
            const int bytes = obs_rows(vf, cols).bytes[0];
            std::vector<char> row((size_t)bytes);                         // exactly the row
            for (int b = 0; b < bytes; b++) row[(size_t)b] = pat[b % period];
            int total = 0;
            for (int b = 0; b < bytes; b++) total += row[(size_t)b] == 'Y';
            EXPECT(total == cols);
            int seen = 0;
            for (int x = 0; x < cols; x++) seen += row[(size_t)(l.first + x * l.stride)] == 'Y';
            EXPECT(seen == cols);
            checked++;
        }
    }
    // the formats that are not fused say "a plane of luma": the walk of launch_stats_plane
    for (int vf : {LVK_VIDEO_FORMAT_I420, LVK_VIDEO_FORMAT_NV12, LVK_VIDEO_FORMAT_Y800, LVK_VIDEO_FORMAT_I444})
        EXPECT(luma_bytes(vf).first == 0 && luma_bytes(vf).stride == 1);
}

} // namespace

int main()
{
    routes();
    luma();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("deblock route ok: %lld checks\n", checked);
    return 0;
}
