// The routing of lvk_hip_fsr_obs (fsr_route of livevisionkit_amd/csrc/obs_planes.hpp) on the CPU: g++ only, no HIP, built with
// -fsanitize=address,undefined by tests/test_fsr_route_check_cpp.py.
//
// The route table: sixteen formats and four numbers that are none, on both paths (the tile's footprint fits the LDS stage, or it does not).  4:2:0 goes
// to the body of lvk_hip_fsr_yuv420, Y800 to the gray kernel, BGR3 and the 4-byte DirectIngest formats to the packed kernel on three-byte pixels -- on
// either path, the choice is theirs --, and the eight formats with a plane sink run planes to planes when staged and through a pooled packed frame
// when not.
#include "obs_planes.hpp"

#include <cstdio>
#include <initializer_list>

using namespace obs;

namespace {

long long checked = 0;
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; if (failures < 20) std::printf("FAIL line %d: %s\n", __LINE__, #cond); } } while (0)

const int kAll[] = {LVK_VIDEO_FORMAT_I420, LVK_VIDEO_FORMAT_NV12, LVK_VIDEO_FORMAT_YVYU, LVK_VIDEO_FORMAT_YUY2, LVK_VIDEO_FORMAT_UYVY, LVK_VIDEO_FORMAT_RGBA,
                    LVK_VIDEO_FORMAT_BGRA, LVK_VIDEO_FORMAT_BGRX, LVK_VIDEO_FORMAT_Y800, LVK_VIDEO_FORMAT_I444, LVK_VIDEO_FORMAT_BGR3, LVK_VIDEO_FORMAT_I422,
                    LVK_VIDEO_FORMAT_I40A, LVK_VIDEO_FORMAT_I42A, LVK_VIDEO_FORMAT_YUVA, LVK_VIDEO_FORMAT_AYUV};

void routes()
{
    int fused = 0, planes420 = 0, bgr = 0, gray = 0;
    for (int vf : kAll)
    {
        const FsrRoute s = fsr_route(vf, true), d = fsr_route(vf, false);
        if (is_420(vf)) { EXPECT(s == FsrRoute::Planes420 && d == s); planes420++; }
        else if (vf == LVK_VIDEO_FORMAT_Y800) { EXPECT(s == FsrRoute::Gray && d == s); gray++; }
        else if (vf == LVK_VIDEO_FORMAT_BGR3 || is_direct4(vf)) { EXPECT(s == FsrRoute::Bgr && d == s); bgr++; }
        else { EXPECT(s == FsrRoute::FusedPlanes && d == FsrRoute::FusedPacked); fused++; }
        EXPECT(s != FsrRoute::None && d != FsrRoute::None && obs_rows(vf, 2).n > 0 == !is_420(vf));
        // the fused routes are the ones with a plane sink: 4:2:2 takes an even width at both sizes, every other fused format any
        if (s == FsrRoute::FusedPlanes) EXPECT(obs_size_ok(vf, 3, 5) == !is_422(vf) && obs_size_ok(vf, 3, 6));
        // 4:2:0 takes even sizes only
        if (s == FsrRoute::Planes420) EXPECT(!obs_size_ok(vf, 3, 6) && !obs_size_ok(vf, 4, 5) && obs_size_ok(vf, 4, 6));
        // the packed kernel runs on three-byte pixels: a row of the plane holds at least that many bytes, at the source and at the output size
        if (s == FsrRoute::Bgr) EXPECT(obs_rows(vf, 7).bytes[0] >= 3 * 7 && obs_rows(vf, 9).bytes[0] >= 3 * 9);
        if (s == FsrRoute::Gray) EXPECT(obs_rows(vf, 7).bytes[0] == 7);
        checked += 2;
    }
    EXPECT(planes420 == 3 && fused == 8 && bgr == 4 && gray == 1);
    for (int bad : {0, 17, -1, 99}) { EXPECT(fsr_route(bad, true) == FsrRoute::None && fsr_route(bad, false) == FsrRoute::None); checked += 2; }
}

} // namespace

int main()
{
    routes();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("fsr route ok: %lld checks\n", checked);
    return 0;
}
