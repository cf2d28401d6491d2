// The routing of lvk_hip_cas_obs (cas_route of livevisionkit_amd/csrc/obs_planes.hpp) on the CPU: g++ only, no HIP, built with
// -fsanitize=address,undefined by tests/test_cas_route_check_cpp.py.
//
// The route table: sixteen formats and four numbers that are none.  4:2:0 goes to the 4:2:0 kernel, Y800 to the gray kernel, BGR3 and the 4-byte
// DirectIngest formats to the packed kernel on three-byte pixels, and a route is Fused exactly where the format has planes and is none of these: the
// eight formats with a plane sink, of which the 4:2:2 ones take an even width only.
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
        const CasRoute r = cas_route(vf);
        if (is_420(vf)) { EXPECT(r == CasRoute::Planes420); planes420++; }
        else if (vf == LVK_VIDEO_FORMAT_Y800) { EXPECT(r == CasRoute::Gray); gray++; }
        else if (vf == LVK_VIDEO_FORMAT_BGR3 || is_direct4(vf)) { EXPECT(r == CasRoute::Bgr); bgr++; }
        else { EXPECT(r == CasRoute::Fused); fused++; }
        EXPECT(r != CasRoute::None && obs_rows(vf, 2).n > 0 == !is_420(vf));
        // the fused route is the one with a plane sink: 4:2:2 takes an even width, every other fused format any
        if (r == CasRoute::Fused) EXPECT(obs_size_ok(vf, 3, 5) == !is_422(vf) && obs_size_ok(vf, 3, 6));
        // the packed kernel runs on three-byte pixels: a row of the plane holds at least that many bytes
        if (r == CasRoute::Bgr) EXPECT(obs_rows(vf, 7).bytes[0] >= 3 * 7);
        if (r == CasRoute::Gray) EXPECT(obs_rows(vf, 7).bytes[0] == 7);
        checked++;
    }
    EXPECT(planes420 == 3 && fused == 8 && bgr == 4 && gray == 1);
    for (int bad : {0, 17, -1, 99}) { EXPECT(cas_route(bad) == CasRoute::None); checked++; }
}

} // namespace

int main()
{
    routes();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("cas route ok: %lld checks\n", checked);
    return 0;
}
