// The host's description of the planes of the OBS video formats and the routing of lvk_hip_scale_obs (livevisionkit_amd/csrc/obs_planes.hpp) on the CPU:
// g++ only, no HIP, built with -fsanitize=address,undefined by tests/test_obs_planes_check_cpp.py.
//
// 1. obs_rows / obs_spans against a brute-force byte map: for every format outside 4:2:0, sizes 1 .. 6 x 1 .. 6 with the format's parity and pitches from
//    the row to the row + 3, the planes laid out in an arena; every byte the span rule calls occupied is marked, "inputs clear of outputs" and "outputs
//    pairwise disjoint" are compared with the map while one output plane slides over the arena.
// 2. The parity rules (obs_size_ok), the 4:2:0 plane sets (plane_set_420) and the route table (scale_route) on hand-written cases.
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

void sweep(int vf, int rows, int cols, int pad)
{
    const ObsRows t = obs_rows(vf, cols);
    EXPECT(t.n >= 1 && t.n <= 3);
    int steps[3] = {0, 0, 0}, size[3] = {0, 0, 0};
    for (int i = 0; i < t.n; i++) { steps[i] = t.bytes[i] + (is_direct4(vf) ? 0 : pad + i); size[i] = (rows - 1) * steps[i] + t.bytes[i]; }
    const int arena_bytes = 2 * (size[0] + size[1] + size[2]) + 16;
    std::vector<uint8_t> arena((size_t)arena_bytes);                     // exactly sized: a span past its end is the sanitizer's to find
    // inputs back to back at the start
    const void* in_p[3] = {nullptr, nullptr, nullptr};
    int at = 0;
    std::vector<int> in_map((size_t)arena_bytes, 0);
    for (int i = 0; i < t.n; i++)
    {
        in_p[i] = arena.data() + at;
        for (int b = 0; b < size[i]; b++) in_map[(size_t)at + b]++;
        at += size[i];
    }
    const Spans in = obs_spans(vf, in_p, steps, rows, cols);
    EXPECT(in.n == t.n && disjoint(in));
    for (int i = 0; i < t.n; i++) EXPECT((int)(in.s[i].hi - in.s[i].lo) == size[i] && std::memchr((const void*)in.s[i].lo, 0, 1) != nullptr && ((const uint8_t*)in.s[i].hi)[-1] == 0);
    // outputs behind them; each in turn slides over the whole arena
    int base[3] = {0, 0, 0};
    for (int i = 0; i < t.n; i++) { base[i] = at + 1; at += size[i] + 1; }
    for (int moved = 0; moved < t.n; moved++)
        for (int o = 0; o + size[moved] <= arena_bytes; o++)
        {
            int off[3] = {base[0], base[1], base[2]};
            off[moved] = o;
            const void* out_p[3] = {nullptr, nullptr, nullptr};
            std::vector<int> out_map((size_t)arena_bytes, 0);
            for (int i = 0; i < t.n; i++)
            {
                out_p[i] = arena.data() + off[i];
                for (int b = 0; b < size[i]; b++) out_map[(size_t)off[i] + b]++;
            }
            const Spans out = obs_spans(vf, out_p, steps, rows, cols);
            bool twice = false, shared = false;
            for (int b = 0; b < arena_bytes; b++) { twice |= out_map[(size_t)b] > 1; shared |= out_map[(size_t)b] && in_map[(size_t)b]; }
            EXPECT(disjoint(out) == !twice);
            EXPECT(clear_of(in.s, in.n, out) == !shared);
            checked++;
        }
}

void hand_written()
{
    // the planes of each family and the bytes of their rows
    EXPECT(obs_rows(LVK_VIDEO_FORMAT_I422, 10).n == 3 && obs_rows(LVK_VIDEO_FORMAT_I42A, 10).bytes[1] == 5 && obs_rows(LVK_VIDEO_FORMAT_I422, 10).bytes[2] == 5);
    EXPECT(obs_rows(LVK_VIDEO_FORMAT_I444, 9).n == 3 && obs_rows(LVK_VIDEO_FORMAT_YUVA, 9).bytes[2] == 9);
    EXPECT(obs_rows(LVK_VIDEO_FORMAT_UYVY, 10).n == 1 && obs_rows(LVK_VIDEO_FORMAT_YUY2, 10).bytes[0] == 20 && obs_rows(LVK_VIDEO_FORMAT_YVYU, 10).bytes[0] == 20);
    EXPECT(obs_rows(LVK_VIDEO_FORMAT_AYUV, 9).bytes[0] == 36 && obs_rows(LVK_VIDEO_FORMAT_BGRX, 9).bytes[0] == 36 && obs_rows(LVK_VIDEO_FORMAT_BGR3, 9).bytes[0] == 27);
    EXPECT(obs_rows(LVK_VIDEO_FORMAT_Y800, 9).n == 1 && obs_rows(LVK_VIDEO_FORMAT_Y800, 9).bytes[0] == 9);
    for (int bad : {0, 17, -1, 99}) EXPECT(obs_rows(bad, 8).n == 0 && scale_route(bad, true) == ScaleRoute::None && scale_route(bad, false) == ScaleRoute::None);
    // parity: even cols on 4:2:2, even rows and cols on 4:2:0, anything positive elsewhere
    for (int vf : kAll)
    {
        const bool f420 = is_420(vf), f422 = is_422(vf);
        EXPECT(obs_size_ok(vf, 6, 8) && !obs_size_ok(vf, 0, 8) && !obs_size_ok(vf, 6, 0) && !obs_size_ok(vf, -2, 8) && !obs_size_ok(vf, 6, -2));
        EXPECT(obs_size_ok(vf, 6, 9) == !(f420 || f422));
        EXPECT(obs_size_ok(vf, 7, 8) == !f420);
        EXPECT(obs_size_ok(vf, 1, 1) == !(f420 || f422));
        EXPECT(!(f420 && f422) && is_direct4(vf) == (vf == LVK_VIDEO_FORMAT_RGBA || vf == LVK_VIDEO_FORMAT_BGRA || vf == LVK_VIDEO_FORMAT_BGRX));
    }
    // the route table: sixteen formats, two size relations
    for (int vf : kAll)
        for (int equal = 0; equal < 2; equal++)
        {
            const ScaleRoute r = scale_route(vf, equal != 0);
            if (is_420(vf)) EXPECT(r == ScaleRoute::Planes420);
            else if (vf == LVK_VIDEO_FORMAT_Y800) EXPECT(r == ScaleRoute::Gray);
            else if (vf == LVK_VIDEO_FORMAT_BGR3 || is_direct4(vf)) EXPECT(r == ScaleRoute::Bgr);
            else EXPECT(r == (equal ? ScaleRoute::FusedPlanes : ScaleRoute::FusedPacked));
        }
    // 4:2:0 plane sets from the arrays of the entry: NV12 folds the missing V plane onto the UV plane, I40A is I420
    uint8_t a[64] = {};
    const void* p[3] = {a, a + 32, a + 48};
    const void* p2[3] = {a, a + 32, nullptr};
    const int s[3] = {8, 4, 4}, s2[3] = {8, 8, 0};
    EXPECT(well_formed(plane_set_420(LVK_VIDEO_FORMAT_I420, p, s, 4, 8)) && plane_set_420(LVK_VIDEO_FORMAT_I40A, p, s, 4, 8).nv12 == 0);
    EXPECT(well_formed(plane_set_420(LVK_VIDEO_FORMAT_NV12, p2, s2, 4, 8)) && plane_set_420(LVK_VIDEO_FORMAT_NV12, p2, s2, 4, 8).p.v == a + 32);
    EXPECT(!well_formed(plane_set_420(LVK_VIDEO_FORMAT_I420, p2, s, 4, 8)) && !well_formed(plane_set_420(LVK_VIDEO_FORMAT_I420, p, s, 3, 8)));
}

} // namespace

int main()
{
    for (int vf : kAll)
    {
        if (is_420(vf)) continue;
        for (int rows = 1; rows <= 6; rows++)
            for (int cols = 1; cols <= 6; cols++)
                for (int pad = 0; pad < 4; pad++)
                    if (obs_size_ok(vf, rows, cols)) sweep(vf, rows, cols, pad);
    }
    hand_written();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("obs planes ok: %lld plane sets checked\n", checked);
    return 0;
}
