// The planes of an I420 / NV12 frame as every 4:2:0 entry of the C-ABI takes them, and the host's rules about them: the planes
// as a kernel argument (Planes, PlanesOut), the description an entry builds ONCE from its C arguments (plane_set -- the only place that folds NV12's
// missing V plane onto the UV plane), "well formed", the byte spans, "the outputs are pairwise disjoint" and "these inputs are clear of these outputs".
// Plain C++, no HIP: tests/cpp/planes420_check.cpp compiles it on the CPU.
#pragma once

#include <cstdint>

namespace yuv420 {

struct Planes { const uint8_t* y; const uint8_t* u; const uint8_t* v; int ys, us, vs; };     // NV12: u is the UV plane, v (vs) repeats it
struct PlanesOut { uint8_t* y; uint8_t* u; uint8_t* v; int ys, us, vs; };

// [first byte, one past the last byte) of a plane of `prows` rows of `row` bytes at pitch `step`: the bounding range, padding between rows included
struct Span { uintptr_t lo, hi; };

inline Span span_of(const void* p, int step, int prows, long long row)
{
    const uintptr_t lo = (uintptr_t)p;
    return {lo, lo + (uintptr_t)((long long)(prows - 1) * step + row)};
}

inline bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

inline bool aligned_to(const void* p, int step, unsigned a) { return (((uintptr_t)p | (uintptr_t)step) & (a - 1)) == 0; }

// The remap family addresses a plane with ONE 32-bit byte offset built from 24-bit factors (easu_gather, the sinks): the whole plane must lie within
// 4 GB of its base and rows / pitch below 2^24 (an 8K packed frame is 100 MB with a 23 KB pitch).
inline bool fits_u32(int step, int rows) { return step > 0 && rows > 0 && step < (1 << 24) && rows < (1 << 24) && (uint64_t)step * (uint64_t)rows < (1ull << 32); }

// the planes of one rows x cols frame, inputs or outputs
struct PlaneSet
{
    Planes p; int nv12, rows, cols;

    int crow() const { return nv12 ? cols : cols / 2; }                                      // bytes of a chroma row
    int count() const { return nv12 ? 2 : 3; }                                               // planes in use
    Planes in() const { return p; }
    PlanesOut out() const { return {const_cast<uint8_t*>(p.y), const_cast<uint8_t*>(p.u), const_cast<uint8_t*>(p.v), p.ys, p.us, p.vs}; }   // of a set built from writable planes
};

inline PlaneSet plane_set(const void* y, int y_step, const void* u, int u_step, const void* v, int v_step, int nv12, int rows, int cols)
{
    return {{(const uint8_t*)y, (const uint8_t*)u, (const uint8_t*)(nv12 ? u : v), y_step, u_step, nv12 ? u_step : v_step}, nv12, rows, cols};
}

// the planes in use are there, 4:2:0 has even sizes of at least 2, every row lies inside its pitch; u32: every plane also fits_u32
inline bool well_formed(const PlaneSet& s, bool u32 = false)
{
    if (!s.p.y || !s.p.u || !s.p.v) return false;
    if (s.rows < 2 || s.cols < 2 || ((s.rows | s.cols) & 1) != 0) return false;
    if (s.p.ys < s.cols || s.p.us < s.crow() || s.p.vs < s.crow()) return false;
    return !u32 || (fits_u32(s.p.ys, s.rows) && fits_u32(s.p.us, s.rows / 2) && fits_u32(s.p.vs, s.rows / 2));
}

// the spans of the planes in use (of a well-formed set)
struct Spans { Span s[3]; int n; };

inline Spans spans_of(const PlaneSet& s)
{
    return {{span_of(s.p.y, s.p.ys, s.rows, s.cols), span_of(s.p.u, s.p.us, s.rows / 2, s.crow()), span_of(s.p.v, s.p.vs, s.rows / 2, s.crow())}, s.count()};
}

// no byte belongs to two of the planes
inline bool disjoint(const Spans& out)
{
    for (int i = 0; i < out.n; i++)
        for (int j = i + 1; j < out.n; j++)
            if (overlap(out.s[i], out.s[j])) return false;
    return true;
}

// none of the `n_in` input spans shares a byte with an output plane
inline bool clear_of(const Span* in, int n_in, const Spans& out)
{
    for (int i = 0; i < out.n; i++)
        for (int j = 0; j < n_in; j++)
            if (overlap(in[j], out.s[i])) return false;
    return true;
}

} // namespace yuv420
