// The little of HLSL that the OBS plugin's CAS and FSR effect files use, as host C++ (test infrastructure only).
//
// `make -C oracle ref` pipes the reference's effect text into g++ behind this header; nothing in here is taken from that text.  What
// this header decides, and the reference leaves to the graphics API, is stated in DESIGN.md sections 14 and 16:
//   texture2d::Load    a texel outside the frame reads as 0
//   texture2d::Sample  the texel clamp(floor(u W), 0, W - 1) x clamp(floor(v H), 0, H - 1); the sampler argument is not looked at, the
//                      EASU path only ever passes the point sampler.  Every sampled u W, v H leaves its distance from k + 0.5 behind
//   rcp, rsqrt         1.0f / x and 1.0f / sqrtf(x), correctly rounded
//   min, max, saturate IEEE minNum / maxNum: a NaN operand loses (D3D's rule)
//   mul, float4x4      the vertex shader is compiled and never run
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace ffx_shim {

typedef unsigned int uint;

struct f2pod { float x, y; };
struct f3pod { float x, y, z; };

struct float2 {
    union { struct { float x, y; }; struct { float r, g; }; f2pod xy; };
    float2() : x(0), y(0) {}
    float2(float a, float b) : x(a), y(b) {}
    float2(f2pod p) : x(p.x), y(p.y) {}
    enum { N = 2 };
    float& operator[](int i) { return (&x)[i]; }
};
struct float3 {
    union { struct { float x, y, z; }; struct { float r, g, b; }; f3pod xyz; f3pod rgb; };
    float3() : x(0), y(0), z(0) {}
    float3(float a, float b, float c) : x(a), y(b), z(c) {}
    float3(f3pod p) : x(p.x), y(p.y), z(p.z) {}
    enum { N = 3 };
    float& operator[](int i) { return (&x)[i]; }
};
struct float4 {
    union { struct { float x, y, z, w; }; struct { float r, g, b, a; }; struct { f2pod xy, zw; }; f3pod xyz; f3pod rgb; };
    float4() : x(0), y(0), z(0), w(0) {}
    float4(float a, float b, float c, float d) : x(a), y(b), z(c), w(d) {}
    float4(float3 v, float d) : x(v.x), y(v.y), z(v.z), w(d) {}
    float4(f3pod v, float d) : x(v.x), y(v.y), z(v.z), w(d) {}
    enum { N = 4 };
    float& operator[](int i) { return (&x)[i]; }
};
struct int2 {
    int x, y;
    int2() : x(0), y(0) {}
    int2(int a, int b) : x(a), y(b) {}
    explicit int2(float2 v) : x((int)v.x), y((int)v.y) {}
};
struct int3 {
    int x, y, z;
    int3() : x(0), y(0), z(0) {}
    int3(int a, int b, int c) : x(a), y(b), z(c) {}
    int3(int2 p, int c) : x(p.x), y(p.y), z(c) {}
};
struct int4 { int x, y, z, w; };
struct bool2 { bool x, y; };
struct bool3 { bool x, y, z; };
struct bool4 { bool x, y, z, w; };
inline int2 operator+(int2 a, int2 b) { return int2(a.x + b.x, a.y + b.y); }

struct uvec2 { uint v[2]; enum { N = 2 }; uvec2() : v{0, 0} {} uvec2(uint a, uint b) : v{a, b} {} uint& operator[](int i) { return v[i]; } };
struct uvec3 { uint v[3]; enum { N = 3 }; uvec3() : v{0, 0, 0} {} uvec3(uint a, uint b, uint c) : v{a, b, c} {} uint& operator[](int i) { return v[i]; } };
struct uvec4 {
    uint v[4];
    enum { N = 4 };
    uvec4() : v{0, 0, 0, 0} {}
    uvec4(uint a, uint b, uint c, uint d) : v{a, b, c, d} {}
    uint& operator[](int i) { return v[i]; }
};
#define FFX_SHIM_UVEC(V)                                                                                                  \
    inline V operator+(V a, V b) { V r; for (int i = 0; i < V::N; i++) r[i] = a[i] + b[i]; return r; }                    \
    inline V operator-(V a, V b) { V r; for (int i = 0; i < V::N; i++) r[i] = a[i] - b[i]; return r; }                    \
    inline V operator>>(V a, V b) { V r; for (int i = 0; i < V::N; i++) r[i] = a[i] >> b[i]; return r; }
FFX_SHIM_UVEC(uvec2)
FFX_SHIM_UVEC(uvec3)
FFX_SHIM_UVEC(uvec4)

inline float asfloat(uint u) { float f; std::memcpy(&f, &u, 4); return f; }
inline uint asuint(float f) { uint u; std::memcpy(&u, &f, 4); return u; }
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline float saturate(float a) { return fminf(fmaxf(a, 0.0f), 1.0f); }
inline float rcp(float a) { return 1.0f / a; }
inline float rsqrt(float a) { return 1.0f / sqrtf(a); }
inline float abs(float a) { return fabsf(a); }
inline float floor(float a) { return floorf(a); }

#define FFX_SHIM_FVEC(V, U)                                                                                               \
    inline V operator+(V a, V b) { V r; for (int i = 0; i < V::N; i++) r[i] = a[i] + b[i]; return r; }                    \
    inline V operator-(V a, V b) { V r; for (int i = 0; i < V::N; i++) r[i] = a[i] - b[i]; return r; }                    \
    inline V operator*(V a, V b) { V r; for (int i = 0; i < V::N; i++) r[i] = a[i] * b[i]; return r; }                    \
    inline V operator/(V a, V b) { V r; for (int i = 0; i < V::N; i++) r[i] = a[i] / b[i]; return r; }                    \
    inline V operator*(V a, float b) { V r; for (int i = 0; i < V::N; i++) r[i] = a[i] * b; return r; }                   \
    inline V operator-(V a) { V r; for (int i = 0; i < V::N; i++) r[i] = -a[i]; return r; }                               \
    inline V& operator+=(V& a, V b) { a = a + b; return a; }                                                              \
    inline V& operator-=(V& a, V b) { a = a - b; return a; }                                                              \
    inline V& operator*=(V& a, V b) { a = a * b; return a; }                                                              \
    inline V min(V a, V b) { V r; for (int i = 0; i < V::N; i++) r[i] = min(a[i], b[i]); return r; }                      \
    inline V max(V a, V b) { V r; for (int i = 0; i < V::N; i++) r[i] = max(a[i], b[i]); return r; }                      \
    inline V saturate(V a) { V r; for (int i = 0; i < V::N; i++) r[i] = saturate(a[i]); return r; }                       \
    inline V rcp(V a) { V r; for (int i = 0; i < V::N; i++) r[i] = rcp(a[i]); return r; }                                 \
    inline V rsqrt(V a) { V r; for (int i = 0; i < V::N; i++) r[i] = rsqrt(a[i]); return r; }                             \
    inline V floor(V a) { V r; for (int i = 0; i < V::N; i++) r[i] = floor(a[i]); return r; }                             \
    inline V asfloat(U a) { V r; for (int i = 0; i < V::N; i++) r[i] = asfloat(a[i]); return r; }                         \
    inline U asuint(V a) { U r; for (int i = 0; i < V::N; i++) r[i] = asuint(a[i]); return r; }
FFX_SHIM_FVEC(float2, uvec2)
FFX_SHIM_FVEC(float3, uvec3)
FFX_SHIM_FVEC(float4, uvec4)

struct float4x4 {};
inline float4 mul(float4 v, float4x4) { return v; }

struct sampler {};
static const sampler PointSampler, LinearSampler;

// the largest | frac(u W) - 0.5 | and | frac(v H) - 0.5 | of every Sample since the last reset
static float g_sample_dev;

struct texture2d {
    const float *r, *g, *b;   // channel bases; texel (x, y) of a channel sits at base[(y * W + x) * stride]
    int stride, W, H;
    texture2d() : r(nullptr), g(nullptr), b(nullptr), stride(0), W(0), H(0) {}
    texture2d(const float* r_, const float* g_, const float* b_, int stride_, int W_, int H_)
        : r(r_), g(g_), b(b_), stride(stride_), W(W_), H(H_) {}
    float4 texel(int x, int y) const {
        const long o = ((long)y * W + x) * stride;
        return float4(r[o], g[o], b[o], 1.0f);
    }
    float4 Load(int3 p) const {
        if (p.x < 0 || p.y < 0 || p.x >= W || p.y >= H) return float4(0.0f, 0.0f, 0.0f, 0.0f);
        return texel(p.x, p.y);
    }
    float4 Sample(const sampler&, float2 uv) const {
        const float su = uv.x * (float)W, sv = uv.y * (float)H;
        const float fu = floorf(su), fv = floorf(sv);
        g_sample_dev = fmaxf(g_sample_dev, fmaxf(fabsf((su - fu) - 0.5f), fabsf((sv - fv) - 0.5f)));
        const int x = (int)fminf(fmaxf(fu, 0.0f), (float)(W - 1));
        const int y = (int)fminf(fmaxf(fv, 0.0f), (float)(H - 1));
        return texel(x, y);
    }
};

}  // namespace ffx_shim

#define uniform static
