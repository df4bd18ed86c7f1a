// ref_shim_core.h — TEST INFRASTRUCTURE. Host stand-ins for what the reference's device programs include from CUDA and
// the OptiX SDK, so that its .cu files compile with a host C++ compiler, unmodified and from where they lie
// (oracle/ref_programs_wrap.cpp). Written from the published definitions (CUDA vector types, OptiX 8 device API, the SDK's
// sutil/vec_math.h and cuda/random.h); it holds no text of the reference. Every header under oracle/ref_shim/ forwards here.
//
// Two kinds of content:
//   1. types, constants and vector algebra (below): their operation order decides bits, every choice is stated;
//   2. the OptiX device intrinsics, declared here and emulated in ref_programs_wrap.cpp (namespace refemu holds the state).
#ifndef RTW_REF_SHIM_CORE_H
#define RTW_REF_SHIM_CORE_H

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

// ---- CUDA qualifiers: nothing on the host. `extern "C" __constant__ T x;` thereby becomes a plain declaration.
#define __host__
#define __device__
#define __global__
#define __constant__
#define __forceinline__ inline
#define __inline__ inline

// ---- vector_types.h
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct uint2 { unsigned int x, y; };
struct uint3 { unsigned int x, y, z; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
typedef unsigned long long CUdeviceptr;
typedef unsigned long long cudaTextureObject_t;

// ---- math_constants.h
#define CUDART_PI_F 3.141592654f
#define CUDART_PIO2_F 1.570796327f
// ---- sutil/vec_math.h constants
#ifndef M_PIf
#define M_PIf 3.14159265358979323846f
#endif
#ifndef M_1_PIf
#define M_1_PIf 0.318309886183790671538f
#endif
// OptiX 6 optix_device.h (scene/camera.cuh); the oracle and include/rtw.h use the same 1e27
#define RT_DEFAULT_MAX 1.e27f

// ---- device bit casts
inline float __int_as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }
inline float __uint_as_float(unsigned int i) { float f; std::memcpy(&f, &i, 4); return f; }
inline unsigned int __float_as_uint(float f) { unsigned int i; std::memcpy(&i, &f, 4); return i; }
inline int __float_as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }

// ---- constructors (vec_math.h make_* overloads)
inline float2 make_float2(float x, float y) { float2 r = {x, y}; return r; }
inline float2 make_float2(float s) { return make_float2(s, s); }
// make_float3 is a macro over a braced initialiser: the reference draws inside its argument lists
// (make_float3(rnd(seed), rnd(seed), rnd(seed)), lib/sampling.cuh:30, pdf/rectPdf.cu:128-130), C++ leaves the order of
// function arguments open and g++ on x86-64 takes them right to left, while a braced list is evaluated left to right by rule.
// Left to right is the oracle's DEFINITION (rtw_oracle.c header); the shim adopts it, so the referee cannot judge that question:
// what order the device compiler takes has not been measured here.
struct ref_shim_mk3 {
    float3 v;
    template <typename A, typename B, typename C> ref_shim_mk3(A x, B y, C z) { v.x = (float)x; v.y = (float)y; v.z = (float)z; }
    ref_shim_mk3(float s) { v.x = v.y = v.z = s; }
    ref_shim_mk3(const float4& a) { v.x = a.x; v.y = a.y; v.z = a.z; }
};
#define make_float3(...) (ref_shim_mk3{__VA_ARGS__}.v)
inline float4 make_float4(float x, float y, float z, float w) { float4 r = {x, y, z, w}; return r; }
inline float4 make_float4(const float3& a, float w) { return make_float4(a.x, a.y, a.z, w); }
inline uint2 make_uint2(unsigned int x, unsigned int y) { uint2 r = {x, y}; return r; }
inline uint3 make_uint3(unsigned int x, unsigned int y, unsigned int z) { uint3 r = {x, y, z}; return r; }

// ---- scalar helpers. CUDA's min / max on floats are fminf / fmaxf; vec_math.h's clamp is max(a, min(f, b)).
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline float clamp(float f, float a, float b) { return fmaxf(a, fminf(f, b)); }
inline int clamp(int f, int a, int b) { return max(a, min(f, b)); }

// ---- float3 algebra, component by component, each product and sum rounded on its own unless the compiler is told to
// contract (the _fma build). Choices that decide bits:
//   a / s (s scalar)   multiplies by the reciprocal 1.0f / s, as vec_math.h does (the oracle divides by r the same way: Q13 code)
//   a / b (vectors)    divides component by component
//   dot                (a.x * b.x + a.y * b.y) + a.z * b.z, left to right (the oracle nests fmaf from x outwards: same order)
//   normalize          v * (1.0f / sqrtf(dot(v, v)))                       (rtw_oracle.c normalize3 agrees)
//   length             sqrtf(dot(v, v))
//   reflect(i, n)      i - 2.0f * n * dot(n, i): the vector 2 n first, then its product with the dot
//                      (the oracle forms k = -2 dot and fma(n, k, i): same real number, other roundings)
//   cross              (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)
//   fmaxf(a)           fmaxf(fmaxf(a.x, a.y), a.z); fminf(a) alike
inline float3 operator-(const float3& a) { return make_float3(-a.x, -a.y, -a.z); }
inline float3 operator+(const float3& a, const float3& b) { return make_float3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline float3 operator+(const float3& a, float b) { return make_float3(a.x + b, a.y + b, a.z + b); }
inline float3 operator+(float a, const float3& b) { return make_float3(a + b.x, a + b.y, a + b.z); }
inline float3 operator-(const float3& a, const float3& b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline float3 operator-(const float3& a, float b) { return make_float3(a.x - b, a.y - b, a.z - b); }
inline float3 operator-(float a, const float3& b) { return make_float3(a - b.x, a - b.y, a - b.z); }
inline float3 operator*(const float3& a, const float3& b) { return make_float3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline float3 operator*(const float3& a, float s) { return make_float3(a.x * s, a.y * s, a.z * s); }
inline float3 operator*(float s, const float3& a) { return make_float3(s * a.x, s * a.y, s * a.z); }
inline float3 operator/(const float3& a, const float3& b) { return make_float3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline float3 operator/(const float3& a, float s) { float inv = 1.0f / s; return a * inv; }
inline float3 operator/(float s, const float3& a) { return make_float3(s / a.x, s / a.y, s / a.z); }
inline void operator+=(float3& a, const float3& b) { a.x += b.x; a.y += b.y; a.z += b.z; }
inline void operator-=(float3& a, const float3& b) { a.x -= b.x; a.y -= b.y; a.z -= b.z; }
inline void operator*=(float3& a, const float3& b) { a.x *= b.x; a.y *= b.y; a.z *= b.z; }
inline void operator*=(float3& a, float s) { a.x *= s; a.y *= s; a.z *= s; }
inline void operator/=(float3& a, const float3& b) { a.x /= b.x; a.y /= b.y; a.z /= b.z; }
inline void operator/=(float3& a, float s) { float inv = 1.0f / s; a *= inv; }
inline float dot(const float3& a, const float3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline float length(const float3& v) { return sqrtf(dot(v, v)); }
inline float3 normalize(const float3& v) { float invLen = 1.0f / sqrtf(dot(v, v)); return v * invLen; }
inline float3 cross(const float3& a, const float3& b) {
    return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
inline float3 reflect(const float3& i, const float3& n) { return i - 2.0f * n * dot(n, i); }
inline float3 fminf(const float3& a, const float3& b) { return make_float3(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z)); }
inline float3 fmaxf(const float3& a, const float3& b) { return make_float3(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z)); }
inline float fminf(const float3& a) { return fminf(fminf(a.x, a.y), a.z); }
inline float fmaxf(const float3& a) { return fmaxf(fmaxf(a.x, a.y), a.z); }
inline float3 expf(const float3& v) { return make_float3(::expf(v.x), ::expf(v.y), ::expf(v.z)); }
inline float2 operator*(const float2& a, float s) { return make_float2(a.x * s, a.y * s); }
inline float2 operator+(const float2& a, const float2& b) { return make_float2(a.x + b.x, a.y + b.y); }

// ---- cuda/random.h of the OptiX SDK (published definition; DESIGN.md restates the same lcg / rnd for the oracle).
// tea<N> is the SDK's too, but the reference carries its own copy in lib/random.cuh, which the wrapper includes: none here.
namespace refemu { extern thread_local unsigned long long rnd_calls; }
static inline unsigned int lcg(unsigned int& prev) {
    const unsigned int LCG_A = 1664525u;
    const unsigned int LCG_C = 1013904223u;
    prev = (LCG_A * prev + LCG_C);
    return prev & 0x00FFFFFF;
}
static inline float rnd(unsigned int& prev) {
    refemu::rnd_calls++;
    return ((float)lcg(prev) / (float)0x01000000);
}

// ---- OptiX device API (optix.h, optix_types.h): what the reference's programs name
typedef unsigned long long OptixTraversableHandle;
typedef unsigned int OptixVisibilityMask;
enum OptixPayloadTypeID { OPTIX_PAYLOAD_TYPE_DEFAULT = 0, OPTIX_PAYLOAD_TYPE_ID_0 = 1u << 0 };
enum OptixRayFlags {
    OPTIX_RAY_FLAG_NONE = 0u,
    OPTIX_RAY_FLAG_DISABLE_ANYHIT = 1u << 0,
    OPTIX_RAY_FLAG_ENFORCE_ANYHIT = 1u << 1,
    OPTIX_RAY_FLAG_TERMINATE_ON_FIRST_HIT = 1u << 2,
    OPTIX_RAY_FLAG_DISABLE_CLOSESTHIT = 1u << 3
};

namespace refemu {
// the direct-callable table: one untyped entry point per SBT callable index (shaders/FunctionIdx.h lays the indices out)
extern void* callables[64];
[[noreturn]] void missing_callable(unsigned int idx);
void traverse(float3 o, float3 d, float tmin, float tmax, float ray_time, unsigned int flags, unsigned int p0, unsigned int p1);
void invoke();
}

// optixDirectCall<Ret, Args...>(sbt index, args...): the entry is called with exactly the signature the CALL SITE names, as
// the device does (a callable whose own parameter list differs is the caller's business there as well).
template <typename ReturnT, typename... ArgTypes>
inline ReturnT optixDirectCall(unsigned int sbtIndex, ArgTypes... args) {
    if (sbtIndex >= 64u || !refemu::callables[sbtIndex]) refemu::missing_callable(sbtIndex);
    typedef ReturnT (*fn_t)(ArgTypes...);
    return reinterpret_cast<fn_t>(refemu::callables[sbtIndex])(args...);
}

void* optixGetSbtDataPointer();
float3 optixGetObjectRayOrigin();
float3 optixGetObjectRayDirection();
float3 optixGetWorldRayOrigin();
float3 optixGetWorldRayDirection();
float optixGetRayTmin();
float optixGetRayTmax();
float optixGetRayTime();
float3 optixTransformPointFromObjectToWorldSpace(float3 p);
float3 optixTransformNormalFromObjectToWorldSpace(float3 n);
bool optixReportIntersection(float t, unsigned int kind, unsigned int a0, unsigned int a1, unsigned int a2, unsigned int a3,
                             unsigned int a4, unsigned int a5, unsigned int a6, unsigned int a7);
unsigned int optixGetPayload_0();
unsigned int optixGetPayload_1();
unsigned int optixGetAttribute_0();
unsigned int optixGetAttribute_1();
unsigned int optixGetAttribute_2();
unsigned int optixGetAttribute_3();
unsigned int optixGetAttribute_4();
unsigned int optixGetAttribute_5();
unsigned int optixGetAttribute_6();
unsigned int optixGetAttribute_7();
unsigned int optixGetInstanceId();
uint3 optixGetLaunchIndex();
uint3 optixGetLaunchDimensions();
bool optixHitObjectIsHit();
inline void optixReorder() {}
// optixTraverse fills the hit object and runs no closest-hit or miss program; optixInvoke runs the one the hit object names.
inline void optixTraverse(OptixPayloadTypeID, OptixTraversableHandle, float3 o, float3 d, float tmin, float tmax, float rayTime,
                          OptixVisibilityMask, unsigned int rayFlags, unsigned int, unsigned int, unsigned int, unsigned int& p0,
                          unsigned int& p1) {
    refemu::traverse(o, d, tmin, tmax, rayTime, rayFlags, p0, p1);
}
inline void optixTraverse(OptixTraversableHandle, float3 o, float3 d, float tmin, float tmax, float rayTime, OptixVisibilityMask,
                          unsigned int rayFlags, unsigned int, unsigned int, unsigned int, unsigned int& p0, unsigned int& p1) {
    refemu::traverse(o, d, tmin, tmax, rayTime, rayFlags, p0, p1);
}
inline void optixInvoke(OptixPayloadTypeID, unsigned int&, unsigned int&) { refemu::invoke(); }

// ---- OptiX 6 names that scene/camera.cuh (the environment and orthographic cameras) is written in
#define rtDeclareVariable(type, name, semantic, annotation) type name
namespace optix {
struct Ray { float3 origin, direction; unsigned int ray_type; float tmin, tmax; };
inline Ray make_Ray(float3 o, float3 d, unsigned int type, float tmin, float tmax) { Ray r = {o, d, type, tmin, tmax}; return r; }
inline float3 normalize(const float3& v) { return ::normalize(v); }
}

#endif
