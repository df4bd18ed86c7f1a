// rtw_cast.h — declarations of the ray-query kernel (rtw_cast.hip): closest-hit and occlusion queries on the caller's own rays
// (rtw.h rtw_cast / rtw_cast_device). Included by rtw_hip.hip, which launches it.
#pragma once
#include "rtw_kernels.h"

namespace rtwk {

// Device pointers of one k_cast launch: n rays of two float4 each (origin, dx | dy, dz, tmin, tmax: rtw.h's eight floats), their
// times (null: 0 for every ray) and the outputs, a null pointer being an output nobody asked for.
struct CastArgs {
    const float4* rays;
    const float* ray_time;
    const float* gather_time;
    uint64_t n;
    float* t;
    int32_t* prim;
    int32_t* material;
    float4* normal;  // xyz the shading normal, w = 1.0f front face / 0.0f
    float2* uv;
};

// One lane per ray, grid-stride over 64-bit ray indices: the launch is persistent, the result of ray i depends on ray i alone.
// ANY_HIT: traverse<>'s occlusion walk (prim = the first accepted candidate, t = tmax). ATTR: the instantiation that also loads the
// hit record and writes material, normal and uv; the other two carry none of that code. Volumes are skipped.
// Dynamic LDS: the scene's traversal stacks and tree nodes (rtw_ctx::lds_bytes, stride kBlock) in tree scenes, as for k_guides.
template <bool ANY_HIT, bool ATTR>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_cast(const DScene sc, const CastArgs a);

}  // namespace rtwk
