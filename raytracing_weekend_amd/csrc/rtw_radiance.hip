// rtw_radiance.hip - the radiance-query kernels (rtw_radiance.h), a translation unit of its own (__graft_entry__.py UNITS).
//
//   k_radiance<KIND, TEX>  whole paths along the caller's rays: a camera path of rtw_render whose camera ray is replaced. The draws
//                          are raygen<>'s for a perspective camera path of pixel key0 + ray, the segments k_bounce's inner loop
//                          (traverse<> over the lists or the tree, volumes included; shade_a, the inline probe, shade_b), the sums
//                          rtw.h's blocks and units. One flattened loop whose body is one path segment, as k_path's: the loop is
//                          rtw_radiance_body.h's, which k_probe (rtw_probe.hip) shares.
//   k_radiance_resolve     the unit sums of renders beyond 128 spp, added in order
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_radiance.h"
#include "rtw_radiance_body.h"

namespace rtwk {

template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_radiance(const DScene sc, const RadianceArgs a) {
    RTW_RADIANCE_BODY(false)
}

__global__ void __launch_bounds__(kBlock) k_radiance_resolve(const float4* __restrict__ slab, float4* __restrict__ out, uint32_t n, uint32_t n_units, float spp) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (uint32_t u = 0; u < n_units; u++) {
            const float4 l = slab[(size_t)u * n + i];
            sx += l.x; sy += l.y; sz += l.z;
        }
        out[i] = make_float4(sx / spp, sy / spp, sz / spp, 1.0f);
    }
}

#define RTW_INST(R_) \
    template __global__ void k_radiance<R_, 0>(const DScene, const RadianceArgs); \
    template __global__ void k_radiance<R_, 1>(const DScene, const RadianceArgs); \
    template __global__ void k_radiance<R_, 2>(const DScene, const RadianceArgs);
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST

}  // namespace rtwk
