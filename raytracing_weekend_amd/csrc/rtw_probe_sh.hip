// rtw_probe_sh.hip - the spherical-harmonic probe kernels (rtw_probe_sh.h), a translation unit of its own (__graft_entry__.py UNITS).
//
//   k_probe_sh<KIND, TEX>  light probes at free points: k_radiance's loop (rtw_radiance_body.h: the same job queue, units, path
//                          segments - traverse<>, shade_a, shade_b - and summation order) whose regeneration step draws the first
//                          direction uniformly over the sphere from the two raygen uniforms that k_radiance drops, and whose
//                          finished paths add Y_j(d) * L to the 27 sums of nine coefficients. The open block's sums and the
//                          path's first direction live in LDS, the unit sums in the words that receive them.
//   k_probe_sh_resolve     the unit sums of calls beyond 128 spp, added in order; the mean times 4 pi
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_probe_sh.h"
#include "rtw_radiance_body.h"

namespace rtwk {

template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_sh(const DScene sc, const RadianceArgs a) {
    RTW_RADIANCE_BODY(2)
}

__global__ void __launch_bounds__(kBlock) k_probe_sh_resolve(const float4* __restrict__ slab, float4* __restrict__ out, uint32_t n, uint32_t n_units, float spp) {
    const size_t per_unit = 9 * (size_t)n;  // (below 2^31: rtw_radiance_plan.h)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_unit; i += (size_t)gridDim.x * blockDim.x) {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (uint32_t u = 0; u < n_units; u++) {
            const float4 l = slab[(size_t)u * per_unit + i];
            sx += l.x; sy += l.y; sz += l.z;
        }
        out[i] = make_float4((sx / spp) * kProbeSh4Pi, (sy / spp) * kProbeSh4Pi, (sz / spp) * kProbeSh4Pi, 0.0f);
    }
}

#define RTW_INST(R_) \
    template __global__ void k_probe_sh<R_, 0>(const DScene, const RadianceArgs); \
    template __global__ void k_probe_sh<R_, 1>(const DScene, const RadianceArgs); \
    template __global__ void k_probe_sh<R_, 2>(const DScene, const RadianceArgs);
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST

}  // namespace rtwk
