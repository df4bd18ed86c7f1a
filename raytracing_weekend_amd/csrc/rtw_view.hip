// rtw_view.hip - the view kernel (rtw_view.h), a translation unit of its own under __graft_entry__.build(); a single-file build
// of rtw_hip.hip (scripts/build_variant.sh) includes this file instead.
//
//   k_view<KIND, TEX>  frames from the caller's cameras: k_radiance's loop (rtw_radiance_body.h: the same job queue, units, path
//                      segments - traverse<>, shade_a, shade_b - and summation order) whose "ray" is a pixel of the flattened
//                      (view, y, x) index and whose regeneration step is raygen<>'s camera, read from the pixel's view record:
//                      the jitter and lens draws that k_radiance drops are used. Frames beyond 128 spp resolve through
//                      k_radiance_resolve.
#include <hip/hip_runtime.h>

#ifndef RTW_TEMPLATES_ONLY
#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#endif
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_view.h"
#include "rtw_radiance_body.h"

namespace rtwk {

template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_view(const DScene sc, const ViewArgs a) {
    RTW_RADIANCE_BODY(3)
}

#define RTW_INST(R_) \
    template __global__ void k_view<R_, 0>(const DScene, const ViewArgs); \
    template __global__ void k_view<R_, 1>(const DScene, const ViewArgs); \
    template __global__ void k_view<R_, 2>(const DScene, const ViewArgs);
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST

}  // namespace rtwk
