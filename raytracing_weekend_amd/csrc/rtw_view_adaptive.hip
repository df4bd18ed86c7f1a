// rtw_view_adaptive.hip - the kernels of rtw_views_adaptive (rtw_view_adaptive.h), a translation unit of its own (__graft_entry__.py UNITS).
//
//   k_view_list<KIND, TEX>   k_view's samples for the pixels of an active list, blocks [n_from / 16, n_to / 16) of each: the unit of
//                            work is (list position, run of R whole blocks), every block's sum goes to the slab
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_view.h"
#include "rtw_view_adaptive.h"
#include "rtw_radiance_body.h"
#include "rtw_list_body.h"

namespace rtwk {

// RTW_LIST_BODY's regeneration step (rtw_list_body.h) where the entry is a flattened pixel of the call: k_view's, statement for
// statement, so that sample s of a pixel is the sample rtw_views takes. The pixel's key and its view's seed are taken from it again
// in every iteration, as k_view takes them, and nothing of the camera lives across the segment loop: beside the path, a lane keeps
// its position and its pixel.
#define RTW_VIEW_LIST_REGEN \
    view_raygen<KIND>(sc, a.v, entry, seed, sample, g, gt, ray_time, o, d); \
    seg_tmin = sc.ray_tmin; seg_tmax = 1.e27f;  /* the estimator's start distance, as a render's camera ray */

template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_view_list(const DScene sc, const ViewListArgs a) {
    RTW_LIST_BODY(view_key(a.v, entry), view_seed(a.v, entry), RTW_VIEW_LIST_REGEN)
}
#undef RTW_VIEW_LIST_REGEN

#define RTW_INST(R_) \
    template __global__ void k_view_list<R_, 0>(const DScene, const ViewListArgs); \
    template __global__ void k_view_list<R_, 1>(const DScene, const ViewListArgs); \
    template __global__ void k_view_list<R_, 2>(const DScene, const ViewListArgs);
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST

}  // namespace rtwk
