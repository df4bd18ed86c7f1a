// rtw_inst_list.hip - the list instantiations (LIST = 1) of k_path and k_first that rtw_render_adaptive's passes run, in a
// translation unit of their own so that the parallel build does not get slower (-DRTW_SPLIT_BUILD: rtw_hip.hip only declares them).
// __graft_entry__.build() compiles it three times: -DRTW_INST_LIST=0 with -DRTW_INST_KIND=0 / 1 (k_path, one generator each, with
// rtw_inst_path.hip's flags: iterative-minreg, RTW_PATH_WAVES=6) and -DRTW_INST_LIST=1 (k_first, default flags, like rtw_inst_shade.hip).
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"

namespace rtwk {
#if !defined(RTW_INST_LIST) || RTW_INST_LIST == 0
// every path_kernel() case: hot, cold, cold + mixture estimator, cold with media (MEDIA5)
#define RTW_INST(R_) \
    template __global__ void k_path<R_, 0, 0, 1>(const KArgs); template __global__ void k_path<R_, 1, 0, 1>(const KArgs); \
    template __global__ void k_path<R_, 2, 0, 1>(const KArgs); template __global__ void k_path<R_, 1, 1, 1>(const KArgs);
#if !defined(RTW_INST_KIND) || RTW_INST_KIND == 0
RTW_INST(RTW_RNG_PHILOX)
template __global__ void k_path<RTW_RNG_PHILOX, 0, 0, 1, 1>(const KArgs);  // the one-light instantiation (NEE1)
template __global__ void k_path<RTW_RNG_PHILOX, 0, 0, 1, 1, WALK_SHAPE_CORNELL>(const KArgs);  // and its fixed-shape twin (SHAPE)
#endif
#if !defined(RTW_INST_KIND) || RTW_INST_KIND == 1
RTW_INST(RTW_RNG_TEA_LCG)
#endif
#undef RTW_INST
#endif
#if !defined(RTW_INST_LIST) || RTW_INST_LIST == 1
#define RTW_INST(R_) \
    template __global__ void k_first<R_, 0, 1>(const KArgs); template __global__ void k_first<R_, 1, 1>(const KArgs); \
    template __global__ void k_first<R_, 2, 1>(const KArgs);
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST
#endif
}  // namespace rtwk
