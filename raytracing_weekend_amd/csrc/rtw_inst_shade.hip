// rtw_inst_shade.hip - the rows of the wavefront kernels that shade (k_first's frame rows, k_shade, k_bounce: rtw_variants.h),
// instantiated in a translation unit of their own. It is the longest of the units, so __graft_entry__.py UNITS compiles it twice,
// side by side: -DRTW_INST_KIND=0 / 1 leaves the rows of one generator (rtw_variants.h RTW_IF_<generator>).
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_variants.h"

namespace rtwk {
#define RTW_INST(K_, name, KIND, ...) RTW_IF_##KIND(template __global__ void K_<KIND, __VA_ARGS__> RTW_SIG_##K_;)
RTW_K_FIRST_FRAME_ROWS(RTW_INST)
RTW_K_SHADE_ROWS(RTW_INST)
RTW_K_BOUNCE_ROWS(RTW_INST)
}  // namespace rtwk
