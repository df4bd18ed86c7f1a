// rtw_inst_path.hip - k_path's frame rows and k_classify's rows of rtw_variants.h, instantiated in a translation unit of their own
// (__graft_entry__.py UNITS compiles the library's kernels side by side, this unit with UNIT_FLAGS; rtw_hip.hip only declares them).
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_variants.h"

namespace rtwk {
#define RTW_INST(K_, name, ...) template __global__ void K_<__VA_ARGS__> RTW_SIG_##K_;
RTW_K_PATH_FRAME_ROWS(RTW_INST)
RTW_K_CLASSIFY_ROWS(RTW_INST)
}  // namespace rtwk
