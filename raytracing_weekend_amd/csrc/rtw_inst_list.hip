// rtw_inst_list.hip - the list rows (LIST = 1) of rtw_variants.h that rtw_render_adaptive's passes run, in translation units of their
// own so that the parallel build does not get slower. __graft_entry__.py UNITS compiles it three times: k_path's list rows, one generator
// each (-DRTW_INST_KIND=0 / 1, with rtw_inst_path.hip's UNIT_FLAGS), and with -DRTW_INST_FIRST k_first's (default flags, like rtw_inst_shade.hip).
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_variants.h"

namespace rtwk {
#define RTW_INST(K_, name, KIND, ...) RTW_IF_##KIND(template __global__ void K_<KIND, __VA_ARGS__> RTW_SIG_##K_;)
#ifdef RTW_INST_FIRST
RTW_K_FIRST_LIST_ROWS(RTW_INST)
#else
RTW_K_PATH_LIST_ROWS(RTW_INST)
#endif
}  // namespace rtwk
