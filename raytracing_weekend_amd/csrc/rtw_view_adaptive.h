// rtw_view_adaptive.h — declarations of the kernels of rtw_views_adaptive / rtw_views_adaptive_device (rtw.h): the pixels of a batch of
// views sampled from checkpoint to checkpoint over a list of the pixels that are still active, every 16-sample block sum left in
// memory for the batch-means error. The state, the checkpoint loop and its kernels are the adaptive family's (rtw_adaptive.h, run
// over the flattened (view, y, x) index, the stop rule's neighbourhood kept inside the pixel's own view); what is the views' own is
// the pass, k_view_list. Included by rtw_hip.hip, which launches it; the kernel is in rtw_view_adaptive.hip.
#pragma once
#include "rtw_kernels.h"
#include "rtw_list_body.h"
#include "rtw_view.h"

namespace rtwk {

// One pass launch (rtw_list_body.h ListPass) over the flattened pixels of the call.
// `v` is what view_split / view_raygen read (rtw_radiance_body.h): the call's records, width, height, first = 0 and the two divisors;
// its other members are unused.
struct ViewListArgs {
    ViewArgs v;
    ListPass p;
    uint32_t sample0, max_depth;
};
static_assert(offsetof(ViewListArgs, p) == sizeof(ViewArgs) && offsetof(ViewListArgs, sample0) == sizeof(ViewArgs) + 72 &&
                  sizeof(ViewListArgs) == sizeof(ViewArgs) + 80,
              "ListPass stands where its members stood: no kernel argument moves");

// k_view's path (view_raygen<KIND>, then traverse / shade_a / the inline shadow ray / shade_b per segment) in k_probe_list's
// persistent scheme: a wave takes jobs from the queue with one atomic by one lane, its lanes take units by ballot rank. A finished
// block's sum goes straight to the slab: nothing is summed across blocks in the kernel.
template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_view_list(const DScene sc, const ViewListArgs a);

}  // namespace rtwk
