// rtw_probe_adaptive.h — declarations of the kernels of rtw_probe_adaptive / rtw_probe_adaptive_device (rtw.h): probes sampled from
// checkpoint to checkpoint over a list of the probes that are still active, every 16-sample block sum left in memory for the
// batch-means error. The state, the checkpoint loop and its kernels are the adaptive family's (rtw_adaptive.h, run over a "frame" of
// n x 1 probes); what is the probes' own is the pass (k_probe_list, k_probe_occlusion_list) and what occlusion counts need.
// Included by rtw_hip.hip, which launches them; the kernels are in rtw_probe_adaptive.hip.
#pragma once
#include "rtw_kernels.h"
#include "rtw_list_body.h"
#include "rtw_probe.h"

namespace rtwk {

// One pass launch (rtw_list_body.h ListPass) over the call's probes, two float4 each; probe p draws from the stream of key0 + p
struct ProbeListArgs {
    const float4* probes;
    ListPass p;
    uint32_t sample0, seed, max_depth, key0;
};
static_assert(offsetof(ProbeListArgs, p) == 8 && offsetof(ProbeListArgs, sample0) == 80 && sizeof(ProbeListArgs) == 96,
              "ListPass stands where its members stood: no kernel argument moves");

// k_probe's path (radiance_raygen<KIND, true> + probe_direction, then traverse / shade_a / the inline shadow ray / shade_b per
// segment) in k_radiance's persistent scheme: a wave takes jobs from the queue with one atomic by one lane, its lanes take units by
// ballot rank. A finished block's sum goes straight to the slab: nothing is summed across blocks in the kernel.
template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_list(const DScene sc, const ProbeListArgs a);

// k_probe_occlusion's sample (traverse<NoRng, true, true>) over the same units, lanes striding over them: one count per block
template <int KIND>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_occlusion_list(const DScene sc, const ProbeListArgs a);

// an occlusion pass's counts [block][position] into the listed probes' totals and moments: y_b = (float)c_b * 0.0625f
__global__ void __launch_bounds__(kBlock) k_probe_adapt_resolve_counts(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ list,
                                                                       uint32_t n_list, uint32_t n_blocks, uint32_t* __restrict__ total,
                                                                       double2* __restrict__ mom);

// an occlusion call's results: (float)open / (float)n_i in three channels, alpha 1; spp_out and err_out where they are not null
__global__ void __launch_bounds__(kBlock) k_probe_adapt_finish_occlusion(const uint32_t* __restrict__ total, const uint32_t* __restrict__ n,
                                                                         const float* __restrict__ err, float4* __restrict__ out,
                                                                         int32_t* __restrict__ spp_out, float* __restrict__ err_out, uint32_t n_probes);

}  // namespace rtwk
