// rtw_probe_adaptive.h — declarations of the kernels of rtw_probe_adaptive / rtw_probe_adaptive_device (rtw.h): probes sampled from
// checkpoint to checkpoint over a list of the probes that are still active, every 16-sample block sum left in memory for the
// batch-means error (rtw_adaptive.h: the moments, the error, the stop rule and the list's layout are rtw_render_adaptive's, and its
// k_adapt_resolve_blocks / k_adapt_decide / k_adapt_scan / k_adapt_compact run here unchanged, over a "frame" of n x 1 probes).
// Included by rtw_hip.hip, which launches them; the kernels are in rtw_probe_adaptive.hip.
#pragma once
#include "rtw_kernels.h"
#include "rtw_probe.h"

namespace rtwk {

// One pass launch over `n` list positions: position i is probe list[1 + i] of the call (the host hands in the list pointer moved to
// the range's first position). The pass adds n_blocks blocks to each, the samples [s_from, s_from + 16 * n_blocks) counted from
// sample0. The unit of work is (position, run of run_blocks whole blocks), numbered run-major: u -> position = u % n, run = u / n,
// so that neighbouring lanes hold neighbouring positions. n_units = n * runs < 2^31 (rtw_probe_adaptive_plan.h).
struct ProbeListArgs {
    const float4* probes;       // the call's probes, two float4 each
    const uint32_t* list;
    float4* out;                // block sums [block of the pass][position]; k_probe_occlusion_list: uint32 counts, the same index
    uint32_t* queue;            // k_probe_list: [0] next job of the launch, zeroed by the host on the launch stream
    unsigned long long* stats;  // k_probe_list: kStatRows rows of 8: [0] segments, [1] shadow rays
    uint32_t n, n_blocks, run_blocks, n_units;
    uint32_t job_units, n_jobs;
    uint32_t divn_m, divn_s1, divn_s2;  // exact division by n (magic_div)
    uint32_t s_from, sample0, seed, max_depth, key0;  // probe p draws from the stream of key0 + p
};

// k_probe's path (radiance_raygen<KIND, true> + probe_direction, then traverse / shade_a / the inline shadow ray / shade_b per
// segment) in k_radiance's persistent scheme: a wave takes jobs from the queue with one atomic by one lane, its lanes take units by
// ballot rank. A finished block's sum goes straight to the slab: nothing is summed across blocks in the kernel.
template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_list(const DScene sc, const ProbeListArgs a);

// k_probe_occlusion's sample (traverse<NoRng, true, true>) over the same units, lanes striding over them: one count per block
template <int KIND>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_occlusion_list(const DScene sc, const ProbeListArgs a);

// the start of a call: every probe active (identity list), sums, moments and totals zero
__global__ void __launch_bounds__(kBlock) k_probe_adapt_init(uint32_t* __restrict__ list, float4* __restrict__ accum, float4* __restrict__ upart,
                                                             double2* __restrict__ mom, uint32_t* __restrict__ n, float* __restrict__ err,
                                                             uint32_t* __restrict__ total, uint32_t n_probes);

// an occlusion pass's counts [block][position] into the listed probes' totals and moments: y_b = (float)c_b * 0.0625f
__global__ void __launch_bounds__(kBlock) k_probe_adapt_resolve_counts(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ list,
                                                                       uint32_t n_list, uint32_t n_blocks, uint32_t* __restrict__ total,
                                                                       double2* __restrict__ mom);

// the results: the open unit joins the total, (sum / (float)n_i) * pi, alpha 1 - or (float)open / (float)n_i; spp_out and err_out
// where they are not null
__global__ void __launch_bounds__(kBlock) k_probe_adapt_finish(const float4* __restrict__ accum, const float4* __restrict__ upart,
                                                               const uint32_t* __restrict__ n, const float* __restrict__ err, float4* __restrict__ out,
                                                               int32_t* __restrict__ spp_out, float* __restrict__ err_out, uint32_t n_probes);
__global__ void __launch_bounds__(kBlock) k_probe_adapt_finish_occlusion(const uint32_t* __restrict__ total, const uint32_t* __restrict__ n,
                                                                         const float* __restrict__ err, float4* __restrict__ out,
                                                                         int32_t* __restrict__ spp_out, float* __restrict__ err_out, uint32_t n_probes);

}  // namespace rtwk
