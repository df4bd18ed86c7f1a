// rtw_view_adaptive.h — declarations of the kernels of rtw_views_adaptive / rtw_views_adaptive_device (rtw.h): the pixels of a batch of
// views sampled from checkpoint to checkpoint over a list of the pixels that are still active, every 16-sample block sum left in
// memory for the batch-means error. The list, the per-pixel state, the moments and the error are rtw_render_adaptive's
// (rtw_adaptive.h): its k_adapt_resolve_blocks / k_adapt_scan / k_adapt_compact run here unchanged over the flattened
// (view, y, x) index, and the stop rule is k_adapt_decide's with the neighbourhood kept inside the pixel's own view. The start and
// the end of a call are rtw_probe_adaptive's k_probe_adapt_init and k_view_adapt_finish, its k_probe_adapt_finish without the factor pi.
// Included by rtw_hip.hip, which launches them; the kernels are in rtw_view_adaptive.hip.
#pragma once
#include "rtw_kernels.h"
#include "rtw_view.h"

namespace rtwk {

// One pass launch over `n` list positions: position i is flattened pixel list[1 + i] of the call (the host hands in the list pointer
// moved to the range's first position). The pass adds n_blocks blocks to each, the samples [s_from, s_from + 16 * n_blocks) counted
// from sample0. The unit of work is (position, run of run_blocks whole blocks), numbered run-major as ProbeListArgs' units are:
// u -> position = u % n, run = u / n. n_units = n * runs < 2^31 (rtw_probe_adaptive_plan.h).
// `v` is what view_split / view_raygen read (rtw_radiance_body.h): the call's records, width, height, first = 0 and the two divisors;
// its other members are unused.
struct ViewListArgs {
    ViewArgs v;
    const uint32_t* list;
    float4* out;                // block sums [block of the pass][position]
    uint32_t* queue;            // [0] next job of the launch, zeroed by the host on the launch stream
    unsigned long long* stats;  // kStatRows rows of 8: [0] segments, [1] shadow rays
    uint32_t n, n_blocks, run_blocks, n_units;
    uint32_t job_units, n_jobs;
    uint32_t divn_m, divn_s1, divn_s2;  // exact division by n (magic_div)
    uint32_t s_from, sample0, max_depth;
};

// k_view's path (view_raygen<KIND>, then traverse / shade_a / the inline shadow ray / shade_b per segment) in k_probe_list's
// persistent scheme: a wave takes jobs from the queue with one atomic by one lane, its lanes take units by ballot rank. A finished
// block's sum goes straight to the slab: nothing is summed across blocks in the kernel.
template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_view_list(const DScene sc, const ViewListArgs a);

// k_adapt_decide (rtw_adaptive.h) over n_views frames of width x height: one wave per 64 consecutive flattened pixels (a wave may
// span two views), p -> (view, y, x) by the exact divisions of view_split, the 3x3 neighbourhood clamped to the pixel's own frame:
// neighbour (xx, yy) is pixel view * width * height + yy * width + xx, so a tap never reads another view. With dilate = 0, or with
// one view, masks and err are k_adapt_decide's.
struct ViewDecideArgs {
    uint32_t width, height, npix;  // npix = n_views * width * height
    uint32_t divw_m, divw_s1, divw_s2;  // exact division by width
    uint32_t divf_m, divf_s1, divf_s2;  // exact division by width * height
    uint32_t B, at_cap, dilate;
    float threshold;
};
__global__ void __launch_bounds__(kBlock) k_view_adapt_decide(const double2* __restrict__ mom, const uint32_t* __restrict__ n, float* __restrict__ err,
                                                              unsigned long long* __restrict__ masks, const ViewDecideArgs a);

// the results: k_adapt_finish's mean (the open unit joins the total, sum / (float)n_p, alpha 1), spp_out and err_out where they are
// not null
__global__ void __launch_bounds__(kBlock) k_view_adapt_finish(const float4* __restrict__ accum, const float4* __restrict__ upart,
                                                              const uint32_t* __restrict__ n, const float* __restrict__ err, float4* __restrict__ out,
                                                              int32_t* __restrict__ spp_out, float* __restrict__ err_out, uint32_t npix);

}  // namespace rtwk
