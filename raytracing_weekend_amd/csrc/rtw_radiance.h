// rtw_radiance.h — declarations of the radiance-query kernels (rtw_radiance.hip): whole paths along the caller's own rays
// (rtw.h rtw_radiance / rtw_radiance_device). Included by rtw_hip.hip, which launches them.
#pragma once
#include "rtw_kernels.h"

namespace rtwk {

// One k_radiance launch: n rays of two float4 each (rtw_cast's layout), spp samples of each from sample index sample0, ray i on the
// stream of key0 + i. The unit of work is (ray, summation unit of up to 128 samples), numbered unit-major: u -> ray = u % n,
// unit = u / n, so that neighbouring lanes hold neighbouring rays. n_units = n * units_per_ray < 2^31 (rtw_radiance_plan.h).
struct RadianceArgs {
    const float4* rays;
    float4* out;                // units_per_ray == 1: the mean of ray i at [i]; else the unit sums, [unit][ray]
    uint32_t* queue;            // [0]: next job of the launch, zeroed by the host on the launch stream
    unsigned long long* stats;  // kStatRows rows of 8: [0] segments, [1] shadow rays (row = workgroup & 63)
    uint32_t n, units_per_ray, n_units;
    uint32_t job_units, n_jobs;  // a job is job_units consecutive units (a multiple of 64), the last one shorter
    uint32_t divn_m, divn_s1, divn_s2;  // exact division by n (magic_div)
    uint32_t spp, sample0, seed, max_depth, key0;
};

// KIND x TEX as k_bounce (the generator; 0 hot, 1 cold features, 2 cold features + the mixture estimator). Persistent launch: a
// wave takes jobs from the queue, its lanes take units by ballot rank, a lane whose path ended starts its next sample in the same
// iteration. Dynamic LDS: the scene's traversal stacks and tree nodes (rtw_ctx::lds_bytes, stride kBlock) in tree scenes.
template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_radiance(const DScene sc, const RadianceArgs a);

// mean of ray i: its n_units unit sums slab[unit][i] added in ascending order, divided by spp, alpha 1 (n_units = 0: zeros)
__global__ void __launch_bounds__(kBlock) k_radiance_resolve(const float4* __restrict__ slab, float4* __restrict__ out, uint32_t n, uint32_t n_units, float spp);

}  // namespace rtwk
