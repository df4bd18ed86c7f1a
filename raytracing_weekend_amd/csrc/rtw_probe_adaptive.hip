// rtw_probe_adaptive.hip - the kernels of rtw_probe_adaptive (rtw_probe_adaptive.h), a translation unit of its own (__graft_entry__.py UNITS).
//
//   k_probe_list<KIND, TEX>            k_probe's samples for the probes of an active list, blocks [n_from / 16, n_to / 16) of each: the
//                                      unit of work is (list position, run of R whole blocks), every block's sum goes to the slab
//   k_probe_occlusion_list<KIND>       k_probe_occlusion's samples over the same units: one unoccluded count per block
//   k_probe_adapt_resolve_counts       an occlusion pass's counts into totals and moments (irradiance passes are resolved by
//                                      rtw_adaptive.h's k_adapt_resolve_blocks)
//   k_probe_adapt_finish_occlusion     an occlusion call's results, the sample counts and the errors
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_probe.h"
#include "rtw_probe_adaptive.h"
#include "rtw_list_body.h"
#include "rtw_radiance_body.h"

namespace rtwk {

// RTW_LIST_BODY's regeneration step (rtw_list_body.h) where the entry is a probe of the call: k_probe's, statement for statement, so
// that sample s of probe p is the sample rtw_probe takes
#define RTW_PROBE_LIST_REGEN \
    const float4 r0 = a.probes[2 * (size_t)entry], r1 = a.probes[2 * (size_t)entry + 1];  /* two 16-byte loads */ \
    o = V(r0.x, r0.y, r0.z); d = V(r0.w, r1.x, r1.y); \
    seg_tmin = r1.z; seg_tmax = r1.w;  /* the caller's interval bounds the first segment only */ \
    float jitter[2]; \
    radiance_raygen<KIND, true>(sc, seed, key, sample, g, gt, ray_time, jitter); \
    d = probe_direction(d, jitter[0], jitter[1]);

template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_list(const DScene sc, const ProbeListArgs a) {
    RTW_LIST_BODY(a.key0 + entry, a.seed, RTW_PROBE_LIST_REGEN)
}
#undef RTW_PROBE_LIST_REGEN

// the first two raygen uniforms of the path of stream key `key`, sample `sample` (k_probe_occlusion's probe_uniforms)
template <int KIND>
RTW_DEV void probe_list_uniforms(const uint32_t seed, const uint32_t key, const uint32_t sample, float& r1, float& r2) {
    if (KIND == RTW_RNG_TEA_LCG) {
        uint32_t s = tea<64>(key, sample);
        r1 = lcg_rnd(s); r2 = lcg_rnd(s);
    } else {
        uint32_t o[4];
        philox4x32_10(key, sample, 0u, 0u, seed, 0u, o);
        r1 = u24(o[0]); r2 = u24(o[1]);
    }
}

template <int KIND>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_occlusion_list(const DScene sc, const ProbeListArgs a) {
    extern __shared__ uint32_t s_stack[];
    // it holds a barrier: every thread, before the loop and before any exit; the branch is uniform (a property of the scene)
    TravMem tm{};
    if (sc.use_bvh) tm = trav_mem(sc, s_stack, kBlock, threadIdx.x);
    uint32_t* const counts = (uint32_t*)a.p.out;
    const uint32_t step = gridDim.x * blockDim.x;  // (at most the device's resident lanes: u + step stays below 2^32)
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < a.p.n_units; u += step) {
        const uint32_t run = fastdiv(u, a.p.divn_m, a.p.divn_s1, a.p.divn_s2);
        const uint32_t pos = u - run * a.p.n;
        const uint32_t probe = a.p.list[1u + pos];
        const float4 r0 = a.probes[2 * (size_t)probe], r1 = a.probes[2 * (size_t)probe + 1];
        const v3 o = V(r0.x, r0.y, r0.z), nrm = V(r0.w, r1.x, r1.y);
        const uint32_t key = a.key0 + probe;
        const uint32_t b1 = min(run * a.p.run_blocks + a.p.run_blocks, a.p.n_blocks);
        for (uint32_t b = run * a.p.run_blocks; b < b1; b++) {
            const uint32_t s0 = a.p.s_from + b * kSumBlock;
            uint32_t open = 0;
            for (uint32_t s = s0; s < s0 + kSumBlock; s++) {
                float j0, j1;
                probe_list_uniforms<KIND>(a.seed, key, a.sample0 + s, j0, j1);
                const v3 d = probe_direction(nrm, j0, j1);
                NoRng g;
                float t;
                int prim;
                traverse<NoRng, true, true>(sc, o, d, r1.z, r1.w, 0.0f, 0.0f, g, tm, t, prim);
                open += prim < 0 ? 1u : 0u;
            }
            counts[(size_t)b * a.p.n + pos] = open;
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_probe_adapt_resolve_counts(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ list,
                                                                       uint32_t n_list, uint32_t n_blocks, uint32_t* __restrict__ total,
                                                                       double2* __restrict__ mom) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_list; i += gridDim.x * blockDim.x) {
        const uint32_t p = list[1u + i];
        uint32_t t = total[p];
        double2 m = mom[p];
        for (uint32_t b = 0; b < n_blocks; b++) {
            const uint32_t c = counts[(size_t)b * n_list + i];
            const double y = (double)((float)c * 0.0625f);  // the block's unoccluded fraction (rtw.h), then adapt_moments' two sums
            m.x = m.x + y;
            m.y = m.y + y * y;
            t += c;
        }
        total[p] = t; mom[p] = m;
    }
}

__global__ void __launch_bounds__(kBlock) k_probe_adapt_finish_occlusion(const uint32_t* __restrict__ total, const uint32_t* __restrict__ n,
                                                                         const float* __restrict__ err, float4* __restrict__ out,
                                                                         int32_t* __restrict__ spp_out, float* __restrict__ err_out, uint32_t n_probes) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_probes; i += gridDim.x * blockDim.x) {
        const float f = (float)total[i] / (float)n[i];
        out[i] = make_float4(f, f, f, 1.0f);
        if (spp_out) spp_out[i] = (int32_t)n[i];
        if (err_out) err_out[i] = err[i];
    }
}

#define RTW_INST(R_) \
    template __global__ void k_probe_list<R_, 0>(const DScene, const ProbeListArgs); \
    template __global__ void k_probe_list<R_, 1>(const DScene, const ProbeListArgs); \
    template __global__ void k_probe_list<R_, 2>(const DScene, const ProbeListArgs); \
    template __global__ void k_probe_occlusion_list<R_>(const DScene, const ProbeListArgs);
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST

}  // namespace rtwk
