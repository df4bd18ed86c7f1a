// rtw_probe.hip - the probe kernels (rtw_probe.h), a translation unit of its own (__graft_entry__.py UNITS).
//
//   k_probe<KIND, TEX>         irradiance at surface points: k_radiance's loop (rtw_radiance_body.h: the same job queue, units, path
//                              segments - traverse<>, shade_a, shade_b - and sums) whose regeneration step draws the first direction
//                              about the probe's normal from the two raygen uniforms that k_radiance drops, so that sample s of
//                              probe i is the rtw_radiance sample of ray (p, d) with the same key and sample index
//   k_probe_resolve            the unit sums of calls beyond 128 spp, added in order; the mean times pi
//   k_probe_occlusion<KIND>    the unoccluded fraction of the same directions: traverse<NoRng, true, true> per sample, integer counts
//   k_probe_occlusion_resolve  the units' counts of calls beyond 128 spp, added as integers
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_probe.h"
#include "rtw_radiance_body.h"

namespace rtwk {

template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe(const DScene sc, const RadianceArgs a) {
    RTW_RADIANCE_BODY(true)
}

__global__ void __launch_bounds__(kBlock) k_probe_resolve(const float4* __restrict__ slab, float4* __restrict__ out, uint32_t n, uint32_t n_units, float spp) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (uint32_t u = 0; u < n_units; u++) {
            const float4 l = slab[(size_t)u * n + i];
            sx += l.x; sy += l.y; sz += l.z;
        }
        out[i] = make_float4((sx / spp) * kProbePi, (sy / spp) * kProbePi, (sz / spp) * kProbePi, 1.0f);
    }
}

// the first two raygen uniforms of the path of stream key `key`, sample `sample`: radiance_raygen's j0 and j1, without the rest
template <int KIND>
RTW_DEV void probe_uniforms(const uint32_t seed, const uint32_t key, const uint32_t sample, float& r1, float& r2) {
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
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_occlusion(const DScene sc, const OcclusionArgs a) {
    extern __shared__ uint32_t s_stack[];
    // it holds a barrier: every thread, before the loop and before any exit; the branch is uniform (a property of the scene)
    TravMem tm{};
    if (sc.use_bvh) tm = trav_mem(sc, s_stack, kBlock, threadIdx.x);
    const uint32_t step = gridDim.x * blockDim.x;  // (at most the device's resident lanes: u + step stays below 2^32)
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < a.n_units; u += step) {
        const uint32_t unit = fastdiv(u, a.divn_m, a.divn_s1, a.divn_s2);
        const uint32_t i = u - unit * a.n;
        const float4 r0 = a.probes[2 * (size_t)i], r1 = a.probes[2 * (size_t)i + 1];
        const v3 o = V(r0.x, r0.y, r0.z), nrm = V(r0.w, r1.x, r1.y);
        const uint32_t s0 = unit * (kSumBlock * kSumUnitBlocks);
        const uint32_t s1 = min(s0 + kSumBlock * kSumUnitBlocks, a.spp);
        const uint32_t key = a.key0 + i;
        uint32_t open = 0;
        for (uint32_t s = s0; s < s1; s++) {
            float j0, j1;
            probe_uniforms<KIND>(a.seed, key, a.sample0 + s, j0, j1);
            const v3 d = probe_direction(nrm, j0, j1);
            NoRng g;
            float t;
            int prim;
            traverse<NoRng, true, true>(sc, o, d, r1.z, r1.w, 0.0f, 0.0f, g, tm, t, prim);
            open += prim < 0 ? 1u : 0u;
        }
        if (a.units_per_probe == 1u) {
            const float f = (float)open / (float)a.spp;
            a.out[i] = make_float4(f, f, f, 1.0f);
        } else {
            a.counts[(size_t)unit * a.n + i] = open;
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_probe_occlusion_resolve(const uint32_t* __restrict__ counts, float4* __restrict__ out, uint32_t n, uint32_t n_units, float spp) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t open = 0;
        for (uint32_t u = 0; u < n_units; u++) open += counts[(size_t)u * n + i];
        const float f = (float)open / spp;
        out[i] = make_float4(f, f, f, 1.0f);
    }
}

#define RTW_INST(R_) \
    template __global__ void k_probe<R_, 0>(const DScene, const RadianceArgs); \
    template __global__ void k_probe<R_, 1>(const DScene, const RadianceArgs); \
    template __global__ void k_probe<R_, 2>(const DScene, const RadianceArgs); \
    template __global__ void k_probe_occlusion<R_>(const DScene, const OcclusionArgs);
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST

}  // namespace rtwk
