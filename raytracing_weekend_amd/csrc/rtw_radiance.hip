// rtw_radiance.hip - the radiance-query kernels (rtw_radiance.h), a translation unit of its own under __graft_entry__.build(); a
// single-file build of rtw_hip.hip (scripts/build_variant.sh) includes this file instead.
//
//   k_radiance<KIND, TEX>  whole paths along the caller's rays: a camera path of rtw_render whose camera ray is replaced. The draws
//                          are raygen<>'s for a perspective camera path of pixel key0 + ray, the segments k_bounce's inner loop
//                          (traverse<> over the lists or the tree, volumes included; shade_a, the inline probe, shade_b), the sums
//                          rtw.h's blocks and units. One flattened loop whose body is one path segment, as k_path's.
//   k_radiance_resolve     the unit sums of renders beyond 128 spp, added in order
#include <hip/hip_runtime.h>

#ifndef RTW_TEMPLATES_ONLY
#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#endif
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_radiance.h"

namespace rtwk {

// raygen<>'s draws for a perspective camera path of pixel `key`, sample `sample`, without the camera: the jitter and lens draws
// are consumed and dropped (Philox: words 0-3 of block (key, sample, 0, 0); TEA+LCG: four lcg_rnd), the generator is left where
// raygen<> leaves it, gt is the gather time and ray_time the first segment's
template <int KIND>
RTW_DEV void radiance_raygen(const DScene& sc, const uint32_t seed, const uint32_t key, const uint32_t sample, Rng<KIND>& g, float& gt, float& ray_time) {
    float r4;
    if (KIND == RTW_RNG_TEA_LCG) {
        uint32_t s = tea<64>(key, sample);
        (void)lcg_rnd(s); (void)lcg_rnd(s); (void)lcg_rnd(s); (void)lcg_rnd(s);
        g.init(seed, key, sample, s, s);
        r4 = lcg_rnd(s);
    } else {
        uint32_t o[4];
        philox4x32_10(key, sample, 0u, 0u, seed, 0u, o);
        r4 = (float)(((o[0] & 0xffu) << 16) | ((o[1] & 0xffu) << 8) | (o[2] & 0xffu)) * (1.0f / 16777216.0f);
        g.init(seed, key, sample, 0u, sample);
    }
    gt = fma_(r4, sc.cam.time1 - sc.cam.time0, sc.cam.time0);  // (r4 = k / 2^24: gather_time_of's value for gk = k)
    ray_time = (KIND == RTW_RNG_TEA_LCG || sc.has_motion) ? g.ray_time(0u) : 0.0f;
}

template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_radiance(const DScene sc, const RadianceArgs a) {
    extern __shared__ uint32_t s_stack[];
    RTW_NOISE_SHARED
    // running sum of the lane's summation unit (the sums of its finished blocks, in order): touched once per 16 samples
    __shared__ float s_usum[3][kBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t* noise_lds = stage_noise<(TEX != 0)>(sc, s_noise);
    // it holds a barrier: every thread, before the loop; the branch is uniform (a property of the scene)
    TravMem tm{};
    if (sc.use_bvh) tm = trav_mem(sc, s_stack, kBlock, tid);
    const uint32_t lane = tid & 63u;
    // wave-uniform: the job stream
    uint32_t u_next = 0, u_end = 0;
    bool exhausted = false;
    // per lane, the unit: its ray, the current sample and the unit's end (both relative to sample0), the open block's sum
    bool need = true;
    uint32_t ray = 0, s_cur = 0, s_end = 0;
    v3 bsum = V(0.f, 0.f, 0.f);
    // per lane, the path
    bool alive = false;
    uint32_t depth = 0, rng_a = 0, rng_b = 0, nee_prev = 0;
    float ray_time = 0.f, gt = 0.f, seg_tmin = 0.f, seg_tmax = 0.f;
    v3 o = V(0.f, 0.f, 0.f), d = o, T = o, L = o;
    uint32_t n_seg = 0, n_shadow = 0;
    for (;;) {
        unsigned long long need_mask = __ballot(need);
        while (need_mask != 0ull && !exhausted) {
            if (u_next >= u_end) {  // the wave's next job: one returning atomic by one lane
                uint32_t q = 0;
                if (lane == 0) q = atomicAdd(a.queue, 1u);
                q = __builtin_amdgcn_readfirstlane(q);
                if (q >= a.n_jobs) { exhausted = true; break; }
                u_next = q * a.job_units;
                u_end = min(u_next + a.job_units, a.n_units);
                continue;
            }
            const uint32_t avail = u_end - u_next;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need_mask, 0u));
            if (need && rank < avail) {
                const uint32_t u = u_next + rank;
                const uint32_t unit = fastdiv(u, a.divn_m, a.divn_s1, a.divn_s2);
                ray = u - unit * a.n;
                s_cur = unit * (kSumBlock * kSumUnitBlocks);
                s_end = min(s_cur + kSumBlock * kSumUnitBlocks, a.spp);
                bsum = V(0.f, 0.f, 0.f);
                need = false;
                alive = false;
            }
            u_next += min((uint32_t)__popcll(need_mask), avail);
            need_mask = __ballot(need);
        }
        if (__ballot(!need) == 0ull) break;
        const bool busy = !need;
        const uint32_t key = a.key0 + ray, sample = a.sample0 + s_cur;
        Rng<KIND> g;
        if (busy && !alive) {  // regeneration: the next sample of this lane's unit starts on the caller's ray
            const float4 r0 = a.rays[2 * (size_t)ray], r1 = a.rays[2 * (size_t)ray + 1];  // two 16-byte loads
            o = V(r0.x, r0.y, r0.z); d = V(r0.w, r1.x, r1.y);
            seg_tmin = r1.z; seg_tmax = r1.w;  // the caller's interval bounds the first segment only
            radiance_raygen<KIND>(sc, a.seed, key, sample, g, gt, ray_time);
            rng_a = g.a; rng_b = g.b;
            T = V(1.f, 1.f, 1.f); L = V(0.f, 0.f, 0.f);
            nee_prev = 0; depth = 0; alive = true;
        }
        if (busy) g.init(a.seed, key, sample, rng_a, KIND == RTW_RNG_TEA_LCG ? rng_b : sample);
        if (busy) {
            float th;
            int prim;
            traverse<Rng<KIND>, false, false>(sc, o, d, seg_tmin, seg_tmax, ray_time, gt, g, tm, th, prim);
            v3 so, sd, att, radiance;
            Nee nee;
            const int ev = shade_a<KIND, TEX>(sc, g, o, d, gt, th, prim, so, sd, att, radiance, nee, noise_lds, nee_prev);
            n_seg++;
            if (nee.has) {  // traceOcclusion, closehit.cu:16-42
                float st;
                int sprim;
                traverse<Rng<KIND>, true, false>(sc, so, nee.dir, nee.tmin, nee.tmax, 0.0f, gt, g, tm, st, sprim);
                n_shadow++;
                if (sprim < 0) radiance = vadd(radiance, nee.rad);
            }
            alive = shade_b<KIND>(depth, a.max_depth, g, ev, so, sd, att, radiance, o, d, T, L, TEX == 2 && sc.estimator == RTW_EST_MIXTURE);
            depth++;
            rng_a = g.a;
            if (alive) {
                ray_time = (KIND == RTW_RNG_TEA_LCG || sc.has_motion) ? g.ray_time(depth) : 0.0f;
                rng_b = g.b;
                seg_tmin = sc.ray_tmin; seg_tmax = 1.e27f;  // later segments: the estimator's start distance, as a render
            } else {
                // removeNaNs (raygen.cu:17-24), then the block's running sum, in sample order
                bsum = vadd(bsum, V((L.x == L.x) ? L.x : 0.f, (L.y == L.y) ? L.y : 0.f, (L.z == L.z) ? L.z : 0.f));
                s_cur++;
                if ((s_cur % kSumBlock) == 0u || s_cur >= s_end) {  // a block is complete: its sum joins the unit's
                    const uint32_t b_done = (s_cur - 1u) / kSumBlock;
                    v3 prev = V(0.f, 0.f, 0.f);
                    if ((b_done % kSumUnitBlocks) != 0u) prev = V(s_usum[0][tid], s_usum[1][tid], s_usum[2][tid]);
                    const v3 u = vadd(prev, bsum);
                    bsum = V(0.f, 0.f, 0.f);
                    if (s_cur >= s_end) {  // the unit is complete
                        need = true;
                        if (a.units_per_ray == 1u) {  // at most 128 spp: the unit sum is the total, the lane writes the mean
                            const v3 sum = vadd(V(0.f, 0.f, 0.f), u);
                            const float nf = (float)a.spp;
                            a.out[ray] = make_float4(sum.x / nf, sum.y / nf, sum.z / nf, 1.0f);
                        } else {
                            a.out[(size_t)(b_done / kSumUnitBlocks) * a.n + ray] = make_float4(u.x, u.y, u.z, 0.f);
                        }
                    } else {
                        s_usum[0][tid] = u.x; s_usum[1][tid] = u.y; s_usum[2][tid] = u.z;
                    }
                }
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        n_seg += __shfl_down(n_seg, off);
        n_shadow += __shfl_down(n_shadow, off);
    }
    if (lane == 0) {
        unsigned long long* row = a.stats + (size_t)(blockIdx.x & (kStatRows - 1u)) * 8u;
        if (n_seg) atomicAdd(&row[0], (unsigned long long)n_seg);
        if (n_shadow) atomicAdd(&row[1], (unsigned long long)n_shadow);
    }
}

__global__ void __launch_bounds__(kBlock) k_radiance_resolve(const float4* __restrict__ slab, float4* __restrict__ out, uint32_t n, uint32_t n_units, float spp) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (uint32_t u = 0; u < n_units; u++) {
            const float4 l = slab[(size_t)u * n + i];
            sx += l.x; sy += l.y; sz += l.z;
        }
        out[i] = make_float4(sx / spp, sy / spp, sz / spp, 1.0f);
    }
}

#define RTW_INST(R_) \
    template __global__ void k_radiance<R_, 0>(const DScene, const RadianceArgs); \
    template __global__ void k_radiance<R_, 1>(const DScene, const RadianceArgs); \
    template __global__ void k_radiance<R_, 2>(const DScene, const RadianceArgs);
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST

}  // namespace rtwk
