// rtw_probe_adaptive.hip - the kernels of rtw_probe_adaptive (rtw_probe_adaptive.h), a translation unit of its own (__graft_entry__.py UNITS).
//
//   k_probe_list<KIND, TEX>            k_probe's samples for the probes of an active list, blocks [n_from / 16, n_to / 16) of each: the
//                                      unit of work is (list position, run of R whole blocks), every block's sum goes to the slab
//   k_probe_occlusion_list<KIND>       k_probe_occlusion's samples over the same units: one unoccluded count per block
//   k_probe_adapt_init                 identity list, zero state
//   k_probe_adapt_resolve_counts       an occlusion pass's counts into totals and moments (irradiance passes are resolved by
//                                      rtw_adaptive.h's k_adapt_resolve_blocks)
//   k_probe_adapt_finish[_occlusion]   the results, the sample counts and the errors
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_probe.h"
#include "rtw_probe_adaptive.h"
#include "rtw_radiance_body.h"

namespace rtwk {

// The body is RTW_RADIANCE_BODY(true)'s with another unit: a lane owns (position, run of blocks) instead of (ray, summation unit),
// and a finished block is stored instead of joining a unit sum in LDS. The regeneration step and the segment are k_probe's,
// statement for statement, so that sample s of probe p is the sample rtw_probe takes.
template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_list(const DScene sc, const ProbeListArgs a) {
    extern __shared__ uint32_t s_stack[];
    RTW_NOISE_SHARED
    const uint32_t tid = threadIdx.x;
    const uint32_t* noise_lds = stage_noise<(TEX != 0)>(sc, s_noise);
    // it holds a barrier: every thread, before the loop; the branch is uniform (a property of the scene)
    TravMem tm{};
    if (sc.use_bvh) tm = trav_mem(sc, s_stack, kBlock, tid);
    const uint32_t lane = tid & 63u;
    // wave-uniform: the job stream
    uint32_t u_next = 0, u_end = 0;
    bool exhausted = false;
    // per lane, the unit: its list position and probe, the current sample and the run's end (both relative to sample0), the open block's sum
    bool need = true;
    uint32_t pos = 0, probe = 0, s_cur = 0, s_end = 0;
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
                const uint32_t u = u_next + rank;  // (< n_units)
                const uint32_t run = fastdiv(u, a.divn_m, a.divn_s1, a.divn_s2);
                pos = u - run * a.n;  // (< n)
                probe = a.list[1u + pos];
                const uint32_t b0 = run * a.run_blocks;  // (< n_blocks: run < runs = ceil(n_blocks / run_blocks))
                s_cur = a.s_from + b0 * kSumBlock;
                s_end = a.s_from + min(b0 + a.run_blocks, a.n_blocks) * kSumBlock;
                bsum = V(0.f, 0.f, 0.f);
                need = false;
                alive = false;
            }
            u_next += min((uint32_t)__popcll(need_mask), avail);
            need_mask = __ballot(need);
        }
        if (__ballot(!need) == 0ull) break;
        const bool busy = !need;
        const uint32_t key = a.key0 + probe, sample = a.sample0 + s_cur;
        const uint32_t seed = a.seed;
        Rng<KIND> g;
        if (busy && !alive) {  // regeneration: the next sample of this lane's run starts at the probe
            const float4 r0 = a.probes[2 * (size_t)probe], r1 = a.probes[2 * (size_t)probe + 1];  // two 16-byte loads
            o = V(r0.x, r0.y, r0.z); d = V(r0.w, r1.x, r1.y);
            seg_tmin = r1.z; seg_tmax = r1.w;  // the caller's interval bounds the first segment only
            float jitter[2];
            radiance_raygen<KIND, true>(sc, seed, key, sample, g, gt, ray_time, jitter);
            d = probe_direction(d, jitter[0], jitter[1]);
            rng_a = g.a; rng_b = g.b;
            T = V(1.f, 1.f, 1.f); L = V(0.f, 0.f, 0.f);
            nee_prev = 0; depth = 0; alive = true;
        }
        if (busy) g.init(seed, key, sample, rng_a, KIND == RTW_RNG_TEA_LCG ? rng_b : sample);
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
                if ((s_cur % kSumBlock) == 0u) {  // a block is complete (s_from and the run's ends are multiples of 16): its sum is stored
                    const uint32_t b_done = (s_cur - a.s_from) / kSumBlock - 1u;  // (< n_blocks)
                    a.out[(size_t)b_done * a.n + pos] = make_float4(bsum.x, bsum.y, bsum.z, 0.f);
                    bsum = V(0.f, 0.f, 0.f);
                    if (s_cur >= s_end) need = true;
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
    uint32_t* const counts = (uint32_t*)a.out;
    const uint32_t step = gridDim.x * blockDim.x;  // (at most the device's resident lanes: u + step stays below 2^32)
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < a.n_units; u += step) {
        const uint32_t run = fastdiv(u, a.divn_m, a.divn_s1, a.divn_s2);
        const uint32_t pos = u - run * a.n;
        const uint32_t probe = a.list[1u + pos];
        const float4 r0 = a.probes[2 * (size_t)probe], r1 = a.probes[2 * (size_t)probe + 1];
        const v3 o = V(r0.x, r0.y, r0.z), nrm = V(r0.w, r1.x, r1.y);
        const uint32_t key = a.key0 + probe;
        const uint32_t b1 = min(run * a.run_blocks + a.run_blocks, a.n_blocks);
        for (uint32_t b = run * a.run_blocks; b < b1; b++) {
            const uint32_t s0 = a.s_from + b * kSumBlock;
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
            counts[(size_t)b * a.n + pos] = open;
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_probe_adapt_init(uint32_t* __restrict__ list, float4* __restrict__ accum, float4* __restrict__ upart,
                                                             double2* __restrict__ mom, uint32_t* __restrict__ n, float* __restrict__ err,
                                                             uint32_t* __restrict__ total, uint32_t n_probes) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_probes; i += gridDim.x * blockDim.x) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        list[1u + i] = i;
        if (i == 0u) list[0] = n_probes;
        accum[i] = z; upart[i] = z;
        mom[i] = make_double2(0.0, 0.0);
        n[i] = 0u;
        err[i] = 0.f;
        total[i] = 0u;
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

__global__ void __launch_bounds__(kBlock) k_probe_adapt_finish(const float4* __restrict__ accum, const float4* __restrict__ upart,
                                                               const uint32_t* __restrict__ n, const float* __restrict__ err, float4* __restrict__ out,
                                                               int32_t* __restrict__ spp_out, float* __restrict__ err_out, uint32_t n_probes) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_probes; i += gridDim.x * blockDim.x) {
        float4 a = accum[i];
        const float4 u = upart[i];
        a.x += u.x; a.y += u.y; a.z += u.z;
        const float spp = (float)n[i];
        out[i] = make_float4((a.x / spp) * kProbePi, (a.y / spp) * kProbePi, (a.z / spp) * kProbePi, 1.0f);
        if (spp_out) spp_out[i] = (int32_t)n[i];
        if (err_out) err_out[i] = err[i];
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
