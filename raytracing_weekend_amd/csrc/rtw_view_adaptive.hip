// rtw_view_adaptive.hip - the kernels of rtw_views_adaptive (rtw_view_adaptive.h), a translation unit of its own (__graft_entry__.py UNITS).
//
//   k_view_list<KIND, TEX>   k_view's samples for the pixels of an active list, blocks [n_from / 16, n_to / 16) of each: the unit of
//                            work is (list position, run of R whole blocks), every block's sum goes to the slab
//   k_view_adapt_decide      k_adapt_decide's stop rule with the 3x3 neighbourhood clamped to the pixel's own view
//   k_view_adapt_finish      the frames, the sample counts and the errors
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_view.h"
#include "rtw_view_adaptive.h"
#include "rtw_radiance_body.h"
#include "rtw_adaptive_stat.h"

namespace rtwk {

// The body is k_probe_list's (rtw_probe_adaptive.hip) - a lane owns (position, run of blocks), a finished block is stored - with
// k_view's regeneration step and segment, statement for statement, so that sample s of a pixel is the sample rtw_views takes. The
// list entry is a flattened pixel; its key and its view's seed are taken from it again in every iteration, as k_view takes them,
// and nothing of the camera lives across the segment loop: beside the path, a lane keeps its position and its pixel.
template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_view_list(const DScene sc, const ViewListArgs a) {
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
    // per lane, the unit: its list position and pixel, the current sample and the run's end (both relative to sample0), the open block's sum
    bool need = true;
    uint32_t pos = 0, pixel = 0, s_cur = 0, s_end = 0;
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
                pixel = a.list[1u + pos];  // (< the call's pixels: k_adapt_compact lists pixels below npix alone)
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
        const uint32_t key = view_key(a.v, pixel), sample = a.sample0 + s_cur;
        const uint32_t seed = view_seed(a.v, pixel);
        Rng<KIND> g;
        if (busy && !alive) {  // regeneration: the next sample of this lane's pixel starts at its view's camera
            view_raygen<KIND>(sc, a.v, pixel, seed, sample, g, gt, ray_time, o, d);
            seg_tmin = sc.ray_tmin; seg_tmax = 1.e27f;  // the estimator's start distance, as a render's camera ray
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

__global__ void __launch_bounds__(kBlock) k_view_adapt_decide(const double2* __restrict__ mom, const uint32_t* __restrict__ n, float* __restrict__ err,
                                                              unsigned long long* __restrict__ masks, const ViewDecideArgs a) {
    const uint32_t n_waves = (a.npix + 63u) / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t w = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6); w < n_waves; w += gridDim.x * (kBlock / 64u)) {
        const uint32_t p = w * 64u + lane;
        bool keep = false;
        if (p < a.npix && n[p] == 0u) {
            const float e = adapt_err(mom[p], a.B);
            err[p] = e;
            bool stop = a.at_cap != 0u || e < a.threshold;
            if (stop && a.at_cap == 0u && a.dilate != 0u) {
                const uint32_t view = fastdiv(p, a.divf_m, a.divf_s1, a.divf_s2);
                const uint32_t base = view * (a.width * a.height), in = p - base;  // the view's first pixel, p's index inside its frame
                const int y = (int)fastdiv(in, a.divw_m, a.divw_s1, a.divw_s2), x = (int)(in - (uint32_t)y * a.width);
                for (int dy = -1; dy <= 1; dy++) {
                    const int yy = min(max(y + dy, 0), (int)a.height - 1);
                    for (int dx = -1; dx <= 1; dx++) {
                        const int xx = min(max(x + dx, 0), (int)a.width - 1);
                        const uint32_t q = base + (uint32_t)yy * a.width + (uint32_t)xx;  // (inside view's frame: < npix)
                        if (q != p && n[q] == 0u && !(adapt_err(mom[q], a.B) < a.threshold)) stop = false;
                    }
                }
            }
            keep = !stop;
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0u) masks[w] = mask;
    }
}

__global__ void __launch_bounds__(kBlock) k_view_adapt_finish(const float4* __restrict__ accum, const float4* __restrict__ upart,
                                                              const uint32_t* __restrict__ n, const float* __restrict__ err, float4* __restrict__ out,
                                                              int32_t* __restrict__ spp_out, float* __restrict__ err_out, uint32_t npix) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        float4 a = accum[i];
        const float4 u = upart[i];
        a.x += u.x; a.y += u.y; a.z += u.z;
        const float spp = (float)n[i];
        out[i] = make_float4(a.x / spp, a.y / spp, a.z / spp, 1.0f);
        if (spp_out) spp_out[i] = (int32_t)n[i];
        if (err_out) err_out[i] = err[i];
    }
}

#define RTW_INST(R_) \
    template __global__ void k_view_list<R_, 0>(const DScene, const ViewListArgs); \
    template __global__ void k_view_list<R_, 1>(const DScene, const ViewListArgs); \
    template __global__ void k_view_list<R_, 2>(const DScene, const ViewListArgs);
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST

}  // namespace rtwk
