// rtw_list_body.h - what k_probe_list (rtw_probe_adaptive.hip) and k_view_list (rtw_view_adaptive.hip) share: ListPass, the launch
// record of one range of one pass, and RTW_LIST_BODY, the one piece of source that is both kernels' body. A lane owns (list position,
// run of whole blocks) instead of RTW_RADIANCE_BODY's (ray, summation unit), and a finished block's sum is stored instead of joining a
// unit sum in LDS; the job queue, the units taken by ballot rank and the flattened segment loop are that body's.
//
// The kernels differ in where an entry's key and seed come from and in the regeneration step alone, and those are the macro's three
// arguments, as text: KEY_ and SEED_, expressions over a and `entry` (the lane's list entry), and REGEN_, the statements that start
// sample `sample` (they set o, d, seg_tmin, seg_tmax, gt, ray_time and leave g where the family's raygen leaves it).
// It is a macro, as RTW_RADIANCE_BODY is (rtw_radiance_body.h), because both function forms moved the kernels' machine code. A function
// template over a source policy (SRC::key / seed / regen<KIND>, as k_paths<KIND, TEX, SRC> takes its source) changed the instruction
// count of all twelve instantiations by one to four in 12 000 to 18 000; the same policy called from a body macro kept the counts
// and renamed some 250 registers per kernel. With key, seed and regeneration pasted as text every instantiation is the parent's,
// instruction for instruction (scripts/isa_compare.py, profiles/adaptive_core_isa.txt).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"

namespace rtwk {

// One pass launch over `n` list positions: position i is entry list[1 + i] of the call (the host hands in the list pointer moved to
// the range's first position). The pass adds n_blocks blocks to each, the samples [s_from, s_from + 16 * n_blocks) counted from the
// call's sample0. The unit of work is (position, run of run_blocks whole blocks), numbered run-major: u -> position = u % n,
// run = u / n, so that neighbouring lanes hold neighbouring positions. n_units = n * runs < 2^31 (rtw_probe_adaptive_plan.h).
// ProbeListArgs and ViewListArgs hold one as member `p`; the host fills it once per range (rtw_hip.hip list_pass).
struct ListPass {
    const uint32_t* list;
    float4* out;                // block sums [block of the pass][position]; k_probe_occlusion_list: uint32 counts, the same index
    uint32_t* queue;            // [0] next job of the launch, zeroed by the host on the launch stream
    unsigned long long* stats;  // kStatRows rows of 8: [0] segments, [1] shadow rays
    uint32_t n, n_blocks, run_blocks, n_units;
    uint32_t job_units, n_jobs;
    uint32_t divn_m, divn_s1, divn_s2;  // exact division by n (magic_div)
    uint32_t s_from;
};
static_assert(sizeof(ListPass) == 72 && alignof(ListPass) == 8, "four pointers and ten words: the kernels' arguments keep their places");
static_assert(offsetof(ListPass, n) == 32 && offsetof(ListPass, s_from) == 68, "ListPass's words follow its pointers, s_from last");

// The kernels' body; sc and a are the kernel's parameters (a.p: the pass; a.sample0, a.max_depth: the call's), KIND and TEX its
// template parameters, SRC_ the source policy.
#define RTW_LIST_BODY(KEY_, SEED_, REGEN_) \
    extern __shared__ uint32_t s_stack[]; \
    RTW_NOISE_SHARED \
    const uint32_t tid = threadIdx.x; \
    const uint32_t* noise_lds = stage_noise<(TEX != 0)>(sc, s_noise); \
    /* it holds a barrier: every thread, before the loop; the branch is uniform (a property of the scene) */ \
    TravMem tm{}; \
    if (sc.use_bvh) tm = trav_mem(sc, s_stack, kBlock, tid); \
    const uint32_t lane = tid & 63u; \
    /* wave-uniform: the job stream */ \
    uint32_t u_next = 0, u_end = 0; \
    bool exhausted = false; \
    /* per lane, the unit: its list position and entry, the current sample and the run's end (both relative to sample0), the open block's sum */ \
    bool need = true; \
    uint32_t pos = 0, entry = 0, s_cur = 0, s_end = 0; \
    v3 bsum = V(0.f, 0.f, 0.f); \
    /* per lane, the path */ \
    bool alive = false; \
    uint32_t depth = 0, rng_a = 0, rng_b = 0, nee_prev = 0; \
    float ray_time = 0.f, gt = 0.f, seg_tmin = 0.f, seg_tmax = 0.f; \
    v3 o = V(0.f, 0.f, 0.f), d = o, T = o, L = o; \
    uint32_t n_seg = 0, n_shadow = 0; \
    for (;;) { \
        unsigned long long need_mask = __ballot(need); \
        while (need_mask != 0ull && !exhausted) { \
            if (u_next >= u_end) {  /* the wave's next job: one returning atomic by one lane */ \
                uint32_t q = 0; \
                if (lane == 0) q = atomicAdd(a.p.queue, 1u); \
                q = __builtin_amdgcn_readfirstlane(q); \
                if (q >= a.p.n_jobs) { exhausted = true; break; } \
                u_next = q * a.p.job_units; \
                u_end = min(u_next + a.p.job_units, a.p.n_units); \
                continue; \
            } \
            const uint32_t avail = u_end - u_next; \
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need_mask, 0u)); \
            if (need && rank < avail) { \
                const uint32_t u = u_next + rank;  /* (< n_units) */ \
                const uint32_t run = fastdiv(u, a.p.divn_m, a.p.divn_s1, a.p.divn_s2); \
                pos = u - run * a.p.n;  /* (< n) */ \
                entry = a.p.list[1u + pos];  /* (< the call's entries: k_adapt_compact lists entries below their count alone) */ \
                const uint32_t b0 = run * a.p.run_blocks;  /* (< n_blocks: run < runs = ceil(n_blocks / run_blocks)) */ \
                s_cur = a.p.s_from + b0 * kSumBlock; \
                s_end = a.p.s_from + min(b0 + a.p.run_blocks, a.p.n_blocks) * kSumBlock; \
                bsum = V(0.f, 0.f, 0.f); \
                need = false; \
                alive = false; \
            } \
            u_next += min((uint32_t)__popcll(need_mask), avail); \
            need_mask = __ballot(need); \
        } \
        if (__ballot(!need) == 0ull) break; \
        const bool busy = !need; \
        const uint32_t key = (KEY_), sample = a.sample0 + s_cur; \
        const uint32_t seed = (SEED_); \
        Rng<KIND> g; \
        if (busy && !alive) {  /* regeneration: the next sample of this lane's run starts where the family's uniform call starts it */ \
            REGEN_ \
            rng_a = g.a; rng_b = g.b; \
            T = V(1.f, 1.f, 1.f); L = V(0.f, 0.f, 0.f); \
            nee_prev = 0; depth = 0; alive = true; \
        } \
        if (busy) g.init(seed, key, sample, rng_a, KIND == RTW_RNG_TEA_LCG ? rng_b : sample); \
        if (busy) { \
            float th; \
            int prim; \
            traverse<Rng<KIND>, false, false>(sc, o, d, seg_tmin, seg_tmax, ray_time, gt, g, tm, th, prim); \
            v3 so, sd, att, radiance; \
            Nee nee; \
            const int ev = shade_a<KIND, TEX>(sc, g, o, d, gt, th, prim, so, sd, att, radiance, nee, noise_lds, nee_prev); \
            n_seg++; \
            if (nee.has) {  /* traceOcclusion, closehit.cu:16-42 */ \
                float st; \
                int sprim; \
                traverse<Rng<KIND>, true, false>(sc, so, nee.dir, nee.tmin, nee.tmax, 0.0f, gt, g, tm, st, sprim); \
                n_shadow++; \
                if (sprim < 0) radiance = vadd(radiance, nee.rad); \
            } \
            alive = shade_b<KIND>(depth, a.max_depth, g, ev, so, sd, att, radiance, o, d, T, L, TEX == 2 && sc.estimator == RTW_EST_MIXTURE); \
            depth++; \
            rng_a = g.a; \
            if (alive) { \
                ray_time = (KIND == RTW_RNG_TEA_LCG || sc.has_motion) ? g.ray_time(depth) : 0.0f; \
                rng_b = g.b; \
                seg_tmin = sc.ray_tmin; seg_tmax = 1.e27f;  /* later segments: the estimator's start distance, as a render */ \
            } else { \
                /* removeNaNs (raygen.cu:17-24), then the block's running sum, in sample order */ \
                bsum = vadd(bsum, V((L.x == L.x) ? L.x : 0.f, (L.y == L.y) ? L.y : 0.f, (L.z == L.z) ? L.z : 0.f)); \
                s_cur++; \
                if ((s_cur % kSumBlock) == 0u) {  /* a block is complete (s_from and the run's ends are multiples of 16): its sum is stored */ \
                    const uint32_t b_done = (s_cur - a.p.s_from) / kSumBlock - 1u;  /* (< n_blocks) */ \
                    a.p.out[(size_t)b_done * a.p.n + pos] = make_float4(bsum.x, bsum.y, bsum.z, 0.f); \
                    bsum = V(0.f, 0.f, 0.f); \
                    if (s_cur >= s_end) need = true; \
                } \
            } \
        } \
    } \
    for (int off = 32; off > 0; off >>= 1) { \
        n_seg += __shfl_down(n_seg, off); \
        n_shadow += __shfl_down(n_shadow, off); \
    } \
    if (lane == 0) { \
        unsigned long long* row = a.p.stats + (size_t)(blockIdx.x & (kStatRows - 1u)) * 8u; \
        if (n_seg) atomicAdd(&row[0], (unsigned long long)n_seg); \
        if (n_shadow) atomicAdd(&row[1], (unsigned long long)n_shadow); \
    }

}  // namespace rtwk
