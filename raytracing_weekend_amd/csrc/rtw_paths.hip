// rtw_paths.hip - the path-record kernel (rtw_paths.h), a translation unit of its own (__graft_entry__.py UNITS).
//
//   k_paths<KIND, TEX, SRC>  samples replayed one by one: the path of sample s of ray (pixel) i is k_radiance's (k_view's) - the
//                            regeneration step is radiance_raygen<> or view_raygen<> of rtw_radiance_body.h, a segment the
//                            statements of RTW_RADIANCE_BODY's segment in their order (traverse<>, shade_a, the inline probe,
//                            shade_b, the ray time) - and instead of joining a sum every segment leaves a 64-byte vertex and
//                            every sample a 32-byte head. Nothing is summed, so there is no queue, no unit and no LDS row: a lane
//                            owns one (ray, sample) pair at a time and strides over the pairs of the launch, in one flattened loop
//                            whose body is one segment (a lane whose path ended starts its next pair at once).
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_paths.h"
#include "rtw_radiance_body.h"

namespace rtwk {

// Regeneration, as the body's: the camera ray of flattened pixel a.v.first + ray from its view record, or the caller's ray, and
// the raygen draws of (key, sample); g is left where raygen<> leaves it
template <int KIND, int SRC>
RTW_DEV void paths_regen(const DScene& sc, const PathsArgs& a, const uint32_t ray, const uint32_t seed, const uint32_t key, const uint32_t sample,
                         Rng<KIND>& g, float& gt, float& ray_time, v3& o, v3& d, float& seg_tmin, float& seg_tmax) {
    if (SRC == kPathsViews) {
        view_raygen<KIND>(sc, a.v, ray, seed, sample, g, gt, ray_time, o, d);
        seg_tmin = sc.ray_tmin; seg_tmax = 1.e27f;  // the estimator's start distance, as a render's camera ray
    } else {
        const float4 r0 = a.v.rays[2 * (size_t)ray], r1 = a.v.rays[2 * (size_t)ray + 1];  // two 16-byte loads
        o = V(r0.x, r0.y, r0.z); d = V(r0.w, r1.x, r1.y);
        seg_tmin = r1.z; seg_tmax = r1.w;  // the caller's interval bounds the first segment only
        radiance_raygen<KIND, false>(sc, seed, key, sample, g, gt, ray_time, nullptr);
    }
}

// The head of pair p: two 16-byte stores. The radiance is the sample after removeNaNs (raygen.cu:17-24) as it joins an empty block
// sum: 0.0f + x
RTW_DEV void paths_head(const PathsArgs& a, const uint32_t p, const v3 L, const uint32_t segments, const float gt, const uint32_t shadows,
                        const uint32_t key, const uint32_t sample) {
    const v3 Ln = vadd(V(0.f, 0.f, 0.f), V((L.x == L.x) ? L.x : 0.f, (L.y == L.y) ? L.y : 0.f, (L.z == L.z) ? L.z : 0.f));
    float4* const head = a.heads + (size_t)p * kPathHeadFloat4;
    head[0] = make_float4(Ln.x, Ln.y, Ln.z, __int_as_float((int)segments));
    head[1] = make_float4(gt, __int_as_float((int)shadows), __uint_as_float(key), __uint_as_float(sample));
}

template <int KIND, int TEX, int SRC>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_paths(const DScene sc, const PathsArgs a) {
    extern __shared__ uint32_t s_stack[];
    RTW_NOISE_SHARED
    const uint32_t tid = threadIdx.x;
    // both hold a barrier: every thread, before the loop and before any exit; the branch is uniform (a property of the scene)
    const uint32_t* noise_lds = stage_noise<(TEX != 0)>(sc, s_noise);
    TravMem tm{};
    if (sc.use_bvh) tm = trav_mem(sc, s_stack, kBlock, tid);
    const uint32_t step = gridDim.x * blockDim.x;
    // per lane, the pair it owns (n_pairs <= 2^31 - 1 and step < 2^31: p + step does not wrap) ...
    uint32_t p = blockIdx.x * blockDim.x + tid;
    bool busy = p < a.n_pairs;
    if (a.v.max_depth == 0u) {  // no segment is traced: a head of zeros per pair, with the sample's gather time, key and index
        for (; p < a.n_pairs; p += step) {
            const uint32_t ray = fastdiv(p, a.divs_m, a.divs_s1, a.divs_s2);
            const uint32_t sample = a.v.sample0 + (p - ray * a.v.spp);
            const uint32_t key = SRC == kPathsViews ? view_key(a.v, ray) : a.v.key0 + ray;
            const uint32_t seed = SRC == kPathsViews ? view_seed(a.v, ray) : a.v.seed;
            Rng<KIND> g;
            float gt, ray_time, seg_tmin, seg_tmax;
            v3 o, d;
            paths_regen<KIND, SRC>(sc, a, ray, seed, key, sample, g, gt, ray_time, o, d, seg_tmin, seg_tmax);
            paths_head(a, p, V(0.f, 0.f, 0.f), 0u, gt, 0u, key, sample);
        }
        return;
    }
    // ... and its path. One flattened loop whose body is one segment, as the body's: a lane whose path ended starts its next pair
    // in the same iteration, so a wave does not wait for its longest path.
    bool alive = false;
    uint32_t depth = 0, shadows = 0, rng_a = 0, rng_b = 0, nee_prev = 0;
    float ray_time = 0.f, gt = 0.f, seg_tmin = 0.f, seg_tmax = 0.f;
    v3 o = V(0.f, 0.f, 0.f), d = o, T = o, L = o;
    uint32_t n_seg = 0, n_shadow = 0;
    while (__ballot(busy) != 0ull) {
        if (busy) {
            const uint32_t ray = fastdiv(p, a.divs_m, a.divs_s1, a.divs_s2);
            const uint32_t sample = a.v.sample0 + (p - ray * a.v.spp);
            const uint32_t key = SRC == kPathsViews ? view_key(a.v, ray) : a.v.key0 + ray;
            const uint32_t seed = SRC == kPathsViews ? view_seed(a.v, ray) : a.v.seed;
            Rng<KIND> g;
            if (!alive) {
                paths_regen<KIND, SRC>(sc, a, ray, seed, key, sample, g, gt, ray_time, o, d, seg_tmin, seg_tmax);
                rng_a = g.a; rng_b = g.b;
                T = V(1.f, 1.f, 1.f); L = V(0.f, 0.f, 0.f);
                nee_prev = 0; depth = 0; shadows = 0; alive = true;
            }
            g.init(seed, key, sample, rng_a, KIND == RTW_RNG_TEA_LCG ? rng_b : sample);
            float th;
            int prim;
            traverse<Rng<KIND>, false, false>(sc, o, d, seg_tmin, seg_tmax, ray_time, gt, g, tm, th, prim);
            v3 so, sd, att, radiance;
            Nee nee;
            const int ev = shade_a<KIND, TEX>(sc, g, o, d, gt, th, prim, so, sd, att, radiance, nee, noise_lds, nee_prev);
            uint32_t flags = (uint32_t)ev;
            if (nee.has) {  // traceOcclusion, closehit.cu:16-42
                float st;
                int sprim;
                traverse<Rng<KIND>, true, false>(sc, so, nee.dir, nee.tmin, nee.tmax, 0.0f, gt, g, tm, st, sprim);
                shadows++;
                flags |= RTW_PATH_LIGHT_SAMPLED;
                if (sprim < 0) { radiance = vadd(radiance, nee.rad); flags |= RTW_PATH_LIGHT_ADDED; }
            }
            if (depth < a.max_records) {  // the vertex: four 16-byte stores, from what the segment holds before shade_b moves on
                const v3 c = vmul(radiance, T);
                float4* const rec = a.vertices + ((size_t)p * a.max_records + depth) * kPathVertexFloat4;
                rec[0] = make_float4(o.x, o.y, o.z, prim < 0 ? seg_tmax : th);
                rec[1] = make_float4(d.x, d.y, d.z, __int_as_float(prim));
                rec[2] = make_float4(c.x, c.y, c.z, __uint_as_float(flags));
                rec[3] = make_float4(T.x, T.y, T.z, ray_time);
            }
            alive = shade_b<KIND>(depth, a.v.max_depth, g, ev, so, sd, att, radiance, o, d, T, L, TEX == 2 && sc.estimator == RTW_EST_MIXTURE);
            depth++;
            rng_a = g.a;
            if (alive) {
                ray_time = (KIND == RTW_RNG_TEA_LCG || sc.has_motion) ? g.ray_time(depth) : 0.0f;
                rng_b = g.b;
                seg_tmin = sc.ray_tmin; seg_tmax = 1.e27f;  // later segments: the estimator's start distance, as a render
            } else {  // the path ended: its head, and the lane's next pair
                paths_head(a, p, L, depth, gt, shadows, key, sample);
                n_seg += depth;
                n_shadow += shadows;
                p += step;
                busy = p < a.n_pairs;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        n_seg += __shfl_down(n_seg, off);
        n_shadow += __shfl_down(n_shadow, off);
    }
    if ((tid & 63u) == 0) {
        unsigned long long* row = a.v.stats + (size_t)(blockIdx.x & (kStatRows - 1u)) * 8u;
        if (n_seg) atomicAdd(&row[0], (unsigned long long)n_seg);
        if (n_shadow) atomicAdd(&row[1], (unsigned long long)n_shadow);
    }
}

#define RTW_INST_S(R_, S_) \
    template __global__ void k_paths<R_, 0, S_>(const DScene, const PathsArgs); \
    template __global__ void k_paths<R_, 1, S_>(const DScene, const PathsArgs); \
    template __global__ void k_paths<R_, 2, S_>(const DScene, const PathsArgs);
#define RTW_INST(R_) RTW_INST_S(R_, kPathsRays) RTW_INST_S(R_, kPathsViews)
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST
#undef RTW_INST_S

}  // namespace rtwk
