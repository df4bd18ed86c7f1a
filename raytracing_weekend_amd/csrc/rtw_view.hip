// rtw_view.hip - the view kernel (rtw_view.h), a translation unit of its own (__graft_entry__.py UNITS).
//
//   k_view<KIND, TEX>  frames from the caller's cameras: k_radiance's loop (rtw_radiance_body.h: the same job queue, units, path
//                      segments - traverse<>, shade_a, shade_b - and summation order) whose "ray" is a pixel of the flattened
//                      (view, y, x) index and whose regeneration step is raygen<>'s camera, read from the pixel's view record:
//                      the jitter and lens draws that k_radiance drops are used. Frames beyond 128 spp resolve through
//                      k_radiance_resolve.
//   k_view_guides      the first-hit guides of the same pixels (rtw.h rtw_views_guides): k_guides' loop (rtw_guides.hip) whose camera
//                      path is view_raygen<>'s, from the pixel's view record
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_view.h"
#include "rtw_radiance_body.h"

namespace rtwk {

template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_view(const DScene sc, const ViewArgs a) {
    RTW_RADIANCE_BODY(3)
}

// The camera path of sample `sample` of flattened pixel `ray` through view_raygen<> (the generator it seeds is not needed after
// it): the generator is chosen per launch, as k_guides' guide_ray chooses it per call
RTW_DEV void view_guide_ray(const DScene& sc, const ViewArgs& a, const int rng_kind, const uint32_t ray, const uint32_t seed, const uint32_t sample,
                            float& gt, float& ray_time, v3& o, v3& d) {
    if (rng_kind == RTW_RNG_TEA_LCG) {
        Rng<RTW_RNG_TEA_LCG> g;
        view_raygen<RTW_RNG_TEA_LCG>(sc, a, ray, seed, sample, g, gt, ray_time, o, d);
    } else {
        Rng<RTW_RNG_PHILOX> g;
        view_raygen<RTW_RNG_PHILOX>(sc, a, ray, seed, sample, g, gt, ray_time, o, d);
    }
}

// k_guides' loop (rtw_guides.hip) over the flattened pixels [a.first, a.first + a.n): pixel a.first + i of the call is entry i of
// every buffer of G. After the camera path the statements are k_guides', in its order.
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_view_guides(const DScene sc, const ViewArgs a, const GuideOut G) {
    extern __shared__ uint32_t s_stack[];
    __shared__ uint32_t s_noise[1536];
    // both hold a barrier: every thread, before any exit; the branch is uniform (a property of the scene)
    const uint32_t* noise_lds = stage_noise<true>(sc, s_noise);
    TravMem tm{};
    if (sc.use_bvh) tm = trav_mem(sc, s_stack, kBlock, threadIdx.x);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
        const uint32_t seed = view_seed(a, i);
        // sums in the order of rtw.h's summation contract: samples inside blocks (b), blocks inside units (u), units (a); index 0
        // albedo, 1 normal
        v3 a0 = V(0.f, 0.f, 0.f), u0 = a0, b0 = a0, a1 = a0, u1 = a0, b1 = a0;
        uint32_t hits = 0;
        float depth = __builtin_inff();
        int first_prim = -1;
        for (uint32_t s = 0; s < a.spp; s++) {
            if (s != 0u && (s % kSumBlock) == 0u) {
                u0 = vadd(u0, b0); u1 = vadd(u1, b1);
                b0 = V(0.f, 0.f, 0.f); b1 = b0;
                if ((s % (kSumBlock * kSumUnitBlocks)) == 0u) {
                    a0 = vadd(a0, u0); a1 = vadd(a1, u1);
                    u0 = V(0.f, 0.f, 0.f); u1 = u0;
                }
            }
            float gt, ray_time;
            v3 o, d;
            // The record does not change over the samples, and left to itself the compiler loads its 28 words once per pixel and
            // keeps them across the traversal: 136 VGPRs, 8 of them in scratch. The pixel index is made opaque per sample, so that
            // the record is read again (from the cache, as in k_view) and nothing of the camera lives across the walk.
            uint32_t ray = i;
            asm volatile("" : "+v"(ray));
            view_guide_ray(sc, a, G.rng_kind, ray, seed, a.sample0 + s, gt, ray_time, o, d);
            NoRng ng;
            float th;
            int prim;
            traverse<NoRng, false, true>(sc, o, d, sc.ray_tmin, 1.e27f, ray_time, gt, ng, tm, th, prim);
            v3 alb = V(0.f, 0.f, 0.f), nrm = alb;
            if (prim >= 0) {
                const HitRec hr = load_hitrec(sc, prim);
                v3 hp;
                hit_attributes(sc, hr, prim, o, d, th, gt, hp, nrm);
                const int mtype = hr.mat_type;
                if (mtype == RTW_MAT_DIELECTRIC) {
                    alb = V(1.f, 1.f, 1.f);
                } else if (mtype == RTW_MAT_NORMAL) {
                    alb = vfma(nrm, 0.5f, V(0.5f, 0.5f, 0.5f));
                } else {
                    v3 tex = V(hr.r, hr.g, hr.b);
                    if (hr.tex_dyn >= 0) tex = texture_eval(sc, hr, prim, o, d, th, 0.0f, hp, nrm, noise_lds);
                    if (mtype == RTW_MAT_DIFFUSE_LIGHT) {  // emits on the front face only
                        tex = dot3(nrm, d) < 0.0f ? tex : V(0.f, 0.f, 0.f);
                        tex = V(__builtin_fminf(__builtin_fmaxf(tex.x, 0.f), 1.f), __builtin_fminf(__builtin_fmaxf(tex.y, 0.f), 1.f),
                                __builtin_fminf(__builtin_fmaxf(tex.z, 0.f), 1.f));
                    }
                    alb = tex;
                }
                hits++;
            }
            if (s == 0u) {
                first_prim = prim;
                if (prim >= 0) depth = th * length3(d);
            }
            b0 = vadd(b0, alb); b1 = vadd(b1, nrm);
        }
        u0 = vadd(u0, b0); u1 = vadd(u1, b1);
        a0 = vadd(a0, u0); a1 = vadd(a1, u1);
        const float spp = (float)a.spp, cover = (float)hits / spp;
        if (G.albedo) G.albedo[i] = make_float4(a0.x / spp, a0.y / spp, a0.z / spp, cover);
        if (G.normal) G.normal[i] = make_float4(a1.x / spp, a1.y / spp, a1.z / spp, cover);
        if (G.depth) G.depth[i] = depth;
        if (G.prim) G.prim[i] = first_prim;
    }
}

#define RTW_INST(R_) \
    template __global__ void k_view<R_, 0>(const DScene, const ViewArgs); \
    template __global__ void k_view<R_, 1>(const DScene, const ViewArgs); \
    template __global__ void k_view<R_, 2>(const DScene, const ViewArgs);
RTW_INST(RTW_RNG_PHILOX)
RTW_INST(RTW_RNG_TEA_LCG)
#undef RTW_INST

}  // namespace rtwk
