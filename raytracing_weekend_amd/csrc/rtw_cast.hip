// rtw_cast.hip - the ray-query kernel (rtw_cast.h), a translation unit of its own (__graft_entry__.py UNITS).
//
//   k_cast<ANY_HIT, ATTR>  the caller's rays through traverse<NoRng, ANY_HIT, true> (the candidate lists of small scenes or the
//                          4-wide tree, whichever the scene was uploaded with; volumes skipped), then - ATTR only - the closest-hit
//                          code's hit record, shading normal and texture coordinates of the hit
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_cast.h"

namespace rtwk {

template <bool ANY_HIT, bool ATTR>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_cast(const DScene sc, const CastArgs a) {
    static_assert(!(ANY_HIT && ATTR), "an occlusion query has no hit to describe");
    extern __shared__ uint32_t s_stack[];
    // it holds a barrier: every thread, before the loop and before any exit (a thread without a ray still stages its share of the
    // tree); the branch is uniform (a property of the scene)
    TravMem tm{};
    if (sc.use_bvh) tm = trav_mem(sc, s_stack, kBlock, threadIdx.x);
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += step) {
        const float4 r0 = a.rays[2 * i], r1 = a.rays[2 * i + 1];  // two 16-byte loads, consecutive lanes 32 bytes apart
        const v3 o = V(r0.x, r0.y, r0.z), d = V(r0.w, r1.x, r1.y);
        const float rt = a.ray_time ? a.ray_time[i] : 0.f;
        const float gt = a.gather_time ? a.gather_time[i] : 0.f;
        NoRng g;
        float t;
        int prim;
        traverse<NoRng, ANY_HIT, true>(sc, o, d, r1.z, r1.w, rt, gt, g, tm, t, prim);
        // an occlusion query returns tmax (the tree walk leaves the accepted candidate's t in `t`, the list walk tmax: neither is a
        // closest hit, and the bits must not depend on the walk)
        if (a.t) a.t[i] = ANY_HIT ? r1.w : t;
        if (a.prim) a.prim[i] = prim;
        if (ATTR) {
            int material = -1;
            float4 nrm = make_float4(0.f, 0.f, 0.f, 0.f);
            float2 uv = make_float2(0.f, 0.f);
            if (prim >= 0) {
                // shade_a's hit record and shading normal, texture_eval's coordinates
                const HitRec hr = load_hitrec(sc, prim);
                v3 hp, n;
                hit_attributes(sc, hr, prim, o, d, t, gt, hp, n);
                nrm = make_float4(n.x, n.y, n.z, dot3(n, d) < 0.0f ? 1.0f : 0.0f);  // the shading code's front-face rule
                if (a.uv) hit_uv(sc, hr, prim, o, d, t, rt, n, uv.x, uv.y);
                if (a.material) material = sc.prims[prim].material;
            }
            if (a.material) a.material[i] = material;
            if (a.normal) a.normal[i] = nrm;
            if (a.uv) a.uv[i] = uv;
        }
    }
}

template __global__ void k_cast<false, false>(const DScene, const CastArgs);
template __global__ void k_cast<false, true>(const DScene, const CastArgs);
template __global__ void k_cast<true, false>(const DScene, const CastArgs);

}  // namespace rtwk
