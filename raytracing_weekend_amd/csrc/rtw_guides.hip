// rtw_guides.hip - the guide kernels (rtw_guides.h), a translation unit of their own (__graft_entry__.py UNITS).
//
//   k_guides         first-hit albedo / normal means, depth and primitive of the first sample: the beauty's own camera rays
//                    (raygen<>), closest hit through traverse<> with volumes skipped, the closest-hit code's hit record,
//                    shading normal and texture evaluation
//   k_atrous_guided  k_atrous with albedo and normal edge-stopping terms
//   k_atrous_guided_views  k_atrous_guided over the frames of a batch of views, every tap inside its pixel's frame
#include <hip/hip_runtime.h>

#define RTW_TEMPLATES_ONLY  // (the plain kernels of rtw_kernels.h belong to rtw_hip.hip)
#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_guides.h"

namespace rtwk {

// The camera path of sample `sample` of pixel (x, y) through raygen<> (the generator it seeds is not needed after it)
RTW_DEV void guide_ray(const KArgs& A, const int rng_kind, const uint32_t x, const uint32_t y, const uint32_t sample, Path& p) {
    if (rng_kind == RTW_RNG_TEA_LCG) {
        Rng<RTW_RNG_TEA_LCG> g;
        raygen<RTW_RNG_TEA_LCG>(A, x, y, sample, 0u, p, g);
    } else {
        Rng<RTW_RNG_PHILOX> g;
        raygen<RTW_RNG_PHILOX>(A, x, y, sample, 0u, p, g);
    }
}

__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_guides(const KArgs A, const GuideOut G) {
    extern __shared__ uint32_t s_stack[];
    __shared__ uint32_t s_noise[1536];
    // both hold a barrier: every thread, before any exit; the branch is uniform (a property of the scene)
    const uint32_t* noise_lds = stage_noise<true>(A.sc, s_noise);
    TravMem tm{};
    if (A.sc.use_bvh) tm = trav_mem(A.sc, s_stack, A.stack_stride, threadIdx.x);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < A.npix; i += gridDim.x * blockDim.x) {
        const uint32_t yl = i / A.width;
        const uint32_t x = i - yl * A.width;
        const uint32_t y = A.row0 + yl * A.row_stride;
        // sums in the order of rtw.h's summation contract (k_resolve / k_finish): samples inside blocks (b), blocks inside
        // units (u), units (a); index 0 albedo, 1 normal
        v3 a0 = V(0.f, 0.f, 0.f), u0 = a0, b0 = a0, a1 = a0, u1 = a0, b1 = a0;
        uint32_t hits = 0;
        float depth = __builtin_inff();
        int first_prim = -1;
        for (uint32_t s = 0; s < A.spp; s++) {
            if (s != 0u && (s % kSumBlock) == 0u) {
                u0 = vadd(u0, b0); u1 = vadd(u1, b1);
                b0 = V(0.f, 0.f, 0.f); b1 = b0;
                if ((s % (kSumBlock * kSumUnitBlocks)) == 0u) {
                    a0 = vadd(a0, u0); a1 = vadd(a1, u1);
                    u0 = V(0.f, 0.f, 0.f); u1 = u0;
                }
            }
            Path p;
            guide_ray(A, G.rng_kind, x, y, A.sample0 + s, p);
            const float gt = gather_time_of(A, p.gk);
            NoRng ng;
            float th;
            int prim;
            traverse<NoRng, false, true>(A.sc, p.o, p.d, A.sc.ray_tmin, 1.e27f, p.ray_time, gt, ng, tm, th, prim);
            v3 alb = V(0.f, 0.f, 0.f), nrm = alb;
            if (prim >= 0) {
                // shade_a's hit record, shading normal and texture value
                const HitRec hr = load_hitrec(A.sc, prim);
                v3 hp;
                hit_attributes(A.sc, hr, prim, p.o, p.d, th, gt, hp, nrm);
                const int mtype = hr.mat_type;
                if (mtype == RTW_MAT_DIELECTRIC) {
                    alb = V(1.f, 1.f, 1.f);
                } else if (mtype == RTW_MAT_NORMAL) {
                    alb = vfma(nrm, 0.5f, V(0.5f, 0.5f, 0.5f));
                } else {
                    v3 tex = V(hr.r, hr.g, hr.b);
                    if (hr.tex_dyn >= 0) tex = texture_eval(A.sc, hr, prim, p.o, p.d, th, 0.0f, hp, nrm, noise_lds);
                    if (mtype == RTW_MAT_DIFFUSE_LIGHT) {  // emits on the front face only (diffuseLight.cu:48-69)
                        tex = dot3(nrm, p.d) < 0.0f ? tex : V(0.f, 0.f, 0.f);
                        tex = V(__builtin_fminf(__builtin_fmaxf(tex.x, 0.f), 1.f), __builtin_fminf(__builtin_fmaxf(tex.y, 0.f), 1.f),
                                __builtin_fminf(__builtin_fmaxf(tex.z, 0.f), 1.f));
                    }
                    alb = tex;
                }
                hits++;
            }
            if (s == 0u) {
                first_prim = prim;
                if (prim >= 0) depth = th * length3(p.d);
            }
            b0 = vadd(b0, alb); b1 = vadd(b1, nrm);
        }
        u0 = vadd(u0, b0); u1 = vadd(u1, b1);
        a0 = vadd(a0, u0); a1 = vadd(a1, u1);
        const float spp = (float)A.spp, cover = (float)hits / spp;
        if (G.albedo) G.albedo[i] = make_float4(a0.x / spp, a0.y / spp, a0.z / spp, cover);
        if (G.normal) G.normal[i] = make_float4(a1.x / spp, a1.y / spp, a1.z / spp, cover);
        if (G.depth) G.depth[i] = depth;
        if (G.prim) G.prim[i] = first_prim;
    }
}

// k_atrous (rtw_kernels.h) with two more divisors; their operands are formed like its colour term. Kept in k_atrous's operation
// order: with constant guides both divisors are 1.0f exactly and the result is k_atrous's, bit for bit.
__global__ void __launch_bounds__(kBlock) k_atrous_guided(const float4* __restrict__ in, const float4* __restrict__ alb, const float4* __restrict__ nrm,
                                                          float4* __restrict__ out, int width, int height, int step, float inv_sigma2,
                                                          float inv_sigma_a2, float inv_sigma_n2) {
    const int n = width * height;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int y = i / width, x = i - y * width;
        const float4 c = in[i], ca = alb[i], cn = nrm[i];
        const float kern[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
        for (int dy = -2; dy <= 2; dy++) {
            int yy = y + dy * step;
            yy = yy < 0 ? 0 : (yy > height - 1 ? height - 1 : yy);
            for (int dx = -2; dx <= 2; dx++) {
                int xx = x + dx * step;
                xx = xx < 0 ? 0 : (xx > width - 1 ? width - 1 : xx);
                const int j = yy * width + xx;
                const float4 q = in[j], qa = alb[j], qn = nrm[j];
                const float dr = c.x - q.x, dg = c.y - q.y, db = c.z - q.z;
                const float d2 = (dr * dr + dg * dg) + db * db;
                const float ar = ca.x - qa.x, ag = ca.y - qa.y, ab = ca.z - qa.z;
                const float a2 = (ar * ar + ag * ag) + ab * ab;
                const float nx = cn.x - qn.x, ny = cn.y - qn.y, nz = cn.z - qn.z;
                const float n2 = (nx * nx + ny * ny) + nz * nz;
                float w = (kern[dy + 2] * kern[dx + 2]) / (1.0f + d2 * inv_sigma2);
                w = w / (1.0f + a2 * inv_sigma_a2);
                w = w / (1.0f + n2 * inv_sigma_n2);
                sr = sr + w * q.x; sg = sg + w * q.y; sb = sb + w * q.z; sw = sw + w;
            }
        }
        out[i] = make_float4(sr / sw, sg / sw, sb / sw, c.w);
    }
}

// k_atrous_guided over the flattened index of n_views frames: the frame by exact division, the taps clamped and addressed inside
// it, the operations and their order unchanged (frame v of the result is k_atrous_guided's of frame v alone, bit for bit).
// n < 2^31 and the grid is at most n / kBlock blocks: i does not wrap.
__global__ void __launch_bounds__(kBlock) k_atrous_guided_views(const float4* __restrict__ in, const float4* __restrict__ alb,
                                                                const float4* __restrict__ nrm, float4* __restrict__ out, uint32_t n, int width,
                                                                int height, uint32_t divf_m, uint32_t divf_s1, uint32_t divf_s2, int step,
                                                                float inv_sigma2, float inv_sigma_a2, float inv_sigma_n2) {
    const uint32_t frame = (uint32_t)width * (uint32_t)height;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t view = fastdiv(i, divf_m, divf_s1, divf_s2);
        const uint32_t base = view * frame;
        const int p = (int)(i - base);
        const int y = p / width, x = p - y * width;
        const float4 c = in[i], ca = alb[i], cn = nrm[i];
        const float kern[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
        for (int dy = -2; dy <= 2; dy++) {
            int yy = y + dy * step;
            yy = yy < 0 ? 0 : (yy > height - 1 ? height - 1 : yy);
            for (int dx = -2; dx <= 2; dx++) {
                int xx = x + dx * step;
                xx = xx < 0 ? 0 : (xx > width - 1 ? width - 1 : xx);
                const uint32_t j = base + (uint32_t)(yy * width + xx);
                const float4 q = in[j], qa = alb[j], qn = nrm[j];
                const float dr = c.x - q.x, dg = c.y - q.y, db = c.z - q.z;
                const float d2 = (dr * dr + dg * dg) + db * db;
                const float ar = ca.x - qa.x, ag = ca.y - qa.y, ab = ca.z - qa.z;
                const float a2 = (ar * ar + ag * ag) + ab * ab;
                const float nx = cn.x - qn.x, ny = cn.y - qn.y, nz = cn.z - qn.z;
                const float n2 = (nx * nx + ny * ny) + nz * nz;
                float w = (kern[dy + 2] * kern[dx + 2]) / (1.0f + d2 * inv_sigma2);
                w = w / (1.0f + a2 * inv_sigma_a2);
                w = w / (1.0f + n2 * inv_sigma_n2);
                sr = sr + w * q.x; sg = sg + w * q.y; sb = sb + w * q.z; sw = sw + w;
            }
        }
        out[i] = make_float4(sr / sw, sg / sw, sb / sw, c.w);
    }
}

}  // namespace rtwk
