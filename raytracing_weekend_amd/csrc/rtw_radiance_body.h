// rtw_radiance_body.h - what k_radiance (rtw_radiance.hip) and k_probe (rtw_probe.hip) share: the raygen draws, a probe's direction,
// and - RTW_RADIANCE_BODY - the text of the kernels' body: the job queue, units taken by ballot rank, one flattened loop whose body is
// one path segment, the sums in rtw.h's blocks and units. The two kernels differ in the regeneration step alone (PROBE_: the first
// direction is drawn from the sample's own raygen uniforms, and the mean is multiplied by pi); everything else is one piece of
// source. It is a macro and not a function so that k_radiance's text, and with it its generated code, stays what it was before
// k_probe existed (as a function inlined into both kernels the same statements were scheduled differently: a few lines of ISA in
// 15 000 moved; profiles/probe_rates.txt).
// A third value of the macro's argument, 2, makes k_probe_sh's body (rtw_probe_sh.hip): the first direction is uniform over the sphere
// and every sample adds Y_j(d) * L to nine coefficients. Every statement of that kernel alone stands under a compile-time
// (int)(PROBE_) == 2, so the two older kernels' generated code does not move.
// A fourth value, 3, makes k_view's body (rtw_view.hip): the lane's "ray" is a pixel of the flattened (view, y, x) index and the
// regeneration step is raygen<>'s camera, read from the pixel's view record. The stream key is the pixel's own (width * y + x) and
// the seed the view's; both are taken from the pixel index again in every iteration and nothing of the camera lives across the
// segment loop. Every statement of that kernel alone stands under a compile-time (int)(PROBE_) == 3.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rtw.h"
#include "rtw_device.h"
#include "rtw_kernels.h"
#include "rtw_radiance.h"
#include "rtw_probe.h"
#include "rtw_probe_sh.h"
#include "rtw_view.h"

namespace rtwk {

// raygen<>'s draws for a perspective camera path of pixel `key`, sample `sample`, without the camera: the jitter and lens draws
// are consumed (Philox: words 0-3 of block (key, sample, 0, 0); TEA+LCG: four lcg_rnd), the generator is left where raygen<> leaves
// it, gt is the gather time and ray_time the first segment's. KEEP: jitter[0 .. 1] receive the first two of those draws, the pixel
// jitter, which k_probe turns into its direction; k_radiance drops them (KEEP = false: jitter is not touched)
template <int KIND, bool KEEP>
RTW_DEV void radiance_raygen(const DScene& sc, const uint32_t seed, const uint32_t key, const uint32_t sample, Rng<KIND>& g, float& gt, float& ray_time,
                             float* jitter) {
    float r4;
    if (KIND == RTW_RNG_TEA_LCG) {
        uint32_t s = tea<64>(key, sample);
        if (KEEP) { jitter[0] = lcg_rnd(s); jitter[1] = lcg_rnd(s); (void)lcg_rnd(s); (void)lcg_rnd(s); }
        else { (void)lcg_rnd(s); (void)lcg_rnd(s); (void)lcg_rnd(s); (void)lcg_rnd(s); }
        g.init(seed, key, sample, s, s);
        r4 = lcg_rnd(s);
    } else {
        uint32_t o[4];
        philox4x32_10(key, sample, 0u, 0u, seed, 0u, o);
        if (KEEP) { jitter[0] = u24(o[0]); jitter[1] = u24(o[1]); }
        r4 = (float)(((o[0] & 0xffu) << 16) | ((o[1] & 0xffu) << 8) | (o[2] & 0xffu)) * (1.0f / 16777216.0f);
        g.init(seed, key, sample, 0u, sample);
    }
    gt = fma_(r4, sc.cam.time1 - sc.cam.time0, sc.cam.time0);  // (r4 = k / 2^24: gather_time_of's value for gk = k)
    ray_time = (KIND == RTW_RNG_TEA_LCG || sc.has_motion) ? g.ray_time(0u) : 0.0f;
}

// A probe's direction (rtw.h rtw_probe): the Lambertian material's basis about normal n and its cosine-weighted lobe at the
// uniforms (r1, r2), operation for operation as shade_a writes them for a hit record without a baked basis (rtw_kernels.h)
RTW_DEV v3 probe_direction(const v3 n, const float r1, const float r2) {
    const v3 w = normalize3(n);
    const v3 a = (w.x > 0.9f || w.x < -0.9f) ? V(0.f, 1.f, 0.f) : V(1.f, 0.f, 0.f);
    const v3 v = normalize3(cross3(w, a));
    const v3 u = cross3(w, v);
    float sn, cs;
    sincos2pi(r1, sn, cs);
    const float sq = sqrt_(r2);
    const float lx = cs * sq;
    const float ly = sn * sq;
    const float lz = sqrt_inside_(1.0f - r2);  // r2 is a multiple of 2^-24 in [0, 1): 1 - r2 is exact and in [2^-24, 1]
    return normalize3(V(fma_(lz, w.x, fma_(ly, v.x, lx * u.x)),
                        fma_(lz, w.y, fma_(ly, v.y, lx * u.y)),
                        fma_(lz, w.z, fma_(ly, v.z, lx * u.z))));
}

// A spherical-harmonic probe's direction (rtw.h rtw_probe_sh): uniform over the sphere, in world axes, from the same two uniforms
RTW_DEV v3 probe_sh_direction(const float r1, const float r2) {
    const float z = 1.0f - 2.0f * r2;  // exact: r2 is a multiple of 2^-24 in [0, 1)
    const float s2 = fma_(-z, z, 1.0f);
    const float sq = sqrt_(s2);  // (s2 may be 0: the full-range root)
    float sn, cs;
    sincos2pi(r1, sn, cs);
    return V(cs * sq, sn * sq, z);
}

// The nine real spherical harmonics of bands 0 to 2 at d (rtw.h rtw_probe_sh, "Basis"): one rounding per operation, as written
RTW_DEV void probe_sh_basis(const v3 d, float* Y) {
    const float x = d.x, y = d.y, z = d.z;
    Y[0] = 0.282094792f;
    Y[1] = 0.488602512f * y;
    Y[2] = 0.488602512f * z;
    Y[3] = 0.488602512f * x;
    Y[4] = 1.092548431f * (x * y);
    Y[5] = 1.092548431f * (y * z);
    Y[6] = 0.315391565f * (3.0f * (z * z) - 1.0f);
    Y[7] = 1.092548431f * (x * z);
    Y[8] = 0.546274215f * ((x * x) - (y * y));
}

// k_view (rtw.h rtw_views): pixel `ray` of a launch is pixel a.first + ray of the call's flattened index
// (view * height + y) * width + x. The stream key of a pixel is width * y + x, its index inside its frame.
RTW_DEV void view_split(const ViewArgs& a, const uint32_t ray, uint32_t& view, uint32_t& key) {
    const uint32_t p = a.first + ray;
    view = fastdiv(p, a.divf_m, a.divf_s1, a.divf_s2);
    key = p - view * (a.width * a.height);
}
RTW_DEV uint32_t view_key(const ViewArgs& a, const uint32_t ray) {
    uint32_t view, key;
    view_split(a, ray, view, key);
    return key;
}
RTW_DEV uint32_t view_seed(const ViewArgs& a, const uint32_t ray) {
    uint32_t view, key;
    view_split(a, ray, view, key);
    return ((const uint32_t*)a.rays)[(size_t)view * (kViewFloat4 * 4u) + kViewSeedWord];
}

// raygen<>'s camera path of sample `sample` of pixel `ray` (rtw_kernels.h), statement for statement, with the camera, its type and
// its times read from the pixel's view record instead of the scene: the draws (the TEA+LCG stream takes its lens sample for a
// perspective camera only; a type that is neither environment nor orthographic is a perspective camera), the generator left where
// raygen<> leaves it, the gather time from the view's own time0 / time1, the first ray time, origin and direction
template <int KIND>
RTW_DEV void view_raygen(const DScene& sc, const ViewArgs& a, const uint32_t ray, const uint32_t seed, const uint32_t sample, Rng<KIND>& g, float& gt,
                         float& ray_time, v3& o, v3& d) {
    uint32_t view, pixel;
    view_split(a, ray, view, pixel);
    const uint32_t y = fastdiv(pixel, a.divw_m, a.divw_s1, a.divw_s2);
    const uint32_t x = pixel - y * a.width;
    const float4* const rec = a.rays + (size_t)view * kViewFloat4;  // seven 16-byte loads
    const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3], q4 = rec[4], q5 = rec[5], q6 = rec[6];
    const v3 c_origin = V(q0.x, q0.y, q0.z), c_u = V(q0.w, q1.x, q1.y), c_v = V(q1.z, q1.w, q2.x), c_w = V(q2.y, q2.z, q2.w);
    const v3 c_ll = V(q3.x, q3.y, q3.z), c_h = V(q3.w, q4.x, q4.y), c_vert = V(q4.z, q4.w, q5.x);
    const float lens_radius = q5.y, time0 = q5.z, time1 = q5.w;
    const int cam_type = (int)__float_as_uint(q6.x);
    const bool perspective = cam_type != RTW_CAM_ENVIRONMENT && cam_type != RTW_CAM_ORTHOGRAPHIC;
    float r0, r1, r2, r3, r4;
    if (KIND == RTW_RNG_TEA_LCG) {
        uint32_t s = tea<64>(pixel, sample);
        r0 = lcg_rnd(s); r1 = lcg_rnd(s);
        r2 = 0.0f; r3 = 0.0f;
        if (perspective) { r2 = lcg_rnd(s); r3 = lcg_rnd(s); }
        g.init(seed, pixel, sample, s, s);
        r4 = lcg_rnd(s);
    } else {
        uint32_t w[4];
        philox4x32_10(pixel, sample, 0u, 0u, seed, 0u, w);
        r0 = u24(w[0]); r1 = u24(w[1]); r2 = u24(w[2]); r3 = u24(w[3]);
        r4 = (float)(((w[0] & 0xffu) << 16) | ((w[1] & 0xffu) << 8) | (w[2] & 0xffu)) * (1.0f / 16777216.0f);
        g.init(seed, pixel, sample, 0u, sample);
    }
    const float s = ((float)x + r0) / (float)a.width;
    const float t = ((float)y + r1) / (float)a.height;
    o = c_origin;
    if (lens_radius != 0.0f) {
        float sn, cs;
        sincos2pi(r2, sn, cs);
        float sq = __builtin_sqrtf(r3);
        float rx = lens_radius * (sn * sq);
        float ry = lens_radius * (cs * sq);
        o = vadd(o, vfma(c_v, ry, vscale(c_u, rx)));
    }
    d = vfma(c_h, s, c_ll);
    d = vfma(c_vert, t, d);
    if (cam_type == RTW_CAM_ENVIRONMENT) {
        float sx, cx, sy, cy;
        sincos2pi(s, sx, cx);
        sincos2pi(t * 0.5f, sy, cy);
        const v3 e = V(cx * sy, -cy, sx * sy);
        o = c_origin;
        d = normalize3(vfma(c_w, e.z, vfma(c_v, e.y, vscale(c_u, e.x))));
    } else if (cam_type == RTW_CAM_ORTHOGRAPHIC) {
        o = vadd(d, c_origin);
        d = vneg(normalize3(c_w));
    } else {
        d = vsub(d, o);
    }
    gt = fma_(r4, time1 - time0, time0);  // (r4 = k / 2^24: gather_time_of's value for gk = k)
    ray_time = (KIND == RTW_RNG_TEA_LCG || sc.has_motion) ? g.ray_time(0u) : 0.0f;
}
// the three names for the launches of the older kernels, whose body names them under a condition that is never true there
RTW_DEV uint32_t view_key(const RadianceArgs&, const uint32_t) { return 0u; }
RTW_DEV uint32_t view_seed(const RadianceArgs&, const uint32_t) { return 0u; }
template <int KIND>
RTW_DEV void view_raygen(const DScene&, const RadianceArgs&, const uint32_t, const uint32_t, const uint32_t, Rng<KIND>&, float&, float&, v3&, v3&) {}

// k_probe_sh's per-lane LDS rows (stride kBlock): the 27 sums of the open block of 16 samples, coefficient-major, then the first
// direction of the lane's current path. Both are touched once per path (a path is hundreds of instructions) and would otherwise
// have to live in VGPRs across the segment loop, which is full at 128. The unit sums - touched once per 16 paths - run in the words
// that receive them in the end: the lane's nine float4 of the output (at most 128 spp) or of the slab [unit][point][9].
constexpr uint32_t kShSums = 27, kShRows = kShSums + 3;

// The kernels' body; sc and a are the kernel's parameters, KIND and TEX its template parameters. s_usum: the running sum of the lane's
// summation unit (the sums of its finished blocks, in order): touched once per 16 samples.
#define RTW_RADIANCE_BODY(PROBE_) \
    extern __shared__ uint32_t s_stack[]; \
    RTW_NOISE_SHARED \
    __shared__ float s_usum[3][kBlock]; \
    __shared__ float s_sh[kShRows][kBlock];  /* (never referenced, and dropped, in the two older kernels; s_usum in k_probe_sh) */ \
    const uint32_t tid = threadIdx.x; \
    const uint32_t* noise_lds = stage_noise<(TEX != 0)>(sc, s_noise); \
    /* it holds a barrier: every thread, before the loop; the branch is uniform (a property of the scene) */ \
    TravMem tm{}; \
    if (sc.use_bvh) tm = trav_mem(sc, s_stack, kBlock, tid); \
    const uint32_t lane = tid & 63u; \
    /* wave-uniform: the job stream */ \
    uint32_t u_next = 0, u_end = 0; \
    bool exhausted = false; \
    /* per lane, the unit: its ray, the current sample and the unit's end (both relative to sample0), the open block's sum */ \
    bool need = true; \
    uint32_t ray = 0, s_cur = 0, s_end = 0; \
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
                if (lane == 0) q = atomicAdd(a.queue, 1u); \
                q = __builtin_amdgcn_readfirstlane(q); \
                if (q >= a.n_jobs) { exhausted = true; break; } \
                u_next = q * a.job_units; \
                u_end = min(u_next + a.job_units, a.n_units); \
                continue; \
            } \
            const uint32_t avail = u_end - u_next; \
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need_mask, 0u)); \
            if (need && rank < avail) { \
                const uint32_t u = u_next + rank; \
                const uint32_t unit = fastdiv(u, a.divn_m, a.divn_s1, a.divn_s2); \
                ray = u - unit * a.n; \
                s_cur = unit * (kSumBlock * kSumUnitBlocks); \
                s_end = min(s_cur + kSumBlock * kSumUnitBlocks, a.spp); \
                bsum = V(0.f, 0.f, 0.f); \
                if ((int)(PROBE_) == 2) { \
                    _Pragma("unroll") for (uint32_t j = 0; j < kShSums; j++) s_sh[j][tid] = 0.f; \
                } \
                need = false; \
                alive = false; \
            } \
            u_next += min((uint32_t)__popcll(need_mask), avail); \
            need_mask = __ballot(need); \
        } \
        if (__ballot(!need) == 0ull) break; \
        const bool busy = !need; \
        const uint32_t key = (int)(PROBE_) == 3 ? view_key(a, ray) : a.key0 + ray, sample = a.sample0 + s_cur; \
        const uint32_t seed = (int)(PROBE_) == 3 ? view_seed(a, ray) : a.seed; \
        Rng<KIND> g; \
        if ((int)(PROBE_) == 3 && busy && !alive) {  /* regeneration: the next sample of this lane's pixel starts at its view's camera */ \
            view_raygen<KIND>(sc, a, ray, seed, sample, g, gt, ray_time, o, d); \
            seg_tmin = sc.ray_tmin; seg_tmax = 1.e27f;  /* the estimator's start distance, as a render's camera ray */ \
            rng_a = g.a; rng_b = g.b; \
            T = V(1.f, 1.f, 1.f); L = V(0.f, 0.f, 0.f); \
            nee_prev = 0; depth = 0; alive = true; \
        } \
        if ((int)(PROBE_) != 3 && busy && !alive) {  /* regeneration: the next sample of this lane's unit starts on the caller's ray, or at the caller's probe */ \
            const float4 r0 = a.rays[2 * (size_t)ray], r1 = a.rays[2 * (size_t)ray + 1];  /* two 16-byte loads */ \
            o = V(r0.x, r0.y, r0.z); d = V(r0.w, r1.x, r1.y); \
            seg_tmin = r1.z; seg_tmax = r1.w;  /* the caller's interval bounds the first segment only */ \
            if ((int)(PROBE_) == 2) { \
                /* floats 3..5 are loaded and unused; the direction waits in LDS for the path's end, where the basis is taken */ \
                float jitter[2]; \
                radiance_raygen<KIND, true>(sc, seed, key, sample, g, gt, ray_time, jitter); \
                d = probe_sh_direction(jitter[0], jitter[1]); \
                s_sh[kShSums][tid] = d.x; s_sh[kShSums + 1][tid] = d.y; s_sh[kShSums + 2][tid] = d.z; \
            } else if (PROBE_) { \
                /* a probe keeps nothing between its samples: the basis is rebuilt from the normal that the two loads above bring anyway */ \
                float jitter[2]; \
                radiance_raygen<KIND, true>(sc, seed, key, sample, g, gt, ray_time, jitter); \
                d = probe_direction(d, jitter[0], jitter[1]); \
            } else { \
                radiance_raygen<KIND, false>(sc, seed, key, sample, g, gt, ray_time, nullptr); \
            } \
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
            } else if ((int)(PROBE_) == 2) { \
                /* removeNaNs, then Y_j * L_c joins each of the block's 27 running sums, in sample order */ \
                const v3 Ln = V((L.x == L.x) ? L.x : 0.f, (L.y == L.y) ? L.y : 0.f, (L.z == L.z) ? L.z : 0.f); \
                float Y[9]; \
                probe_sh_basis(V(s_sh[kShSums][tid], s_sh[kShSums + 1][tid], s_sh[kShSums + 2][tid]), Y); \
                _Pragma("unroll") for (uint32_t j = 0; j < 9; j++) { \
                    s_sh[3 * j][tid] += Y[j] * Ln.x; s_sh[3 * j + 1][tid] += Y[j] * Ln.y; s_sh[3 * j + 2][tid] += Y[j] * Ln.z; \
                } \
                s_cur++; \
                if ((s_cur % kSumBlock) == 0u || s_cur >= s_end) {  /* a block is complete: its sums join the unit's */ \
                    const uint32_t b_done = (s_cur - 1u) / kSumBlock; \
                    const bool first = (b_done % kSumUnitBlocks) == 0u, last = s_cur >= s_end; \
                    const bool mean = last && a.units_per_ray == 1u;  /* at most 128 spp: the unit sum is the total */ \
                    float4* const dst = a.out + 9u * (a.units_per_ray == 1u ? (size_t)ray : (size_t)(b_done / kSumUnitBlocks) * a.n + ray); \
                    const float nf = (float)a.spp; \
                    _Pragma("unroll") for (uint32_t j = 0; j < 9; j++) { \
                        v3 prev = V(0.f, 0.f, 0.f); \
                        if (!first) { const float4 p = dst[j]; prev = V(p.x, p.y, p.z); } \
                        v3 u = vadd(prev, V(s_sh[3 * j][tid], s_sh[3 * j + 1][tid], s_sh[3 * j + 2][tid])); \
                        s_sh[3 * j][tid] = 0.f; s_sh[3 * j + 1][tid] = 0.f; s_sh[3 * j + 2][tid] = 0.f; \
                        if (mean) { \
                            u = vadd(V(0.f, 0.f, 0.f), u); \
                            u = V((u.x / nf) * kProbeSh4Pi, (u.y / nf) * kProbeSh4Pi, (u.z / nf) * kProbeSh4Pi); \
                        } \
                        dst[j] = make_float4(u.x, u.y, u.z, 0.f); \
                    } \
                    if (last) need = true; \
                } \
            } else { \
                /* removeNaNs (raygen.cu:17-24), then the block's running sum, in sample order */ \
                bsum = vadd(bsum, V((L.x == L.x) ? L.x : 0.f, (L.y == L.y) ? L.y : 0.f, (L.z == L.z) ? L.z : 0.f)); \
                s_cur++; \
                if ((s_cur % kSumBlock) == 0u || s_cur >= s_end) {  /* a block is complete: its sum joins the unit's */ \
                    const uint32_t b_done = (s_cur - 1u) / kSumBlock; \
                    v3 prev = V(0.f, 0.f, 0.f); \
                    if ((b_done % kSumUnitBlocks) != 0u) prev = V(s_usum[0][tid], s_usum[1][tid], s_usum[2][tid]); \
                    const v3 u = vadd(prev, bsum); \
                    bsum = V(0.f, 0.f, 0.f); \
                    if (s_cur >= s_end) {  /* the unit is complete */ \
                        need = true; \
                        if (a.units_per_ray == 1u) {  /* at most 128 spp: the unit sum is the total, the lane writes the mean */ \
                            const v3 sum = vadd(V(0.f, 0.f, 0.f), u); \
                            const float nf = (float)a.spp; \
                            if ((int)(PROBE_) == 1) a.out[ray] = make_float4((sum.x / nf) * kProbePi, (sum.y / nf) * kProbePi, (sum.z / nf) * kProbePi, 1.0f); \
                            else a.out[ray] = make_float4(sum.x / nf, sum.y / nf, sum.z / nf, 1.0f); \
                        } else { \
                            a.out[(size_t)(b_done / kSumUnitBlocks) * a.n + ray] = make_float4(u.x, u.y, u.z, 0.f); \
                        } \
                    } else { \
                        s_usum[0][tid] = u.x; s_usum[1][tid] = u.y; s_usum[2][tid] = u.z; \
                    } \
                } \
            } \
        } \
    } \
    for (int off = 32; off > 0; off >>= 1) { \
        n_seg += __shfl_down(n_seg, off); \
        n_shadow += __shfl_down(n_shadow, off); \
    } \
    if (lane == 0) { \
        unsigned long long* row = a.stats + (size_t)(blockIdx.x & (kStatRows - 1u)) * 8u; \
        if (n_seg) atomicAdd(&row[0], (unsigned long long)n_seg); \
        if (n_shadow) atomicAdd(&row[1], (unsigned long long)n_shadow); \
    }

}  // namespace rtwk
