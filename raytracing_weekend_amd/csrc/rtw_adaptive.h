// rtw_adaptive.h — the per-entry kernels of the adaptive family (include/rtw.h: rtw_render_adaptive, rtw_probe_adaptive,
// rtw_views_adaptive): the start of a call, running sums and error moments of the listed entries, the stop rule and the compaction of
// the next active list, the results. An entry is a shard pixel, a probe or a pixel of a batch of views; the passes themselves are the
// families' own (k_path / k_first with LIST = 1, rtw_kernels.h; k_probe_list, k_view_list). Included by rtw_hip.hip, whose
// adaptive_run launches them.
//
// Per entry p the state (rtw_adaptive_plan.h) is: accum (sum of finished summation units), upart (running sum of the current unit's
// finished blocks), part (running sum of the current block: wavefront pipeline only), mom = (M1, M2) in fp64, n (0 while active, else
// the sample count the entry stopped at), err, and total (occlusion probes only). A list of active entries is list[0] = n,
// list[1 + i] = the entry of position i (the layout k_path / k_first read with LIST = 1), in ascending order. Checkpoints fall on
// block boundaries but not on unit boundaries, so a pass leaves the unit open (upart) and only k_adapt_finish closes it - the order
// in which k_resolve_blocks / k_resolve + k_finish close it.
#pragma once
#include "rtw_adaptive_stat.h"
#include "rtw_kernels.h"
#include "rtw_probe.h"

namespace rtwk {

// the start of a call: every entry active (identity list), sums and moments zero; part and total where the family keeps them (not null)
__global__ void __launch_bounds__(kBlock) k_adapt_init(uint32_t* __restrict__ list, float4* __restrict__ accum, float4* __restrict__ upart,
                                                       float4* __restrict__ part, double2* __restrict__ mom, uint32_t* __restrict__ n,
                                                       float* __restrict__ err, uint32_t* __restrict__ total, uint32_t n_entries) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_entries; i += gridDim.x * blockDim.x) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        list[1u + i] = i;
        if (i == 0u) list[0] = n_entries;
        accum[i] = z; upart[i] = z;
        if (part) part[i] = z;
        mom[i] = make_double2(0.0, 0.0);
        n[i] = 0u;
        err[i] = 0.f;
        if (total) total[i] = 0u;
    }
}

// the list counterpart of k_resolve_blocks: n_blocks block sums [block][list position] of one k_path list pass, whose first block
// is block first_block of the render (counted from sample_offset). The unit is carried across passes in upart, not flushed.
__global__ void __launch_bounds__(kBlock) k_adapt_resolve_blocks(const float4* __restrict__ slots, const uint32_t* __restrict__ list, uint32_t n_list,
                                                                 uint32_t n_blocks, uint32_t first_block, float4* __restrict__ accum,
                                                                 float4* __restrict__ upart, double2* __restrict__ mom) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_list; i += gridDim.x * blockDim.x) {
        const uint32_t p = list[1u + i];
        float4 a = accum[p], u = upart[p];
        double2 m = mom[p];
        for (uint32_t b = 0; b < n_blocks; b++) {
            const float4 S = slots[(size_t)b * n_list + i];
            adapt_moments(m, S);
            u.x += S.x; u.y += S.y; u.z += S.z;
            if (((first_block + b + 1u) % kSumUnitBlocks) == 0u) {
                a.x += u.x; a.y += u.y; a.z += u.z;
                u = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        accum[p] = a; upart[p] = u; mom[p] = m;
    }
}

// the list counterpart of k_resolve: nslots sample slots of one wavefront batch (radiance of path slot * npix + p), whose first
// sample is sample first_sample of the render. A block is closed (moments, unit sum) as soon as its last sample is in.
__global__ void __launch_bounds__(kBlock) k_adapt_resolve_samples(const float4* __restrict__ lbuf, const uint32_t* __restrict__ list, uint32_t n_list,
                                                                  uint32_t npix, uint32_t nslots, uint32_t first_sample, float4* __restrict__ accum,
                                                                  float4* __restrict__ upart, float4* __restrict__ part, double2* __restrict__ mom) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_list; i += gridDim.x * blockDim.x) {
        const uint32_t p = list[1u + i];
        float4 a = accum[p], u = upart[p], b = part[p];
        double2 m = mom[p];
        for (uint32_t s = 0; s < nslots; s++) {
            const float4 l = lbuf[(size_t)s * npix + p];
            b.x += l.x; b.y += l.y; b.z += l.z;
            const uint32_t done = first_sample + s + 1u;
            if ((done % kSumBlock) == 0u) {
                adapt_moments(m, b);
                u.x += b.x; u.y += b.y; u.z += b.z;
                b = make_float4(0.f, 0.f, 0.f, 0.f);
                if ((done % (kSumBlock * kSumUnitBlocks)) == 0u) {
                    a.x += u.x; a.y += u.y; a.z += u.z;
                    u = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        }
        accum[p] = a; upart[p] = u; part[p] = b;
        mom[p] = m;
    }
}

// Checkpoint n_k = 16 B: err of every active entry (n == 0) and the stop rule (rtw.h), dilation against the current active set (a
// neighbour's err is recomputed from its moments: no pass over the frame has to finish first). The entries are n_views frames of
// width x height: the renderer's shard is one view of width x rows, a probe batch one view of n x 1 with dilate 0. One wave per 64
// consecutive flattened pixels (a wave may span two views), p -> (view, y, x) by the exact divisions of view_split, the 3x3
// neighbourhood clamped to the pixel's own frame: neighbour (xx, yy) is pixel view * width * height + yy * width + xx, so a tap never
// reads another view (rtw_view_adaptive_plan.h view_adaptive_neighbour). masks[w] = the ballot of the pixels of wave w that stay
// active. n is only read here (k_adapt_compact writes it).
struct AdaptDecideArgs {
    uint32_t width, height, npix;  // npix = n_views * width * height
    uint32_t divw_m, divw_s1, divw_s2;  // exact division by width (magic_div)
    uint32_t divf_m, divf_s1, divf_s2;  // exact division by width * height
    uint32_t B, at_cap, dilate;
    float threshold;
};
__global__ void __launch_bounds__(kBlock) k_adapt_decide(const double2* __restrict__ mom, const uint32_t* __restrict__ n, float* __restrict__ err,
                                                         unsigned long long* __restrict__ masks, const AdaptDecideArgs a) {
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

// exclusive prefix of the masks' population counts (one workgroup of 1024 threads, each a contiguous run of waves); *count = total
// (the next list's length word)
__global__ void __launch_bounds__(1024) k_adapt_scan(const unsigned long long* __restrict__ masks, uint32_t* __restrict__ offsets, uint32_t n_waves,
                                                     uint32_t* __restrict__ count) {
    __shared__ uint32_t s_sum[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n_waves + 1023u) / 1024u, w0 = min(tid * per, n_waves), w1 = min(w0 + per, n_waves);
    uint32_t sum = 0;
    for (uint32_t w = w0; w < w1; w++) sum += (uint32_t)__popcll(masks[w]);
    s_sum[tid] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {  // inclusive Hillis-Steele scan
        const uint32_t v = tid >= off ? s_sum[tid - off] : 0u;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    uint32_t run = s_sum[tid] - sum;
    for (uint32_t w = w0; w < w1; w++) {
        offsets[w] = run;
        run += (uint32_t)__popcll(masks[w]);
    }
    if (tid == 1023u) *count = s_sum[1023];
}

// the next active list, in ascending pixel order; a pixel that stops records its sample count n_k
__global__ void __launch_bounds__(kBlock) k_adapt_compact(const unsigned long long* __restrict__ masks, const uint32_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ n, uint32_t* __restrict__ list_next, uint32_t npix, uint32_t n_k) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
        const uint32_t w = p >> 6, lane = p & 63u;
        const unsigned long long mask = masks[w];
        if ((mask >> lane) & 1ull) list_next[1u + offsets[w] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = p;
        else if (n[p] == 0u) n[p] = n_k;
    }
}

// the results: the open unit joins the total (as k_resolve_blocks / k_finish close the last unit), then the division by (float)n_p,
// alpha 1; times_pi (launch-uniform: the irradiance probe's estimate, rtw_probe.h kProbePi) multiplies the quotient afterwards.
// spp_out and err_out where they are not null.
__global__ void __launch_bounds__(kBlock) k_adapt_finish(const float4* __restrict__ accum, const float4* __restrict__ upart, const uint32_t* __restrict__ n,
                                                         const float* __restrict__ err, float4* __restrict__ out, int32_t* __restrict__ spp_out,
                                                         float* __restrict__ err_out, uint32_t n_entries, uint32_t times_pi) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_entries; i += gridDim.x * blockDim.x) {
        float4 a = accum[i];
        const float4 u = upart[i];
        a.x += u.x; a.y += u.y; a.z += u.z;
        const float spp = (float)n[i];
        float4 r = make_float4(a.x / spp, a.y / spp, a.z / spp, 1.0f);
        if (times_pi != 0u) { r.x *= kProbePi; r.y *= kProbePi; r.z *= kProbePi; }
        out[i] = r;
        if (spp_out) spp_out[i] = (int32_t)n[i];
        if (err_out) err_out[i] = err[i];
    }
}

}  // namespace rtwk
