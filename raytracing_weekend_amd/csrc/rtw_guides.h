// rtw_guides.h — declarations of the guide kernels (rtw_guides.hip): first-hit albedo / normal / depth / primitive buffers
// (rtw.h rtw_render_guides) and the guided a-trous pass (rtw_denoise_guided). Included by rtw_hip.hip, which launches them.
#pragma once
#include "rtw_kernels.h"

namespace rtwk {

// Device outputs of k_guides (shard-local pixel order, as rtw_render's); a null pointer is a buffer nobody asked for
struct GuideOut {
    float4* albedo;
    float4* normal;
    float* depth;
    int32_t* prim;
    int32_t rng_kind;  // rtw_rng_kind of the camera rays
};

// One lane per pixel of the shard A describes (A.npix, A.width, A.height, A.row0, A.row_stride, A.seed, A.sample0, A.spp), looping
// over its samples. Dynamic LDS: the scene's traversal stacks and tree nodes (rtw_ctx::lds_bytes, stride kBlock) in tree scenes.
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_guides(const KArgs A, const GuideOut G);

// One guided a-trous pass (rtw.h rtw_denoise_guided): k_atrous's taps and colour weight, divided by the albedo and normal terms
__global__ void __launch_bounds__(kBlock) k_atrous_guided(const float4* __restrict__ in, const float4* __restrict__ alb, const float4* __restrict__ nrm,
                                                          float4* __restrict__ out, int width, int height, int step, float inv_sigma2,
                                                          float inv_sigma_a2, float inv_sigma_n2);

// The same pass over n_views frames of width x height at once (rtw.h rtw_denoise_views): pixel i of the flattened index
// (view * height + y) * width + x, n = n_views * width * height of them; divf_*: magic_div's constants of width * height, by which
// the frame is found. A tap is clamped and addressed inside the pixel's own frame.
__global__ void __launch_bounds__(kBlock) k_atrous_guided_views(const float4* __restrict__ in, const float4* __restrict__ alb,
                                                                const float4* __restrict__ nrm, float4* __restrict__ out, uint32_t n, int width,
                                                                int height, uint32_t divf_m, uint32_t divf_s1, uint32_t divf_s2, int step,
                                                                float inv_sigma2, float inv_sigma_a2, float inv_sigma_n2);

}  // namespace rtwk
