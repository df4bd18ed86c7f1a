// rtw_view.h — declarations of the view kernel (rtw_view.hip): frames from the caller's own cameras, every frame the frame
// rtw_render makes of the uploaded scene with that camera in its header (rtw.h rtw_views / rtw_views_device). Included by
// rtw_hip.hip, which launches it.
#pragma once
#include <cstddef>

#include "../../include/rtw.h"
#include "rtw_guides.h"
#include "rtw_kernels.h"
#include "rtw_radiance.h"

namespace rtwk {

constexpr uint32_t kViewFloat4 = sizeof(rtw_view) / 16;  // a view record is seven 16-byte loads
static_assert(sizeof(rtw_view) == 112 && sizeof(rtw_view) % 16 == 0, "rtw_view is 7 float4");
constexpr uint32_t kViewSeedWord = offsetof(rtw_view, seed) / 4;  // its 32-bit word inside a record

// One k_view launch: k_radiance's (RadianceArgs' members under their names, so that the shared body reads them) over n pixels of
// the flattened index (view * height + y) * width + x, from pixel `first` of the call. `rays` holds the call's view records, all
// of them: lane "ray" i is pixel first + i, which the kernel splits into (view, y, x) by exact division. key0 and seed are unused:
// the stream key is width * y + x and the seed is the view's. first + n <= n_views * width * height < 2^31.
struct ViewArgs {
    const float4* rays;         // the view records (kViewFloat4 each)
    float4* out;                // units_per_ray == 1: the mean of pixel first + i at [i]; else the unit sums, [unit][pixel]
    uint32_t* queue;
    unsigned long long* stats;
    uint32_t n, units_per_ray, n_units;
    uint32_t job_units, n_jobs;
    uint32_t divn_m, divn_s1, divn_s2;
    uint32_t spp, sample0, seed, max_depth, key0;
    uint32_t width, height, first;
    uint32_t divw_m, divw_s1, divw_s2;  // exact division by width
    uint32_t divf_m, divf_s1, divf_s2;  // exact division by width * height, the pixels of a frame
};

// k_radiance's instantiations and launch (KIND x TEX, persistent, the scene's dynamic LDS); the regeneration step builds the camera
// ray of the lane's pixel from its view record with raygen<>'s statements and draws (rtw_radiance_body.h)
template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_view(const DScene sc, const ViewArgs a);

// The guides of the same pixels (rtw.h rtw_views_guides): k_guides' loop, one lane per flattened pixel, grid-stride over a.n pixels
// from pixel a.first; entry i of G's buffers is pixel a.first + i. Of a it reads rays, n, spp, sample0, width, height, first and the
// two divisors; the camera rays' generator is G.rng_kind. Dynamic LDS: as k_guides (rtw_ctx::lds_bytes, stride kBlock).
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_view_guides(const DScene sc, const ViewArgs a, const GuideOut G);

}  // namespace rtwk
