// rtw_paths.h — declarations of the path-record kernel (rtw_paths.hip): samples replayed one by one, a head per sample and a vertex
// per traced segment (rtw.h rtw_paths / rtw_paths_device / rtw_paths_views / rtw_paths_views_device). Included by rtw_hip.hip,
// which launches it.
#pragma once
#include "../../include/rtw.h"
#include "rtw_kernels.h"
#include "rtw_view.h"

namespace rtwk {

static_assert(sizeof(rtw_path_vertex) == 64 && sizeof(rtw_path_head) == 32 && sizeof(rtw_paths_params) == 40, "rtw.h states these sizes");
static_assert((int)RTW_PATH_MISS == (int)EV_MISS && (int)RTW_PATH_SCATTER == (int)EV_HIT && (int)RTW_PATH_END == (int)EV_FINISH &&
                  (int)RTW_PATH_CANCEL == (int)EV_CANCEL,
              "RTW_PATH_* are the kernels' EV_*");
constexpr uint32_t kPathVertexFloat4 = sizeof(rtw_path_vertex) / 16, kPathHeadFloat4 = sizeof(rtw_path_head) / 16;

constexpr int kPathsRays = 0, kPathsViews = 1;  // k_paths' SRC: where a pair's first segment comes from

// One k_paths launch over the n_pairs = v.n * v.spp (ray, sample) pairs of v.n rays or pixels, pair p = ray * spp + s. `v` is
// k_view's argument block under its names, so that view_raygen<> and view_split read it as they are: rays (kPathsRays: two float4
// per ray; kPathsViews: the call's view records, lane "ray" i being flattened pixel v.first + i), stats, n, spp, sample0, seed,
// max_depth, key0, and for views width, height, first and the two divisors. Its out, queue, units and jobs are unused: nothing is
// summed here.
struct PathsArgs {
    ViewArgs v;
    float4* heads;     // kPathHeadFloat4 per pair
    float4* vertices;  // kPathVertexFloat4 per record, max_records records per pair (null when max_records == 0)
    uint32_t n_pairs, max_records;
    uint32_t divs_m, divs_s1, divs_s2;  // exact division by spp
};

// KIND x TEX as k_radiance; SRC kPathsRays or kPathsViews. Persistent launch sized as k_cast's: one lane owns one pair at a time
// and strides over the pairs. Dynamic LDS: the scene's traversal stacks and tree nodes (rtw_ctx::lds_bytes, stride kBlock).
template <int KIND, int TEX, int SRC>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_paths(const DScene sc, const PathsArgs a);

}  // namespace rtwk
