// rtw_stage_plan.h — the layout of the staging slab that the host variants of the query family share (rtw_cast, rtw_radiance, rtw_probe,
// rtw_probe_sh, rtw_views, rtw_views_guides, rtw_probe_adaptive, rtw_views_adaptive), decided on the host from sizes alone (no HIP in
// here, in the style of rtw_radiance_plan.h). tests/native/stage_plan_check.cpp pins it with g++.
#pragma once
#include <stdint.h>

namespace rtwk {

constexpr int kStageMaxSections = 8;

// One chunk's inputs and outputs in the slab: section k holds `chunk` items of width[k] bytes and begins at off[k], 256-byte aligned;
// a section nobody wants takes nothing (off[k] is valid where want[k]). `bytes` is what the slab has to hold. A call computes this from
// its own chunk: where the sections lie does not depend on how large an earlier call has made the slab.
struct StagePlan { uint64_t off[kStageMaxSections]; uint64_t bytes; };
inline StagePlan stage_plan(uint64_t chunk, int n_sections, const uint64_t* width, const bool* want) {
    StagePlan s{};
    for (int k = 0; k < n_sections && k < kStageMaxSections; k++) {
        s.off[k] = s.bytes;
        if (want[k]) s.bytes += (chunk * width[k] + 255ull) & ~255ull;
    }
    return s;
}

}  // namespace rtwk
