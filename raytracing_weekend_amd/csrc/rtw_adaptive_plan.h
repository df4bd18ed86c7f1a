// rtw_adaptive_plan.h — the per-entry state of the adaptive family (rtw_render_adaptive, rtw_probe_adaptive, rtw_views_adaptive), laid
// out on the host from sizes alone (no HIP in here, in the style of rtw_radiance_plan.h). An entry is a shard pixel, a probe, or a
// pixel of the views at hand. tests/native/probe_adaptive_plan_check.cpp pins the layout with g++.
#pragma once
#include <stdint.h>

namespace rtwk {

// The state of a call over n entries (one context-owned allocation, sections 256-byte aligned): accum, upart (float4), part (float4:
// the running sum of the current block, which only the renderer's wavefront passes keep; present where asked for, else 0 bytes),
// moments (double2), the stop count n, err, the occlusion total, two lists (a length word, then the entries), and the compaction's
// masks and offsets (one per 64 entries). The layout for n fits in an allocation made for more entries with the same want_part.
struct AdaptiveLayout {
    enum { kAccum, kUpart, kPart, kMom, kN, kErr, kTotal, kList0, kList1, kMasks, kOffsets, kSections };
    uint64_t off[kSections + 1];
    uint64_t bytes() const { return off[kSections]; }
};
inline AdaptiveLayout adaptive_layout(uint64_t n, bool want_part) {
    const uint64_t nw = (n + 63) / 64;
    const uint64_t sz[AdaptiveLayout::kSections] = {n * 16, n * 16, want_part ? n * 16 : 0, n * 16, n * 4, n * 4, n * 4, n * 4 + 4, n * 4 + 4, nw * 8, nw * 4};
    AdaptiveLayout l{};
    for (int k = 0; k < AdaptiveLayout::kSections; k++) l.off[k + 1] = l.off[k] + ((sz[k] + 255) & ~(uint64_t)255);
    return l;
}

}  // namespace rtwk
