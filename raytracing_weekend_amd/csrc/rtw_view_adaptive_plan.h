// rtw_view_adaptive_plan.h — what rtw_views_adaptive / rtw_views_adaptive_device decide on the host from sizes alone (no HIP in here, in
// the style of rtw_radiance_plan.h). A pass is rtw_probe_adaptive's (rtw_probe_adaptive_plan.h: the blocks of a pass, R, J, the slab,
// the ranges of list positions and the per-entry state, with n = the pixels of the call or batch); what views add is the cut of the
// host entry into batches of whole views and, restated here for the check, the pixel that k_adapt_decide (rtw_adaptive.h) reads for a tap.
// tests/native/view_adaptive_plan_check.cpp pins them with g++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>

#include "../../include/rtw.h"
#include "rtw_probe_adaptive_plan.h"
#include "rtw_radiance_plan.h"

namespace rtwk {

// Views of one batch of the host entry. The dilated stop rule reads a pixel's neighbours inside its own view, so a batch holds whole
// views: as many as RTW_RADIANCE_CHUNK pixels hold, at least one (a frame larger than the knob is a batch of its own).
inline uint64_t view_adaptive_batch_views(int32_t width, int32_t height, uint64_t chunk) {
    const uint64_t frame = (uint64_t)(uint32_t)width * (uint64_t)(uint32_t)height;
    return std::max<uint64_t>(1, chunk / frame);
}
// batch b of the cut of n_views views: views [first, first + count); count = 0 past the end (radiance_range over views)
inline uint64_t view_adaptive_n_batches(uint64_t n_views, uint64_t per) { return radiance_n_ranges(n_views, per); }
inline RadianceRange view_adaptive_batch(uint64_t n_views, uint64_t per, uint64_t b) { return radiance_range(n_views, per, b); }
// The host entry walks the call's flattened pixels in uniform chunks of this many: `per` whole views. Chunk b then is pixels
// [b * chunk, min((b + 1) * chunk, n_views * frame)), which are exactly the views of view_adaptive_batch(n_views, per, b): both ends
// are multiples of the frame.
inline uint64_t view_adaptive_chunk(uint64_t per, int32_t width, int32_t height) { return per * (uint64_t)(uint32_t)width * (uint64_t)(uint32_t)height; }

// The pixel that tap (dx, dy), each in -1..1, of flattened pixel p reads under dilate = 1: p's own view, the row and the column
// clamped to the frame (k_adapt_decide: view * width * height + yy * width + xx). It never leaves the view's frame.
inline uint64_t view_adaptive_neighbour(uint64_t p, int32_t width, int32_t height, int32_t dx, int32_t dy) {
    const ViewPixel v = view_pixel(p, width, height);
    const int64_t yy = std::min<int64_t>(std::max<int64_t>((int64_t)v.y + dy, 0), (int64_t)height - 1);
    const int64_t xx = std::min<int64_t>(std::max<int64_t>((int64_t)v.x + dx, 0), (int64_t)width - 1);
    return v.view * (uint64_t)(uint32_t)width * (uint64_t)(uint32_t)height + (uint64_t)(yy * (int64_t)width + xx);
}

}  // namespace rtwk
